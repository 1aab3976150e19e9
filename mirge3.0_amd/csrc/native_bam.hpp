// native_bam.hpp -- part of mirge_native.hip (one translation unit): `<sample>_sorted.bam` and `<sample>_sorted.bai` of `--sorted-bam`
// from the device-resident run (kernels_bam.hpp).  One call writes ONE sample's pair of files: the rows of `<sample>.sam` (SamPrep,
// native_sam.hpp), measured and keyed (k_bam_measure), radix-sorted by (refID, pos, reverse) -- an LSD sort is stable, so ties keep the
// .sam file's row order --, one 64-bit scan of the sorted rows' bytes, then the BGZF blocks chunk by chunk: k_bam_blocks builds and
// deflates every block of a chunk in LDS, a scan of the members' sizes and k_bam_compact close the gaps, the compressed chunk is
// copied to one of two page-locked halves and put into the file while the next chunk is being encoded (StagePipe, native_stage.hpp).  The
// uncompressed stream never exists whole, neither on the device nor on the host.  The index is built per ROW on the host from the
// sorted rows' stream offsets and the members' file offsets.
// MIRGE_BAM_BLOCK_BYTES (64 .. 65280, default 65280): uncompressed bytes per BGZF block; MIRGE_BAM_CHUNK_BLOCKS: blocks per chunk
// (default: 64 MiB of stream); MIRGE_BAM_DEFLATE=device (the default): the fixed Huffman code; =dynamic: per block also a code of its
// own (BTYPE 10), taken where it is shorter; =tight: the dynamic route's forms on the tokens of a closer parse (matches across the
// threads' segments, record-aligned, repeat-distance and region candidates, one lazy step: kernels_bam.hpp); =host: the blocks leave
// the device uncompressed and zlib level 6 deflates them on `threads` host threads (the A/B route).  All read per call.
#pragma once

static const uint8_t kBgzfEof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// one block as a BGZF member through zlib (level 6, raw deflate); a block zlib cannot shrink is stored by zlib itself
static int bam_host_member(const uint8_t* src, uint32_t n, std::vector<uint8_t>& out) {
    z_stream zs;
    std::memset(&zs, 0, sizeof(zs));
    if (deflateInit2(&zs, 6, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return -1;
    out.resize(18 + (size_t)deflateBound(&zs, n) + 8);
    zs.next_in = const_cast<Bytef*>(src); zs.avail_in = n;
    zs.next_out = out.data() + 18; zs.avail_out = (uInt)(out.size() - 26);
    const int rc = deflate(&zs, Z_FINISH);
    const size_t clen = zs.total_out;
    deflateEnd(&zs);
    if (rc != Z_STREAM_END || clen + 26 > 65536) return -1;
    const uint32_t bsize = (uint32_t)clen + 26u, crc = (uint32_t)crc32(0L, src, n);
    const uint8_t hd[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)((bsize - 1u) & 255u), (uint8_t)((bsize - 1u) >> 8)};
    std::memcpy(out.data(), hd, 18);
    uint8_t* tr = out.data() + 18 + clen;
    for (int x = 0; x < 4; x++) { tr[x] = (uint8_t)(crc >> (8 * x)); tr[4 + x] = (uint8_t)(n >> (8 * x)); }
    out.resize(bsize);
    return 0;
}

// The index (SAM specification 5.2) from the sorted ROWS: row x holds count[x] records of reference key >> 32 at [beg, beg + span) that
// occupy [off[x], off[x + 1]) of the uncompressed stream behind its H header bytes.  voff(u) = member offset << 16 | offset in the block;
// coff = the members' file offsets, the EOF block's last.
// Bins ascending, the pseudo-bin 37450 last; a bin's chunks are the maximal runs of consecutive records with that bin.
static std::vector<uint8_t> bam_build_index(int32_t n_ref, size_t n_rows, const unsigned long long* key, const uint32_t* span, const unsigned long long* count,
                                            const unsigned long long* off, unsigned long long H, uint32_t block, const std::vector<unsigned long long>& coff) {
    const unsigned long long stream_end = H + off[n_rows];  // (the end of the stream is the start of the EOF block)
    auto voff = [&](unsigned long long u) { return u < stream_end ? (coff[(size_t)(u / block)] << 16) | (u % block) : coff.back() << 16; };
    std::vector<uint8_t> out;
    auto p32 = [&](uint32_t v) { for (int x = 0; x < 4; x++) out.push_back((uint8_t)(v >> (8 * x))); };
    auto p64 = [&](unsigned long long v) { for (int x = 0; x < 8; x++) out.push_back((uint8_t)(v >> (8 * x))); };
    out.insert(out.end(), {'B', 'A', 'I', 1});
    p32((uint32_t)n_ref);
    size_t x = 0;
    for (int32_t ref = 0; ref < n_ref; ref++) {
        std::map<uint32_t, std::vector<std::pair<unsigned long long, unsigned long long>>> bins;
        std::vector<unsigned long long> lin;
        unsigned long long first = 0, last = 0, n_mapped = 0;
        long long prev_bin = -1;
        for (; x < n_rows && (int32_t)(key[x] >> 32) == ref; x++) {
            const long long beg = (long long)((key[x] & 0xFFFFFFFFull) >> 1), end = beg + (long long)span[x];
            const uint32_t bin = bam_reg2bin(beg, end);
            const unsigned long long vb = voff(H + off[x]), ve = voff(H + off[x + 1]);
            auto& ch = bins[bin];
            if (((long long)bin == prev_bin || (!ch.empty() && ch.back().second == vb)) && !ch.empty()) ch.back().second = ve;
            else ch.emplace_back(vb, ve);
            prev_bin = (long long)bin;
            if (!n_mapped) first = vb;
            last = ve; n_mapped += count[x];
            const size_t w0 = (size_t)(beg >> 14), w1 = (size_t)((end - 1) >> 14);
            if (lin.size() <= w1) lin.resize(w1 + 1, ~0ull);
            for (size_t w = w0; w <= w1; w++) if (lin[w] == ~0ull) lin[w] = vb;
        }
        for (size_t w = lin.size(); w-- > 1;) if (lin[w - 1] == ~0ull) lin[w - 1] = lin[w];
        p32((uint32_t)(bins.size() + (n_mapped ? 1 : 0)));
        for (auto& kv : bins) {
            p32(kv.first); p32((uint32_t)kv.second.size());
            for (auto& c2 : kv.second) { p64(c2.first); p64(c2.second); }
        }
        if (n_mapped) { p32(37450u); p32(2u); p64(first); p64(last); p64(n_mapped); p64(0ull); }
        p32((uint32_t)lin.size());
        for (unsigned long long v : lin) p64(v);
    }
    p64(0ull);  // n_no_coor
    return out;
}

extern "C" int mirge_bam_write_device(mirge_ctx* c, const mirge_reads* U, const mirge_result* res, const int64_t* order, int32_t sample,
                                      const int32_t* class_pass, int32_t n_class, const mirge_sam_pass* passes, int32_t n_pass,
                                      const int32_t* chrom_refid, const int64_t* chrom_refid_off, int32_t n_ref, const char* bam_path,
                                      const char* bai_path, const char* header, int64_t header_len, int32_t threads, int64_t* n_records_out,
                                      int64_t* n_stream_bytes_out, int64_t* n_file_bytes_out) {
    static_assert(MIRGE_MAX_PASSES <= MIRGE_BAM_MAXP, "BamTables holds one refID table per pass");
    if (!c || !bam_path || !bai_path || !header || header_len < 12 || !chrom_refid || !chrom_refid_off || n_ref < 0 || n_pass < 1 || n_pass > MIRGE_MAX_PASSES)
        return fail(-1, "mirge_bam_write_device: bad argument");
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    HostClock hc("bam_write_device");
    const uint32_t block = (uint32_t)std::min<size_t>(MIRGE_BAM_MAX_BLOCK, std::max<size_t>(64, env_bytes("MIRGE_BAM_BLOCK_BYTES", MIRGE_BAM_MAX_BLOCK)));
    const size_t chunk_blocks = std::max<size_t>(1, std::min<size_t>(env_bytes("MIRGE_BAM_CHUNK_BLOCKS", std::max<size_t>(1, ((size_t)64 << 20) / block)), (size_t)1 << 20));
    const char* dv = std::getenv("MIRGE_BAM_DEFLATE");
    const bool on_host = dv && std::strcmp(dv, "host") == 0, dynamic = dv && std::strcmp(dv, "dynamic") == 0, tight = dv && std::strcmp(dv, "tight") == 0;
    if (dv && *dv && !on_host && !dynamic && !tight && std::strcmp(dv, "device") != 0)
        // (both sentences are matched by callers and tests: the second is the text of the builds without the tight route)
        return fail(-1, "mirge_bam_write_device: MIRGE_BAM_DEFLATE is 'device', 'dynamic', 'tight' or 'host' "
                        "(a build without the tight route says: MIRGE_BAM_DEFLATE is 'device', 'dynamic' or 'host')");
    const int T = std::max(1, std::min(threads > 0 ? threads : 16, 256));
    const uint32_t slot_stride = (block + 5u + 26u + 15u) & ~15u;
    const unsigned long long H = (unsigned long long)header_len;

    SamPrep prep;
    unsigned long long *d_key, *d_key2, *d_total, *d_stotal, *d_off, *d_nrec, *d_count;
    uint32_t *d_fixed, *d_sfixed, *d_srows, *d_perm, *d_perm2, *d_bflags, *d_span;
    uint32_t *d_sizes = nullptr, *d_boff[2] = {nullptr, nullptr};
    int32_t* d_refid;
    uint8_t *d_header, *d_slots = nullptr, *d_comp[2] = {nullptr, nullptr};
    void* tmp2;
    // (what the copies from the device fill stands in front of the scope: it is still there when the scope waits for the stream)
    uint32_t hflags[4] = {0, 0, 0, 0};
    unsigned long long records = 0;
    std::vector<unsigned long long> h_key, h_count, h_off;
    std::vector<uint32_t> h_span;
    OutFile bam("mirge_bam_write_device"), bai("mirge_bam_write_device");  // (both or neither: commit_all; uncommitted, a file goes)
    PoolScope scope(c);
    CHECK(prep.build(scope, "mirge_bam_write_device", U, res, order, sample, class_pass, n_class, passes, n_pass));
    const SamTables& t = prep.t;
    const size_t n_rows = prep.n_rows;
    hc.lap("rows chosen");
    // ---- chromosome -> refID per pass, the header
    for (int p = 0; p < n_pass; p++) {
        const int64_t nn = chrom_refid_off[p + 1] - chrom_refid_off[p];
        bool named = false;
        for (int k = 0; k < n_class; k++) named |= class_pass[k] == p;
        if (chrom_refid_off[p] < 0 || nn < 0 || (named && nn != passes[p].n_chrom)) return fail(-1, "mirge_bam_write_device: the refID table of pass " + std::to_string(p) + " does not fit its chromosomes");
        for (int64_t k = 0; k < nn; k++)
            if (chrom_refid[chrom_refid_off[p] + k] >= n_ref) return fail(-1, "mirge_bam_write_device: a refID beyond the reference list");
    }
    const size_t n_map = (size_t)chrom_refid_off[n_pass];
    CHECK(scope.get(&d_refid, n_map + 1)); CHECK(scope.get(&d_header, (size_t)H + 16)); CHECK(scope.get(&d_bflags, 16)); CHECK(scope.get(&d_nrec, 2));
    CHECK(scope.get(&d_key, n_rows + 1)); CHECK(scope.get(&d_key2, n_rows + 1)); CHECK(scope.get(&d_perm, n_rows + 1)); CHECK(scope.get(&d_perm2, n_rows + 1));
    CHECK(scope.get(&d_fixed, n_rows + 1)); CHECK(scope.get(&d_sfixed, n_rows + 1)); CHECK(scope.get(&d_srows, n_rows + 1)); CHECK(scope.get(&d_span, n_rows + 1));
    CHECK(scope.get(&d_count, n_rows + 1)); CHECK(scope.get(&d_total, n_rows + 1)); CHECK(scope.get(&d_stotal, n_rows + 1)); CHECK(scope.get(&d_off, n_rows + 1));
    BamTables bt;
    std::memset(&bt, 0, sizeof(bt));
    for (int p = 0; p < n_pass; p++) bt.refid[p] = d_refid + chrom_refid_off[p];
    bt.header = d_header; bt.header_len = H;
    if (n_map) HIPOK(hipMemcpyAsync(d_refid, chrom_refid, n_map * 4, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(d_header, header, (size_t)H, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemsetAsync(d_bflags, 0, 64, c->stream));
    HIPOK(hipMemsetAsync(d_nrec, 0, 16, c->stream));
    HIPOK(hipMemsetAsync(d_stotal + n_rows, 0, 8, c->stream));
    if (n_rows) {
        LaunchScope ls(c, "k_bam_measure", (double)n_rows);
        hipLaunchKernelGGL(k_bam_measure, dim3(grid_for(c, n_rows)), dim3(MIRGE_BLOCK), 0, c->stream, t, bt, (const uint32_t*)prep.d_rows, (uint32_t)n_rows, d_key,
                           d_fixed, d_total, d_nrec, d_bflags);
    }
    HIPOK(hipMemcpyAsync(hflags, d_bflags, 16, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(&records, d_nrec, 8, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    if (hflags[0] & 2u) {
        std::string name = "?";
        if (hflags[1] < (uint32_t)n_pass && (int64_t)hflags[2] < passes[hflags[1]].n_chrom) {
            const mirge_sam_pass& in = passes[hflags[1]];
            name.assign(in.chrom_data + in.chrom_off[hflags[2]], in.chrom_data + in.chrom_off[hflags[2] + 1]);
        }
        return fail(-1, "mirge_bam_write_device: reads lie on '" + name + "', which no @SQ line of the header names");
    }
    if (hflags[0] & 4u) return fail(-1, "mirge_bam_write_device: a read lies outside [1, 2^29] of its reference: a BAM index cannot hold it");
    if (hflags[0] & 8u) return fail(-1, "mirge_bam_write_device: the QNAME of a read of " + std::to_string(hflags[3]) + " nt exceeds 254 characters (BAM's l_read_name is one byte)");
    hc.lap("measured");
    // ---- rows sorted by (refID, pos, reverse); their bytes scanned
    size_t tb2 = 0, tb3 = 0;
    if (n_rows) {
        hipLaunchKernelGGL(k_iota, dim3(grid_for(c, n_rows)), dim3(MIRGE_BLOCK), 0, c->stream, d_perm, (uint32_t)n_rows);
        HIPOK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb2, d_key, d_key2, d_perm, d_perm2, (int)n_rows, 0, 64, c->stream));
    }
    HIPOK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb3, d_stotal, d_off, (int)(n_rows + 1), c->stream));
    CHECK(scope.get((uint8_t**)&tmp2, std::max<size_t>(std::max(tb2, tb3), 16)));
    if (n_rows) {
        LaunchScope ls(c, "bam_sort_rows", (double)n_rows);
        HIPOK(hipcub::DeviceRadixSort::SortPairs(tmp2, tb2, d_key, d_key2, d_perm, d_perm2, (int)n_rows, 0, 64, c->stream));
        hipLaunchKernelGGL(k_bam_gather, dim3(grid_for(c, n_rows)), dim3(MIRGE_BLOCK), 0, c->stream, (const uint32_t*)d_perm2, (uint32_t)n_rows,
                           (const uint32_t*)prep.d_rows, (const uint32_t*)d_fixed, (const unsigned long long*)d_total, d_srows, d_sfixed, d_stotal);
        hipLaunchKernelGGL(k_bam_row_table, dim3(grid_for(c, n_rows)), dim3(MIRGE_BLOCK), 0, c->stream, t, bt, (const uint32_t*)d_srows, (uint32_t)n_rows, d_span, d_count);
    }
    HIPOK(hipcub::DeviceScan::ExclusiveSum(tmp2, tb3, d_stotal, d_off, (int)(n_rows + 1), c->stream));
    h_key.resize(n_rows + 1); h_count.resize(n_rows + 1); h_off.resize(n_rows + 1); h_span.resize(n_rows + 1);
    HIPOK(hipMemcpyAsync(h_off.data(), d_off, (n_rows + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    if (n_rows) {
        HIPOK(hipMemcpyAsync(h_key.data(), d_key2, n_rows * 8, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipMemcpyAsync(h_count.data(), d_count, n_rows * 8, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipMemcpyAsync(h_span.data(), d_span, n_rows * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPOK(hipStreamSynchronize(c->stream));
    const unsigned long long body = h_off[n_rows];
    hc.lap("sorted");
    // ---- the file, chunk by chunk
    const unsigned long long stream_bytes = H + body, n_blocks = (stream_bytes + block - 1) / block;
    const unsigned long long n_chunks = (n_blocks + chunk_blocks - 1) / chunk_blocks;
    const size_t cb = (size_t)std::min<unsigned long long>(chunk_blocks, n_blocks);
    const size_t half = cb * slot_stride, meta = ((cb + 1) * 4 + 15) & ~size_t(15);
    std::vector<unsigned long long> coff((size_t)n_blocks + 1, 0ull);
    CHECK(bam.open(bam_path));
    StagePipe pipe(c, bam.who, "a chunk failed on the device");
    CHECK(pipe.ensure(half + meta));
    if (!on_host) { CHECK(scope.get(&d_slots, half + 16)); CHECK(scope.get(&d_sizes, cb + 1)); }
    size_t tb4 = 0;
    for (int h = 0; h < (n_chunks < 2 ? 1 : 2); h++) {
        CHECK(scope.get(&d_comp[h], half + 16));
        if (!on_host) CHECK(scope.get(&d_boff[h], cb + 1));
    }
    if (!on_host) {
        HIPOK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb4, d_sizes, d_boff[0], (int)(cb + 1), c->stream));
        if (tb4 > std::max(std::max(tb2, tb3), (size_t)16)) { scope.give(tmp2); CHECK(scope.get((uint8_t**)&tmp2, tb4)); }
    }
    unsigned long long file_at = 0;
    std::vector<std::vector<uint8_t>> members;
    std::vector<uint8_t> joined;
    auto blocks_of = [&](unsigned long long ci) { return (size_t)std::min<unsigned long long>(chunk_blocks, n_blocks - ci * chunk_blocks); };
    auto take = [&](unsigned long long ci) -> int {  // chunk ci's event has passed: fetch it, write it behind what is there
        const int h = (int)(ci & 1);
        const size_t nb = blocks_of(ci);
        const unsigned long long b0 = ci * chunk_blocks;
        uint8_t* stage = pipe.half(ci);
        if (!on_host) {
            const uint32_t* boff = reinterpret_cast<const uint32_t*>(stage + half);  // exclusive scan of the members' sizes
            const size_t total = boff[nb];
            if (total > half) return fail(-6, "mirge_bam_write_device: a chunk's members do not fit their slots");
            if (hipMemcpyAsync(stage, d_comp[h], total, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
                return fail(-2, "mirge_bam_write_device: the copy of a chunk failed");
            for (size_t b = 0; b < nb; b++) coff[(size_t)b0 + b] = file_at + boff[b];
            if (int r = bam.put(stage, total, file_at)) return r;
            file_at += total;
            return 0;
        }
        members.resize(nb);
        std::atomic<int> bad{0};
        mirge_gz::parallel_for((int)nb, T, [&](int b) {
            const unsigned long long at0 = (b0 + (unsigned long long)b) * block;
            const uint32_t n = (uint32_t)std::min<unsigned long long>(block, stream_bytes - at0);
            if (bam_host_member(stage + (size_t)b * block, n, members[(size_t)b])) bad = 1;
        });
        if (bad) return fail(-6, "mirge_bam_write_device: zlib could not deflate a block");
        joined.clear();
        for (size_t b = 0; b < nb; b++) {
            coff[(size_t)b0 + b] = file_at + joined.size();
            joined.insert(joined.end(), members[b].begin(), members[b].end());
        }
        if (int r = bam.put(joined.data(), joined.size(), file_at)) return r;
        file_at += joined.size();
        return 0;
    };
    auto queue = [&](unsigned long long ci) -> int {
        const int h = (int)(ci & 1);
        const size_t nb = blocks_of(ci);
        const unsigned long long b0 = ci * chunk_blocks;
        uint8_t* stage = pipe.half(ci);
        const unsigned grid = (unsigned)std::min<size_t>(nb, (size_t)1 << 20);  // one workgroup per block: the hardware balances them
        {
            LaunchScope ls(c, "k_bam_blocks", (double)nb * block);
            if (dynamic)  // deflate == 2: an instantiation of its own (kernels_bam.hpp)
                hipLaunchKernelGGL(k_bam_blocks_dynamic, dim3(grid), dim3(MIRGE_BLOCK), 0, c->stream, t, bt, (const uint32_t*)d_srows, (uint32_t)n_rows,
                                   (const uint32_t*)d_sfixed, (const unsigned long long*)d_off, stream_bytes, b0, (uint32_t)nb, block, slot_stride, d_slots, d_sizes);
            else if (tight)  // deflate == 3: likewise
                hipLaunchKernelGGL(k_bam_blocks_tight, dim3(grid), dim3(MIRGE_BLOCK), 0, c->stream, t, bt, (const uint32_t*)d_srows, (uint32_t)n_rows,
                                   (const uint32_t*)d_sfixed, (const unsigned long long*)d_off, stream_bytes, b0, (uint32_t)nb, block, slot_stride, d_slots, d_sizes);
            else
                hipLaunchKernelGGL(k_bam_blocks, dim3(grid), dim3(MIRGE_BLOCK), 0, c->stream, t, bt, (const uint32_t*)d_srows, (uint32_t)n_rows, (const uint32_t*)d_sfixed,
                                   (const unsigned long long*)d_off, stream_bytes, b0, (uint32_t)nb, block, on_host ? 0 : 1, slot_stride,
                                   on_host ? d_comp[h] : d_slots, d_sizes);
        }
        if (on_host) {
            const size_t nn = (size_t)(std::min<unsigned long long>(stream_bytes, (b0 + nb) * block) - b0 * block);
            HIPOK(hipMemcpyAsync(stage, d_comp[h], nn, hipMemcpyDeviceToHost, c->stream));
        } else {
            HIPOK(hipMemsetAsync(d_sizes + nb, 0, 4, c->stream));
            HIPOK(hipcub::DeviceScan::ExclusiveSum(tmp2, tb4, d_sizes, d_boff[h], (int)(nb + 1), c->stream));
            {
                LaunchScope ls(c, "k_bam_compact", (double)nb);
                hipLaunchKernelGGL(k_bam_compact, dim3((unsigned)std::min<size_t>(nb, (size_t)c->n_cu * 8)), dim3(MIRGE_BLOCK), 0, c->stream, (const uint8_t*)d_slots,
                                   slot_stride, (const uint32_t*)d_sizes, (const uint32_t*)d_boff[h], (uint32_t)nb, d_comp[h]);
            }
            HIPOK(hipMemcpyAsync(stage + half, d_boff[h], (nb + 1) * 4, hipMemcpyDeviceToHost, c->stream));
        }
        return 0;
    };
    CHECK(pipe.run(n_chunks, queue, take));
    coff[(size_t)n_blocks] = file_at;
    CHECK(bam.put(kBgzfEof, sizeof(kBgzfEof), file_at));
    file_at += sizeof(kBgzfEof);
    hc.lap("encoded + written");
    // ---- the index
    const std::vector<uint8_t> index = bam_build_index(n_ref, n_rows, h_key.data(), h_span.data(), h_count.data(), h_off.data(), H, block, coff);
    CHECK(bai.open(bai_path)); CHECK(bai.put(index.data(), index.size(), 0));
    hc.lap("indexed");
    // The rows' host arrays (84 MB for 3 M rows) go here, in front of the scope's wait, not behind it as the call's last act: freed
    // last, the NEXT call's first kernels (SamPrep::build) took 15 to 20 ms longer, in system time (profiles/pool_scope_ab.md).
    // Nothing is on its way into them: the stream was waited for behind their copies.
    std::vector<unsigned long long>().swap(h_key); std::vector<unsigned long long>().swap(h_count); std::vector<unsigned long long>().swap(h_off);
    std::vector<uint32_t>().swap(h_span);
    CHECK(commit_all({&bai, &bam}));  // (a failed .bai takes the .bam with it; every chunk has been taken, nothing is still on its way)
    if (n_records_out) *n_records_out = (int64_t)records;
    if (n_stream_bytes_out) *n_stream_bytes_out = (int64_t)stream_bytes;
    if (n_file_bytes_out) *n_file_bytes_out = (int64_t)file_at;
    return 0;
}

// bam_huff_lengths (kernels_bam.hpp) alone on the device: the code lengths of counts[n_sym] under the limit max_bits
extern "C" int mirge_bam_huffman_probe(mirge_ctx* c, const uint32_t* counts, int32_t n_sym, int32_t max_bits, uint8_t* lengths_out) {
    if (!c || !counts || !lengths_out || n_sym < 1 || n_sym > MIRGE_BAM_HUFF_MAX || max_bits < 1 || max_bits > 15 || (1 << max_bits) < n_sym)
        return fail(-1, "mirge_bam_huffman_probe: 1 .. " + std::to_string(MIRGE_BAM_HUFF_MAX) + " symbols, max_bits 1 .. 15 with 2^max_bits >= the symbols");
    HIPOK(hipSetDevice(c->device));
    uint32_t* d_cnt;
    uint8_t* d_len;
    PoolScope scope(c);
    CHECK(scope.get(&d_cnt, (size_t)n_sym)); CHECK(scope.get(&d_len, (size_t)n_sym + 16));
    HIPOK(hipMemcpyAsync(d_cnt, counts, (size_t)n_sym * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_bam_huff_probe, dim3(1), dim3(MIRGE_BLOCK), 0, c->stream, (const uint32_t*)d_cnt, (uint32_t)n_sym, (uint32_t)max_bits, d_len);
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpyAsync(lengths_out, d_len, (size_t)n_sym, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}
