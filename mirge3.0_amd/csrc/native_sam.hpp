// native_sam.hpp -- part of mirge_native.hip (one translation unit): `<sample>.sam` of `--sam-out` from the device-resident run
// (kernels_sam.hpp).  One call writes ONE sample's file: rows chosen and ordered (k_sam_select, one scan), measured (k_sam_measure,
// one 64-bit scan), then the text produced chunk by chunk (k_sam_write) into one of two device buffers, copied to page-locked
// staging and put into the file while the next chunk is being formatted (StagePipe, native_stage.hpp).  The text of a sample is one
// line per RAW read (a gigabyte for 10 M reads): it never exists whole, neither on the device nor on the host.
// MIRGE_SAM_CHUNK_BYTES / MIRGE_SAM_TILE_BYTES (read per call): the chunk and the workgroup's tile; tests make them small so that
// their boundaries fall inside lines, inside a QNAME's digits and inside a row of many copies.
#pragma once

// What `--sam-out` and `--sorted-bam` share: the passes' lift tables on the device (ONE blob: 8-byte items first, then 4-byte, then
// bytes) and the file's rows in class order (k_sam_select, one scan, k_sam_rows).  build() leaves the stream synchronised; the blocks are
// the calling export's (its PoolScope).
struct SamPrep {
    uint8_t* d_blob = nullptr;
    uint32_t *d_order = nullptr, *d_keep = nullptr, *d_pos = nullptr, *d_rows = nullptr, *d_flags = nullptr;
    void* tmp = nullptr;
    size_t tb = 0, n_rows = 0;
    SamTables t;
    int build(PoolScope& scope, const std::string& who, const mirge_reads* U, const mirge_result* res, const int64_t* order, int32_t sample,
              const int32_t* class_pass, int32_t n_class, const mirge_sam_pass* passes, int32_t n_pass) {
        mirge_ctx* const c = scope.c;
        if (!U || !res || (U->n && !order) || !class_pass || n_class < 1 || n_class > MIRGE_SAM_NCLASS || !passes || n_pass < 1 ||
            n_pass > MIRGE_MAX_PASSES || n_pass < res->n_pass || U->n_samples < 1 || sample < 0 || sample >= U->n_samples || res->n != U->n)
            return fail(-1, who + ": bad argument");
        // hipCUB's scans take an `int` item count, and the flag array holds one entry per class and frame row
        if ((unsigned long long)U->n * MIRGE_SAM_NCLASS >= 0x7FFFFFF0ull) return fail(-5, who + ": too many unique reads for one call");
        for (int gi = 0; gi < MIRGE_NGROUPS; gi++) {
            if (U->g[gi].n && U->g[gi].orig) return fail(-1, who + ": the read set is not a collapse result");
            if (U->g[gi].n != res->g[gi].n && !res->dmeta) return fail(-1, who + ": result and read set differ");
        }
        const size_t n = (size_t)U->n;
        std::vector<SamPass> hp((size_t)n_pass);
        std::memset(hp.data(), 0, hp.size() * sizeof(SamPass));
        std::vector<long long> b8;
        std::vector<uint32_t> b4;
        std::vector<uint8_t> b1;
        struct At { size_t lo, hi, chrom, minus, ptr, s, e, coff, cdata; };
        std::vector<At> at((size_t)n_pass);
        for (int p = 0; p < n_pass; p++) hp[(size_t)p].cls = -1;
        for (int k = 0; k < n_class; k++) {
            const int32_t p = class_pass[k];
            if (p < 0 || p >= n_pass || hp[(size_t)p].cls >= 0) return fail(-1, who + ": class order names a pass twice or out of range");
            hp[(size_t)p].cls = k;
        }
        for (int p = 0; p < n_pass; p++) {
            SamPass& sp = hp[(size_t)p];
            if (sp.cls < 0) continue;
            const mirge_sam_pass& in = passes[p];
            if (!in.lib || in.n_refs != in.lib->n_refs || in.n_refs < 0 || in.n_refs >= 0x7FFFFFF0ll || in.trim5 < 0 || in.trim3 < 0 ||
                in.n_chrom < 0 || (in.n_refs && (!in.chrom_of_ref || !in.minus || !in.seg_ptr)) || (in.n_chrom && (!in.chrom_off || !in.chrom_data)))
                return fail(-1, who + ": lift tables of pass " + std::to_string(p) + " do not fit its library");
            const int64_t n_seg = in.n_refs ? in.seg_ptr[in.n_refs] : 0;
            const int64_t n_cb = in.n_chrom ? in.chrom_off[in.n_chrom] - in.chrom_off[0] : 0;
            if (n_seg < 0 || n_seg >= 0x7FFFFFF0ll || n_cb < 0 || n_cb >= 0x7FFFFFF0ll || in.n_chrom >= 0x7FFFFFF0ll ||
                (n_seg && (!in.seg_s || !in.seg_e || !in.cds_lo || !in.cds_hi)))
                return fail(-1, who + ": lift tables of pass " + std::to_string(p) + " are malformed");
            for (int64_t r = 0; r < in.n_refs; r++)
                if (in.seg_ptr[r] < 0 || in.seg_ptr[r + 1] < in.seg_ptr[r] || in.chrom_of_ref[r] >= in.n_chrom)
                    return fail(-1, who + ": lift tables of pass " + std::to_string(p) + " are malformed");
            At& a = at[(size_t)p];
            a.lo = b8.size(); b8.insert(b8.end(), in.cds_lo, in.cds_lo + n_seg);
            a.hi = b8.size(); b8.insert(b8.end(), in.cds_hi, in.cds_hi + n_seg);
            a.chrom = b4.size(); for (int64_t r = 0; r < in.n_refs; r++) b4.push_back((uint32_t)in.chrom_of_ref[r]);
            a.ptr = b4.size(); for (int64_t r = 0; r <= in.n_refs; r++) b4.push_back(in.n_refs ? (uint32_t)in.seg_ptr[r] : 0u);
            a.s = b4.size(); for (int64_t s = 0; s < n_seg; s++) b4.push_back((uint32_t)in.seg_s[s]);
            a.e = b4.size(); for (int64_t s = 0; s < n_seg; s++) b4.push_back((uint32_t)in.seg_e[s]);
            a.coff = b4.size(); for (int64_t k = 0; k <= in.n_chrom; k++) b4.push_back(in.n_chrom ? (uint32_t)(in.chrom_off[k] - in.chrom_off[0]) : 0u);
            a.minus = b1.size(); b1.insert(b1.end(), in.minus, in.minus + in.n_refs);
            a.cdata = b1.size();
            if (n_cb) b1.insert(b1.end(), (const uint8_t*)in.chrom_data + in.chrom_off[0], (const uint8_t*)in.chrom_data + in.chrom_off[0] + n_cb);
            sp.T = in.lib->dT; sp.inv = in.lib->dinv; sp.ref_start = in.lib->dref_start;
            sp.n_refs = (uint32_t)in.n_refs; sp.n_chrom = (uint32_t)in.n_chrom; sp.trim5 = in.trim5; sp.trim3 = in.trim3;
        }
        const size_t bytes8 = b8.size() * 8, bytes4 = b4.size() * 4, bytesP = hp.size() * sizeof(SamPass);
        const size_t o4 = bytes8, o1 = o4 + bytes4, oP = (o1 + b1.size() + 15) & ~size_t(15), blob_bytes = oP + bytesP;
        std::vector<uint8_t> blob(blob_bytes, 0);
        if (bytes8) std::memcpy(blob.data(), b8.data(), bytes8);
        if (bytes4) std::memcpy(blob.data() + o4, b4.data(), bytes4);
        if (!b1.empty()) std::memcpy(blob.data() + o1, b1.data(), b1.size());
        const size_t nf = n * MIRGE_SAM_NCLASS;
        std::vector<uint32_t> o32(std::max<size_t>(n, 1));
        for (size_t k = 0; k < n; k++) {
            if (order[k] < 0 || order[k] >= U->n) return fail(-1, who + ": row index out of range");
            o32[k] = (uint32_t)order[k];
        }
        CHECK(scope.get(&d_blob, blob_bytes + 16)); CHECK(scope.get(&d_order, std::max<size_t>(n, 1)));
        CHECK(scope.get(&d_keep, nf + 1)); CHECK(scope.get(&d_pos, nf + 1)); CHECK(scope.get(&d_flags, 16));
        std::memset(&t, 0, sizeof(t));
        t.n_pass = n_pass; t.S = U->n_samples; t.sample = sample;
        for (int gi = 0; gi < MIRGE_NGROUPS; gi++) {
            const ReadGroup& g = U->g[gi];
            const ResGroup& r = res->g[gi];
            t.g[gi] = CsvGroup{g.seq, g.nmask, g.len, g.counts, r.pass, r.ref, g.base, g.n, g.W, is_long_group(gi) ? 1 : 0};
            t.off[gi] = r.off; t.mm[gi] = r.mm;
        }
        for (int p = 0; p < n_pass; p++) {
            SamPass& sp = hp[(size_t)p];
            if (sp.cls < 0) continue;
            const At& a = at[(size_t)p];
            sp.cds_lo = reinterpret_cast<const long long*>(d_blob) + a.lo;
            sp.cds_hi = reinterpret_cast<const long long*>(d_blob) + a.hi;
            const uint32_t* w4 = reinterpret_cast<const uint32_t*>(d_blob + o4);
            sp.chrom_of_ref = reinterpret_cast<const int32_t*>(w4 + a.chrom);
            sp.seg_ptr = w4 + a.ptr;
            sp.seg_s = reinterpret_cast<const int32_t*>(w4 + a.s);
            sp.seg_e = reinterpret_cast<const int32_t*>(w4 + a.e);
            sp.chrom_off = w4 + a.coff;
            sp.minus = d_blob + o1 + a.minus;
            sp.chrom_data = d_blob + o1 + a.cdata;
        }
        std::memcpy(blob.data() + oP, hp.data(), bytesP);
        t.pass = reinterpret_cast<const SamPass*>(d_blob + oP);
        hipError_t e = hipMemcpyAsync(d_blob, blob.data(), blob_bytes, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess && n) e = hipMemcpyAsync(d_order, o32.data(), n * 4, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(d_keep, 0, (nf + 1) * 4, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(d_flags, 0, 64, c->stream);
        if (e != hipSuccess) { (void)hipStreamSynchronize(c->stream); return fail(-2, who + ": " + hipGetErrorString(e)); }
        // ---- the file's rows, in class order
        if (n) {
            LaunchScope ls(c, "k_sam_select", (double)n);
            hipLaunchKernelGGL(k_sam_select, dim3(grid_for(c, n)), dim3(MIRGE_BLOCK), 0, c->stream, t, (const uint32_t*)d_order, (uint32_t)n, d_keep, d_flags);
        }
        e = hipcub::DeviceScan::ExclusiveSum(nullptr, tb, d_keep, d_pos, (int)(nf + 1), c->stream);
        int rc = 0;
        if (e == hipSuccess && (rc = scope.get((uint8_t**)&tmp, std::max<size_t>(tb, 16)))) { (void)hipStreamSynchronize(c->stream); return rc; }
        if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(tmp, tb, d_keep, d_pos, (int)(nf + 1), c->stream);
        uint32_t n_rows32 = 0, hflag = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&n_rows32, d_pos + nf, 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&hflag, d_flags, 4, hipMemcpyDeviceToHost, c->stream);
        const hipError_t e2 = hipStreamSynchronize(c->stream);  // (also when a call failed: the host vectors above leave scope)
        if (e == hipSuccess) e = e2;
        if (e != hipSuccess) return fail(-2, who + ": " + hipGetErrorString(e));
        if (hflag) return fail(-1, who + ": pass, reference or offset out of range");
        n_rows = n_rows32;
        CHECK(scope.get(&d_rows, std::max<size_t>(n_rows, 1)));
        if (n_rows)
            hipLaunchKernelGGL(k_sam_rows, dim3(grid_for(c, nf)), dim3(MIRGE_BLOCK), 0, c->stream, (const uint32_t*)d_order, (uint32_t)n, (const uint32_t*)d_keep,
                               (const uint32_t*)d_pos, d_rows);
        return 0;
    }
};

// mirge_sam_write_device and mirge_sam_write_device_bgzf: gzi_path == nullptr is the plain file, else `path` is the .gz (BgzfSink)
static int sam_write_impl(const std::string& who, mirge_ctx* c, const mirge_reads* U, const mirge_result* res, const int64_t* order, int32_t sample,
                          const int32_t* class_pass, int32_t n_class, const mirge_sam_pass* passes, int32_t n_pass, const char* path,
                          const char* header, int64_t header_len, int64_t* n_lines_out, int64_t* n_bytes_out, const char* gzi_path,
                          int64_t block_bytes, int64_t* stats_out) {
    if (!c || !path || (!header && header_len) || header_len < 0) return fail(-1, who + ": bad argument");
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    HostClock hc("sam_write_device");
    const bool bgzf = gzi_path != nullptr;
    // ---- sizes of the chunked output
    size_t tile = env_bytes("MIRGE_SAM_TILE_BYTES", 8160);  // 255 probe points of 32 bytes + the one behind the tile's end: one per thread
    tile = std::min<size_t>(MIRGE_SAM_MAX_TILE, std::max<size_t>(64, tile)) & ~size_t(15);
    size_t chunk = env_bytes("MIRGE_SAM_CHUNK_BYTES", (size_t)32 << 20);
    chunk = std::min<size_t>((size_t)1 << 30, std::max(chunk, tile)) / tile * tile;

    SamPrep prep;
    uint8_t* d_text[2] = {nullptr, nullptr};
    uint32_t* d_fixed;
    unsigned long long *d_total, *d_off, *d_nlines, body = 0, lines = 0;
    OutFile out(who);  // (not committed: it takes its file with it, behind the scope's wait)
    BgzfStream gz(who);
    BgzfStream* const gzs[1] = {&gz};
    PoolScope scope(c);
    BgzfSink sink(scope, who);
    if (bgzf) CHECK(sink.configure(block_bytes));  // (a wrong MIRGE_BGZF_* value: before anything is done)
    CHECK(prep.build(scope, who, U, res, order, sample, class_pass, n_class, passes, n_pass));
    const SamTables& t = prep.t;
    uint32_t* const d_rows = prep.d_rows;
    const size_t n_rows = prep.n_rows;
    hc.lap("rows chosen");
    CHECK(scope.get(&d_nlines, 2)); CHECK(scope.get(&d_fixed, std::max<size_t>(n_rows, 1)));
    CHECK(scope.get(&d_total, n_rows + 1)); CHECK(scope.get(&d_off, n_rows + 1));
    HIPOK(hipMemsetAsync(d_total + n_rows, 0, 8, c->stream));
    HIPOK(hipMemsetAsync(d_nlines, 0, 16, c->stream));
    if (n_rows) {
        LaunchScope ls(c, "k_sam_measure", (double)n_rows);
        hipLaunchKernelGGL(k_sam_measure, dim3(grid_for(c, n_rows)), dim3(MIRGE_BLOCK), 0, c->stream, t, (const uint32_t*)d_rows, (uint32_t)n_rows, d_fixed,
                           d_total, d_nlines);
    }
    size_t tb2 = 0;
    HIPOK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb2, d_total, d_off, (int)(n_rows + 1), c->stream));
    if (tb2 > prep.tb) { scope.give(prep.tmp); CHECK(scope.get((uint8_t**)&prep.tmp, tb2)); }
    HIPOK(hipcub::DeviceScan::ExclusiveSum(prep.tmp, tb2, d_total, d_off, (int)(n_rows + 1), c->stream));
    HIPOK(hipMemcpyAsync(&body, d_off + n_rows, 8, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(&lines, d_nlines, 8, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    hc.lap("measured");
    if (bgzf) {  // ---- the stream is the header and the body in one; its chunks are whole BGZF blocks
        const unsigned long long H = (unsigned long long)header_len;
        uint8_t* d_header = nullptr;
        if (H) {
            CHECK(scope.get(&d_header, (size_t)H + 16));
            HIPOK(hipMemcpyAsync(d_header, header, (size_t)H, hipMemcpyHostToDevice, c->stream));
        }
        gz.bytes = H + body;
        CHECK(gz.open(path, gzi_path));
        // the header's part of a chunk lies in front of a multiple of 16, where k_sam_write's 16-byte stores start
        auto fill = [&](int, unsigned long long at, uint32_t nn, uint8_t* dst, const uint8_t** text) -> int {
            const uint32_t hpart = at < H ? (uint32_t)std::min<unsigned long long>(nn, H - at) : 0u, pad = (16u - (hpart & 15u)) & 15u, bn = nn - hpart;
            if (hpart) HIPOK(hipMemcpyAsync(dst + pad, d_header + at, hpart, hipMemcpyDeviceToDevice, c->stream));
            if (bn) {
                const size_t tiles = ((size_t)bn + tile - 1) / tile;
                LaunchScope ls(c, "k_sam_write", (double)bn);
                hipLaunchKernelGGL(k_sam_write, dim3((unsigned)std::min<size_t>(tiles, (size_t)c->n_cu * 32)), dim3(MIRGE_BLOCK), 0, c->stream, t,
                                   (const uint32_t*)d_rows, (uint32_t)n_rows, (const uint32_t*)d_fixed, (const unsigned long long*)d_off, at + hpart - H, bn,
                                   (uint32_t)tile, dst + pad + hpart);
            }
            *text = dst + pad;
            return 0;
        };
        CHECK(sink.run(gzs, 1, chunk, fill));
        hc.lap("formatted + deflated + written");
        CHECK(commit_all({&gz.gz, &gz.gzi}));
        if (stats_out) gz.stats(stats_out);
        if (n_lines_out) *n_lines_out = (int64_t)lines;
        if (n_bytes_out) *n_bytes_out = (int64_t)body;
        return 0;
    }
    // ---- the file: header, then the body chunk by chunk
    CHECK(out.open(path));
    if (header_len && out.put(header, (size_t)header_len, 0)) return fail(-8, std::string("cannot write ") + path);
    if (body) {
        const size_t buf = (size_t)std::min<unsigned long long>(chunk, body);
        StagePipe pipe(c, out.who);
        CHECK(pipe.ensure(buf));
        CHECK(scope.get(&d_text[0], buf + 16));
        if (body > buf) CHECK(scope.get(&d_text[1], buf + 16));
        auto queue = [&](unsigned long long ci) -> int {
            const unsigned long long at0 = ci * chunk;
            const uint32_t nn = (uint32_t)std::min<unsigned long long>(chunk, body - at0);
            const size_t tiles = ((size_t)nn + tile - 1) / tile;
            {
                LaunchScope ls(c, "k_sam_write", (double)nn);
                hipLaunchKernelGGL(k_sam_write, dim3((unsigned)std::min<size_t>(tiles, (size_t)c->n_cu * 32)), dim3(MIRGE_BLOCK), 0, c->stream, t,
                                   (const uint32_t*)d_rows, (uint32_t)n_rows, (const uint32_t*)d_fixed, (const unsigned long long*)d_off, at0, nn,
                                   (uint32_t)tile, d_text[ci & 1]);
            }
            HIPOK(hipMemcpyAsync(pipe.half(ci), d_text[ci & 1], nn, hipMemcpyDeviceToHost, c->stream));
            return 0;
        };
        auto take = [&](unsigned long long ci) -> int {  // chunk ci is in its half: write it at its place
            const unsigned long long at0 = ci * chunk;
            return out.put(pipe.half(ci), (size_t)std::min<unsigned long long>(chunk, body - at0), (unsigned long long)header_len + at0);
        };
        CHECK(pipe.run((body + chunk - 1) / chunk, queue, take));
    }
    hc.lap("formatted + written");
    CHECK(out.commit());  // (every chunk has been taken: nothing of the file is still on its way)
    if (n_lines_out) *n_lines_out = (int64_t)lines;
    if (n_bytes_out) *n_bytes_out = (int64_t)body;
    return 0;
}

extern "C" int mirge_sam_write_device(mirge_ctx* c, const mirge_reads* U, const mirge_result* res, const int64_t* order, int32_t sample,
                                      const int32_t* class_pass, int32_t n_class, const mirge_sam_pass* passes, int32_t n_pass,
                                      const char* path, const char* header, int64_t header_len, int64_t* n_lines_out,
                                      int64_t* n_bytes_out) {
    return sam_write_impl("mirge_sam_write_device", c, U, res, order, sample, class_pass, n_class, passes, n_pass, path, header, header_len, n_lines_out,
                          n_bytes_out, nullptr, 0, nullptr);
}
// `path` is `<sample>.sam.gz`, gzi_path its block index; block_bytes <= 0: MIRGE_BGZF_BLOCK_BYTES; stats_out[8]: BgzfStream::stats
extern "C" int mirge_sam_write_device_bgzf(mirge_ctx* c, const mirge_reads* U, const mirge_result* res, const int64_t* order, int32_t sample,
                                           const int32_t* class_pass, int32_t n_class, const mirge_sam_pass* passes, int32_t n_pass,
                                           const char* path, const char* header, int64_t header_len, int64_t* n_lines_out,
                                           int64_t* n_bytes_out, const char* gzi_path, int64_t block_bytes, int64_t* stats_out) {
    if (!gzi_path) return fail(-1, "mirge_sam_write_device_bgzf: bad argument");
    return sam_write_impl("mirge_sam_write_device_bgzf", c, U, res, order, sample, class_pass, n_class, passes, n_pass, path, header, header_len,
                          n_lines_out, n_bytes_out, gzi_path, block_bytes, stats_out);
}
