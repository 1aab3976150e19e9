// native_bw.hpp -- part of mirge_native.hip (one translation unit, behind native_cov.hpp): `<sample>.bw` of `--coverage-bigwig`
// (kernels_bw.hpp; the format: mirge3_amd/bigwig.py).  BwJob takes the resident runs of CovDev::runs as they are and writes one file per
// strand: the run range of every (strand, rank), the zoom levels' counts (which decide how many levels the header names), then the
// sections and every kept level's blocks, group by group through StagePipe (native_stage.hpp), and last the indexes and the
// front of the file from the sizes and bounds copied back (bw_layout.hpp).  MIRGE_BW_SECTION_ITEMS / MIRGE_BW_ZOOM_BASE /
// MIRGE_BW_DEFLATE / MIRGE_BW_CHUNK_BYTES are read per call.  Both exports write to `<path>.tmp` (OutFile) and rename when every file is whole.
// The job's blocks are the calling export's (PoolScope); the job stands in front of that scope, for copies from the device fill its words.
#pragma once
#include "bw_layout.hpp"

struct BwJob {
    mirge_ctx* c;
    PoolScope* scope = nullptr;  // write()'s
    std::string who;
    CovDev& dev;
    uint32_t n_rank = 0, S = MIRGE_BW_MAX_SECTION, base = 64;
    int deflate = 1;
    size_t chunk = (size_t)32 << 20;
    std::vector<std::string> keys;        // names by chromId
    std::vector<uint32_t> size_by_cid, rank_of_cid, h_cid, h_ln, first;
    uint32_t *d_ln = nullptr, *d_cid = nullptr, *d_first = nullptr, *d_err = nullptr, *d_sizes = nullptr, *d_off = nullptr, *d_bounds = nullptr;
    uint32_t *d_rec_run = nullptr, *d_rec_bin = nullptr;
    unsigned long long *d_max = nullptr, *d_cnt = nullptr, *d_cnt_off = nullptr, *d_pick = nullptr;
    BwBlk* d_blk = nullptr;
    BwPart* d_part = nullptr;
    uint8_t *d_slots = nullptr, *d_out[2] = {nullptr, nullptr};
    std::vector<BwRec*> d_recs;
    unsigned long long max_depth[2] = {0, 0}, n_k = 0;  // (with herr, pick and part: what copies from the device fill)
    uint32_t herr = MIRGE_BW_NONE;
    std::vector<unsigned long long> pick;
    std::vector<BwPart> part;
    OutFile out[2];  // the strands' files, written as `<path>.tmp`: both are renamed, or neither stays (commit_all)

    BwJob(mirge_ctx* c_, const std::string& w, CovDev& d) : c(c_), who(w), dev(d), out{{w, true}, {w, true}} {}

    int env() {
        const size_t s = env_bytes("MIRGE_BW_SECTION_ITEMS", MIRGE_BW_MAX_SECTION), b = env_bytes("MIRGE_BW_ZOOM_BASE", 64);
        if (s < 1 || s > MIRGE_BW_MAX_SECTION) return fail(-1, who + ": MIRGE_BW_SECTION_ITEMS takes 1 to 1024");
        if (b < 1 || b > MIRGE_BW_MAX_REDUCTION) return fail(-1, who + ": MIRGE_BW_ZOOM_BASE takes 1 to 2^20");
        S = (uint32_t)s; base = (uint32_t)b;
        const char* m = std::getenv("MIRGE_BW_DEFLATE");
        if (m && *m && std::strcmp(m, "device") != 0 && std::strcmp(m, "none") != 0) return fail(-1, who + ": MIRGE_BW_DEFLATE takes device or none");
        deflate = (m && std::strcmp(m, "none") == 0) ? 0 : 1;
        chunk = std::min<size_t>((size_t)1 << 30, std::max<size_t>(env_bytes("MIRGE_BW_CHUNK_BYTES", (size_t)32 << 20), 64));
        return 0;
    }
    // names (rank order), sizes and byte-order ids as the caller gives them: ids must be the ranks of the names sorted by bytes
    int chromosomes(int32_t n, const char* name_data, const int64_t* name_off, const int64_t* ln, const int32_t* cid) {
        if (n < 1 || n > (1 << 24) || !name_data || !name_off || !ln || !cid) return fail(-1, who + ": 1 to 2^24 chromosomes with names, sizes and ids");
        n_rank = (uint32_t)n;
        keys.assign(n_rank, std::string()); size_by_cid.assign(n_rank, 0); rank_of_cid.assign(n_rank, MIRGE_BW_NONE);
        h_cid.resize(n_rank); h_ln.resize(n_rank);
        for (uint32_t r = 0; r < n_rank; r++) {
            if (name_off[r + 1] < name_off[r] || ln[r] < 0 || ln[r] > 0xFFFFFFFFll) return fail(-1, who + ": a chromosome size beyond 2^32 - 1, or malformed names");
            if (cid[r] < 0 || (uint32_t)cid[r] >= n_rank || rank_of_cid[cid[r]] != MIRGE_BW_NONE) return fail(-1, who + ": the chromosome ids are no permutation");
            rank_of_cid[cid[r]] = r;
            keys[cid[r]].assign(name_data + name_off[r], name_data + name_off[r + 1]);
            size_by_cid[cid[r]] = (uint32_t)ln[r];
            h_cid[r] = (uint32_t)cid[r]; h_ln[r] = (uint32_t)ln[r];
        }
        for (uint32_t k = 0; k + 1 < n_rank; k++)  // (memcmp order, a shorter name first: what the B+ tree is searched by)
            if (!(keys[k] < keys[k + 1])) return fail(-1, who + ": the chromosome ids do not follow the byte order of the names (or a name twice)");
        return 0;
    }
    int scan64(size_t n) {  // d_cnt[0 .. n] -> d_cnt_off
        size_t tb = 0;
        HIPOK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, d_cnt, d_cnt_off, (int)(n + 1), c->stream));
        CHECK(dev.need_tmp(*scope, tb));
        HIPOK(hipcub::DeviceScan::ExclusiveSum(dev.tmp, tb, d_cnt, d_cnt_off, (int)(n + 1), c->stream));
        return 0;
    }
    // the blocks of `blk` (sections of the runs, or records of `recs`) to the file from `pos` on; placed / pos / largest are updated
    int stream(OutFile& file, bool records, const BwRec* recs, const std::vector<BwBlk>& blk, uint64_t& pos, std::vector<BwPlaced>& placed, uint32_t& largest) {
        const size_t nb = blk.size();
        if (nb == 0) return 0;
        const uint32_t payload = records ? S * 32u : 24u + S * 12u, stride = (payload + 11u + 15u) & ~15u;
        const size_t G = std::min(nb, std::max<size_t>(1, chunk / stride)), buf = G * stride;
        scope->give(d_blk); scope->give(d_slots); scope->give(d_out[0]); scope->give(d_out[1]);  // (the stretch before this one's)
        scope->give(d_sizes); scope->give(d_off); scope->give(d_bounds);
        CHECK(scope->get(&d_blk, nb)); CHECK(scope->get(&d_slots, buf)); CHECK(scope->get(&d_out[0], buf)); CHECK(scope->get(&d_out[1], buf));
        CHECK(scope->get(&d_sizes, G + 1)); CHECK(scope->get(&d_off, G + 1)); CHECK(scope->get(&d_bounds, 3 * G));
        std::vector<uint32_t> h_sizes(G), h_bounds(3 * G);  // (in front of the pipe: it waits for the stream on its way out)
        StagePipe pipe(c, who, "the copy of a group of blocks failed");
        CHECK(pipe.ensure(buf));
        HIPOK(hipMemcpyAsync(d_blk, blk.data(), nb * sizeof(BwBlk), hipMemcpyHostToDevice, c->stream));
        size_t tb = 0;
        HIPOK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, d_sizes, d_off, (int)(G + 1), c->stream));
        CHECK(dev.need_tmp(*scope, tb));
        uint64_t at[2] = {0, 0};
        size_t bytes[2] = {0, 0};
        auto take = [&](unsigned long long g) -> int { return file.put(pipe.half(g), bytes[g & 1], at[g & 1]); };  // group g is in its half
        auto queue = [&](unsigned long long g) -> int {
            const size_t g0 = g * G, ng = std::min(G, nb - g0);
            HIPOK(hipMemsetAsync(d_sizes + ng, 0, 4, c->stream));
            {
                LaunchScope ls(c, records ? "k_bw_blocks<records>" : "k_bw_blocks<sections>", (double)ng);
                const dim3 grid((unsigned)std::min<size_t>(ng, (size_t)c->n_cu * 8)), block(MIRGE_BLOCK);
                if (records)
                    hipLaunchKernelGGL((k_bw_blocks<true>), grid, block, 0, c->stream, dev.r, recs, (const BwBlk*)(d_blk + g0), (uint32_t)ng, deflate, stride, d_slots, d_sizes, d_bounds);
                else
                    hipLaunchKernelGGL((k_bw_blocks<false>), grid, block, 0, c->stream, dev.r, recs, (const BwBlk*)(d_blk + g0), (uint32_t)ng, deflate, stride, d_slots, d_sizes, d_bounds);
            }
            HIPOK(hipcub::DeviceScan::ExclusiveSum(dev.tmp, tb, d_sizes, d_off, (int)(ng + 1), c->stream));
            {
                LaunchScope ls(c, "k_bam_compact", (double)ng);
                hipLaunchKernelGGL(k_bam_compact, dim3((unsigned)std::min<size_t>(ng, (size_t)c->n_cu * 8)), dim3(MIRGE_BLOCK), 0, c->stream, (const uint8_t*)d_slots, stride,
                                   (const uint32_t*)d_sizes, (const uint32_t*)d_off, (uint32_t)ng, d_out[g & 1]);
            }
            HIPOK(hipMemcpyAsync(h_sizes.data(), d_sizes, ng * 4, hipMemcpyDeviceToHost, c->stream));
            HIPOK(hipMemcpyAsync(h_bounds.data(), d_bounds, ng * 12, hipMemcpyDeviceToHost, c->stream));
            HIPOK(hipStreamSynchronize(c->stream));
            HIPOK(hipGetLastError());
            size_t total = 0;
            for (size_t b = 0; b < ng; b++) {
                if (h_sizes[b] == 0 || h_sizes[b] > stride) return fail(-3, who + ": a block of impossible size");
                placed.push_back(BwPlaced{h_bounds[3 * b], h_bounds[3 * b + 1], h_bounds[3 * b + 2], pos + total, h_sizes[b]});
                total += h_sizes[b];
                largest = std::max(largest, records ? blk[g0 + b].count * 32u : 24u + blk[g0 + b].count * 12u);
            }
            at[g & 1] = pos; bytes[g & 1] = total;
            pos += total;
            HIPOK(hipMemcpyAsync(pipe.half(g), d_out[g & 1], total, hipMemcpyDeviceToHost, c->stream));
            return 0;
        };
        return pipe.run((nb + G - 1) / G, queue, take);
    }
    // blocks of up to S of [lo, hi) on chromId cidx
    void cut(std::vector<BwBlk>& blk, uint64_t lo, uint64_t hi, uint32_t cidx) const {
        for (uint64_t a = lo; a < hi; a += S) blk.push_back(BwBlk{(uint32_t)a, (uint32_t)std::min<uint64_t>(S, hi - a), cidx});
    }
    // file f (strand f of a stranded run) to `path`; stats[0..15] = sections, items, levels, bytes, largest depth, records per level
    int one_file(int f, const char* path, int64_t* stats) {
        OutFile& file = out[f];
        CHECK(file.open(path));
        const uint32_t* fr = first.data() + (size_t)f * n_rank;
        const uint32_t r0 = dev.n_runs ? fr[0] : 0, r1 = dev.n_runs ? fr[n_rank] : 0, n = r1 - r0;
        std::vector<BwBlk> secs;
        for (uint32_t k = 0; k < n_rank && n; k++) cut(secs, fr[rank_of_cid[k]], fr[rank_of_cid[k] + 1], k);
        // ---- the zoom levels: counts first (they decide what is kept), then the records of the kept ones
        std::vector<BwZoomHead> zoom;
        std::vector<std::vector<BwBlk>> zblk;
        std::vector<uint64_t> zcount;
        for (auto p : d_recs) scope->give(p);
        d_recs.clear();
        unsigned long long prev = n;
        pick.assign((size_t)n_rank + 1, 0);
        for (int k = 0; k < MIRGE_BW_MAX_LEVELS && n; k++) {
            const unsigned long long R64 = (unsigned long long)base << (2 * k);
            if (R64 > MIRGE_BW_MAX_REDUCTION) break;
            const uint32_t R = (uint32_t)R64;
            HIPOK(hipMemsetAsync(d_cnt + n, 0, 8, c->stream));
            { LaunchScope ls(c, "k_bw_zoom_count", (double)n);
              hipLaunchKernelGGL(k_bw_zoom_count, dim3(grid_for(c, n)), dim3(MIRGE_BLOCK), 0, c->stream, dev.r, r0, r1, R, d_cnt); }
            CHECK(scan64(n));
            n_k = 0;
            HIPOK(hipMemcpyAsync(&n_k, d_cnt_off + n, 8, hipMemcpyDeviceToHost, c->stream));
            HIPOK(hipStreamSynchronize(c->stream));
            if (2 * n_k > prev) break;
            BwRec* recs;
            scope->give(d_rec_run); scope->give(d_rec_bin);
            CHECK(scope->get(&d_rec_run, (size_t)n_k)); CHECK(scope->get(&d_rec_bin, (size_t)n_k)); CHECK(scope->get(&recs, (size_t)n_k));
            d_recs.push_back(recs);
            { LaunchScope ls(c, "k_bw_zoom_bins", (double)n);
              hipLaunchKernelGGL(k_bw_zoom_bins, dim3(grid_for(c, n)), dim3(MIRGE_BLOCK), 0, c->stream, dev.r, r0, r1, R, (const unsigned long long*)d_cnt_off, d_rec_run, d_rec_bin); }
            { LaunchScope ls(c, "k_bw_zoom_reduce", (double)n_k);
              hipLaunchKernelGGL(k_bw_zoom_reduce, dim3(grid_for(c, (size_t)n_k)), dim3(MIRGE_BLOCK), 0, c->stream, dev.r, r1, (const uint32_t*)d_rec_run, (const uint32_t*)d_rec_bin,
                                 (uint32_t)n_k, R, (const uint32_t*)d_ln, (const uint32_t*)d_cid, recs); }
            { LaunchScope ls(c, "k_bw_pick", (double)n_rank);
              hipLaunchKernelGGL(k_bw_pick, dim3(grid_for(c, (size_t)n_rank + 1)), dim3(MIRGE_BLOCK), 0, c->stream, (const unsigned long long*)d_cnt_off,
                                 (const uint32_t*)(d_first + (size_t)f * n_rank), n_rank + 1u, r0, d_pick); }
            HIPOK(hipMemcpyAsync(pick.data(), d_pick, ((size_t)n_rank + 1) * 8, hipMemcpyDeviceToHost, c->stream));
            HIPOK(hipStreamSynchronize(c->stream));
            zblk.emplace_back();
            for (uint32_t cx = 0; cx < n_rank; cx++) cut(zblk.back(), pick[rank_of_cid[cx]], pick[rank_of_cid[cx] + 1], cx);
            zoom.push_back(BwZoomHead{R, 0, 0});
            zcount.push_back(n_k);
            prev = n_k;
        }
        // ---- the total summary: the sections' partials in section order
        BwTotals tot;
        if (!secs.empty()) {
            scope->give(d_blk); scope->give(d_part);
            CHECK(scope->get(&d_blk, secs.size())); CHECK(scope->get(&d_part, secs.size()));
            part.assign(secs.size(), BwPart{});
            HIPOK(hipMemcpyAsync(d_blk, secs.data(), secs.size() * sizeof(BwBlk), hipMemcpyHostToDevice, c->stream));
            { LaunchScope ls(c, "k_bw_summary", (double)secs.size());
              hipLaunchKernelGGL(k_bw_summary, dim3(grid_for(c, secs.size())), dim3(MIRGE_BLOCK), 0, c->stream, dev.r, (const BwBlk*)d_blk, (uint32_t)secs.size(), d_part); }
            HIPOK(hipMemcpyAsync(part.data(), d_part, secs.size() * sizeof(BwPart), hipMemcpyDeviceToHost, c->stream));
            HIPOK(hipStreamSynchronize(c->stream));
            tot.vmin = part[0].vmin; tot.vmax = part[0].vmax;
            for (const BwPart& p : part) {
                tot.bases += p.bases; tot.vmin = std::min(tot.vmin, p.vmin); tot.vmax = std::max(tot.vmax, p.vmax);
                tot.sum = bw_add(tot.sum, p.sum); tot.sq = bw_add(tot.sq, p.sq);
            }
        }
        // ---- data, index, zoom levels, magic, and last the front
        const uint64_t data_at = bw_front_bytes(keys, zoom.size());
        uint64_t pos = data_at + 8;
        uint32_t largest = 0;
        std::vector<BwPlaced> placed;
        CHECK(stream(file, false, nullptr, secs, pos, placed, largest));
        BwBytes o;
        o.u64(secs.size());
        CHECK(file.put(o.b.data(), 8, data_at));
        const uint64_t index_at = pos;
        o.b.clear();
        bw_rtree(placed, index_at, index_at, o);
        CHECK(file.put(o.b.data(), o.b.size(), pos));
        pos += o.b.size();
        for (size_t k = 0; k < zoom.size(); k++) {
            zoom[k].data_at = pos;
            o.b.clear(); o.u32((uint32_t)zcount[k]);
            CHECK(file.put(o.b.data(), 4, pos));
            pos += 4;
            placed.clear();
            CHECK(stream(file, true, d_recs[k], zblk[k], pos, placed, largest));
            zoom[k].index_at = pos;
            o.b.clear();
            bw_rtree(placed, pos, pos, o);
            CHECK(file.put(o.b.data(), o.b.size(), pos));
            pos += o.b.size();
        }
        o.b.clear(); o.u32(MIRGE_BW_MAGIC);
        CHECK(file.put(o.b.data(), 4, pos));
        pos += 4;
        o.b.clear();
        bw_front(keys, size_by_cid, zoom, index_at, tot, deflate ? largest : 0u, o);
        if (o.b.size() != data_at) return fail(-3, who + ": the front of the file is not the size it was planned with");
        CHECK(file.put(o.b.data(), o.b.size(), 0));
        if (stats) {
            stats[0] = (int64_t)secs.size(); stats[1] = (int64_t)n; stats[2] = (int64_t)zoom.size(); stats[3] = (int64_t)pos; stats[4] = (int64_t)max_depth[f];
            for (size_t k = 0; k < zoom.size(); k++) stats[5 + k] = (int64_t)zcount[k];
        }
        return 0;
    }
    // the runs of dev -> paths[0] (and paths[1] when stranded); err_out = {3, rank, end, LN} for a run beyond its chromosome
    int write(PoolScope& sc, bool stranded, const char* const* paths, int64_t* stats, int64_t* err_out) {
        scope = &sc;
        const uint32_t n_str = stranded ? 2u : 1u, n_runs = (uint32_t)dev.n_runs;
        const size_t nq = (size_t)n_str * n_rank + 1;
        first.assign(nq, 0);
        CHECK(sc.get(&d_ln, (size_t)n_rank)); CHECK(sc.get(&d_cid, (size_t)n_rank)); CHECK(sc.get(&d_first, nq));
        CHECK(sc.get(&d_err, (size_t)1)); CHECK(sc.get(&d_max, (size_t)2)); CHECK(sc.get(&d_pick, (size_t)n_rank + 1));
        CHECK(sc.get(&d_cnt, (size_t)n_runs + 1)); CHECK(sc.get(&d_cnt_off, (size_t)n_runs + 1));
        if (n_runs) {
            herr = MIRGE_BW_NONE;
            HIPOK(hipMemcpyAsync(d_ln, h_ln.data(), (size_t)n_rank * 4, hipMemcpyHostToDevice, c->stream));
            HIPOK(hipMemcpyAsync(d_cid, h_cid.data(), (size_t)n_rank * 4, hipMemcpyHostToDevice, c->stream));
            HIPOK(hipMemsetAsync(d_err, 0xFF, 4, c->stream));
            HIPOK(hipMemsetAsync(d_max, 0, 16, c->stream));
            { LaunchScope ls(c, "k_bw_limits", (double)n_runs);
              hipLaunchKernelGGL(k_bw_limits, dim3(grid_for(c, n_runs)), dim3(MIRGE_BLOCK), 0, c->stream, dev.r, n_runs, (const uint32_t*)d_ln, d_err, d_max); }
            { LaunchScope ls(c, "k_bw_ranges", (double)nq);
              hipLaunchKernelGGL(k_bw_ranges, dim3(grid_for(c, nq)), dim3(MIRGE_BLOCK), 0, c->stream, dev.r, n_runs, n_rank, n_str, d_first); }
            HIPOK(hipMemcpyAsync(&herr, d_err, 4, hipMemcpyDeviceToHost, c->stream));
            HIPOK(hipMemcpyAsync(max_depth, d_max, 16, hipMemcpyDeviceToHost, c->stream));
            HIPOK(hipMemcpyAsync(first.data(), d_first, nq * 4, hipMemcpyDeviceToHost, c->stream));
            HIPOK(hipStreamSynchronize(c->stream));
            HIPOK(hipGetLastError());
            if (herr != MIRGE_BW_NONE) {
                int32_t ch = 0;
                long long end = 0;
                HIPOK(hipMemcpy(&ch, dev.r.chrom + herr, 4, hipMemcpyDeviceToHost));
                HIPOK(hipMemcpy(&end, dev.r.end + herr, 8, hipMemcpyDeviceToHost));
                if (err_out) { err_out[0] = 3; err_out[1] = ch; err_out[2] = end; err_out[3] = h_ln[ch]; }
                return fail(-1, who + ": a run on '" + keys[h_cid[ch]] + "' ends at " + std::to_string(end) + ", beyond its LN " + std::to_string(h_ln[ch]));
            }
        }
        for (uint32_t f = 0; f < n_str; f++) {
            const int rc = one_file((int)f, paths[f], stats ? stats + 16 * f : nullptr);
            (void)hipStreamSynchronize(c->stream);
            if (rc) return rc;
        }
        return commit_all({&out[0], &out[1]});  // (renamed only now that every file is whole)
    }
};

extern "C" int mirge_bigwig_from_intervals(mirge_ctx* c, int64_t n, const int32_t* chrom_rank, const int64_t* start, const int32_t* len, const uint32_t* weight,
                                           const uint8_t* minus, int32_t stranded, int32_t n_rank, const char* rank_names, const int64_t* rank_name_off,
                                           const int64_t* chrom_size, const int32_t* chrom_id, const char* path, const char* path_minus,
                                           int64_t* stats_out, int64_t* err_out) {
    const std::string who = "mirge_bigwig_from_intervals";
    if (!c || n < 0 || !path || (stranded && !path_minus) || (n && (!chrom_rank || !start || !len || !weight || !minus))) return fail(-1, who + ": bad argument");
    if (err_out) for (int k = 0; k < 4; k++) err_out[k] = 0;
    if (stats_out) for (int k = 0; k < 32; k++) stats_out[k] = 0;
    if (2 * (unsigned long long)n >= 0x7FFFFFF0ull) return fail(-5, who + ": too many intervals for one call (two events each must fit 32-bit indices)");
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    const size_t sn = (size_t)n;
    CovUpload up;
    CovDev dev;
    BwJob job(c, who, dev);
    const char* paths[2] = {path, stranded ? path_minus : nullptr};
    PoolScope scope(c);
    CHECK(job.env());
    CHECK(job.chromosomes(n_rank, rank_names, rank_name_off, chrom_size, chrom_id));
    for (size_t i = 0; i < sn; i++) if (chrom_rank[i] >= n_rank) return fail(-1, who + ": a chromosome rank beyond the names given");
    CHECK(up.upload(scope, sn, chrom_rank, start, len, weight, minus));
    CHECK(dev.runs(scope, who, up.intervals(), sn, (uint32_t)n_rank, stranded != 0));
    return job.write(scope, stranded != 0, paths, stats_out, err_out);
}

extern "C" int mirge_bigwig_write_device(mirge_ctx* c, const mirge_reads* U, const mirge_result* res, const int64_t* order, int32_t sample,
                                         const int32_t* class_pass, int32_t n_class, const mirge_sam_pass* passes, int32_t n_pass,
                                         const int32_t* chrom_rank, const int64_t* chrom_rank_off, int32_t n_rank, const char* rank_names,
                                         const int64_t* rank_name_off, const int64_t* chrom_size, const int32_t* chrom_id, int32_t stranded,
                                         const char* path, const char* path_minus, int64_t* stats_out, int64_t* err_out) {
    const std::string who = "mirge_bigwig_write_device";
    if (!c || !path || (stranded && !path_minus) || !chrom_rank || !chrom_rank_off || n_pass < 1 || n_pass > MIRGE_MAX_PASSES || !passes)
        return fail(-1, who + ": bad argument");
    if (err_out) for (int k = 0; k < 4; k++) err_out[k] = 0;
    if (stats_out) for (int k = 0; k < 32; k++) stats_out[k] = 0;
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    HostClock hc("bigwig_write_device");
    CovInput in;
    CovDev dev;
    BwJob job(c, who, dev);
    const char* paths[2] = {path, stranded ? path_minus : nullptr};
    PoolScope scope(c);
    CHECK(job.env());
    CHECK(job.chromosomes(n_rank, rank_names, rank_name_off, chrom_size, chrom_id));
    CHECK(in.build(scope, who, U, res, order, sample, class_pass, n_class, passes, n_pass, chrom_rank, chrom_rank_off, n_rank, err_out, hc));
    CHECK(dev.runs(scope, who, in.intervals(), in.n_rows, (uint32_t)n_rank, stranded != 0));
    hc.lap("runs");
    CHECK(job.write(scope, stranded != 0, paths, stats_out, err_out));
    hc.lap("files written");
    return 0;
}
