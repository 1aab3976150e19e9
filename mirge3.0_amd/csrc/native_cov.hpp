// native_cov.hpp -- part of mirge_native.hip (one translation unit): `<sample>.bedgraph` of `--coverage` (kernels_cov.hpp).  CovDev is
// everything behind the interval list -- events, radix sort, inclusive sum, three compactions, the runs, their text -- and serves both
// exports: mirge_coverage_runs (intervals from the host, runs back to the host: tests and other callers) and
// mirge_coverage_write_device (intervals from the resident run through SamPrep, the rows of `--sam-out`; text to one or two files, chunk
// by chunk through StagePipe, native_stage.hpp).  CovUpload: the host's intervals on the device.  Their blocks are the calling export's
// (its PoolScope); a CovDev stands in front of that scope, for copies from the device fill its words.  MIRGE_COV_CHUNK_BYTES / MIRGE_COV_TILE_BYTES (read per call): the chunk
// and the workgroup's tile; tests make them small so that their boundaries fall inside numbers and names.
#pragma once

struct CovDev {
    unsigned long long *kA = nullptr, *kB = nullptr, *d_sum = nullptr, *d_bytes = nullptr, *d_off = nullptr;
    long long *vA = nullptr, *vB = nullptr;
    uint32_t *flag = nullptr, *pos = nullptr, *words = nullptr, *d_name_off = nullptr;
    uint8_t* d_name_data = nullptr;
    void* tmp = nullptr;
    size_t tmp_bytes = 0;
    CovRuns r{nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t n_runs = 0, n_plus = 0;
    unsigned long long weight = 0, body = 0, split = 0;  // split: the bytes of the plus strand's lines
    uint32_t n1 = 0, n2 = 0, n3 = 0, hw[4] = {0, 0, 0, 0};  // runs(): counts and flag words that copies from the device fill

    int need_tmp(PoolScope& scope, size_t bytes) {
        if (bytes <= tmp_bytes) return 0;
        scope.give(tmp); tmp_bytes = 0;
        CHECK(scope.get((uint8_t**)&tmp, bytes));
        tmp_bytes = bytes;
        return 0;
    }
    // flag[0 .. m) is queued: pos = its exclusive sum, *count = the flags set (synchronises the stream)
    int count_flags(PoolScope& scope, size_t m, uint32_t* count) {
        mirge_ctx* const c = scope.c;
        size_t tb = 0;
        HIPOK(hipMemsetAsync(flag + m, 0, 4, c->stream));
        HIPOK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, flag, pos, (int)(m + 1), c->stream));
        CHECK(need_tmp(scope, tb));
        HIPOK(hipcub::DeviceScan::ExclusiveSum(tmp, tb, flag, pos, (int)(m + 1), c->stream));
        HIPOK(hipMemcpyAsync(count, pos + m, 4, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipStreamSynchronize(c->stream));
        return 0;
    }
    // the runs of n intervals (device arrays) over n_rank chromosome ranks, in file order
    int runs(PoolScope& scope, const std::string& who, const CovIntervals& iv, size_t n, uint32_t n_rank, bool stranded) {
        mirge_ctx* const c = scope.c;
        n_runs = n_plus = 0; weight = 0;
        if (n == 0) return 0;
        if (2 * (unsigned long long)n >= 0x7FFFFFF0ull) return fail(-5, who + ": too many intervals for one call (two events each must fit 32-bit indices)");
        if (n_rank < 1 || n_rank > (1u << 24)) return fail(-1, who + ": 1 to 2^24 chromosome ranks");
        int rbits = 0;
        while ((1ull << rbits) < (unsigned long long)n_rank) rbits++;
        const int strand_shift = MIRGE_COV_POS_BITS + rbits, end_bit = strand_shift + (stranded ? 1 : 0);
        const size_t m = 2 * n;
        CHECK(scope.get(&kA, m)); CHECK(scope.get(&kB, m)); CHECK(scope.get(&vA, m)); CHECK(scope.get(&vB, m));
        CHECK(scope.get(&flag, m + 1)); CHECK(scope.get(&pos, m + 1)); CHECK(scope.get(&words, (size_t)4)); CHECK(scope.get(&d_sum, (size_t)1));
        HIPOK(hipMemsetAsync(words, 0, 16, c->stream));
        HIPOK(hipMemsetAsync(d_sum, 0, 8, c->stream));
        size_t tb_sort = 0, tb_sum = 0;
        HIPOK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb_sort, kA, kB, vA, vB, (int)m, 0, end_bit, c->stream));
        HIPOK(hipcub::DeviceScan::InclusiveSum(nullptr, tb_sum, vB, vA, (int)m, c->stream));
        CHECK(need_tmp(scope, std::max(tb_sort, tb_sum)));
        const dim3 block(MIRGE_BLOCK);
        { LaunchScope ls(c, "k_cov_events", (double)n);
          hipLaunchKernelGGL(k_cov_events, dim3(grid_for(c, n)), block, 0, c->stream, iv, (uint32_t)n, n_rank, stranded ? 1 : 0, strand_shift, kA, vA, words, d_sum); }
        HIPOK(hipcub::DeviceRadixSort::SortPairs(tmp, tb_sort, kA, kB, vA, vB, (int)m, 0, end_bit, c->stream));
        HIPOK(hipcub::DeviceScan::InclusiveSum(tmp, tb_sum, vB, vA, (int)m, c->stream));
        // ---- the last event of every key with its sum: (kB, vA) -> (kA, vB)
        n1 = n2 = n3 = 0; hw[0] = hw[1] = hw[2] = hw[3] = 0;
        { LaunchScope ls(c, "k_cov_last", (double)m);
          hipLaunchKernelGGL(k_cov_last, dim3(grid_for(c, m)), block, 0, c->stream, (const unsigned long long*)kB, (uint32_t)m, flag); }
        HIPOK(hipMemcpyAsync(hw, words, 16, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipMemcpyAsync(&weight, d_sum, 8, hipMemcpyDeviceToHost, c->stream));
        CHECK(count_flags(scope, m, &n1));
        if (hw[0] & 1u)
            return fail(-1, who + ": an interval outside the contract (rank in [0, ranks), start >= 0, length >= 1, weight >= 1, end <= 2^31 - 1)");
        { LaunchScope ls(c, "k_cov_scatter", (double)m);
          hipLaunchKernelGGL(k_cov_scatter, dim3(grid_for(c, m)), block, 0, c->stream, (const unsigned long long*)kB, (const long long*)vA,
                             (const uint32_t*)flag, (const uint32_t*)pos, (uint32_t)m, kA, vB); }
        // ---- of those, the entries where the sum changes: (kA, vB) -> (kB, vA)
        { LaunchScope ls(c, "k_cov_change", (double)n1);
          hipLaunchKernelGGL(k_cov_change, dim3(grid_for(c, n1)), block, 0, c->stream, (const long long*)vB, n1, flag); }
        CHECK(count_flags(scope, n1, &n2));
        { LaunchScope ls(c, "k_cov_scatter", (double)n1);
          hipLaunchKernelGGL(k_cov_scatter, dim3(grid_for(c, n1)), block, 0, c->stream, (const unsigned long long*)kA, (const long long*)vB,
                             (const uint32_t*)flag, (const uint32_t*)pos, n1, kB, vA); }
        // ---- of those, the entries with a sum: the runs
        if (n2 == 0) return 0;
        { LaunchScope ls(c, "k_cov_nonzero", (double)n2);
          hipLaunchKernelGGL(k_cov_nonzero, dim3(grid_for(c, n2)), block, 0, c->stream, (const long long*)vA, n2, flag, words); }
        HIPOK(hipMemcpyAsync(hw, words, 16, hipMemcpyDeviceToHost, c->stream));
        CHECK(count_flags(scope, n2, &n3));
        if (hw[0] & 2u) return fail(-3, who + ": the depth fell below 0 or did not return to 0");
        CHECK(scope.get(&r.strand, std::max<size_t>(n3, 1))); CHECK(scope.get(&r.chrom, std::max<size_t>(n3, 1)));
        CHECK(scope.get(&r.start, std::max<size_t>(n3, 1))); CHECK(scope.get(&r.end, std::max<size_t>(n3, 1)));
        CHECK(scope.get(&r.depth, std::max<size_t>(n3, 1)));
        { LaunchScope ls(c, "k_cov_runs", (double)n2);
          hipLaunchKernelGGL(k_cov_runs, dim3(grid_for(c, n2)), block, 0, c->stream, (const unsigned long long*)kB, (const long long*)vA,
                             (const uint32_t*)flag, (const uint32_t*)pos, n2, strand_shift, r, words + 1); }
        HIPOK(hipMemcpyAsync(hw, words, 16, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipStreamSynchronize(c->stream));
        HIPOK(hipGetLastError());
        n_runs = n3; n_plus = hw[1];
        return 0;
    }
    // the lines' offsets: name_off[n_rank + 1] into name_data (host), the chromosome names in rank order
    int measure(PoolScope& scope, const char* name_data, const int64_t* name_off, uint32_t n_rank) {
        mirge_ctx* const c = scope.c;
        body = split = 0;
        if (n_runs == 0) return 0;
        std::vector<uint32_t> off32((size_t)n_rank + 1);
        for (uint32_t k = 0; k <= n_rank; k++) off32[k] = (uint32_t)(name_off[k] - name_off[0]);
        const size_t nb = off32[n_rank];
        CHECK(scope.get(&d_name_off, (size_t)n_rank + 1)); CHECK(scope.get(&d_name_data, std::max<size_t>(nb, 1)));
        CHECK(scope.get(&d_bytes, n_runs + 1)); CHECK(scope.get(&d_off, n_runs + 1));
        hipError_t e = hipMemcpyAsync(d_name_off, off32.data(), ((size_t)n_rank + 1) * 4, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess && nb) e = hipMemcpyAsync(d_name_data, name_data + name_off[0], nb, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(d_bytes + n_runs, 0, 8, c->stream);
        if (e == hipSuccess) {
            LaunchScope ls(c, "k_cov_measure", (double)n_runs);
            hipLaunchKernelGGL(k_cov_measure, dim3(grid_for(c, n_runs)), dim3(MIRGE_BLOCK), 0, c->stream, r, (uint32_t)n_runs, (const uint32_t*)d_name_off, d_bytes);
        }
        size_t tb = 0;
        if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(nullptr, tb, d_bytes, d_off, (int)(n_runs + 1), c->stream);
        int rc = 0;
        if (e == hipSuccess && (rc = need_tmp(scope, tb))) { (void)hipStreamSynchronize(c->stream); return rc; }
        if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(tmp, tb, d_bytes, d_off, (int)(n_runs + 1), c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&body, d_off + n_runs, 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&split, d_off + n_plus, 8, hipMemcpyDeviceToHost, c->stream);
        const hipError_t e2 = hipStreamSynchronize(c->stream);  // (also when a call failed: off32 leaves scope)
        if (e == hipSuccess) e = e2;
        if (e != hipSuccess) return fail(-2, std::string("coverage: ") + hipGetErrorString(e));
        return 0;
    }
};

// n intervals as the host gives them, on the device: what mirge_coverage_runs and mirge_bigwig_from_intervals hand to CovDev::runs
struct CovUpload {
    int32_t *d_rank = nullptr, *d_len = nullptr;
    long long* d_start = nullptr;
    uint32_t* d_w = nullptr;
    uint8_t* d_minus = nullptr;
    CovIntervals intervals() const { return CovIntervals{d_rank, d_start, d_len, d_w, d_minus}; }
    int upload(PoolScope& scope, size_t n, const int32_t* chrom_rank, const int64_t* start, const int32_t* len, const uint32_t* weight, const uint8_t* minus) {
        mirge_ctx* const c = scope.c;
        if (n == 0) return 0;
        CHECK(scope.get(&d_rank, n)); CHECK(scope.get(&d_len, n)); CHECK(scope.get(&d_start, n)); CHECK(scope.get(&d_w, n)); CHECK(scope.get(&d_minus, n));
        HIPOK(hipMemcpyAsync(d_rank, chrom_rank, n * 4, hipMemcpyHostToDevice, c->stream));
        HIPOK(hipMemcpyAsync(d_start, start, n * 8, hipMemcpyHostToDevice, c->stream));
        HIPOK(hipMemcpyAsync(d_len, len, n * 4, hipMemcpyHostToDevice, c->stream));
        HIPOK(hipMemcpyAsync(d_w, weight, n * 4, hipMemcpyHostToDevice, c->stream));
        HIPOK(hipMemcpyAsync(d_minus, minus, n, hipMemcpyHostToDevice, c->stream));
        return 0;
    }
};

extern "C" int mirge_coverage_runs(mirge_ctx* c, int64_t n, const int32_t* chrom_rank, const int64_t* start, const int32_t* len, const uint32_t* weight,
                                   const uint8_t* minus, int32_t stranded, uint8_t* run_strand, int32_t* run_chrom, int64_t* run_start,
                                   int64_t* run_end, int64_t* run_depth, int64_t* n_runs_out) {
    const std::string who = "mirge_coverage_runs";
    if (!c || n < 0 || !n_runs_out || (n && (!chrom_rank || !start || !len || !weight || !minus || !run_strand || !run_chrom || !run_start || !run_end || !run_depth)))
        return fail(-1, who + ": bad argument");
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    *n_runs_out = 0;
    if (n == 0) return 0;
    if (2 * (unsigned long long)n >= 0x7FFFFFF0ull) return fail(-5, who + ": too many intervals for one call (two events each must fit 32-bit indices)");
    int32_t top = 0;  // (the sort covers the rank bits that are used)
    for (int64_t i = 0; i < n; i++) top = std::max(top, chrom_rank[i]);
    if (top >= (1 << 24)) return fail(-1, who + ": a chromosome rank beyond 2^24");
    const size_t sn = (size_t)n;
    CovUpload up;
    CovDev dev;
    PoolScope scope(c);
    CHECK(up.upload(scope, sn, chrom_rank, start, len, weight, minus));
    CHECK(dev.runs(scope, who, up.intervals(), sn, (uint32_t)top + 1u, stranded != 0));
    if (dev.n_runs > 2 * sn) return fail(-3, who + ": more runs than events");
    if (dev.n_runs) {
        HIPOK(hipMemcpyAsync(run_strand, dev.r.strand, dev.n_runs, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipMemcpyAsync(run_chrom, dev.r.chrom, dev.n_runs * 4, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipMemcpyAsync(run_start, dev.r.start, dev.n_runs * 8, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipMemcpyAsync(run_end, dev.r.end, dev.n_runs * 8, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipMemcpyAsync(run_depth, dev.r.depth, dev.n_runs * 8, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipStreamSynchronize(c->stream));
    }
    *n_runs_out = (int64_t)dev.n_runs;
    return 0;
}

// the intervals of one sample's rows from the resident run (SamPrep, the rows of `--sam-out`): what mirge_coverage_write_device and
// mirge_bigwig_write_device hand to CovDev::runs.  A row on a chromosome without rank or outside [1, 2^31 - 1] fails the call, named.
struct CovInput {
    SamPrep prep;
    int32_t *d_map = nullptr, *d_rank = nullptr, *d_len = nullptr, *d_desc = nullptr;
    long long* d_start = nullptr;
    uint32_t *d_w = nullptr, *d_err = nullptr;
    uint8_t* d_minus = nullptr;
    size_t n_rows = 0;
    CovIntervals intervals() const { return CovIntervals{d_rank, d_start, d_len, d_w, d_minus}; }
    int build(PoolScope& scope, const std::string& who, const mirge_reads* U, const mirge_result* res, const int64_t* order, int32_t sample,
              const int32_t* class_pass, int32_t n_class, const mirge_sam_pass* passes, int32_t n_pass, const int32_t* chrom_rank,
              const int64_t* chrom_rank_off, int32_t n_rank, int64_t* err_out, HostClock& hc) {
        mirge_ctx* const c = scope.c;
        CHECK(prep.build(scope, who, U, res, order, sample, class_pass, n_class, passes, n_pass));
        n_rows = prep.n_rows;
        hc.lap("rows chosen");
        // ---- every named pass's chromosome index -> global rank
        CovRankMap rm;
        std::memset(&rm, 0, sizeof(rm));
        for (int p = 0; p < n_pass; p++) {
            const int64_t nn = chrom_rank_off[p + 1] - chrom_rank_off[p];
            bool named = false;
            for (int k = 0; k < n_class; k++) named = named || class_pass[k] == p;
            if (chrom_rank_off[p] < 0 || chrom_rank_off[p] >= 0x7FFFFFF0ll || nn < 0 || (named && nn != passes[p].n_chrom))
                return fail(-1, who + ": the rank table of pass " + std::to_string(p) + " does not fit its chromosomes");
            for (int64_t k = 0; k < nn; k++)
                if (chrom_rank[chrom_rank_off[p] + k] >= n_rank) return fail(-1, who + ": a chromosome rank beyond the names given");
            rm.rank_off[p] = (uint32_t)chrom_rank_off[p];
        }
        const size_t n_map = (size_t)chrom_rank_off[n_pass];
        CHECK(scope.get(&d_map, std::max<size_t>(n_map, 1))); CHECK(scope.get(&d_err, (size_t)2)); CHECK(scope.get(&d_desc, (size_t)4));
        const size_t cap = std::max<size_t>(n_rows, 1);
        CHECK(scope.get(&d_rank, cap)); CHECK(scope.get(&d_len, cap)); CHECK(scope.get(&d_start, cap)); CHECK(scope.get(&d_w, cap));
        CHECK(scope.get(&d_minus, cap));
        rm.rank_of = d_map;
        uint32_t herr[2] = {MIRGE_COV_NONE, MIRGE_COV_NONE};
        hipError_t e = hipSuccess;
        if (n_map) e = hipMemcpyAsync(d_map, chrom_rank, n_map * 4, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(d_err, 0xFF, 8, c->stream);
        if (e == hipSuccess && n_rows) {
            LaunchScope ls(c, "k_cov_intervals", (double)n_rows);
            hipLaunchKernelGGL(k_cov_intervals, dim3(grid_for(c, n_rows)), dim3(MIRGE_BLOCK), 0, c->stream, prep.t, (const uint32_t*)prep.d_rows, (uint32_t)n_rows, rm,
                               d_rank, d_start, d_len, d_w, d_minus, d_err);
        }
        if (e == hipSuccess) e = hipMemcpyAsync(herr, d_err, 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(-2, who + ": " + hipGetErrorString(e));
        if (herr[0] != MIRGE_COV_NONE || herr[1] != MIRGE_COV_NONE) {  // name the first offending row of the file
            const bool range = herr[0] == MIRGE_COV_NONE || (herr[1] != MIRGE_COV_NONE && herr[1] < herr[0]);
            int32_t d[4] = {0, 0, 0, 0};
            hipLaunchKernelGGL(k_cov_describe, dim3(1), dim3(64), 0, c->stream, prep.t, (const uint32_t*)prep.d_rows, range ? herr[1] : herr[0], d_desc);
            e = hipMemcpyAsync(d, d_desc, 16, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) return fail(-2, who + ": " + hipGetErrorString(e));
            if (err_out) { err_out[0] = range ? 2 : 1; err_out[1] = d[0]; err_out[2] = d[1]; err_out[3] = d[2]; }
            if (range)
                return fail(-1, who + ": a read lies outside [1, 2^31 - 1] of its chromosome (unique read " + std::to_string(d[0]) + ", pass " +
                                    std::to_string(d[1]) + ", reference " + std::to_string(d[2]) + ")");
            std::string name = "?";
            if (d[1] >= 0 && d[1] < n_pass && d[3] >= 0 && (int64_t)d[3] < passes[d[1]].n_chrom) {
                const mirge_sam_pass& in = passes[d[1]];
                name.assign(in.chrom_data + in.chrom_off[d[3]], in.chrom_data + in.chrom_off[d[3] + 1]);
            }
            return fail(-1, who + ": reads lie on '" + name + "', which no @SQ line of the header names");
        }
        hc.lap("intervals");
        return 0;
    }
};

// mirge_coverage_write_device and mirge_coverage_write_device_bgzf: gzi_path == nullptr are the plain files, else `path` / `path_minus`
// are .gz files, each a stream of its own (BgzfSink): the minus file's block 0 starts at the minus text's byte 0
static int coverage_write_impl(const std::string& who, mirge_ctx* c, const mirge_reads* U, const mirge_result* res, const int64_t* order, int32_t sample,
                               const int32_t* class_pass, int32_t n_class, const mirge_sam_pass* passes, int32_t n_pass,
                               const int32_t* chrom_rank, const int64_t* chrom_rank_off, int32_t n_rank, const char* rank_names,
                               const int64_t* rank_name_off, int32_t stranded, const char* path, const char* path_minus,
                               int64_t* n_intervals_out, int64_t* weight_out, int64_t* n_lines_out, int64_t* n_bytes_out,
                               int64_t* err_out, const char* gzi_path, const char* gzi_path_minus, int64_t block_bytes, int64_t* stats_out) {
    const bool bgzf = gzi_path != nullptr;
    if (bgzf && stranded && !gzi_path_minus) return fail(-1, who + ": bad argument");
    if (!c || !path || (stranded && !path_minus) || !chrom_rank || !chrom_rank_off || n_rank < 0 || n_rank > (1 << 24) || !rank_name_off ||
        (n_rank && !rank_names) || n_pass < 1 || n_pass > MIRGE_MAX_PASSES || !passes)
        return fail(-1, who + ": bad argument");
    if (err_out) for (int k = 0; k < 4; k++) err_out[k] = 0;
    for (int32_t k = 0; k < n_rank; k++)
        if (rank_name_off[k + 1] < rank_name_off[k] || rank_name_off[k + 1] - rank_name_off[0] >= 0x7FFFFFF0ll) return fail(-1, who + ": malformed chromosome names");
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    HostClock hc("coverage_write_device");
    size_t tile = env_bytes("MIRGE_COV_TILE_BYTES", 8160);
    tile = std::min<size_t>(MIRGE_COV_MAX_TILE, std::max<size_t>(64, tile)) & ~size_t(15);
    size_t chunk = env_bytes("MIRGE_COV_CHUNK_BYTES", (size_t)32 << 20);
    chunk = std::min<size_t>((size_t)1 << 30, std::max(chunk, tile)) / tile * tile;

    CovInput in;
    CovDev dev;
    uint8_t* d_text[2] = {nullptr, nullptr};
    OutFile out[2] = {{who}, {who}};  // (the strands' files: both or neither, commit_all; uncommitted, a file goes)
    BgzfStream gz0(who), gz1(who);
    BgzfStream* const gzs[2] = {&gz0, &gz1};
    PoolScope scope(c);
    BgzfSink sink(scope, who);
    if (bgzf) CHECK(sink.configure(block_bytes));  // (a wrong MIRGE_BGZF_* value: before anything is done)
    CHECK(in.build(scope, who, U, res, order, sample, class_pass, n_class, passes, n_pass, chrom_rank, chrom_rank_off, n_rank, err_out, hc));
    CHECK(dev.runs(scope, who, in.intervals(), in.n_rows, (uint32_t)std::max(n_rank, 1), stranded != 0));
    hc.lap("runs");
    CHECK(dev.measure(scope, rank_names, rank_name_off, (uint32_t)n_rank));
    hc.lap("measured");
    // ---- the file or files: every error of the data has been raised by now
    const unsigned long long body = dev.body, split = stranded ? dev.split : dev.body;
    if (bgzf) {
        const unsigned long long base[2] = {0ull, split};
        gz0.bytes = split; gz1.bytes = body - split;
        CHECK(gz0.open(path, gzi_path));
        if (stranded) CHECK(gz1.open(path_minus, gzi_path_minus));
        auto fill = [&](int s, unsigned long long at, uint32_t nn, uint8_t* dst, const uint8_t** text) -> int {
            const size_t tiles = ((size_t)nn + tile - 1) / tile;
            LaunchScope ls(c, "k_cov_write", (double)nn);
            hipLaunchKernelGGL(k_cov_write, dim3((unsigned)std::min<size_t>(tiles, (size_t)c->n_cu * 32)), dim3(MIRGE_BLOCK), 0, c->stream, dev.r,
                               (uint32_t)dev.n_runs, (const uint32_t*)dev.d_name_off, (const uint8_t*)dev.d_name_data,
                               (const unsigned long long*)dev.d_off, base[s] + at, nn, (uint32_t)tile, dst);
            *text = dst;
            return 0;
        };
        CHECK(sink.run(gzs, stranded ? 2 : 1, chunk, fill));
        hc.lap("formatted + deflated + written");
        CHECK(commit_all({&gz0.gz, &gz0.gzi, &gz1.gz, &gz1.gzi}));
        if (stats_out) { gz0.stats(stats_out); gz1.stats(stats_out + MIRGE_BGZF_STATS); }
        if (n_intervals_out) *n_intervals_out = (int64_t)in.n_rows;
        if (weight_out) *weight_out = (int64_t)dev.weight;
        if (n_lines_out) *n_lines_out = (int64_t)dev.n_runs;
        if (n_bytes_out) *n_bytes_out = (int64_t)dev.body;
        return 0;
    }
    CHECK(out[0].open(path));
    if (stranded) CHECK(out[1].open(path_minus));
    if (body) {
        const size_t buf = (size_t)std::min<unsigned long long>(chunk, body);
        StagePipe pipe(c, who);
        CHECK(pipe.ensure(buf));
        CHECK(scope.get(&d_text[0], buf + 16));
        if (body > buf) CHECK(scope.get(&d_text[1], buf + 16));
        auto queue = [&](unsigned long long ci) -> int {
            const unsigned long long at0 = ci * chunk;
            const uint32_t nn = (uint32_t)std::min<unsigned long long>(chunk, body - at0);
            const size_t tiles = ((size_t)nn + tile - 1) / tile;
            {
                LaunchScope ls(c, "k_cov_write", (double)nn);
                hipLaunchKernelGGL(k_cov_write, dim3((unsigned)std::min<size_t>(tiles, (size_t)c->n_cu * 32)), dim3(MIRGE_BLOCK), 0, c->stream, dev.r,
                                   (uint32_t)dev.n_runs, (const uint32_t*)dev.d_name_off, (const uint8_t*)dev.d_name_data,
                                   (const unsigned long long*)dev.d_off, at0, nn, (uint32_t)tile, d_text[ci & 1]);
            }
            HIPOK(hipMemcpyAsync(pipe.half(ci), d_text[ci & 1], nn, hipMemcpyDeviceToHost, c->stream));
            return 0;
        };
        auto take = [&](unsigned long long ci) -> int {  // chunk ci is in its half; the plus strand's bytes end at `split`
            const unsigned long long at0 = ci * chunk, at1 = at0 + std::min<unsigned long long>(chunk, body - at0);
            const uint8_t* src = pipe.half(ci);
            if (at0 < split) CHECK(out[0].put(src, (size_t)(std::min(at1, split) - at0), at0));
            if (at1 > split) { const unsigned long long b0 = std::max(at0, split); CHECK(out[1].put(src + (b0 - at0), (size_t)(at1 - b0), b0 - split)); }
            return 0;
        };
        CHECK(pipe.run((body + chunk - 1) / chunk, queue, take));
    }
    hc.lap("formatted + written");
    CHECK(commit_all({&out[0], &out[1]}));  // (every chunk has been taken: nothing of the files is still on its way)
    if (n_intervals_out) *n_intervals_out = (int64_t)in.n_rows;
    if (weight_out) *weight_out = (int64_t)dev.weight;
    if (n_lines_out) *n_lines_out = (int64_t)dev.n_runs;
    if (n_bytes_out) *n_bytes_out = (int64_t)dev.body;
    return 0;
}

extern "C" int mirge_coverage_write_device(mirge_ctx* c, const mirge_reads* U, const mirge_result* res, const int64_t* order, int32_t sample,
                                           const int32_t* class_pass, int32_t n_class, const mirge_sam_pass* passes, int32_t n_pass,
                                           const int32_t* chrom_rank, const int64_t* chrom_rank_off, int32_t n_rank, const char* rank_names,
                                           const int64_t* rank_name_off, int32_t stranded, const char* path, const char* path_minus,
                                           int64_t* n_intervals_out, int64_t* weight_out, int64_t* n_lines_out, int64_t* n_bytes_out,
                                           int64_t* err_out) {
    return coverage_write_impl("mirge_coverage_write_device", c, U, res, order, sample, class_pass, n_class, passes, n_pass, chrom_rank, chrom_rank_off,
                               n_rank, rank_names, rank_name_off, stranded, path, path_minus, n_intervals_out, weight_out, n_lines_out, n_bytes_out,
                               err_out, nullptr, nullptr, 0, nullptr);
}
// `path` / `path_minus` are the .bedgraph.gz files, gzi_path / gzi_path_minus their block indexes; block_bytes <= 0:
// MIRGE_BGZF_BLOCK_BYTES; stats_out[16]: BgzfStream::stats of either file
extern "C" int mirge_coverage_write_device_bgzf(mirge_ctx* c, const mirge_reads* U, const mirge_result* res, const int64_t* order, int32_t sample,
                                                const int32_t* class_pass, int32_t n_class, const mirge_sam_pass* passes, int32_t n_pass,
                                                const int32_t* chrom_rank, const int64_t* chrom_rank_off, int32_t n_rank, const char* rank_names,
                                                const int64_t* rank_name_off, int32_t stranded, const char* path, const char* path_minus,
                                                int64_t* n_intervals_out, int64_t* weight_out, int64_t* n_lines_out, int64_t* n_bytes_out,
                                                int64_t* err_out, const char* gzi_path, const char* gzi_path_minus, int64_t block_bytes,
                                                int64_t* stats_out) {
    if (!gzi_path) return fail(-1, "mirge_coverage_write_device_bgzf: bad argument");
    return coverage_write_impl("mirge_coverage_write_device_bgzf", c, U, res, order, sample, class_pass, n_class, passes, n_pass, chrom_rank,
                               chrom_rank_off, n_rank, rank_names, rank_name_off, stranded, path, path_minus, n_intervals_out, weight_out, n_lines_out,
                               n_bytes_out, err_out, gzi_path, gzi_path_minus, block_bytes, stats_out);
}
