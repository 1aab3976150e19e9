// native_nearest.hpp -- part of mirge_native.hip (one translation unit): --unmapped-nearest (kernels_nearest.hpp).  One pipeline behind both entry
// points: the library's codes and the chunk list (built on the host, as trf's tile list is), the queries' masks, the two instances' query lists
// by hipCUB's flagged selection, k_near_scan<uint32_t> and <uint64_t> over (chunks) x (query tiles) into one 64-bit word per query, the kept
// queries selected, k_near_start on them alone.  mirge_nearest_scan takes its queries as ASCII and keeps every query with a hit;
// mirge_nearest_unmapped selects the dictionary's unannotated rows of 12 .. 64 nt first and keeps D <= min(K, m / 8).  Every call's blocks: one PoolScope.
#pragma once

struct mirge_nearest {  // on the host: the kept rows in ascending handle index
    std::vector<uint32_t> row;
    std::vector<int32_t> dist, hairpin, start, end;
    int64_t stats[5] = {0, 0, 0, 0, 0};  // unannotated, short, long, considered, kept
};

extern "C" void mirge_nearest_destroy(mirge_nearest* h) { delete h; }
extern "C" int64_t mirge_nearest_count(const mirge_nearest* h) { return h ? (int64_t)h->row.size() : 0; }
extern "C" int mirge_nearest_fetch(const mirge_nearest* h, uint32_t* row, int32_t* dist, int32_t* hairpin, int32_t* start, int32_t* end) {
    if (!h) return fail(-1, "mirge_nearest_fetch: bad argument");
    const size_t n = h->row.size();
    if (n && (!row || !dist || !hairpin || !start || !end)) return fail(-1, "mirge_nearest_fetch: bad argument");
    if (n) {
        std::memcpy(row, h->row.data(), n * 4); std::memcpy(dist, h->dist.data(), n * 4); std::memcpy(hairpin, h->hairpin.data(), n * 4);
        std::memcpy(start, h->start.data(), n * 4); std::memcpy(end, h->end.data(), n * 4);
    }
    return 0;
}
extern "C" int mirge_nearest_stats(const mirge_nearest* h, int64_t* stats_out) {
    if (!h || !stats_out) return fail(-1, "mirge_nearest_stats: bad argument");
    std::memcpy(stats_out, h->stats, sizeof(h->stats));
    return 0;
}

// MIRGE_NEAR_CHUNK_BASES, read per call (tests set 64): 1 .. MIRGE_NEAR_LDS_BASES
static int near_chunk_bases(const std::string& who, uint32_t& out) {
    out = MIRGE_NEAR_LDS_BASES;
    const char* const e = std::getenv("MIRGE_NEAR_CHUNK_BASES");
    if (!e || !*e) return 0;
    char* end = nullptr;
    const long v = std::strtol(e, &end, 10);
    if (*end || v < 1 || v > MIRGE_NEAR_LDS_BASES) return fail(-1, who + ": MIRGE_NEAR_CHUNK_BASES is an integer in 1 .. " + std::to_string(MIRGE_NEAR_LDS_BASES));
    out = (uint32_t)v;
    return 0;
}

// runs of whole consecutive hairpins of at most `cap` bases; a longer hairpin is a run of its own; hairpins without a base open no run
static std::vector<NearChunk> near_chunks(const std::vector<uint32_t>& hoff, uint32_t cap) {
    std::vector<NearChunk> out;
    const uint32_t n_h = (uint32_t)hoff.size() - 1;
    uint32_t h = 0;
    while (h < n_h) {
        uint32_t h1 = h + 1;
        while (h1 < n_h && hoff[h1 + 1] - hoff[h] <= cap) h1++;
        if (hoff[h1] > hoff[h]) out.push_back(NearChunk{h, h1});
        h = h1;
    }
    return out;
}

// the library on the device: codes, offsets, chunks
struct NearLib {
    uint8_t* codes = nullptr;
    uint32_t* hoff = nullptr;
    NearChunk* chunks = nullptr;
    uint32_t n_h = 0, n_chunk = 0, total = 0;
};

// hoff32 and chunks are the caller's (declared before the scope: async copies read them)
static int near_upload_lib(const std::string& who, mirge_ctx* c, PoolScope& scope, const char* t_text, const int64_t* t_off, int64_t n_t,
                           std::vector<uint32_t>& hoff32, std::vector<NearChunk>& chunks, NearLib& L) {
    if (n_t < 0 || (n_t && !t_off)) return fail(-1, who + ": bad argument");
    if (n_t > (int64_t)MIRGE_NEAR_MAX_HAIRPINS) return fail(-5, who + ": more than 2^24 hairpins");
    hoff32.assign((size_t)n_t + 1, 0u);
    if (n_t) {
        if (t_off[0] != 0) return fail(-1, who + ": the hairpins' offsets are malformed");
        for (int64_t h = 0; h < n_t; h++)
            if (t_off[h + 1] < t_off[h]) return fail(-1, who + ": the hairpins' offsets are malformed");
        if (t_off[n_t] >= 0xFFFFFFF0ll) return fail(-5, who + ": 2^32 - 16 hairpin bases or more");
        for (int64_t h = 0; h <= n_t; h++) hoff32[(size_t)h] = (uint32_t)t_off[h];
    }
    L.n_h = (uint32_t)n_t;
    L.total = hoff32[(size_t)n_t];
    if (L.total && !t_text) return fail(-1, who + ": bad argument");
    if (!L.total) return 0;
    uint32_t cap;
    CHECK(near_chunk_bases(who, cap));
    chunks = near_chunks(hoff32, cap);
    L.n_chunk = (uint32_t)chunks.size();
    uint8_t* d_ascii;
    // (16 bytes of slack behind the codes: k_near_scan reads a long hairpin's codes in aligned words, up to 7 bytes past a column)
    CHECK(scope.get(&d_ascii, (size_t)L.total)); CHECK(scope.get(&L.codes, (size_t)L.total + 16)); CHECK(scope.get(&L.hoff, (size_t)n_t + 1));
    CHECK(scope.get(&L.chunks, chunks.size()));
    HIPOK(hipMemcpyAsync(d_ascii, t_text, (size_t)L.total, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(L.hoff, hoff32.data(), ((size_t)n_t + 1) * 4, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(L.chunks, chunks.data(), chunks.size() * sizeof(NearChunk), hipMemcpyHostToDevice, c->stream));
    LaunchScope ls(c, "k_near_codes", (double)L.total);
    hipLaunchKernelGGL(k_near_codes, dim3(grid_for(c, (size_t)L.total)), dim3(MIRGE_BLOCK), 0, c->stream, (const uint8_t*)d_ascii, L.total, L.codes);
    return 0;
}

// indices of the flagged among [0, n) -> out (n entries of room), their number -> *d_num (device); hipCUB's selection
static int near_select(mirge_ctx* c, PoolScope& scope, const uint8_t* d_flags, uint32_t n, uint32_t* d_out, uint32_t* d_num) {
    hipcub::CountingInputIterator<uint32_t> first(0u);
    size_t tb = 0;
    HIPOK(hipcub::DeviceSelect::Flagged(nullptr, tb, first, d_flags, d_out, d_num, (int)n, c->stream));
    uint8_t* d_tmp;
    CHECK(scope.get(&d_tmp, std::max<size_t>(tb, 16)));
    HIPOK(hipcub::DeviceSelect::Flagged(d_tmp, tb, first, d_flags, d_out, d_num, (int)n, c->stream));
    return 0;
}

// The queries' masks and lengths are on the device (peq [4][n], qlen [n]: 0 = not considered).  -> best [n] and start [n] filled on the
// device, the kept queries' indices in d_rep and their number in n_rep.
struct NearRun {
    unsigned long long* best = nullptr;
    int32_t* start = nullptr;
    uint32_t* rep = nullptr;
    uint32_t n_rep = 0;
    uint32_t num[3] = {0, 0, 0};  // queries of the 32-bit instance, of the 64-bit instance, kept (filled by async copies: declared before the scope)
};

static int near_pipeline(const std::string& who, mirge_ctx* c, PoolScope& scope, const NearLib& L, const uint64_t* d_peq, const uint8_t* d_qlen,
                         uint32_t n, int32_t K, NearRun& R) {
    const char* const f64e = std::getenv("MIRGE_NEAR_FORCE64");
    const int32_t force64 = f64e && std::atoi(f64e) != 0 ? 1 : 0;
    uint8_t *d_f32, *d_f64, *d_frep;
    uint32_t *d_i32, *d_i64, *d_num;
    uint32_t* const num = R.num;
    CHECK(scope.get(&R.best, (size_t)n)); CHECK(scope.get(&R.start, (size_t)n)); CHECK(scope.get(&R.rep, (size_t)n));
    CHECK(scope.get(&d_f32, (size_t)n)); CHECK(scope.get(&d_f64, (size_t)n)); CHECK(scope.get(&d_frep, (size_t)n));
    CHECK(scope.get(&d_i32, (size_t)n)); CHECK(scope.get(&d_i64, (size_t)n)); CHECK(scope.get(&d_num, 4));
    HIPOK(hipMemsetAsync(R.best, 0xFF, (size_t)n * 8, c->stream));
    HIPOK(hipMemsetAsync(R.start, 0xFF, (size_t)n * 4, c->stream));
    HIPOK(hipMemsetAsync(d_num, 0, 16, c->stream));
    if (!L.n_chunk) return 0;  // a library without a base: no query has a hit
    {
        LaunchScope ls(c, "k_near_width", (double)n);
        hipLaunchKernelGGL(k_near_width, dim3(grid_for(c, (size_t)n)), dim3(MIRGE_BLOCK), 0, c->stream, d_qlen, n, force64, d_f32, d_f64);
    }
    CHECK(near_select(c, scope, d_f32, n, d_i32, d_num));
    CHECK(near_select(c, scope, d_f64, n, d_i64, d_num + 1));
    HIPOK(hipMemcpyAsync(num, d_num, 8, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    HIPOK(hipGetLastError());
    if ((size_t)num[0] + num[1] > n) return fail(-1, who + ": internal: the selection counts more queries than there are");
    for (int inst = 0; inst < 2; inst++) {
        const uint32_t nq = num[inst];
        if (!nq) continue;
        const uint32_t tiles = (nq + MIRGE_BLOCK - 1) / MIRGE_BLOCK;
        const dim3 grid(L.n_chunk, std::min<uint32_t>(tiles, 65535u));
        LaunchScope ls(c, inst ? "k_near_scan64" : "k_near_scan32", (double)nq * (double)L.total);
        if (inst == 0)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_near_scan<uint32_t>), grid, dim3(MIRGE_BLOCK), 0, c->stream, (const uint32_t*)d_i32, nq, n, d_peq, d_qlen,
                               (const uint8_t*)L.codes, (const uint32_t*)L.hoff, (const NearChunk*)L.chunks, R.best);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_near_scan<uint64_t>), grid, dim3(MIRGE_BLOCK), 0, c->stream, (const uint32_t*)d_i64, nq, n, d_peq, d_qlen,
                               (const uint8_t*)L.codes, (const uint32_t*)L.hoff, (const NearChunk*)L.chunks, R.best);
    }
    {
        LaunchScope ls(c, "k_near_report", (double)n);
        hipLaunchKernelGGL(k_near_report, dim3(grid_for(c, (size_t)n)), dim3(MIRGE_BLOCK), 0, c->stream, (const unsigned long long*)R.best, d_qlen, n, K, d_frep);
    }
    CHECK(near_select(c, scope, d_frep, n, R.rep, d_num + 2));
    HIPOK(hipMemcpyAsync(num + 2, d_num + 2, 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    HIPOK(hipGetLastError());
    R.n_rep = num[2];
    if (R.n_rep > n) return fail(-1, who + ": internal: the selection counts more queries than there are");
    if (!R.n_rep) return 0;
    for (int inst = 0; inst < 2; inst++) {
        if (!num[inst]) continue;
        LaunchScope ls(c, inst ? "k_near_start64" : "k_near_start32", (double)R.n_rep);
        const dim3 grid(grid_for(c, (size_t)R.n_rep)), block(MIRGE_BLOCK);
        if (inst == 0)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_near_start<uint32_t>), grid, block, 0, c->stream, (const uint32_t*)R.rep, R.n_rep, n, d_peq, d_qlen,
                               (const uint8_t*)L.codes, (const uint32_t*)L.hoff, (const unsigned long long*)R.best, force64, R.start);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_near_start<uint64_t>), grid, block, 0, c->stream, (const uint32_t*)R.rep, R.n_rep, n, d_peq, d_qlen,
                               (const uint8_t*)L.codes, (const uint32_t*)L.hoff, (const unsigned long long*)R.best, force64, R.start);
    }
    return 0;
}

extern "C" int mirge_nearest_scan(mirge_ctx* c, const char* q_text, const int64_t* q_off, int64_t n_q, const char* t_text, const int64_t* t_off,
                                  int64_t n_t, int32_t* dist, int32_t* hairpin, int32_t* start, int32_t* end) {
    const std::string who = "mirge_nearest_scan";
    if (!c || n_q < 0 || (n_q && (!q_off || !dist || !hairpin || !start || !end))) return fail(-1, who + ": bad argument");
    if (n_q >= 0x7FFFFFF0ll) return fail(-5, who + ": too many queries for one call");
    for (int64_t i = 0; i < n_q; i++) dist[i] = hairpin[i] = start[i] = end[i] = -1;
    if (n_q == 0) return 0;
    if (q_off[0] != 0) return fail(-1, who + ": the queries' offsets are malformed");
    for (int64_t i = 0; i < n_q; i++)
        if (q_off[i + 1] < q_off[i]) return fail(-1, who + ": the queries' offsets are malformed");
    const int64_t q_bytes = q_off[n_q];
    if (q_bytes && !q_text) return fail(-1, who + ": bad argument");
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    const uint32_t n = (uint32_t)n_q;
    std::vector<uint32_t> hoff32;
    std::vector<NearChunk> chunks;
    std::vector<unsigned long long> best((size_t)n);
    std::vector<int32_t> st((size_t)n);
    NearRun R;
    PoolScope scope(c);  // (behind the host vectors, which the copies read or fill: they outlive its wait)
    NearLib L;
    CHECK(near_upload_lib(who, c, scope, t_text, t_off, n_t, hoff32, chunks, L));
    uint8_t *d_text, *d_qlen;
    int64_t* d_off;
    uint64_t* d_peq;
    CHECK(scope.get(&d_text, (size_t)q_bytes + 16)); CHECK(scope.get(&d_off, (size_t)n + 1)); CHECK(scope.get(&d_peq, (size_t)n * 4));
    CHECK(scope.get(&d_qlen, (size_t)n));
    if (q_bytes) HIPOK(hipMemcpyAsync(d_text, q_text, (size_t)q_bytes, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(d_off, q_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    {
        LaunchScope ls(c, "k_near_masks_ascii", (double)n);
        hipLaunchKernelGGL(k_near_masks_ascii, dim3(grid_for(c, (size_t)n)), dim3(MIRGE_BLOCK), 0, c->stream, (const uint8_t*)d_text, (const int64_t*)d_off, n,
                           d_peq, d_qlen);
    }
    CHECK(near_pipeline(who, c, scope, L, d_peq, d_qlen, n, -1, R));
    HIPOK(hipMemcpyAsync(best.data(), R.best, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(st.data(), R.start, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    HIPOK(hipGetLastError());
    for (size_t i = 0; i < (size_t)n; i++) {
        if (best[i] == MIRGE_NEAR_NO_KEY) continue;
        if (st[i] < 0) return fail(-1, who + ": internal: the anchored scan did not reach the distance of query " + std::to_string(i));
        dist[i] = (int32_t)(best[i] >> 56); hairpin[i] = (int32_t)((best[i] >> 32) & 0xFFFFFFull); end[i] = (int32_t)(uint32_t)best[i]; start[i] = st[i];
    }
    return 0;
}

extern "C" int mirge_nearest_unmapped(mirge_ctx* c, const mirge_reads* U, const mirge_result* res, const char* t_text, const int64_t* t_off, int64_t n_t,
                                      int32_t K, mirge_nearest** out) {
    const std::string who = "mirge_nearest_unmapped";
    if (!c || !U || !res || !out || U->ctx != c) return fail(-1, who + ": bad argument");
    if (K < 1 || K > MIRGE_NEAR_MAX_K) return fail(-1, who + ": K is 1 .. " + std::to_string(MIRGE_NEAR_MAX_K));
    if (res->n != U->n) return fail(-1, who + ": result and read set differ");
    if (U->n >= 0x7FFFFFF0ll) return fail(-5, who + ": too many rows for one call");
    static_assert(MIRGE_NEAR_NGROUPS == MIRGE_NGROUPS, "read groups");
    NearGroups t;
    std::memset(&t, 0, sizeof(t));
    for (int gi = 0; gi < MIRGE_NGROUPS; gi++) {
        const ReadGroup& g = U->g[gi];
        if (g.n && g.orig) return fail(-1, who + ": the read set is not a collapse result");
        if (g.n != res->g[gi].n || (g.n && !res->g[gi].pass)) return fail(-1, who + ": the result is not this read set's");
        t.g[gi] = NearGroup{g.seq, g.nmask, g.len, res->g[gi].pass, g.base, g.n, is_long_group(gi) ? 0 : g.W, 0};
    }
    std::unique_ptr<mirge_nearest> hits(new mirge_nearest);
    if (U->n == 0) { *out = hits.release(); return 0; }
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    const uint32_t n_rows = (uint32_t)U->n;
    std::vector<uint32_t> hoff32;
    std::vector<NearChunk> chunks;
    std::vector<unsigned long long> key;
    unsigned long long stats[4] = {0, 0, 0, 0};
    uint32_t n_sel = 0;
    NearRun R;
    PoolScope scope(c);  // (behind the host vectors, `stats` and `n_sel`, which the copies read or fill: they outlive its wait)
    NearLib L;
    CHECK(near_upload_lib(who, c, scope, t_text, t_off, n_t, hoff32, chunks, L));
    uint8_t* d_flags;
    uint32_t *d_sel, *d_nsel;
    unsigned long long* d_stats;
    CHECK(scope.get(&d_flags, (size_t)n_rows)); CHECK(scope.get(&d_sel, (size_t)n_rows)); CHECK(scope.get(&d_nsel, 4)); CHECK(scope.get(&d_stats, 4));
    HIPOK(hipMemsetAsync(d_stats, 0, 32, c->stream));
    HIPOK(hipMemsetAsync(d_nsel, 0, 16, c->stream));
    {
        LaunchScope ls(c, "k_near_flag", (double)n_rows);
        hipLaunchKernelGGL(k_near_flag, dim3(grid_for(c, (size_t)n_rows)), dim3(MIRGE_BLOCK), 0, c->stream, t, n_rows, d_flags, d_stats);
    }
    CHECK(near_select(c, scope, d_flags, n_rows, d_sel, d_nsel));
    HIPOK(hipMemcpyAsync(&n_sel, d_nsel, 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(stats, d_stats, 24, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    HIPOK(hipGetLastError());
    if (n_sel > n_rows) return fail(-1, who + ": internal: the selection counts more rows than there are");
    hits->stats[0] = (int64_t)stats[MIRGE_NEAR_ST_UNMAPPED]; hits->stats[1] = (int64_t)stats[MIRGE_NEAR_ST_SHORT];
    hits->stats[2] = (int64_t)stats[MIRGE_NEAR_ST_LONG]; hits->stats[3] = (int64_t)n_sel;
    if (!n_sel) { *out = hits.release(); return 0; }
    uint64_t* d_peq;
    uint8_t* d_qlen;
    CHECK(scope.get(&d_peq, (size_t)n_sel * 4)); CHECK(scope.get(&d_qlen, (size_t)n_sel));
    {
        LaunchScope ls(c, "k_near_masks_packed", (double)n_sel);
        hipLaunchKernelGGL(k_near_masks_packed, dim3(grid_for(c, (size_t)n_sel)), dim3(MIRGE_BLOCK), 0, c->stream, t, (const uint32_t*)d_sel, n_sel, d_peq, d_qlen);
    }
    CHECK(near_pipeline(who, c, scope, L, d_peq, d_qlen, n_sel, K, R));
    const size_t nr = (size_t)R.n_rep;
    hits->stats[4] = (int64_t)nr;
    if (!nr) { *out = hits.release(); return 0; }
    uint32_t* d_row;
    unsigned long long* d_key;
    int32_t* d_s;
    CHECK(scope.get(&d_row, nr)); CHECK(scope.get(&d_key, nr)); CHECK(scope.get(&d_s, nr));
    {
        LaunchScope ls(c, "k_near_gather", (double)nr);
        hipLaunchKernelGGL(k_near_gather, dim3(grid_for(c, nr)), dim3(MIRGE_BLOCK), 0, c->stream, (const uint32_t*)R.rep, R.n_rep, (const uint32_t*)d_sel,
                           (const unsigned long long*)R.best, (const int32_t*)R.start, d_row, d_key, d_s);
    }
    key.resize(nr); hits->row.resize(nr); hits->start.resize(nr); hits->dist.resize(nr); hits->hairpin.resize(nr); hits->end.resize(nr);
    HIPOK(hipMemcpyAsync(hits->row.data(), d_row, nr * 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(key.data(), d_key, nr * 8, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(hits->start.data(), d_s, nr * 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    HIPOK(hipGetLastError());
    for (size_t i = 0; i < nr; i++) {
        if (hits->start[i] < 0) return fail(-1, who + ": internal: the anchored scan did not reach the distance of row " + std::to_string(hits->row[i]));
        hits->dist[i] = (int32_t)(key[i] >> 56); hits->hairpin[i] = (int32_t)((key[i] >> 32) & 0xFFFFFFull); hits->end[i] = (int32_t)(uint32_t)key[i];
    }
    *out = hits.release();
    return 0;
}
