// native_ec.hpp -- part of mirge_native.hip (one translation unit): --kmer-correct (kernels_ec.hpp): the rounds of mirge_kmer_correct, each
// one the spectrum, with a ratio (mirge_kmer_correct_ratio) the relative threshold's two launches, the classification, the wave kernel
// and, where a read changed, the regrouping through the weighted collapse.
#pragma once

#define MIRGE_EC_MAX_ROUNDS (MIRGE_EC_MAXK - 8 + 1)
#define MIRGE_EC_STAT_WORDS 8
// what the last call on this thread saw, per round: eligible, suspect, corrected, uncorrectable, unsupported, ambiguous, distinct reads
// after the round, slots of the round's table
static thread_local int64_t g_ec_stats[MIRGE_EC_MAX_ROUNDS * MIRGE_EC_STAT_WORDS];
static thread_local int32_t g_ec_rounds = 0;
// with a ratio, per round: distinct k-mers with S > H, the dominated among them (zeros without one)
static thread_local int64_t g_ec_ratio_stats[MIRGE_EC_MAX_ROUNDS * 2];

static int ec_check(const std::string& who, int32_t k_start, int32_t k_end, int32_t threshold) {
    if (threshold < 1) return fail(-1, who + ": the threshold is at least 1");
    if (k_start < 8 || k_end > MIRGE_EC_MAXK || k_start > k_end) return fail(-1, who + ": 8 <= k_start <= k_end <= " + std::to_string(MIRGE_EC_MAXK));
    return 0;
}

static int ec_view_of(const std::string& who, const mirge_reads* T, EcView& v) {
    std::memset(&v, 0, sizeof(v));
    static_assert(MIRGE_EC_NG == MIRGE_NWIDTHS, "the groups without an N come first");
    for (int gi = 0; gi < MIRGE_NGROUPS; gi++) {
        const ReadGroup& g = T->g[gi];
        if (g.n && (g.orig || !g.counts || !g.first)) return fail(-1, who + ": the reads are not a collapse result");
        if (gi < MIRGE_EC_NG && g.n) v.g[gi] = EcGroup{g.seq, g.len, g.counts, g.base, g.n, (uint32_t)g.W, is_long_group(gi) ? 1 : 0};
    }
    v.n_reads = (uint32_t)T->n;
    v.hash_keep = ~0ull;
    if (const char* e = std::getenv("MIRGE_TEST_EC_HASH_BITS")) {  // (tests: collisions on purpose)
        const int bits = std::atoi(e);
        if (bits >= 0 && bits < 64) v.hash_keep = (1ull << bits) - 1;
    }
    return 0;
}

// The round's dictionary D with its corrections (fix: device [D->n]) -> the regrouped dictionary *out, whose `first` are again D's first
// indices; next (device [D->n]): the handle index in *out of every read of D.
static int ec_regroup(mirge_ctx* c, const mirge_reads* D, const uint32_t* fix, mirge_reads** out, uint32_t* next) {
    const std::string who = "mirge_kmer_correct";
    const size_t n = (size_t)D->n;
    PoolScope scope(c);
    uint32_t *ftrue, *src, *dweight = nullptr;
    CHECK(scope.get(&ftrue, n)); CHECK(scope.get(&src, n));
    CHECK(dalloc(c, &dweight, n));  // (the collapse releases it)
    auto raw = std::make_unique<mirge_reads>();
    raw->ctx = c; raw->n = D->n; raw->total_bases = D->total_bases; raw->long_max = D->long_max; raw->iupac_seen = D->iupac_seen;
    std::memcpy(raw->len_hist, D->len_hist, sizeof(raw->len_hist));
    raw->hist_valid = D->hist_valid;
    int rc = 0;
    for (int gi = 0; gi < MIRGE_NGROUPS && rc == 0; gi++) {
        const ReadGroup& g = D->g[gi];
        ReadGroup& r = raw->g[gi];
        r.W = g.W; r.n = g.n; r.base = g.base;
        if (!g.n) continue;
        if (g.n >= 0x7FFFFFFFu) { rc = fail(-5, who + ": too many reads in one group"); break; }
        uint32_t *keys2, *iota, *perm;
        void* tmp = nullptr;
        size_t tmp_bytes = 0;
        if ((rc = dalloc(c, &r.seq, (size_t)g.W * g.n)) || (rc = dalloc(c, &r.len, (size_t)g.n * len_bytes(gi)))) break;
        if (g.nmask && (rc = dalloc(c, &r.nmask, (size_t)g.W * g.n))) break;
        if ((rc = scope.get(&keys2, (size_t)g.n)) || (rc = scope.get(&iota, (size_t)g.n)) || (rc = scope.get(&perm, (size_t)g.n))) break;
        hipLaunchKernelGGL(k_ec_iota, dim3(grid_for(c, g.n)), dim3(MIRGE_BLOCK), 0, c->stream, iota, g.n);
        hipError_t e = hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, (const uint32_t*)g.first, keys2, (const uint32_t*)iota, perm, (int)g.n, 0, 32, c->stream);
        if (e == hipSuccess && (rc = scope.get((uint8_t**)&tmp, std::max<size_t>(tmp_bytes, 16)))) break;
        if (e == hipSuccess) e = hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, (const uint32_t*)g.first, keys2, (const uint32_t*)iota, perm, (int)g.n, 0, 32, c->stream);
        if (e != hipSuccess) { rc = fail(-2, who + ": " + hipGetErrorString(e)); break; }
        EcGather a{g.seq, g.nmask, g.len, g.counts, g.first, perm, r.seq, r.nmask, r.len, g.base, g.n, (uint32_t)g.W, (int32_t)len_bytes(gi)};
        LaunchScope ls(c, "k_ec_gather", (double)g.n);
        hipLaunchKernelGGL(k_ec_gather, dim3(grid_for(c, g.n)), dim3(MIRGE_BLOCK), 0, c->stream, a, fix, dweight, ftrue, src);
    }
    if (rc == 0 && hipGetLastError() != hipSuccess) rc = fail(-2, who + ": a regrouping kernel did not launch");
    mirge_reads* R = nullptr;
    if (rc == 0) { rc = collapse_impl(c, raw.get(), nullptr, 1, &R, nullptr, nullptr, nullptr, nullptr, dweight); dweight = nullptr; }
    c->release(dweight);
    if (rc == 0) {
        hipError_t e = hipMemsetAsync(next, 0xFF, n * 4, c->stream);
        if (e != hipSuccess) rc = fail(-2, who + ": " + hipGetErrorString(e));
        for (int gi = 0; gi < MIRGE_NGROUPS && rc == 0; gi++) {
            const ReadGroup& u = R->g[gi];
            if (u.n) hipLaunchKernelGGL(k_ec_rep, dim3(grid_for(c, u.n)), dim3(MIRGE_BLOCK), 0, c->stream, u.first, u.n, u.base, (const uint32_t*)ftrue,
                                        (const uint32_t*)src, (uint32_t)n, next);
        }
    }
    if (rc == 0 && R->n) {  // the reads that merged into an earlier one
        EcView rv, uv;
        rc = ec_view_of(who, R, uv);
        std::memset(&rv, 0, sizeof(rv));
        for (int gi = 0; gi < MIRGE_EC_NG; gi++) {
            const ReadGroup& r = raw->g[gi];
            if (r.n) rv.g[gi] = EcGroup{r.seq, r.len, nullptr, r.base, r.n, (uint32_t)r.W, is_long_group(gi) ? 1 : 0};
        }
        rv.n_reads = (uint32_t)raw->n;
        uint64_t slots = 256;
        while (slots < 2 * (uint64_t)R->n) slots <<= 1;
        uv.tab_mask = slots - 1;
        uint64_t* rtab;
        if (rc == 0) rc = scope.get(&rtab, (size_t)slots);
        if (rc == 0) {
            hipError_t e = hipMemsetAsync(rtab, 0xFF, (size_t)slots * 8, c->stream);
            if (e != hipSuccess) rc = fail(-2, who + ": " + hipGetErrorString(e));
        }
        if (rc == 0) {
            { LaunchScope ls(c, "k_ec_index", (double)R->n); hipLaunchKernelGGL(k_ec_index, dim3(grid_for(c, (size_t)R->n)), dim3(MIRGE_BLOCK), 0, c->stream, uv, rtab); }
            { LaunchScope ls(c, "k_ec_find", (double)n); hipLaunchKernelGGL(k_ec_find, dim3(grid_for(c, n)), dim3(MIRGE_BLOCK), 0, c->stream, rv, uv, (const uint64_t*)rtab, (const uint32_t*)src, next); }
        }
    }
    if (rc == 0) {
        hipError_t e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) rc = fail(-2, who + ": " + hipGetErrorString(e));
    }
    mirge_reads_destroy(raw.release());
    if (rc) { if (R) mirge_reads_destroy(R); return rc; }
    *out = R;
    return 0;
}

// A collapse result's own copy: the same reads under the same handle indices (no round changed anything: the caller still gets a handle
// of its own to destroy).
static int ec_clone(mirge_ctx* c, const mirge_reads* D, mirge_reads** out) {
    auto R = std::make_unique<mirge_reads>();
    R->ctx = c; R->n = D->n; R->total_bases = D->total_bases; R->n_samples = D->n_samples; R->long_max = D->long_max;
    R->iupac_seen = D->iupac_seen; R->hist_valid = D->hist_valid;
    std::memcpy(R->len_hist, D->len_hist, sizeof(R->len_hist));
    const size_t S = (size_t)std::max(D->n_samples, 1);
    int rc = 0;
    hipError_t e = hipSuccess;
    auto copy = [&](auto** dst, const auto* src, size_t count) {
        if (!src || rc || e != hipSuccess) return;
        if ((rc = dalloc(c, dst, count))) return;
        e = hipMemcpyAsync(*dst, src, count * sizeof(**dst), hipMemcpyDeviceToDevice, c->stream);
    };
    for (int gi = 0; gi < MIRGE_NGROUPS; gi++) {
        const ReadGroup& g = D->g[gi];
        ReadGroup& r = R->g[gi];
        r.W = g.W; r.n = g.n; r.base = g.base;
        if (!g.n) continue;
        copy(&r.seq, g.seq, (size_t)g.W * g.n);
        copy(&r.len, g.len, (size_t)g.n * len_bytes(gi));
        copy(&r.nmask, g.nmask, (size_t)g.W * g.n);
        copy(&r.counts, g.counts, (size_t)g.n * S);
        copy(&r.first, g.first, (size_t)g.n);
    }
    if (rc == 0 && e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (rc == 0 && e != hipSuccess) rc = fail(-2, std::string("mirge_kmer_correct: ") + hipGetErrorString(e));
    if (rc) { mirge_reads_destroy(R.release()); return rc; }
    *out = R.release();
    return 0;
}

// ratio == 0: no relative threshold (mirge_kmer_correct); ratio >= 2: a k-mer above the threshold is weak too when a k-mer one letter
// from it has at least `ratio` times its sum (k_ec_dominate, k_ec_fold between the spectrum and the classification)
extern "C" int mirge_kmer_correct_ratio(mirge_ctx* c, const mirge_reads* uniq, int32_t k_start, int32_t k_end, int32_t threshold, int32_t ratio,
                                        mirge_reads** out, uint32_t* final_of, uint32_t* rounds_mask) {
    const std::string who = ratio ? "mirge_kmer_correct_ratio" : "mirge_kmer_correct";
    if (!c || !uniq || uniq->ctx != c || !out) return fail(-1, who + ": bad argument");
    CHECK(ec_check(who, k_start, k_end, threshold));
    if (ratio == 1 || ratio < 0) return fail(-1, who + ": the ratio is 0 (none) or at least 2");
    if (uniq->n && uniq->n_samples != 1) return fail(-1, who + ": the reads must be a collapse result with one count column");
    if (uniq->n >= 0x7FFFFFF0ll) return fail(-5, who + ": too many reads for one call");
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    g_ec_rounds = k_end - k_start + 1;
    for (int64_t& s : g_ec_stats) s = 0;
    for (int64_t& s : g_ec_ratio_stats) s = 0;
    *out = nullptr;
    const size_t U = (size_t)uniq->n;
    if (U == 0) {
        auto R = std::make_unique<mirge_reads>();
        R->ctx = c; R->n_samples = 1; R->hist_valid = true;
        std::memset(R->len_hist, 0, sizeof(R->len_hist));
        for (int gi = 0; gi < MIRGE_NGROUPS; gi++) R->g[gi].W = kGroupW[gi];
        *out = R.release();
        return 0;
    }
    {
        EcView probe;  // (refuses what is no collapse result)
        CHECK(ec_view_of(who, uniq, probe));
    }
    PoolScope outer(c);
    uint32_t *cur, *mask;
    CHECK(outer.get(&cur, U)); CHECK(outer.get(&mask, U));
    hipLaunchKernelGGL(k_ec_iota, dim3(grid_for(c, U)), dim3(MIRGE_BLOCK), 0, c->stream, cur, (uint32_t)U);
    HIPOK(hipMemsetAsync(mask, 0, U * 4, c->stream));
    const mirge_reads* D = uniq;  // the dictionary the round works on
    mirge_reads* owned = nullptr;  // D, when a round made it
    int rc = 0;
    for (int32_t k = k_start; k <= k_end && rc == 0; k++) {
        int64_t* st = g_ec_stats + (size_t)(k - k_start) * MIRGE_EC_STAT_WORDS;
        EcView v;
        if ((rc = ec_view_of(who, D, v))) break;
        v.k = k; v.H = (uint64_t)threshold;
        // an upper bound on the round's windows from the lengths alone (the lengths of the reads with an N count too)
        uint64_t windows = 0;
        if (D->hist_valid)
            for (int L = k; L <= MIRGE_MAX_READ_LEN; L++) windows += (uint64_t)D->len_hist[L] * (uint64_t)(L - k + 1);
        else
            for (int gi = 0; gi < MIRGE_EC_NG - 1; gi++) windows += (uint64_t)D->g[gi].n * (uint64_t)(std::min(32 * D->g[gi].W, MIRGE_MAX_READ_LEN) - k + 1);
        windows += (uint64_t)D->g[MIRGE_EC_NG - 1].n * (uint64_t)(MIRGE_EC_MAXLEN - k + 1);
        uint64_t slots = 256;
        while (slots < 2 * windows) slots <<= 1;
        v.tab_mask = slots - 1;
        st[7] = (int64_t)slots;
        const size_t n = (size_t)D->n;
        mirge_reads* R = nullptr;
        {
            PoolScope scope(c);
            EcSlot* tab;
            uint32_t *range, *fix, *list, *words, *next;
            uint32_t tally[MIRGE_EC_T_WORDS];
            uint8_t* flag = nullptr;
            unsigned long long *words2 = nullptr, tally2[2] = {0, 0};
            if (ratio && ((rc = scope.get(&flag, (size_t)slots)) || (rc = scope.get(&words2, (size_t)2)))) break;
            if ((rc = scope.get(&tab, (size_t)slots)) || (rc = scope.get(&range, n)) || (rc = scope.get(&fix, n)) ||
                (rc = scope.get(&list, n)) || (rc = scope.get(&words, (size_t)MIRGE_EC_T_WORDS)))
                break;
            hipError_t e = hipMemsetAsync(words, 0, MIRGE_EC_T_WORDS * 4, c->stream);
            if (e == hipSuccess && ratio) e = hipMemsetAsync(words2, 0, sizeof(tally2), c->stream);
            const dim3 grid(grid_for(c, n)), block(MIRGE_BLOCK);
            { LaunchScope ls(c, "k_ec_clear", (double)slots); hipLaunchKernelGGL(k_ec_clear, dim3(grid_for(c, (size_t)slots)), block, 0, c->stream, tab, slots); }
            { LaunchScope ls(c, "k_ec_count", (double)n); hipLaunchKernelGGL(k_ec_count, grid, block, 0, c->stream, v, tab); }
            if (ratio) {  // flags from the complete sums, then the flagged sums to 0: two launches
                const dim3 tgrid(grid_for(c, (size_t)slots));
                { LaunchScope ls(c, "k_ec_dominate", (double)slots);
                  hipLaunchKernelGGL(k_ec_dominate, tgrid, block, 0, c->stream, v, (const EcSlot*)tab, slots, (uint64_t)ratio, flag, words2); }
                { LaunchScope ls(c, "k_ec_fold", (double)slots); hipLaunchKernelGGL(k_ec_fold, tgrid, block, 0, c->stream, tab, slots, (const uint8_t*)flag); }
            }
            { LaunchScope ls(c, "k_ec_classify", (double)n); hipLaunchKernelGGL(k_ec_classify, grid, block, 0, c->stream, v, (const EcSlot*)tab, range, fix, list, words); }
            if (e == hipSuccess) e = hipMemcpyAsync(tally, words, sizeof(tally), hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess && ratio) e = hipMemcpyAsync(tally2, words2, sizeof(tally2), hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e == hipSuccess) e = hipGetLastError();
            if (e == hipSuccess && tally[MIRGE_EC_T_LIST]) {
                const uint32_t n_list = tally[MIRGE_EC_T_LIST];
                { LaunchScope ls(c, "k_ec_correct", (double)n_list);
                  hipLaunchKernelGGL(k_ec_correct, dim3(grid_for(c, (size_t)n_list * 64)), block, 0, c->stream, v, (const EcSlot*)tab, (const uint32_t*)list, n_list,
                                     (const uint32_t*)range, fix, words); }
                e = hipMemcpyAsync(tally, words, sizeof(tally), hipMemcpyDeviceToHost, c->stream);
                if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
                if (e == hipSuccess) e = hipGetLastError();
            }
            if (e != hipSuccess) { rc = fail(-2, who + ": " + hipGetErrorString(e)); break; }
            st[0] = tally[MIRGE_EC_T_ELIG]; st[1] = tally[MIRGE_EC_T_SUSPECT]; st[2] = tally[MIRGE_EC_T_CORRECTED];
            st[3] = tally[MIRGE_EC_T_UNCORRECTABLE]; st[4] = tally[MIRGE_EC_T_UNSUPPORTED]; st[5] = tally[MIRGE_EC_T_AMBIGUOUS];
            st[6] = D->n;
            g_ec_ratio_stats[2 * (k - k_start)] = (int64_t)tally2[0]; g_ec_ratio_stats[2 * (k - k_start) + 1] = (int64_t)tally2[1];
            if (tally[MIRGE_EC_T_CORRECTED]) {  // (no read changed: the dictionary stands, every read is its own successor)
                if ((rc = scope.get(&next, n))) break;
                if ((rc = ec_regroup(c, D, fix, &R, next))) break;
                hipLaunchKernelGGL(k_ec_follow, dim3(grid_for(c, U)), block, 0, c->stream, cur, mask, (uint32_t)U, (const uint32_t*)fix, (const uint32_t*)next,
                                   (uint32_t)n, (int32_t)(k - k_start));
                st[6] = R->n;
            }
        }
        if (R) {
            if (owned) mirge_reads_destroy(owned);
            owned = R; D = R;
        }
    }
    if (rc == 0 && !owned) rc = ec_clone(c, uniq, &owned);  // unchanged: the same reads under the same handle indices
    if (rc == 0 && final_of) {
        hipError_t e = hipMemcpyAsync(final_of, cur, U * 4, hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) rc = fail(-2, who + ": " + hipGetErrorString(e));
    }
    if (rc == 0 && rounds_mask) {
        hipError_t e = hipMemcpyAsync(rounds_mask, mask, U * 4, hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) rc = fail(-2, who + ": " + hipGetErrorString(e));
    }
    if (rc == 0) {
        hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = fail(-2, who + ": " + hipGetErrorString(e));
    }
    if (rc) { if (owned) mirge_reads_destroy(owned); return rc; }
    *out = owned;
    return 0;
}

extern "C" int mirge_kmer_correct(mirge_ctx* c, const mirge_reads* uniq, int32_t k_start, int32_t k_end, int32_t threshold, mirge_reads** out,
                                  uint32_t* final_of, uint32_t* rounds_mask) {
    return mirge_kmer_correct_ratio(c, uniq, k_start, k_end, threshold, 0, out, final_of, rounds_mask);
}

// the last mirge_kmer_correct of this thread: out[8 r + 0..7] for round r (k = k_start + r) = eligible, suspect, corrected, uncorrectable,
// unsupported, ambiguous reads, distinct reads after the round, slots of the round's table; returns the number of rounds
extern "C" int mirge_kmer_correct_stats(int64_t* out) {
    if (!out) return fail(-1, "mirge_kmer_correct_stats: bad argument");
    for (int k = 0; k < g_ec_rounds * MIRGE_EC_STAT_WORDS; k++) out[k] = g_ec_stats[k];
    return g_ec_rounds;
}

// out[2 r + 0..1] for round r of this thread's last call = distinct k-mers with a sum above the threshold, the dominated among them (zeros
// when the call had no ratio); returns the number of rounds
extern "C" int mirge_kmer_correct_ratio_stats(int64_t* out) {
    if (!out) return fail(-1, "mirge_kmer_correct_ratio_stats: bad argument");
    for (int k = 0; k < g_ec_rounds * 2; k++) out[k] = g_ec_ratio_stats[k];
    return g_ec_rounds;
}
