// native_adapter.hpp -- part of mirge_native.hip (one translation unit): -a auto (kernels_adapter.hpp): mirge_adapter_infer, one call per sample on
// the dictionary of its head's untrimmed reads: the table over all 4^12 codes (256 MiB from the call's PoolScope, cleared per call),
// filled by the store-and-sum form (k_ad_nwin, a scan, k_ad_keys, one sort, k_ad_fold) or the atomic one (k_ad_count), then k_ad_seed +
// k_ad_seed_last, k_ad_walk, and for tests the slots of listed codes (k_ad_probe).
#pragma once

#ifndef MIRGE_AD_DEFAULT_SORT
#define MIRGE_AD_DEFAULT_SORT 1  // the store-and-sum form fills the table unless MIRGE_ADAPTER_COUNT says otherwise (profiles/adapter_auto.md)
#endif

static_assert(sizeof(AdResult) == sizeof(mirge_adapter) && offsetof(AdResult, support) == offsetof(mirge_adapter, support) &&
              offsetof(AdResult, seed) == offsetof(mirge_adapter, seed) && offsetof(AdResult, len) == offsetof(mirge_adapter, len),
              "AdResult is mirge_adapter");

extern "C" int mirge_adapter_infer(mirge_ctx* c, const mirge_reads* uniq, mirge_adapter* out, const uint32_t* probe, int64_t n_probe,
                                   uint64_t* probe_sum, uint64_t* probe_mask) {
    const std::string who = "mirge_adapter_infer";
    if (!c || !uniq || uniq->ctx != c || !out) return fail(-1, who + ": bad argument");
    if (n_probe < 0 || n_probe > 0x7FFFFFF0ll || (n_probe && (!probe || !probe_sum || !probe_mask))) return fail(-1, who + ": bad probe list");
    if (uniq->n_samples > 1) return fail(-1, who + ": the reads must be a collapse result with one count column");
    if (uniq->n >= 0x7FFFFFF0ll) return fail(-5, who + ": too many reads for one call");
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    std::memset(out, 0, sizeof(*out));
    if (uniq->n == 0) {  // no adapter, T = 0; no window spells anything
        for (int64_t q = 0; q < n_probe; q++) probe_sum[q] = probe_mask[q] = 0;
        return 0;
    }
    AdResult r;  // (before the scope: its wait ends the copies into these)
    unsigned long long over = 0;
    EcView v;
    CHECK(ec_view_of(who, uniq, v));  // (refuses what is no collapse result)
    v.k = MIRGE_AD_K;
    // an upper bound on the windows from the lengths alone (the lengths of the reads with an N count too): the store-and-sum form's arrays
    uint64_t bound = 0;
    if (uniq->hist_valid)
        for (int L = MIRGE_AD_K; L <= MIRGE_MAX_READ_LEN; L++) bound += (uint64_t)uniq->len_hist[L] * (uint64_t)std::min(L - MIRGE_AD_K + 1, MIRGE_AD_P);
    else
        for (int gi = 0; gi < MIRGE_EC_NG - 1; gi++)
            bound += (uint64_t)uniq->g[gi].n * (uint64_t)std::min(std::min(32 * uniq->g[gi].W, MIRGE_MAX_READ_LEN) - MIRGE_AD_K + 1, MIRGE_AD_P);
    bound += (uint64_t)uniq->g[MIRGE_EC_NG - 1].n * (uint64_t)MIRGE_AD_P;
    // MIRGE_ADAPTER_COUNT=atomic | sort (read per call; A/B and tests): how the table is filled.  Dictionaries of 2^31 windows and more: atomic.
    const char* const form = std::getenv("MIRGE_ADAPTER_COUNT");
    if (form && std::strcmp(form, "atomic") && std::strcmp(form, "sort")) return fail(-1, who + ": MIRGE_ADAPTER_COUNT is atomic or sort");
    const bool by_sort = (form ? !std::strcmp(form, "sort") : MIRGE_AD_DEFAULT_SORT) && bound > 0 && bound < 0x7FFFFFF0ull;
    PoolScope scope(c);
    AdSlot* tab;
    unsigned long long *words, *part_n;  // words[0] = T, words[1] = candidates, words[2] != 0: the window bound did not hold
    AdBest *part, *seed;
    AdResult* res;
    uint32_t* dprobe = nullptr;
    uint64_t *dsum = nullptr, *dmask = nullptr;
    const int seed_grid = grid_for(c, (size_t)MIRGE_AD_SLOTS);
    CHECK(scope.get(&tab, (size_t)MIRGE_AD_SLOTS)); CHECK(scope.get(&words, (size_t)3)); CHECK(scope.get(&part, (size_t)seed_grid));
    CHECK(scope.get(&part_n, (size_t)seed_grid)); CHECK(scope.get(&seed, (size_t)1)); CHECK(scope.get(&res, (size_t)1));
    if (n_probe) { CHECK(scope.get(&dprobe, (size_t)n_probe)); CHECK(scope.get(&dsum, (size_t)n_probe)); CHECK(scope.get(&dmask, (size_t)n_probe)); }
    const dim3 block(MIRGE_BLOCK);
    { LaunchScope ls(c, "k_ad_clear", (double)MIRGE_AD_SLOTS); HIPOK(hipMemsetAsync(tab, 0, (size_t)MIRGE_AD_SLOTS * sizeof(AdSlot), c->stream)); }
    HIPOK(hipMemsetAsync(words, 0, 3 * sizeof(*words), c->stream));
    if (n_probe) HIPOK(hipMemcpyAsync(dprobe, probe, (size_t)n_probe * 4, hipMemcpyHostToDevice, c->stream));
    if (!by_sort) {
        LaunchScope ls(c, "k_ad_count", (double)uniq->n);
        hipLaunchKernelGGL(k_ad_count, dim3(grid_for(c, (size_t)uniq->n)), block, 0, c->stream, v, tab, words);
    } else {
        const size_t n = (size_t)uniq->n;
        uint32_t *nwin, *off, *keys, *keys2, *wts, *wts2;
        void *tmp_scan = nullptr, *tmp_sort = nullptr;
        size_t scan_bytes = 0, sort_bytes = 0;
        CHECK(scope.get(&nwin, n)); CHECK(scope.get(&off, n)); CHECK(scope.get(&keys, (size_t)bound)); CHECK(scope.get(&keys2, (size_t)bound));
        CHECK(scope.get(&wts, (size_t)bound)); CHECK(scope.get(&wts2, (size_t)bound));
        HIPOK(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (const uint32_t*)nwin, off, (int)n, c->stream));
        HIPOK(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (const uint32_t*)keys, keys2, (const uint32_t*)wts, wts2, (int)bound, 0, 32, c->stream));
        CHECK(scope.get((uint8_t**)&tmp_scan, std::max<size_t>(scan_bytes, 16))); CHECK(scope.get((uint8_t**)&tmp_sort, std::max<size_t>(sort_bytes, 16)));
        HIPOK(hipMemsetAsync(keys, 0xFF, (size_t)bound * 4, c->stream));  // (MIRGE_AD_NOKEY: what no window writes sorts last)
        { LaunchScope ls(c, "k_ad_nwin", (double)n); hipLaunchKernelGGL(k_ad_nwin, dim3(grid_for(c, n)), block, 0, c->stream, v, nwin, words); }
        { LaunchScope ls(c, "k_ad_scan", (double)n);
          HIPOK(hipcub::DeviceScan::ExclusiveSum(tmp_scan, scan_bytes, (const uint32_t*)nwin, off, (int)n, c->stream)); }
        { LaunchScope ls(c, "k_ad_keys", (double)n);
          hipLaunchKernelGGL(k_ad_keys, dim3(grid_for(c, n)), block, 0, c->stream, v, (const uint32_t*)off, (const uint32_t*)nwin, (uint32_t)bound, keys,
                             wts, words + 2); }
        { LaunchScope ls(c, "k_ad_sort", (double)bound);
          HIPOK(hipcub::DeviceRadixSort::SortPairs(tmp_sort, sort_bytes, (const uint32_t*)keys, keys2, (const uint32_t*)wts, wts2, (int)bound, 0, 32, c->stream)); }
        { LaunchScope ls(c, "k_ad_fold", (double)bound);
          hipLaunchKernelGGL(k_ad_fold, dim3(grid_for(c, (size_t)((bound + MIRGE_AD_FOLD - 1) / MIRGE_AD_FOLD))), block, 0, c->stream, (const uint32_t*)keys2,
                             (const uint32_t*)wts2, (uint32_t)bound, tab); }
    }
    { LaunchScope ls(c, "k_ad_seed", (double)MIRGE_AD_SLOTS);
      hipLaunchKernelGGL(k_ad_seed, dim3(seed_grid), block, 0, c->stream, (const AdSlot*)tab, (const unsigned long long*)words, part, part_n); }
    { LaunchScope ls(c, "k_ad_seed_last", (double)seed_grid);
      hipLaunchKernelGGL(k_ad_seed_last, dim3(1), block, 0, c->stream, (const AdBest*)part, (const unsigned long long*)part_n, (uint32_t)seed_grid, seed,
                         words + 1); }
    { LaunchScope ls(c, "k_ad_walk", 1.0);
      hipLaunchKernelGGL(k_ad_walk, dim3(1), dim3(64), 0, c->stream, (const AdSlot*)tab, (const AdBest*)seed, (const unsigned long long*)(words + 1),
                         (const unsigned long long*)words, res); }
    if (n_probe) {
        hipLaunchKernelGGL(k_ad_probe, dim3(grid_for(c, (size_t)n_probe)), block, 0, c->stream, (const AdSlot*)tab, (const uint32_t*)dprobe, (uint32_t)n_probe,
                           dsum, dmask);
        HIPOK(hipMemcpyAsync(probe_sum, dsum, (size_t)n_probe * 8, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipMemcpyAsync(probe_mask, dmask, (size_t)n_probe * 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIPOK(hipMemcpyAsync(&r, res, sizeof(r), hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(&over, words + 2, sizeof(over), hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    HIPOK(hipGetLastError());
    if (over) return fail(-3, who + ": more windows than the reads' lengths allow");
    std::memcpy(out, &r, sizeof(r));
    out->seq[sizeof(out->seq) - 1] = 0;
    return 0;
}
