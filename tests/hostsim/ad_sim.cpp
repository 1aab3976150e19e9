// ad_sim.cpp -- the kernels of csrc/kernels_adapter.hpp compiled for the HOST (tests/test_adapter_auto_hostsim.py): the same kernel source, the
// threads of a launch one after the other (an atomic is then a plain read-modify-write), the workgroup reductions and the four lanes of
// a walk step as the loops MIRGE_AD_HOSTSIM makes of them, the launches in the order of csrc/native_adapter.hpp: clear, k_ad_count,
// k_ad_seed, k_ad_seed_last, k_ad_walk, k_ad_probe; with by_sort k_ad_nwin, the scan, k_ad_keys, the sort and k_ad_fold fill the table
// (scan and sort are the host's).  The reads are packed as the device stores them (csrc/kernels_ec.hpp: EcView).
// With -DAD_SIM_MAIN a stand-alone program over generated sets, for a sanitizer build of this host code.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
#define MIRGE_BLOCK 256
#define MIRGE_EC_HOSTSIM 1
#define MIRGE_AD_HOSTSIM 1
struct D3 { unsigned x; };
static D3 threadIdx, blockIdx, blockDim, gridDim;
template <class T> static T atomicCAS(T* p, T expect, T v) { const T o = *p; if (o == expect) *p = v; return o; }
template <class T> static T atomicAdd(T* p, T v) { const T o = *p; *p += v; return o; }
template <class T> static T atomicOr(T* p, T v) { const T o = *p; *p |= v; return o; }
static inline int __popc(unsigned x) { return __builtin_popcount(x); }
static inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }
#include "../../mirge3.0_amd/csrc/kernels_ec.hpp"
#include "../../mirge3.0_amd/csrc/kernels_adapter.hpp"

template <class F> static void launch(unsigned grid, unsigned block, F f) {
    gridDim.x = grid; blockDim.x = block;
    for (unsigned b = 0; b < grid; b++)
        for (unsigned t = 0; t < block; t++) { blockIdx.x = b; threadIdx.x = t; f(); }
}

static std::vector<AdSlot> g_tab;  // 4^12 slots, allocated once

// reads: ASCII, roff[n + 1]; counts per read.  seed_grid: workgroups of k_ad_seed (few: its grid-stride loop runs; 65536: one slot per
// thread).  by_sort: the store-and-sum form fills the table, else the atomic one.  out: the fields of mirge_adapter; psum / pmask: C and M
// of the n_probe listed codes.  -> 0 (-3: the window bound did not hold)
extern "C" int sim_adapter_infer(const char* reads, const int64_t* roff, int64_t n_reads, const uint32_t* counts, int32_t seed_grid, int32_t by_sort, AdResult* out,
                                 const uint32_t* probe, int64_t n_probe, uint64_t* psum, uint64_t* pmask) {
    const size_t n = (size_t)n_reads;
    std::vector<std::string> D(n);
    for (size_t i = 0; i < n; i++) D[i].assign(reads + roff[i], (size_t)(roff[i + 1] - roff[i]));
    std::vector<int> cls(n);
    std::vector<uint32_t> cnt(MIRGE_EC_NG + 1, 0), base(MIRGE_EC_NG + 1, 0), at(MIRGE_EC_NG + 1, 0);
    size_t longest = 256;
    for (size_t i = 0; i < n; i++) {
        const size_t L = D[i].size();
        const bool amb = D[i].find_first_not_of("ACGT") != std::string::npos;
        cls[i] = amb ? MIRGE_EC_NG : (L <= 31 ? 0 : (L <= 64 ? 1 : (L <= 128 ? 2 : (L <= 255 ? 3 : 4))));
        cnt[cls[i]]++;
        longest = std::max(longest, L);
    }
    for (int q = 1; q <= MIRGE_EC_NG; q++) base[q] = base[q - 1] + cnt[q - 1];
    const int Ws[MIRGE_EC_NG] = {1, 2, 4, 8, (int)((longest + 31) / 32)};
    std::vector<uint64_t> seq[MIRGE_EC_NG];
    std::vector<uint8_t> len8[MIRGE_EC_NG];
    std::vector<uint16_t> len16(cnt[4] + 1, 0);
    std::vector<uint32_t> gc[MIRGE_EC_NG];
    for (int q = 0; q < MIRGE_EC_NG; q++) { seq[q].assign((size_t)Ws[q] * cnt[q] + 1, 0ull); len8[q].assign(cnt[q] + 1, 0); gc[q].assign(cnt[q] + 1, 0); }
    for (size_t i = 0; i < n; i++) {
        const int q = cls[i];
        const uint32_t j = at[q]++;
        if (q == MIRGE_EC_NG) continue;
        const std::string& r = D[i];
        for (size_t p = 0; p < r.size(); p++) {
            const char ch = r[p];
            const uint64_t code = ch == 'A' ? 0 : (ch == 'C' ? 1 : (ch == 'G' ? 2 : 3));
            seq[q][(p >> 5) * cnt[q] + j] |= code << (2 * (p & 31));
        }
        if (q == 4) len16[j] = (uint16_t)r.size(); else len8[q][j] = (uint8_t)r.size();
        gc[q][j] = counts[i];
    }
    EcView v;
    std::memset(&v, 0, sizeof(v));
    for (int q = 0; q < MIRGE_EC_NG; q++)
        if (cnt[q]) v.g[q] = EcGroup{seq[q].data(), q == 4 ? reinterpret_cast<const uint8_t*>(len16.data()) : len8[q].data(), gc[q].data(), base[q], cnt[q], (uint32_t)Ws[q], q == 4};
    v.n_reads = (uint32_t)n; v.k = MIRGE_AD_K;
    if (g_tab.empty()) g_tab.resize((size_t)MIRGE_AD_SLOTS);
    std::memset(g_tab.data(), 0, g_tab.size() * sizeof(AdSlot));
    unsigned long long words[2] = {0, 0};
    const unsigned sg = (unsigned)std::max(1, seed_grid);
    std::vector<AdBest> part(sg);
    std::vector<unsigned long long> part_n(sg);
    AdBest seed;
    std::memset(out, 0, sizeof(*out));
    const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>((n + MIRGE_BLOCK - 1) / MIRGE_BLOCK, 3));  // (grid-stride loops: a few workgroups do)
    if (!by_sort) launch(grid, MIRGE_BLOCK, [&] { k_ad_count(v, g_tab.data(), &words[0]); });
    else {  // the store-and-sum form: the scan and the sort are the host's
        uint64_t bound = 0;
        for (size_t i = 0; i < n; i++) bound += D[i].size() >= MIRGE_AD_K ? std::min<size_t>(D[i].size() - MIRGE_AD_K + 1, MIRGE_AD_P) : 0;  // (from the lengths alone)
        std::vector<uint32_t> nwin(n + 1, 7), off(n + 1, 0), keys((size_t)bound + 1, MIRGE_AD_NOKEY), wts((size_t)bound + 1, 7);
        unsigned long long over = 0;
        launch(grid, MIRGE_BLOCK, [&] { k_ad_nwin(v, nwin.data(), &words[0]); });
        for (size_t i = 1; i < n; i++) off[i] = off[i - 1] + nwin[i - 1];
        launch(grid, MIRGE_BLOCK, [&] { k_ad_keys(v, off.data(), nwin.data(), (uint32_t)bound, keys.data(), wts.data(), &over); });
        if (over) return -3;
        std::vector<std::pair<uint32_t, uint32_t>> kv((size_t)bound);
        for (size_t e = 0; e < (size_t)bound; e++) kv[e] = {keys[e], wts[e]};
        std::sort(kv.begin(), kv.end());
        for (size_t e = 0; e < (size_t)bound; e++) { keys[e] = kv[e].first; wts[e] = kv[e].second; }
        if (bound) launch(2, MIRGE_BLOCK, [&] { k_ad_fold(keys.data(), wts.data(), (uint32_t)bound, g_tab.data()); });
    }
    launch(sg, MIRGE_BLOCK, [&] { k_ad_seed(g_tab.data(), &words[0], part.data(), part_n.data()); });
    launch(1, MIRGE_BLOCK, [&] { k_ad_seed_last(part.data(), part_n.data(), sg, &seed, &words[1]); });
    launch(1, 64, [&] { k_ad_walk(g_tab.data(), &seed, &words[1], &words[0], out); });
    if (n_probe) launch(2, MIRGE_BLOCK, [&] { k_ad_probe(g_tab.data(), probe, (uint32_t)n_probe, psum, pmask); });
    return 0;
}

#ifdef AD_SIM_MAIN
int main() {
    uint64_t state = 2024, sum = 0;
    auto rnd = [&](uint64_t m) { state = state * 6364136223846793005ull + 1442695040888963407ull; return (state >> 33) % m; };
    int found = 0;
    for (int set = 0; set < 12; set++) {
        const int letters = set % 3 == 0 ? 2 : 4;
        std::string core(16 + rnd(30), 'A');
        for (char& ch : core) ch = "ACGT"[rnd(letters)];
        core[rnd(12)] = 'G'; core[rnd(12)] = 'T';
        std::map<std::string, uint32_t> seen;
        const size_t lens[] = {12, 13, 31, 32, 33, 63, 64, 65, 128, 129, 255, 256, 257, 11};
        for (int t = 0; t < 40; t++) {
            std::string r(rnd(30), 'A');
            for (char& ch : r) ch = "ACGT"[rnd(letters)];
            r += core;
            if (rnd(3) == 0) r.resize(std::max<size_t>(1, r.size() - rnd(10)));
            if (rnd(10) == 0) r[rnd(r.size())] = 'N';
            if (rnd(4) == 0) { const size_t L = lens[rnd(14)]; while (r.size() < L) r += "ACGT"[rnd(4)]; r.resize(L); }
            seen.emplace(r, (uint32_t)(1 + rnd(40)));
        }
        std::string text;
        std::vector<int64_t> off{0};
        std::vector<uint32_t> counts, probe;
        for (const auto& s : seen) { text += s.first; off.push_back((int64_t)text.size()); counts.push_back(s.second); }
        for (int q = 0; q < 100; q++) probe.push_back((uint32_t)rnd(1u << 25));
        std::vector<uint64_t> ps(probe.size()), pm(probe.size());
        AdResult res;
        if (sim_adapter_infer(text.data(), off.data(), (int64_t)counts.size(), counts.data(), set % 2 ? 5 : 4096, (set / 2) % 2, &res, probe.data(), (int64_t)probe.size(), ps.data(),
                              pm.data()))
            return 1;
        found += res.len > 0;
        sum += res.support + res.eligible + res.candidates + (uint64_t)res.len + std::strlen(res.seq);
        for (size_t q = 0; q < probe.size(); q++) sum += ps[q] + pm[q];
    }
    std::printf("ad_sim: 12 sets, %d with an adapter, checksum %llu\n", found, (unsigned long long)sum);
    return 0;
}
#endif
