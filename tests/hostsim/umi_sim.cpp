// umi_sim.cpp -- the kernels of csrc/kernels_umi.hpp compiled for the HOST (tests/test_umi_cluster_hostsim.py): the same kernel source, the
// threads of a launch one after the other (the kernels have no barrier and no LDS; an atomic is then a plain read-modify-write), the
// launches in the order of csrc/native_umi.hpp (umi_cluster_device).  Running the threads in order is ONE of the interleavings the
// device may take; that the flags do not depend on the interleaving is argued in kernels_umi.hpp and tested on the GPU.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
#define MIRGE_BLOCK 256
struct D3 { unsigned x; };
static D3 threadIdx, blockIdx, blockDim, gridDim;
template <class T> static T atomicCAS(T* p, T expect, T v) { const T o = *p; if (o == expect) *p = v; return o; }
template <class T> static T atomicMin(T* p, T v) { const T o = *p; if (v < o) *p = v; return o; }
template <class T> static T atomicOr(T* p, T v) { const T o = *p; *p |= v; return o; }
template <class T> static T atomicAdd(T* p, T v) { const T o = *p; *p += v; return o; }
#include "../../mirge3.0_amd/csrc/kernels_umi.hpp"

template <class F> static void launch(unsigned grid, unsigned block, F f) {
    gridDim.x = grid; blockDim.x = block;
    for (unsigned b = 0; b < grid; b++)
        for (unsigned t = 0; t < block; t++) { blockIdx.x = b; threadIdx.x = t; f(); }
}

// reads: ASCII, roff[n + 1]; counts, first: per read; founder[n] in the order given; stats[0..3] = founders, eligible, linked, rounds.
// hash_bits < 0: the whole hash.  -> 0, -1 (a bad layout), -3 (the propagation did not settle)
extern "C" int sim_umi_cluster(const char* reads, const int64_t* roff, int64_t n_reads, const uint32_t* counts, const uint32_t* first, int32_t front,
                               int32_t back, int32_t hash_bits, uint8_t* founder, int64_t* stats) {
    if (front < 0 || back < 0 || front + back < 1 || front + back > MIRGE_UMI_MAXTAG) return -1;
    for (int k = 0; k < 4; k++) stats[k] = 0;
    if (n_reads == 0) return 0;
    // the storage groups of csrc/native_reads.hpp: up to 31, 64, 128, 255 nt and longer, without an N; a read with an N is in none of them
    const size_t n = (size_t)n_reads;
    std::vector<int> cls(n);
    std::vector<uint32_t> cnt(MIRGE_UMI_NG + 1, 0), base(MIRGE_UMI_NG + 1, 0), at(MIRGE_UMI_NG + 1, 0), handle(n);
    int64_t longest = 256;
    for (size_t i = 0; i < n; i++) {
        const int64_t L = roff[i + 1] - roff[i];
        bool amb = false;
        for (int64_t p = 0; p < L; p++) { const char ch = reads[roff[i] + p]; amb = amb || !(ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T'); }
        cls[i] = amb ? MIRGE_UMI_NG : (L <= 31 ? 0 : (L <= 64 ? 1 : (L <= 128 ? 2 : (L <= 255 ? 3 : 4))));
        cnt[cls[i]]++;
        longest = std::max(longest, L);
    }
    for (int k = 1; k <= MIRGE_UMI_NG; k++) base[k] = base[k - 1] + cnt[k - 1];
    const int Ws[MIRGE_UMI_NG] = {1, 2, 4, 8, (int)((longest + 31) / 32)};
    std::vector<uint64_t> seq[MIRGE_UMI_NG];
    std::vector<uint8_t> len8[MIRGE_UMI_NG];
    std::vector<uint16_t> len16;
    std::vector<uint32_t> gc[MIRGE_UMI_NG], gf[MIRGE_UMI_NG];
    for (int k = 0; k < MIRGE_UMI_NG; k++) { seq[k].assign((size_t)Ws[k] * cnt[k] + 1, 0ull); len8[k].assign(cnt[k] + 1, 0); gc[k].assign(cnt[k] + 1, 0); gf[k].assign(cnt[k] + 1, 0); }
    len16.assign(cnt[4] + 1, 0);
    for (size_t i = 0; i < n; i++) {
        const int k = cls[i];
        const uint32_t j = at[k]++;
        handle[i] = base[k] + j;
        if (k == MIRGE_UMI_NG) continue;
        const int64_t L = roff[i + 1] - roff[i];
        for (int64_t p = 0; p < L; p++) {
            const char ch = reads[roff[i] + p];
            const uint64_t code = ch == 'A' ? 0 : (ch == 'C' ? 1 : (ch == 'G' ? 2 : 3));
            seq[k][(size_t)(p >> 5) * cnt[k] + j] |= code << (2 * (p & 31));
        }
        if (k == 4) len16[j] = (uint16_t)L; else len8[k][j] = (uint8_t)L;
        gc[k][j] = counts[i]; gf[k][j] = first[i];
    }
    UmiView v;
    std::memset(&v, 0, sizeof(v));
    for (int k = 0; k < MIRGE_UMI_NG; k++)
        if (cnt[k]) v.g[k] = UmiGroup{seq[k].data(), k == 4 ? reinterpret_cast<const uint8_t*>(len16.data()) : len8[k].data(), gc[k].data(), gf[k].data(), base[k], cnt[k], k == 4, 0};
    v.front = front; v.back = back; v.n_nodes = (uint32_t)n;
    v.hash_keep = hash_bits < 0 || hash_bits > 63 ? ~0ull : (1ull << hash_bits) - 1;
    uint64_t slots = 256;
    while (slots < 2 * (uint64_t)n) slots <<= 1;
    v.tab_mask = slots - 1;
    std::vector<uint64_t> tab((size_t)slots, MIRGE_UMI_EMPTY), label(n, MIRGE_UMI_EMPTY);
    std::vector<uint32_t> state(n, 0);
    std::vector<uint8_t> fo(n, 0);
    uint32_t words[4] = {0, 0, 0, 0};
    const unsigned grid = (unsigned)std::min<size_t>((n + MIRGE_BLOCK - 1) / MIRGE_BLOCK, 3);  // (grid-stride loops: a few workgroups do)
    launch(grid, MIRGE_BLOCK, [&] { k_umi_insert(v, tab.data(), state.data()); });
    launch(grid, MIRGE_BLOCK, [&] { k_umi_edges(v, tab.data(), state.data(), label.data()); });
    int64_t rounds = 0;
    for (;;) {
        words[0] = 0;
        launch(grid, MIRGE_BLOCK, [&] { k_umi_round(v, tab.data(), state.data(), label.data(), words); });
        rounds++;
        if (!words[0]) break;
        if (rounds > (int64_t)n + 1) return -3;
    }
    launch(grid, MIRGE_BLOCK, [&] { k_umi_comp_big(v, state.data(), label.data()); });
    launch(grid, MIRGE_BLOCK, [&] { k_umi_founders(v, state.data(), label.data(), fo.data(), words); });
    for (size_t i = 0; i < n; i++) founder[i] = fo[handle[i]];
    stats[0] = words[1]; stats[1] = words[2]; stats[2] = words[3]; stats[3] = rounds;
    return 0;
}
