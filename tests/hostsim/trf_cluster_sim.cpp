// trf_cluster_sim.cpp -- the clustering kernels of csrc/kernels_trf.hpp compiled for the HOST (tests/test_trf_clusters_hostsim.py): the
// same kernel source, a workgroup's threads as std::threads behind a barrier, workgroups one after the other, LDS as statics.  The
// tile list and the order of the launches are those of csrc/native_trf.hpp (mirge_trf_cluster), and the O(n) steps between the
// launches are the same functions (trf_cluster_assign, trf_cluster_halo).  Built with -ffp-contract=off: trf_mul_add's pragma is
// clang's.  The runtime itself and the real device are the GPU tests' business.
#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
#define __shared__ static
#define MIRGE_TRF_CLUSTER_SIM 1
#define MIRGE_BLOCK 256
struct D3 { unsigned x; };
static thread_local D3 threadIdx;
static D3 blockIdx, blockDim, gridDim;
struct Barrier {
    std::mutex m; std::condition_variable cv; int n, count = 0, gen = 0;
    void wait() { std::unique_lock<std::mutex> l(m); int g = gen; if (++count == n) { gen++; count = 0; cv.notify_all(); } else cv.wait(l, [&] { return g != gen; }); }
};
static Barrier* g_bar;
static void __syncthreads() { g_bar->wait(); }
static int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
static std::mutex g_am;
template <class T> T atomicOr(T* p, T v) { std::lock_guard<std::mutex> l(g_am); T o = *p; *p |= v; return o; }
#include "../../mirge3.0_amd/csrc/mirge_core.hpp"
#include "../../mirge3.0_amd/csrc/kernels_trf.hpp"

template <class F> static void launch(unsigned grid, unsigned block, F f) {
    gridDim.x = grid; blockDim.x = block;
    for (unsigned b = 0; b < grid; b++) {
        blockIdx.x = b;
        Barrier bar; bar.n = (int)block; g_bar = &bar;
        std::vector<std::thread> th;
        for (unsigned t = 0; t < block; t++) th.emplace_back([&, t] { threadIdx.x = t; f(); });
        for (auto& x : th) x.join();
    }
}

// the reads as four width groups (up to 31, 64, 128, 255 nt), word-major, as csrc/native_reads.hpp holds them
struct SimReads {
    std::vector<uint64_t> seq[4], nm[4];
    std::vector<uint8_t> len[4];
    std::vector<uint32_t> handle;
    int fill(const char* reads, const int64_t* roff, int64_t n, TrfTables& t) {
        static const int Ws[4] = {1, 2, 4, 8};
        std::vector<uint32_t> cnt(4, 0), at(4, 0), base(4, 0);
        std::vector<int> cls((size_t)n);
        for (int64_t i = 0; i < n; i++) {
            const int64_t L = roff[i + 1] - roff[i];
            if (L < 1 || L > 255) return -6;
            cls[(size_t)i] = L <= 31 ? 0 : (L <= 64 ? 1 : (L <= 128 ? 2 : 3));
            cnt[cls[(size_t)i]]++;
        }
        for (int k = 1; k < 4; k++) base[k] = base[k - 1] + cnt[k - 1];
        handle.resize((size_t)n);
        for (int k = 0; k < 4; k++) {
            seq[k].assign((size_t)Ws[k] * cnt[k] + 1, 0ull); nm[k].assign((size_t)Ws[k] * cnt[k] + 1, 0ull); len[k].assign(cnt[k] + 1, 0);
        }
        for (int64_t i = 0; i < n; i++) {
            const int k = cls[(size_t)i];
            const uint32_t j = at[k]++;
            const int L = (int)(roff[i + 1] - roff[i]);
            for (int p = 0; p < L; p++) {
                const char ch = reads[roff[i] + p];
                const int code = ch == 'A' ? 0 : (ch == 'C' ? 1 : (ch == 'G' ? 2 : (ch == 'T' ? 3 : -1)));
                const size_t w = (size_t)(p >> 5) * cnt[k] + j;
                if (code < 0) nm[k][w] |= 1ull << (2 * (p & 31));
                else seq[k][w] |= (uint64_t)code << (2 * (p & 31));
            }
            len[k][j] = (uint8_t)L;
            handle[(size_t)i] = base[k] + j;
        }
        for (int k = 0; k < 4; k++) t.g[k] = TrfGroup{seq[k].data(), nm[k].data(), len[k].data(), nullptr, nullptr, nullptr, base[k], cnt[k], Ws[k], 0};
        return 0;
    }
};

// read[] indexes the reads given here.  -> 0, or < 0 (-100 - flags: the pack kernel refused a point)
extern "C" int sim_trf_cluster(const char* reads, const int64_t* roff, int64_t n_reads, int64_t n_grp, const int64_t* grp_ptr, const int64_t* read,
                               const int32_t* off, const double* rp, const int32_t* tlen, int64_t n_gauss, const double* gauss, float* rho,
                               float* delta, int32_t* nneigh, int32_t* order, int32_t* cl, int32_t* halo, int32_t* nclust, int32_t* centre) {
    TrfTables t;
    std::memset(&t, 0, sizeof(t));
    SimReads R;
    if (int rc = R.fill(reads, roff, n_reads, t)) return rc;
    const size_t n = (size_t)grp_ptr[n_grp], ng = (size_t)n_grp;
    std::vector<uint32_t> r32(n + 1), p32(ng + 1, 0), tile_grp, tile_first;
    std::vector<int32_t> pt_tlen(n + 1);
    uint32_t n_tile[2] = {0, 0};
    for (size_t k = 0; k < n; k++) r32[k] = R.handle[(size_t)read[k]];
    for (int pass = 0; pass < 2; pass++)
        for (size_t g = 0; g < ng; g++) {
            p32[g + 1] = (uint32_t)grp_ptr[g + 1];
            if (tlen[g] < 1 || tlen[g] > MIRGE_TRF_CL_MAXCOL) return -3;
            if ((tlen[g] > 128) != (pass == 1)) continue;
            for (int64_t k = grp_ptr[g]; k < grp_ptr[g + 1]; k++) pt_tlen[(size_t)k] = tlen[g];
            for (int64_t f = grp_ptr[g]; f < grp_ptr[g + 1]; f += MIRGE_BLOCK) { tile_grp.push_back((uint32_t)g); tile_first.push_back((uint32_t)f); n_tile[pass]++; }
        }
    if (n == 0) { for (size_t g = 0; g < ng; g++) nclust[g] = 0; return 0; }
    std::vector<uint64_t> words(n * 2 * MIRGE_TRF_CL_MAXW, ~0ull);
    std::vector<int32_t> start(n), end(n), cen(n), dcen(n);
    std::vector<float> bmax(n);
    uint32_t flags[16] = {0};
    launch(3, 64, [&] { k_trf_cluster_pack(t, r32.data(), off, pt_tlen.data(), (uint32_t)n, words.data(), start.data(), end.data(), flags); });
    if (flags[0]) return -100 - (int)flags[0];
    tile_grp.push_back(0); tile_first.push_back(0);
    TrfClusterView v{words.data(), start.data(), end.data(), rp, p32.data(), tile_grp.data(), tile_first.data(), gauss, (int32_t)n_gauss, 0};
    if (n_tile[0]) launch(n_tile[0], MIRGE_BLOCK, [&] { k_trf_density<4>(v, 0u, rho); });
    if (n_tile[1]) launch(n_tile[1], MIRGE_BLOCK, [&] { k_trf_density<8>(v, n_tile[0], rho); });
    if (n_tile[0]) launch(n_tile[0], MIRGE_BLOCK, [&] { k_trf_nearest<4>(v, 0u, rho, delta, nneigh, order); });
    if (n_tile[1]) launch(n_tile[1], MIRGE_BLOCK, [&] { k_trf_nearest<8>(v, n_tile[0], rho, delta, nneigh, order); });
    if (trf_cluster_assign(n_grp, grp_ptr, rho, delta, nneigh, order, cl, centre, nclust, cen.data())) return -4;
    if (n_tile[0]) launch(n_tile[0], MIRGE_BLOCK, [&] { k_trf_border<4>(v, 0u, rho, cl, cen.data(), nclust, bmax.data(), dcen.data()); });
    if (n_tile[1]) launch(n_tile[1], MIRGE_BLOCK, [&] { k_trf_border<8>(v, n_tile[0], rho, cl, cen.data(), nclust, bmax.data(), dcen.data()); });
    trf_cluster_halo(n_grp, grp_ptr, rho, cl, nclust, bmax.data(), dcen.data(), halo);
    return 0;
}
