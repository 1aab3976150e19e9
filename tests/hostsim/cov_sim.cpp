// cov_sim.cpp -- csrc/kernels_cov.hpp compiled for the HOST (tests/test_coverage_hostsim.py): the same kernel source, the launches in the
// order of csrc/native_cov.hpp (CovDev::runs, CovDev::measure, the chunk loop).  The kernels without a barrier run a launch's threads
// one after the other (an atomic is then a plain read-modify-write); k_cov_write, which fills an LDS tile behind a barrier, runs a
// workgroup's threads as std::threads.  hipCUB's sort and scans are std::sort and loops.  Built with -DCOV_SIM_MAIN it is a program
// of its own (a fixed set of intervals through both modes) for an ASan / UBSan build of this file.
#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <numeric>
#include <thread>
#include <vector>
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
#define __shared__ static
#define MIRGE_BLOCK 256
#define MIRGE_COV_NO_SAM
struct D3 { unsigned x; };
static thread_local D3 threadIdx;
static D3 blockIdx, blockDim, gridDim;
struct uint4 { uint32_t x, y, z, w; };
struct Barrier {
    std::mutex m; std::condition_variable cv; int n = 1, count = 0, gen = 0;
    void wait() { std::unique_lock<std::mutex> l(m); const int g = gen; if (++count == n) { gen++; count = 0; cv.notify_all(); } else cv.wait(l, [&] { return g != gen; }); }
};
static Barrier* g_bar = nullptr;
static void __syncthreads() { g_bar->wait(); }
template <class T> static T atomicOr(T* p, T v) { const T o = *p; *p |= v; return o; }
template <class T> static T atomicAdd(T* p, T v) { const T o = *p; *p += v; return o; }
#include "../../mirge3.0_amd/csrc/kernels_cov.hpp"

template <class F> static void launch(unsigned grid, unsigned block, F f) {  // kernels without a barrier
    gridDim.x = grid; blockDim.x = block;
    for (unsigned b = 0; b < grid; b++)
        for (unsigned t = 0; t < block; t++) { blockIdx.x = b; threadIdx.x = t; f(); }
}
template <class F> static void launch_threads(unsigned grid, unsigned block, F f) {  // workgroups one after the other, their threads together
    gridDim.x = grid; blockDim.x = block;
    for (unsigned b = 0; b < grid; b++) {
        blockIdx.x = b;
        Barrier bar; bar.n = (int)block; g_bar = &bar;
        std::vector<std::thread> th;
        for (unsigned t = 0; t < block; t++) th.emplace_back([&, t] { threadIdx.x = t; f(); });
        for (auto& x : th) x.join();
    }
}
static unsigned grid_of(size_t n) { return (unsigned)std::min<size_t>((n + MIRGE_BLOCK - 1) / MIRGE_BLOCK, 3); }  // (grid-stride loops: a few workgroups do)

// flag[0 .. m) -> pos (exclusive sum), the number of flags set
static uint32_t count_flags(const std::vector<uint32_t>& flag, std::vector<uint32_t>& pos, size_t m) {
    uint32_t s = 0;
    for (size_t i = 0; i < m; i++) { pos[i] = s; s += flag[i]; }
    pos[m] = s;
    return s;
}

// n intervals -> the runs (capacity 2 n + 1 each) and, when names are given, the text (capacity text_cap): tile / chunk as
// MIRGE_COV_TILE_BYTES / MIRGE_COV_CHUNK_BYTES after the clamping of native_cov.hpp.  stats[0..4] = runs, runs of the plus strand, summed
// weight, bytes, bytes of the plus strand.  -> 0, -1 (an interval outside the contract), -3 (a sum below 0 or not back at 0), -2 (text_cap)
extern "C" int sim_coverage(int64_t n64, const int32_t* rank, const int64_t* start, const int32_t* len, const uint32_t* weight, const uint8_t* minus,
                            int32_t n_rank, int32_t stranded, uint8_t* run_strand, int32_t* run_chrom, int64_t* run_start, int64_t* run_end,
                            int64_t* run_depth, const char* name_data, const int64_t* name_off, uint32_t tile, uint32_t chunk, uint8_t* text_out,
                            int64_t text_cap, int64_t* stats) {
    for (int k = 0; k < 5; k++) stats[k] = 0;
    const size_t n = (size_t)n64, m = 2 * n;
    if (n == 0) return 0;
    int rbits = 0;
    while ((1ull << rbits) < (unsigned long long)n_rank) rbits++;
    const int strand_shift = MIRGE_COV_POS_BITS + rbits;
    std::vector<long long> st(start, start + n);
    const CovIntervals iv{rank, st.data(), len, weight, minus};
    std::vector<unsigned long long> kA(m), kB(m);
    std::vector<long long> vA(m), vB(m);
    std::vector<uint32_t> flag(m + 1, 0), pos(m + 1, 0);
    uint32_t words[4] = {0, 0, 0, 0};
    unsigned long long sum = 0;
    launch(grid_of(n), MIRGE_BLOCK, [&] { k_cov_events(iv, (uint32_t)n, (uint32_t)n_rank, stranded ? 1 : 0, strand_shift, kA.data(), vA.data(), words, &sum); });
    if (words[0] & 1u) return -1;
    std::vector<uint32_t> perm(m);
    std::iota(perm.begin(), perm.end(), 0u);
    std::sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return kA[a] < kA[b]; });  // (not stable on purpose: integer sums commute)
    for (size_t i = 0; i < m; i++) { kB[i] = kA[perm[i]]; vB[i] = vA[perm[i]]; }
    long long run = 0;
    for (size_t i = 0; i < m; i++) { run += vB[i]; vA[i] = run; }
    launch(grid_of(m), MIRGE_BLOCK, [&] { k_cov_last(kB.data(), (uint32_t)m, flag.data()); });
    const uint32_t n1 = count_flags(flag, pos, m);
    launch(grid_of(m), MIRGE_BLOCK, [&] { k_cov_scatter(kB.data(), vA.data(), flag.data(), pos.data(), (uint32_t)m, kA.data(), vB.data()); });
    launch(grid_of(n1), MIRGE_BLOCK, [&] { k_cov_change(vB.data(), n1, flag.data()); });
    const uint32_t n2 = count_flags(flag, pos, n1);
    launch(grid_of(n1), MIRGE_BLOCK, [&] { k_cov_scatter(kA.data(), vB.data(), flag.data(), pos.data(), n1, kB.data(), vA.data()); });
    if (n2 == 0) return 0;
    launch(grid_of(n2), MIRGE_BLOCK, [&] { k_cov_nonzero(vA.data(), n2, flag.data(), words); });
    const uint32_t n3 = count_flags(flag, pos, n2);
    if (words[0] & 2u) return -3;
    std::vector<long long> rs(n3 + 1), re(n3 + 1), rd(n3 + 1);
    const CovRuns r{run_strand, run_chrom, rs.data(), re.data(), rd.data()};
    launch(grid_of(n2), MIRGE_BLOCK, [&] { k_cov_runs(kB.data(), vA.data(), flag.data(), pos.data(), n2, strand_shift, r, words + 1); });
    for (uint32_t x = 0; x < n3; x++) { run_start[x] = rs[x]; run_end[x] = re[x]; run_depth[x] = rd[x]; }
    stats[0] = n3; stats[1] = words[1]; stats[2] = (int64_t)sum;
    if (!name_data || n3 == 0) return 0;
    // ---- the text
    std::vector<uint32_t> noff((size_t)n_rank + 1);
    for (int k = 0; k <= n_rank; k++) noff[k] = (uint32_t)(name_off[k] - name_off[0]);
    std::vector<unsigned long long> bytes(n3 + 1, 0), off(n3 + 1, 0);
    launch(grid_of(n3), MIRGE_BLOCK, [&] { k_cov_measure(r, n3, noff.data(), bytes.data()); });
    for (uint32_t x = 0; x < n3; x++) off[x + 1] = off[x] + bytes[x];
    const unsigned long long body = off[n3];
    stats[3] = (int64_t)body; stats[4] = (int64_t)off[words[1]];
    if ((long long)body > text_cap) return -2;
    tile = std::min<uint32_t>(MIRGE_COV_MAX_TILE, std::max<uint32_t>(64, tile)) & ~15u;
    chunk = std::max(chunk, tile) / tile * tile;
    for (unsigned long long at = 0; at < body; at += chunk) {
        const uint32_t nn = (uint32_t)std::min<unsigned long long>(chunk, body - at);
        std::vector<uint8_t> buf((size_t)nn + 16, 0xEE);
        const unsigned tiles = (nn + tile - 1) / tile;
        launch_threads(std::min(tiles, 3u), 8, [&] {
            k_cov_write(r, n3, noff.data(), reinterpret_cast<const uint8_t*>(name_data + name_off[0]), off.data(), at, nn, tile, buf.data());
        });
        for (int k = 0; k < 16; k++) if (buf[(size_t)nn + k] != 0xEE) return -4;  // (nothing behind the chunk's end)
        std::memcpy(text_out + at, buf.data(), nn);
    }
    return 0;
}

#ifdef COV_SIM_MAIN
int main() {
    const int32_t rank[] = {0, 0, 1, 1, 2, 2, 2}, len[] = {10, 10, 25, 5, 1, 64, 3};
    const int64_t start[] = {0, 10, 10, 20, 2147483646, 99990, 99995};
    const uint32_t weight[] = {3, 3, 4294967295u, 2, 1, 7, 7};
    const uint8_t minus[] = {0, 1, 0, 0, 1, 0, 1};
    const char names[] = "cchr_longer_namex";
    const int64_t name_off[] = {0, 1, 16, 17};
    int bad = 0;
    for (int stranded = 0; stranded < 2; stranded++)
        for (uint32_t tile : {64u, 8160u}) {
            uint8_t rs[15]; int32_t rc[15]; int64_t a[15], b[15], d[15], stats[5];
            std::vector<uint8_t> text(4096);
            const int rcode = sim_coverage(7, rank, start, len, weight, minus, 3, stranded, rs, rc, a, b, d, names, name_off, tile, 128, text.data(), 4096, stats);
            std::printf("stranded %d tile %u: rc %d, %lld runs, %lld bytes\n%.*s", stranded, tile, rcode, (long long)stats[0], (long long)stats[3],
                        (int)stats[3], (const char*)text.data());
            bad |= rcode != 0 || stats[0] == 0;
        }
    return bad;
}
#endif
