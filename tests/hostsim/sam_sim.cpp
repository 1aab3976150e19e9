// sam_sim.cpp -- csrc/kernels_sam.hpp compiled for the HOST (tests/test_sam_out_hostsim.py): the same kernel source, a workgroup's
// threads as std::threads behind a barrier, workgroups one after the other.  It lets the CPU suite hold the --sam-out kernels -- row
// choice, the digit-band closed form, the output-stationary tiling and its probe-point ownership -- against the reference's golden
// files; the host runtime around them (csrc/native_sam.hpp) and the real device are the GPU tests' business.
#include <cstdint>
#include <cstring>
#include <cstdio>
#include <thread>
#include <vector>
#include <mutex>
#include <condition_variable>
#include <atomic>
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
#define __shared__ static
struct D3 { unsigned x; };
static thread_local D3 threadIdx;
static D3 blockIdx, blockDim, gridDim;
struct Barrier { std::mutex m; std::condition_variable cv; int n, count = 0, gen = 0;
  void wait() { std::unique_lock<std::mutex> l(m); int g = gen; if (++count == n) { gen++; count = 0; cv.notify_all(); } else cv.wait(l, [&]{ return g != gen; }); } };
static Barrier* g_bar;
static void __syncthreads() { g_bar->wait(); }
struct uint4 { uint32_t x, y, z, w; };
static std::mutex g_am;
template <class T> T atomicOr(T* p, T v) { std::lock_guard<std::mutex> l(g_am); T o = *p; *p |= v; return o; }
template <class T> T atomicAdd(T* p, T v) { std::lock_guard<std::mutex> l(g_am); T o = *p; *p += v; return o; }
#define MIRGE_BLOCK 256
#define MIRGE_CSV_MAXG 10
struct CsvGroup { const uint64_t* seq; const uint64_t* nmask; const uint8_t* len; const uint32_t* counts; const int8_t* pass; const int32_t* ref; uint32_t base, n; int32_t W; int32_t len16; };
static inline int csv_len(const CsvGroup& g, uint32_t j) { return g.len16 ? (int)reinterpret_cast<const uint16_t*>(g.len)[j] : (int)g.len[j]; }
#include "../../mirge3.0_amd/csrc/kernels_sam.hpp"

template <class F> static void launch(unsigned grid, unsigned block, F f) {
  gridDim.x = grid; blockDim.x = block;
  for (unsigned b = 0; b < grid; b++) {
    blockIdx.x = b; Barrier bar; bar.n = block; g_bar = &bar;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < block; t++) th.emplace_back([&, t]{ threadIdx.x = t; f(); });
    for (auto& x : th) x.join();
  }
}
extern "C" long long sim_run(uint32_t n, int W, const uint64_t* seq, const uint64_t* nmask, const uint8_t* len, const uint32_t* counts, const int8_t* pass,
    const int32_t* ref, const int32_t* off, const int8_t* mm, int S, int sample, const SamPass* passes, int n_pass, const uint32_t* order,
    uint32_t tile, uint32_t chunk, uint8_t* out, long long out_cap, long long* n_lines) {
  SamTables t; std::memset(&t, 0, sizeof(t));
  t.g[0] = CsvGroup{seq, nmask, len, counts, pass, ref, 0, n, W, 1}; t.off[0] = off; t.mm[0] = mm; t.pass = passes; t.n_pass = n_pass; t.S = S; t.sample = sample;
  size_t nf = (size_t)n * MIRGE_SAM_NCLASS;
  std::vector<uint32_t> keep(nf + 1, 0), pos(nf + 1, 0); uint32_t flags[16] = {0};
  launch(2, 64, [&]{ k_sam_select(t, order, n, keep.data(), flags); });
  if (flags[0]) return -1;
  for (size_t i = 0; i < nf; i++) pos[i + 1] = pos[i] + keep[i];
  uint32_t n_rows = pos[nf];
  std::vector<uint32_t> rows(n_rows + 1), fixed(n_rows + 1); std::vector<unsigned long long> total(n_rows + 1, 0), roff(n_rows + 1, 0); unsigned long long nl = 0;
  if (n_rows) { launch(2, 64, [&]{ k_sam_rows(order, n, keep.data(), pos.data(), rows.data()); });
                launch(2, 64, [&]{ k_sam_measure(t, rows.data(), n_rows, fixed.data(), total.data(), &nl); }); }
  for (uint32_t i = 0; i < n_rows; i++) roff[i + 1] = roff[i] + total[i];
  unsigned long long body = roff[n_rows];
  if ((long long)body > out_cap) return -2;
  *n_lines = (long long)nl;
  for (unsigned long long at = 0; at < body; at += chunk) {
    uint32_t nn = (uint32_t)std::min<unsigned long long>(chunk, body - at);
    std::vector<uint8_t> buf(nn + 16, 0xEE);
    unsigned tiles = (nn + tile - 1) / tile;
    launch(std::min(tiles, 3u), 256, [&]{ k_sam_write(t, rows.data(), n_rows, fixed.data(), roff.data(), at, nn, tile, buf.data()); });
    std::memcpy(out + at, buf.data(), nn);
  }
  return (long long)body;
}
