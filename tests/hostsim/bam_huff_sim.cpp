// bam_huff_sim.cpp -- bam_huff_lengths of csrc/kernels_bam.hpp compiled for the HOST (tests/test_bam_dynamic_hostsim.py): k_bam_huff_probe,
// the kernel that mirge_bam_huffman_probe launches on the device, with a workgroup's threads as std::threads behind a barrier -- the
// shim of tests/hostsim/bam_sim.cpp.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <cstdio>
#include <thread>
#include <vector>
#include <mutex>
#include <atomic>
#include <climits>
#include <linux/futex.h>
#include <sys/syscall.h>
#include <unistd.h>
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
struct Barrier { int n = 0; std::atomic<int> count{0}; std::atomic<int> gen{0};
  void wait() {
    static_assert(sizeof(std::atomic<int>) == sizeof(int), "the futex word");
    const int g = gen.load(std::memory_order_acquire);
    if (count.fetch_add(1, std::memory_order_acq_rel) + 1 == n) {
      count.store(0, std::memory_order_relaxed); gen.store(g + 1, std::memory_order_release);
      syscall(SYS_futex, reinterpret_cast<int*>(&gen), FUTEX_WAKE_PRIVATE, INT32_MAX, nullptr, nullptr, 0);
    } else
      while (gen.load(std::memory_order_acquire) == g) syscall(SYS_futex, reinterpret_cast<int*>(&gen), FUTEX_WAIT_PRIVATE, g, nullptr, nullptr, 0);
  } };
static Barrier* g_bar;
static void __syncthreads() { g_bar->wait(); }
struct uint4 { uint32_t x, y, z, w; };
static std::mutex g_am;
template <class T> T atomicOr(T* p, T v) { std::lock_guard<std::mutex> l(g_am); T o = *p; *p |= v; return o; }
template <class T> T atomicXor(T* p, T v) { std::lock_guard<std::mutex> l(g_am); T o = *p; *p ^= v; return o; }
template <class T> T atomicAdd(T* p, T v) { std::lock_guard<std::mutex> l(g_am); T o = *p; *p += v; return o; }
template <class T> T atomicMin(T* p, T v) { std::lock_guard<std::mutex> l(g_am); T o = *p; if (v < o) *p = v; return o; }
template <class T> T atomicMax(T* p, T v) { std::lock_guard<std::mutex> l(g_am); T o = *p; if (v > o) *p = v; return o; }
template <class T> T atomicCAS(T* p, T c, T v) { std::lock_guard<std::mutex> l(g_am); T o = *p; if (o == c) *p = v; return o; }
#define MIRGE_BLOCK 256
#define MIRGE_CSV_MAXG 10
struct CsvGroup { const uint64_t* seq; const uint64_t* nmask; const uint8_t* len; const uint32_t* counts; const int8_t* pass; const int32_t* ref; uint32_t base, n; int32_t W; int32_t len16; };
static inline int csv_len(const CsvGroup& g, uint32_t j) { return g.len16 ? (int)reinterpret_cast<const uint16_t*>(g.len)[j] : (int)g.len[j]; }
#include "../../mirge3.0_amd/csrc/kernels_sam.hpp"
#include "../../mirge3.0_amd/csrc/kernels_bam.hpp"

// n_vec vectors of n_sym counts each -> n_vec vectors of n_sym lengths; one workgroup of 256 threads, reused for every vector.
// -1: arguments the device entry refuses too
extern "C" int sim_huff(const uint32_t* counts, int n_vec, int n_sym, int max_bits, uint8_t* lengths) {
  if (n_sym < 1 || n_sym > MIRGE_BAM_HUFF_MAX || max_bits < 1 || max_bits > 15 || (1 << max_bits) < n_sym) return -1;
  gridDim.x = 1; blockDim.x = MIRGE_BLOCK; blockIdx.x = 0;
  Barrier bar; bar.n = MIRGE_BLOCK; g_bar = &bar;
  std::vector<std::thread> th;
  for (unsigned t = 0; t < MIRGE_BLOCK; t++)
    th.emplace_back([&, t]{
      threadIdx.x = t;
      for (int v = 0; v < n_vec; v++) {
        k_bam_huff_probe(counts + (size_t)v * n_sym, (uint32_t)n_sym, (uint32_t)max_bits, lengths + (size_t)v * n_sym);
        __syncthreads();  // (the kernel's last loop reads the LDS that the next vector's first loop writes)
      }
    });
  for (auto& x : th) x.join();
  return 0;
}
