// bam_sim.cpp -- csrc/kernels_sam.hpp + csrc/kernels_bam.hpp compiled for the HOST (tests/test_sorted_bam_hostsim.py): the same kernel
// source, a workgroup's threads as std::threads behind a barrier, workgroups one after the other (as tests/hostsim/sam_sim.cpp).  The
// kernels use no wave intrinsics, so the LDS deflate, its bit offsets and the CRC-32 combination run here too.  The sort and the scans
// (hipCUB on the device) are std::stable_sort and loops; the host runtime around the kernels (csrc/native_bam.hpp) and the real device
// are the GPU tests' business.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <cstdio>
#include <numeric>
#include <thread>
#include <vector>
#include <mutex>
#include <condition_variable>
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
// (a futex on the generation: the 255 threads the last one wakes do not queue for a mutex again, which is what a block of 64 bytes'
// eight barriers cost when thousands of blocks go through tests/test_bam_deflate_hostsim.py)
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

template <class F> static void launch(unsigned grid, unsigned block, F f) {
  gridDim.x = grid; blockDim.x = block;
  for (unsigned b = 0; b < grid; b++) {
    blockIdx.x = b; Barrier bar; bar.n = block; g_bar = &bar;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < block; t++) th.emplace_back([&, t]{ threadIdx.x = t; f(); });
    for (auto& x : th) x.join();
  }
}
// deflate = 0: out = the uncompressed stream; 1: out = the BGZF members one behind the other (no EOF block).  Returns the bytes in out,
// -1: a row out of range, -2: out too small, -(16 + flags): k_bam_measure's error flags.
extern "C" long long sim_bam(uint32_t n, int W, const uint64_t* seq, const uint64_t* nmask, const uint8_t* len, const uint32_t* counts, const int8_t* pass,
    const int32_t* ref, const int32_t* off, const int8_t* mm, int S, int sample, const SamPass* passes, int n_pass, const uint32_t* order,
    const int32_t* const* refid, const uint8_t* header, long long header_len, uint32_t block, int deflate, uint8_t* out, long long out_cap, long long* n_records) {
  SamTables t; std::memset(&t, 0, sizeof(t));
  t.g[0] = CsvGroup{seq, nmask, len, counts, pass, ref, 0, n, W, 1}; t.off[0] = off; t.mm[0] = mm; t.pass = passes; t.n_pass = n_pass; t.S = S; t.sample = sample;
  BamTables bt; std::memset(&bt, 0, sizeof(bt));
  for (int p = 0; p < n_pass; p++) bt.refid[p] = refid[p];
  bt.header = header; bt.header_len = (unsigned long long)header_len;
  size_t nf = (size_t)n * MIRGE_SAM_NCLASS;
  std::vector<uint32_t> keep(nf + 1, 0), pos(nf + 1, 0); uint32_t flags[16] = {0};
  launch(2, 64, [&]{ k_sam_select(t, order, n, keep.data(), flags); });
  if (flags[0]) return -1;
  for (size_t i = 0; i < nf; i++) pos[i + 1] = pos[i] + keep[i];
  uint32_t n_rows = pos[nf];
  std::vector<uint32_t> rows(n_rows + 1), fixed(n_rows + 1), perm(n_rows), s_rows(n_rows + 1), s_fixed(n_rows + 1);
  std::vector<unsigned long long> key(n_rows + 1), total(n_rows + 1, 0), s_total(n_rows + 1, 0), roff(n_rows + 1, 0); unsigned long long nr = 0;
  uint32_t bflags[16] = {0};
  if (n_rows) { launch(2, 64, [&]{ k_sam_rows(order, n, keep.data(), pos.data(), rows.data()); });
                launch(2, 64, [&]{ k_bam_measure(t, bt, rows.data(), n_rows, key.data(), fixed.data(), total.data(), &nr, bflags); }); }
  if (bflags[0]) return -(16 + (long long)bflags[0]);
  std::iota(perm.begin(), perm.end(), 0u);
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
  if (n_rows) launch(2, 64, [&]{ k_bam_gather(perm.data(), n_rows, rows.data(), fixed.data(), total.data(), s_rows.data(), s_fixed.data(), s_total.data()); });
  for (uint32_t i = 0; i < n_rows; i++) roff[i + 1] = roff[i] + s_total[i];
  const unsigned long long stream = (unsigned long long)header_len + roff[n_rows];
  const uint32_t n_blocks = (uint32_t)((stream + block - 1) / block), slot = (block + 5u + 26u + 15u) & ~15u;
  *n_records = (long long)nr;
  std::vector<uint8_t> buf((size_t)n_blocks * slot + 16, 0xEE); std::vector<uint32_t> sizes(n_blocks + 1, 0);
  launch(std::min(n_blocks, 3u), 256, [&]{ k_bam_blocks(t, bt, s_rows.data(), n_rows, s_fixed.data(), roff.data(), stream, 0ull, n_blocks, block, deflate, slot, buf.data(), sizes.data()); });
  if (!deflate) { if ((long long)stream > out_cap) return -2; std::memcpy(out, buf.data(), stream); return (long long)stream; }
  std::vector<uint32_t> boff(n_blocks + 1, 0);
  for (uint32_t b = 0; b < n_blocks; b++) boff[b + 1] = boff[b] + sizes[b];
  if ((long long)boff[n_blocks] > out_cap) return -2;
  launch(2, 64, [&]{ k_bam_compact(buf.data(), slot, sizes.data(), boff.data(), n_blocks, out); });
  return (long long)boff[n_blocks];
}
