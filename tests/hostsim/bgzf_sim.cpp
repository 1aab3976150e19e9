// bgzf_sim.cpp -- csrc/kernels_bgzf.hpp compiled for the HOST (tests/test_bgzf_hostsim.py): the same kernel source, ONE workgroup of 256
// std::threads behind a futex barrier that takes the blocks in turn (k_bgzf_text's own grid-stride loop), so that a lane's segment is
// what it is on the device; the scan of the members' sizes is a loop, k_bam_compact closes the gaps, and the file is put together as
// csrc/native_bgzf.hpp does: the members, the 28-byte EOF block, the .gzi pairs.  The host runtime around the kernel and the real
// device are the GPU tests' business (tests/test_bgzf_gpu.py holds the device's file against this one byte for byte).
// Built with -DBGZF_SIM_MAIN it is a program of its own over a fixed set of streams, for an ASan / UBSan build.
#include <algorithm>
#include <atomic>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
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
struct alignas(16) uint4 { uint32_t x, y, z, w; };
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
#include "../../mirge3.0_amd/csrc/kernels_bgzf.hpp"

template <class F> static void launch(unsigned grid, unsigned block, F f) {  // kernels without a barrier
    gridDim.x = grid; blockDim.x = block;
    for (unsigned b = 0; b < grid; b++)
        for (unsigned t = 0; t < block; t++) { blockIdx.x = b; threadIdx.x = t; f(); }
}
template <class F> static void launch_group(unsigned block, F f) {  // one workgroup, its threads together
    gridDim.x = 1; blockDim.x = block; blockIdx.x = 0;
    Barrier bar; bar.n = (int)block; g_bar = &bar;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < block; t++) th.emplace_back([&, t] { threadIdx.x = t; f(); });
    for (auto& x : th) x.join();
}

static const uint8_t kEof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// The stream s[0 .. n) in blocks of `block` bytes -> the .gz file in out (returns its bytes; -2: out or gzi too small, -3: a member of
// size 0 or beyond its slot, -4: bytes behind a member in its slot, -5: the buffer is not aligned as assumed).  shift (0 .. 15): the source's offset in its 16 bytes, which is
// what decides how the kernel loads a block.  gzi: the index file's words (count, then pairs); stats: file bytes, members stored,
// fixed, dynamic.
extern "C" long long sim_bgzf(const uint8_t* s, long long n, uint32_t block, uint32_t shift, uint8_t* out, long long out_cap, uint64_t* gzi,
                              long long gzi_cap, long long* stats) {
    for (int k = 0; k < 4; k++) stats[k] = 0;
    const size_t nb = (size_t)(((unsigned long long)n + block - 1) / block);
    const uint32_t stride = (block + 31u + 15u) & ~15u;
    shift &= 15u;
    std::vector<uint8_t> buf((size_t)n + shift);  // (operator new aligns to 16; a load behind the stream's end is the sanitizer's to find)
    if (n) std::memcpy(buf.data() + shift, s, (size_t)n);
    const uint8_t* src = buf.data() + shift;
    if (n && (reinterpret_cast<uintptr_t>(src) & 15u) != shift) return -5;
    std::vector<uint8_t> slots(nb * stride + 16, 0xEE), packed(nb * stride + 16, 0xEE);
    std::vector<uint32_t> sizes(nb + 1, 0), off(nb + 1, 0);
    if (nb) launch_group(MIRGE_BLOCK, [&] { k_bgzf_text(src, (unsigned long long)n, 0ull, (uint32_t)nb, block, stride, slots.data(), sizes.data()); });
    for (size_t b = 0; b < nb; b++) {
        if (sizes[b] == 0 || sizes[b] > stride) return -3;
        for (uint32_t x = sizes[b]; x < stride; x++) if (slots[b * stride + x] != 0xEE) return -4;  // (nothing behind the member in its slot)
        off[b + 1] = off[b] + sizes[b];
        stats[1 + ((slots[b * stride + 18] >> 1) & 3u)]++;
    }
    if (nb) launch(std::min<unsigned>((unsigned)nb, 3), 8, [&] { k_bam_compact(slots.data(), stride, sizes.data(), off.data(), (uint32_t)nb, packed.data()); });
    const long long total = (long long)off[nb] + 28;
    if (total > out_cap || (long long)(1 + 2 * (nb ? nb - 1 : 0)) > gzi_cap) return -2;
    if (nb) std::memcpy(out, packed.data(), off[nb]);
    std::memcpy(out + off[nb], kEof, 28);
    gzi[0] = nb ? nb - 1 : 0;
    for (size_t b = 1; b < nb; b++) { gzi[2 * b - 1] = off[b]; gzi[2 * b] = (uint64_t)b * block; }
    stats[0] = total;
    return total;
}

#ifdef BGZF_SIM_MAIN
int main() {
    struct Case { std::string name; std::vector<uint8_t> s; uint32_t block; };
    std::vector<Case> cases;
    auto text = [](size_t n, uint32_t seed, uint32_t alphabet) {
        std::vector<uint8_t> v(n);
        for (size_t i = 0; i < n; i++) { seed = seed * 1664525u + 1013904223u; v[i] = (uint8_t)((seed >> 24) % alphabet + (alphabet == 256u ? 0u : 'A')); }
        return v;
    };
    for (size_t n : {0u, 1u, 3u, 255u, 256u, 257u, 511u}) cases.push_back({"acgt" + std::to_string(n), text(n, 7u, 4u), 256u});
    cases.push_back({"one letter", std::vector<uint8_t>(65280, 'A'), 65280u});
    cases.push_back({"random", text(4096, 11u, 256u), 4096u});
    cases.push_back({"lines", {}, 4096u});
    for (int k = 0; k < 700; k++) { const std::string l = "chr" + std::to_string(k % 7) + "\t" + std::to_string(1000 + 13 * k) + "\t" + std::to_string(1020 + 13 * k) + "\t" + std::to_string(k % 5 + 1) + "\n"; cases.back().s.insert(cases.back().s.end(), l.begin(), l.end()); }
    std::vector<uint8_t> high(3000);
    for (size_t i = 0; i < high.size(); i++) high[i] = (uint8_t)(144 + (i * i + 3 * i) % 112);
    cases.push_back({"high bytes", high, 1000u});
    int bad = 0;
    for (const Case& c : cases)
        for (uint32_t shift : {0u, 1u, 15u}) {
            std::vector<uint8_t> out(c.s.size() + 31 * (c.s.size() / c.block + 2) + 64);
            std::vector<uint64_t> gzi(2 * (c.s.size() / c.block + 2));
            long long stats[4];
            const long long n = sim_bgzf(c.s.data(), (long long)c.s.size(), c.block, shift, out.data(), (long long)out.size(), gzi.data(), (long long)gzi.size(), stats);
            std::printf("%s shift %u: %zu -> %lld bytes, stored %lld fixed %lld dynamic %lld\n", c.name.c_str(), shift, c.s.size(), n, stats[1], stats[2], stats[3]);
            bad |= n < 28;
        }
    return bad;
}
#endif
