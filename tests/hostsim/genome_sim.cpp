// genome_sim.cpp -- csrc/kernels_genome.hpp compiled for the HOST (tests/test_genome_queries_hostsim.py): k_genome_queries itself, one
// thread after the other (it has no barrier and no atomic), so that the CPU suite holds the query encoding -- 2-bit words, N mask, seed
// mask, the cut of the seed into pieces and every piece's table key -- against a restatement of the header's comment.  The header's
// other kernels only have to compile: the wave intrinsics that the scan alone uses abort.  With -DGENOME_SIM_MAIN the same file is a
// stand-alone program (for a build with -fsanitize=address,undefined) that runs every (length, seed, pieces, strand) once.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
#define __shared__ static
struct D3 { unsigned x; };
static D3 threadIdx, blockIdx, blockDim, gridDim;
[[noreturn]] static void scan_only(const char* what) { std::fprintf(stderr, "genome_sim: %s belongs to k_genome_scan, which has no host twin\n", what); std::abort(); }
static unsigned long long __ballot(bool) { scan_only("__ballot"); }
static int __shfl(int, int, int) { scan_only("__shfl"); }
static int __shfl_xor(int, int, int) { scan_only("__shfl_xor"); }
static int __ffsll(long long v) { return __builtin_ffsll(v); }
static int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
template <class T> T atomicAdd(T* p, T v) { T o = *p; *p += v; return o; }
template <class T> T atomicOr(T* p, T v) { T o = *p; *p |= v; return o; }
template <class T> T atomicMax(T* p, T v) { T o = *p; if (v > o) *p = v; return o; }
#include "../../mirge3.0_amd/csrc/kernels_genome.hpp"

// qs_out: per (query, strand) 8 words: q[0], q[1], nm[0], nm[1], seed[0], seed[1], query | len << 32 | npieces << 40,
// poff[0..2] | plen[0..2] << 24
extern "C" int sim_queries(const char* ascii, const int64_t* off, uint32_t n, int n_mm, int seedlen, int trim5, int trim3, int kmax, int norc,
                           uint64_t* qs_out, uint64_t* keys, uint32_t* vals) {
  std::vector<GenomeQS> qs((size_t)2 * n);
  const GenomeQueryArgs a{ascii, off, n, n_mm, seedlen, trim5, trim3, kmax, norc};
  blockDim.x = 256; gridDim.x = (n + 255) / 256;
  for (unsigned b = 0; b < gridDim.x; b++)
    for (unsigned t = 0; t < blockDim.x; t++) { blockIdx.x = b; threadIdx.x = t; k_genome_queries(a, qs.data(), keys, vals); }
  for (size_t i = 0; i < qs.size(); i++) {
    const GenomeQS& g = qs[i];
    uint64_t* o = qs_out + 8 * i;
    o[0] = g.q[0]; o[1] = g.q[1]; o[2] = g.nm[0]; o[3] = g.nm[1]; o[4] = g.seed[0]; o[5] = g.seed[1];
    o[6] = (uint64_t)g.query | ((uint64_t)g.len << 32) | ((uint64_t)g.npieces << 40);
    o[7] = 0;
    for (int j = 0; j < MIRGE_GENOME_MAXPIECES; j++) o[7] |= ((uint64_t)g.poff[j] << (8 * j)) | ((uint64_t)g.plen[j] << (24 + 8 * j));
  }
  return 0;
}

#ifdef GENOME_SIM_MAIN
int main() {
  uint64_t rnd = 0x9E3779B97F4A7C15ull, sum = 0;
  auto next = [&]() { rnd ^= rnd << 13; rnd ^= rnd >> 7; rnd ^= rnd << 17; return rnd; };
  for (int n_mm = 0; n_mm <= 2; n_mm++)
    for (int seedlen : {5, 12, 15, 25, 28, 33, 64})
      for (int kmax : {8, 12, 13}) {
        std::string text; std::vector<int64_t> off{0};
        for (int L = 0; L <= MIRGE_GENOME_MAXLEN + 1; L++)  // 65 + trims is refused upstream; here it must just stay empty
          for (int rep = 0; rep < 3; rep++) {
            for (int t = 0; t < L + 3; t++) text.push_back(rep == 2 && t == (int)(next() % (L + 3)) ? 'N' : "ACGTacgt"[next() % 8]);
            off.push_back((int64_t)text.size());
          }
        const uint32_t n = (uint32_t)off.size() - 1;
        const int P = n_mm + 1;
        std::vector<uint64_t> qs((size_t)16 * n), keys((size_t)2 * n * P); std::vector<uint32_t> vals((size_t)2 * n * P);
        sim_queries(text.data(), off.data(), n, n_mm, seedlen, 1, 2, kmax, 0, qs.data(), keys.data(), vals.data());
        for (uint64_t k : keys) sum += k;
      }
  std::printf("genome_sim ok %llx\n", (unsigned long long)sum);
  return 0;
}
#endif
