// kernels_nearest.hpp -- part of mirge_kernels.hpp: --unmapped-nearest (mirge3_amd/nearest.py holds the specification): every unannotated
// unique read of 12 .. 64 nt against every base of the hairpin library, by Myers' bit-parallel edit distance (G. Myers, J. ACM 46, 1999; the
// block form with the score taken on bit m - 1 as in H. Hyyro's restatement).
//   k_near_codes        : the library's ASCII -> one code per base (A C G T = 0 .. 3, anything else 4: matches nothing).
//   k_near_flag         : the rows of a dictionary the cascade left unannotated, with a length in range, flagged for hipCUB's compaction; the
//                         counts of the unannotated, the too short and the too long rows on the way.
//   k_near_masks_packed : the four match masks of every selected row from its packed words and its nmask (bit i of mask c: letter i is c).
//   k_near_masks_ascii  : the same from ASCII + offsets (mirge_nearest_scan); a length out of range is written as 0.
//   k_near_width        : the flags of the two instances, by length.
//   k_near_scan<W>      : one lane per query, the masks, Pv, Mv and the score in registers; the grid is (text chunks) x (query tiles), a chunk a
//                         run of whole hairpins.  A chunk's codes are staged once per workgroup in LDS (MIRGE_NEAR_LDS_BASES; a chunk that holds
//                         one hairpin longer than that is read from global memory by uniform loads) and the letter of a column is the same in
//                         every lane, so nothing diverges.  At a hairpin's start Pv = ~0, Mv = 0, score = m.  A lane keeps the first strictly
//                         smaller score with its hairpin and end; its key D << 56 | hairpin << 32 | e goes into the query's word with a 64-bit
//                         atomicMin: the order of the key is the tie rule (lowest hairpin, then smallest end), so timing decides nothing.
//   k_near_report       : the queries with D <= min(K, m / 8) (K < 0: every query with a hit) flagged for the compaction.
//   k_near_start<W>     : the reported queries alone: the same recurrence with the reversed masks over h[e - 1], h[e - 2], ..., anchored at e (a
//                         one is shifted into Ph); the first column j at which the score equals D gives s = e - j, the LARGEST start.
//   k_near_gather       : the reported queries' row, key and start, packed.
// W = uint32_t for m <= 32, uint64_t for m <= 64; bits above m - 1 hold what the carries leave there and are never read.
// Compiled for the host too (tests/hostsim/near_sim.cpp, MIRGE_NEAR_HOSTSIM): a workgroup's threads then run one after the other between its barriers.
#pragma once

#define MIRGE_NEAR_MIN_LEN 12
#define MIRGE_NEAR_MAX_LEN 64
#define MIRGE_NEAR_MAX_K 8
#define MIRGE_NEAR_LDS_BASES 4096       // codes of a chunk held in LDS: the upper bound and the default of MIRGE_NEAR_CHUNK_BASES
#define MIRGE_NEAR_MAX_HAIRPINS (1u << 24)
#define MIRGE_NEAR_NO_KEY 0xFFFFFFFFFFFFFFFFull
#define MIRGE_NEAR_NGROUPS 10            // read groups of a handle (native_reads.hpp: MIRGE_NGROUPS)
// stats of k_near_flag (64-bit words)
#define MIRGE_NEAR_ST_UNMAPPED 0
#define MIRGE_NEAR_ST_SHORT 1
#define MIRGE_NEAR_ST_LONG 2

#ifdef MIRGE_NEAR_HOSTSIM
#define NEAR_EACH_THREAD for (threadIdx.x = 0; threadIdx.x < blockDim.x; threadIdx.x++)
#define NEAR_BARRIER
#define NEAR_SHARED static
#define NEAR_UNIFORM(x) (x)
#else
#define NEAR_EACH_THREAD
#define NEAR_BARRIER __syncthreads()
#define NEAR_SHARED __shared__
#define NEAR_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)
#endif

// the groups of a dictionary with the cascade's answer (as TrfGroup): packed words [W][n], nmask [W][n] or null, lengths, pass
struct NearGroup {
    const uint64_t* seq;
    const uint64_t* nmask;
    const uint8_t* len;   // uint16 behind the pointer for the long class (W == 0)
    const int8_t* pass;
    uint32_t base, n;     // handle index = base + j
    int32_t W, pad;
};
struct NearGroups {
    NearGroup g[MIRGE_NEAR_NGROUPS];
};

// a run of whole consecutive hairpins [h0, h1): one workgroup's text
struct NearChunk {
    uint32_t h0, h1;
};

__host__ __device__ __forceinline__ int near_locate(const NearGroups& t, uint32_t i, uint32_t& j) {
    int gi = 0;
#pragma unroll
    for (int k = 1; k < MIRGE_NEAR_NGROUPS; k++)
        if (t.g[k].n && i >= t.g[k].base) gi = k;
    j = i - t.g[gi].base;
    return gi;
}

__host__ __device__ __forceinline__ uint8_t near_code(uint8_t c) {
    return c == 'A' ? (uint8_t)0 : (c == 'C' ? (uint8_t)1 : (c == 'G' ? (uint8_t)2 : (c == 'T' ? (uint8_t)3 : (uint8_t)4)));
}

__host__ __device__ __forceinline__ uint32_t near_cap(int32_t K, uint32_t m) {
    const uint32_t by_len = m >> 3;
    return K < 0 ? m : ((uint32_t)K < by_len ? (uint32_t)K : by_len);
}

// bits [0, m) of x in reverse order (m <= 64)
__host__ __device__ __forceinline__ uint64_t near_reverse(uint64_t x, uint32_t m) {
    x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    x = ((x >> 8) & 0x00FF00FF00FF00FFull) | ((x & 0x00FF00FF00FF00FFull) << 8);
    x = ((x >> 16) & 0x0000FFFF0000FFFFull) | ((x & 0x0000FFFF0000FFFFull) << 16);
    x = (x >> 32) | (x << 32);
    return x >> (64u - m);
}

// one column of the recurrence: the masks of the column's letter (0 for a letter that matches nothing), the vertical deltas, the score of
// row m (bit `top` = m - 1).  ANCHOR: the cell above row 1 grows by one per column (the start is fixed), else it stays 0 (any start).
template <class W, bool ANCHOR>
__host__ __device__ __forceinline__ void near_step(W Eq, W& Pv, W& Mv, uint32_t& score, uint32_t top) {
    const W Xv = Eq | Mv;
    const W Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
    W Ph = Mv | ~(Xh | Pv);
    W Mh = Pv & Xh;
    score += (uint32_t)((Ph >> top) & (W)1);
    score -= (uint32_t)((Mh >> top) & (W)1);
    Ph = ANCHOR ? (W)((Ph << 1) | (W)1) : (W)(Ph << 1);
    Mh <<= 1;
    Pv = Mh | ~(Xv | Ph);
    Mv = Ph & Xv;
}

template <class W>
__host__ __device__ __forceinline__ W near_eq(W p0, W p1, W p2, W p3, uint32_t c) {
    return c == 0u ? p0 : (c == 1u ? p1 : (c == 2u ? p2 : (c == 3u ? p3 : (W)0)));
}

__global__ void k_near_codes(const uint8_t* __restrict__ ascii, uint32_t n, uint8_t* __restrict__ codes) {
    NEAR_EACH_THREAD {
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) codes[i] = near_code(ascii[i]);
    }
}

// flags[i] = 1: handle row i is unannotated and 12 .. 64 nt long.  stats: MIRGE_NEAR_ST_*, added to.
__global__ void k_near_flag(NearGroups t, uint32_t n, uint8_t* __restrict__ flags, unsigned long long* __restrict__ stats) {
    NEAR_EACH_THREAD {
        unsigned long long unm = 0, sh = 0, lo = 0;
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
            uint32_t j;
            const NearGroup& g = t.g[near_locate(t, i, j)];
            uint8_t f = 0;
            if (g.pass[j] < 0) {
                const uint32_t L = g.W ? (uint32_t)g.len[j] : (uint32_t)reinterpret_cast<const uint16_t*>(g.len)[j];
                unm++;
                if (L < MIRGE_NEAR_MIN_LEN) sh++;
                else if (L > MIRGE_NEAR_MAX_LEN) lo++;
                else f = 1;
            }
            flags[i] = f;
        }
        if (unm) atomicAdd(&stats[MIRGE_NEAR_ST_UNMAPPED], unm);
        if (sh) atomicAdd(&stats[MIRGE_NEAR_ST_SHORT], sh);
        if (lo) atomicAdd(&stats[MIRGE_NEAR_ST_LONG], lo);
    }
}

// peq [4][n]; qlen [n].  rows: handle indices of selected rows (12 .. 64 nt: the first two words of a read hold them)
__global__ void k_near_masks_packed(NearGroups t, const uint32_t* __restrict__ rows, uint32_t n, uint64_t* __restrict__ peq, uint8_t* __restrict__ qlen) {
    NEAR_EACH_THREAD {
        for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x) {
            uint32_t j;
            const NearGroup& g = t.g[near_locate(t, rows[x], j)];
            const uint32_t L = g.W ? (uint32_t)g.len[j] : 0u;
            uint64_t p[4] = {0ull, 0ull, 0ull, 0ull};
            if (L <= MIRGE_NEAR_MAX_LEN) {
                const int nw = L > 32u ? 2 : 1;
                for (int w = 0; w < nw; w++) {
                    const uint64_t word = g.seq[(size_t)w * g.n + j];
                    const uint64_t nm = g.nmask ? g.nmask[(size_t)w * g.n + j] : 0ull;
                    const uint32_t here = L - 32u * (uint32_t)w < 32u ? L - 32u * (uint32_t)w : 32u;
                    for (uint32_t b = 0; b < here; b++) {
                        if ((nm >> (2 * b)) & 1ull) continue;
                        const uint32_t c = (uint32_t)((word >> (2 * b)) & 3ull);
                        const uint64_t bit = 1ull << (32u * (uint32_t)w + b);
                        p[0] |= c == 0u ? bit : 0ull; p[1] |= c == 1u ? bit : 0ull; p[2] |= c == 2u ? bit : 0ull; p[3] |= c == 3u ? bit : 0ull;
                    }
                }
            }
            for (int c = 0; c < 4; c++) peq[(size_t)c * n + x] = p[c];
            qlen[x] = (uint8_t)(L >= MIRGE_NEAR_MIN_LEN && L <= MIRGE_NEAR_MAX_LEN ? L : 0u);
        }
    }
}

__global__ void k_near_masks_ascii(const uint8_t* __restrict__ text, const int64_t* __restrict__ off, uint32_t n, uint64_t* __restrict__ peq,
                                   uint8_t* __restrict__ qlen) {
    NEAR_EACH_THREAD {
        for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x) {
            const int64_t b = off[x], L = off[x + 1] - b;
            const bool in = L >= MIRGE_NEAR_MIN_LEN && L <= MIRGE_NEAR_MAX_LEN;
            uint64_t p[4] = {0ull, 0ull, 0ull, 0ull};
            for (int64_t i = 0; in && i < L; i++) {
                const uint32_t c = near_code(text[b + i]);
                const uint64_t bit = 1ull << i;
                p[0] |= c == 0u ? bit : 0ull; p[1] |= c == 1u ? bit : 0ull; p[2] |= c == 2u ? bit : 0ull; p[3] |= c == 3u ? bit : 0ull;
            }
            for (int c = 0; c < 4; c++) peq[(size_t)c * n + x] = p[c];
            qlen[x] = (uint8_t)(in ? L : 0);
        }
    }
}

// f32[x] = 1: query x runs in the uint32_t instance; f64[x] = 1: in the uint64_t instance.  force64: every query in the uint64_t instance.
__global__ void k_near_width(const uint8_t* __restrict__ qlen, uint32_t n, int32_t force64, uint8_t* __restrict__ f32, uint8_t* __restrict__ f64) {
    NEAR_EACH_THREAD {
        for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x) {
            const uint32_t m = qlen[x];
            const bool narrow = m && m <= 32u && !force64;
            f32[x] = narrow ? 1 : 0;
            f64[x] = m && !narrow ? 1 : 0;
        }
    }
}

// the four codes at bytes [pos, pos + 4) of a 4-byte-aligned text, as one word that is the same in every lane (two aligned loads: up to
// 7 bytes past pos are read, which the text's slack holds)
__host__ __device__ __forceinline__ uint32_t near_fetch4(const uint32_t* __restrict__ words, uint32_t pos) {
    const uint32_t lo = NEAR_UNIFORM(words[pos >> 2]), hi = NEAR_UNIFORM(words[(pos >> 2) + 1]);
    return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8u * (pos & 3u)));
}

template <class W>
__host__ __device__ __forceinline__ void near_column(uint32_t c, W p0, W p1, W p2, W p3, W& Pv, W& Mv, uint32_t& score, uint32_t top, uint32_t h, uint32_t e,
                                                    uint32_t& bestD, uint32_t& bestH, uint32_t& bestE) {
    near_step<W, false>(near_eq<W>(p0, p1, p2, p3, c), Pv, Mv, score, top);
    const bool better = score < bestD;
    bestD = better ? score : bestD;
    bestH = better ? h : bestH;
    bestE = better ? e : bestE;
}

// the columns of hairpins [h0, h1) for one lane; `words` holds the codes from text position t0 on (LDS: the chunk's first base; global: 0),
// four columns per fetched word, the next word fetched before the current one's columns run
template <class W>
__host__ __device__ __forceinline__ void near_scan_chunk(const uint32_t* __restrict__ words, uint32_t t0, const uint32_t* __restrict__ hoff, uint32_t h0,
                                                        uint32_t h1, W p0, W p1, W p2, W p3, uint32_t m, uint32_t& bestD, uint32_t& bestH, uint32_t& bestE) {
    const uint32_t top = m - 1u;
    for (uint32_t h = h0; h < h1; h++) {
        const uint32_t b = NEAR_UNIFORM(hoff[h]), e = NEAR_UNIFORM(hoff[h + 1]);
        W Pv = (W)~(W)0, Mv = (W)0;
        uint32_t score = m;
        uint32_t g = b;
        uint32_t w = near_fetch4(words, g - t0);
        for (; g + 4u <= e; g += 4u) {
            const uint32_t next = near_fetch4(words, g + 4u - t0);
            near_column<W>(w & 0xFFu, p0, p1, p2, p3, Pv, Mv, score, top, h, g - b + 1u, bestD, bestH, bestE);
            near_column<W>((w >> 8) & 0xFFu, p0, p1, p2, p3, Pv, Mv, score, top, h, g - b + 2u, bestD, bestH, bestE);
            near_column<W>((w >> 16) & 0xFFu, p0, p1, p2, p3, Pv, Mv, score, top, h, g - b + 3u, bestD, bestH, bestE);
            near_column<W>(w >> 24, p0, p1, p2, p3, Pv, Mv, score, top, h, g - b + 4u, bestD, bestH, bestE);
            w = next;
        }
        for (; g < e; g++, w >>= 8) near_column<W>(w & 0xFFu, p0, p1, p2, p3, Pv, Mv, score, top, h, g - b + 1u, bestD, bestH, bestE);
    }
}

// idx [n]: the queries of this instance.  hoff [n_h + 1]: the hairpins' offsets into codes.  best [queries]: MIRGE_NEAR_NO_KEY before the launch.
// blockIdx.x = the chunk, blockIdx.y strides over the query tiles.
template <class W>
__global__ void __launch_bounds__(MIRGE_BLOCK) k_near_scan(const uint32_t* __restrict__ idx, uint32_t n, uint32_t n_all, const uint64_t* __restrict__ peq,
                                                           const uint8_t* __restrict__ qlen, const uint8_t* __restrict__ codes,
                                                           const uint32_t* __restrict__ hoff, const NearChunk* __restrict__ chunks,
                                                           unsigned long long* __restrict__ best) {
    NEAR_SHARED uint32_t s_words[MIRGE_NEAR_LDS_BASES / 4 + 2];  // (two words of slack behind the codes: near_fetch4)
    uint8_t* const s_codes = reinterpret_cast<uint8_t*>(s_words);
    const NearChunk ch = chunks[blockIdx.x];
    const uint32_t t0 = hoff[ch.h0], t1 = hoff[ch.h1];
    const bool staged = t1 - t0 <= MIRGE_NEAR_LDS_BASES;
    if (staged) {
        NEAR_EACH_THREAD {
            for (uint32_t i = threadIdx.x; i < t1 - t0; i += blockDim.x) s_codes[i] = codes[t0 + i];
        }
    }
    NEAR_BARRIER;
    NEAR_EACH_THREAD {
        for (uint32_t tile = blockIdx.y; (size_t)tile * blockDim.x < n; tile += gridDim.y) {
            const uint32_t x = tile * blockDim.x + threadIdx.x;
            if (x >= n) continue;
            const uint32_t q = idx[x];
            const uint32_t m = qlen[q];
            const W p0 = (W)peq[q], p1 = (W)peq[(size_t)n_all + q], p2 = (W)peq[2 * (size_t)n_all + q], p3 = (W)peq[3 * (size_t)n_all + q];
            uint32_t bestD = m + 1u, bestH = 0u, bestE = 0u;
            if (staged) near_scan_chunk<W>(s_words, t0, hoff, ch.h0, ch.h1, p0, p1, p2, p3, m, bestD, bestH, bestE);
            else near_scan_chunk<W>(reinterpret_cast<const uint32_t*>(codes), 0u, hoff, ch.h0, ch.h1, p0, p1, p2, p3, m, bestD, bestH, bestE);
            if (bestD <= m)
                atomicMin(&best[q], ((unsigned long long)bestD << 56) | ((unsigned long long)bestH << 32) | (unsigned long long)bestE);
        }
    }
}

__global__ void k_near_report(const unsigned long long* __restrict__ best, const uint8_t* __restrict__ qlen, uint32_t n, int32_t K,
                              uint8_t* __restrict__ flags) {
    NEAR_EACH_THREAD {
        for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x) {
            const unsigned long long key = best[x];
            const uint32_t m = qlen[x];
            flags[x] = (m && key != MIRGE_NEAR_NO_KEY && (uint32_t)(key >> 56) <= near_cap(K, m)) ? 1 : 0;
        }
    }
}

// rep [n]: reported queries.  start[q] = s (0-based); -1 where the anchored scan did not reach D (never: the launch's caller checks).  A launch
// of one instance passes the other's queries by.
template <class W>
__global__ void k_near_start(const uint32_t* __restrict__ rep, uint32_t n, uint32_t n_all, const uint64_t* __restrict__ peq, const uint8_t* __restrict__ qlen,
                             const uint8_t* __restrict__ codes, const uint32_t* __restrict__ hoff, const unsigned long long* __restrict__ best,
                             int32_t force64, int32_t* __restrict__ start) {
    NEAR_EACH_THREAD {
        for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x) {
            const uint32_t q = rep[x];
            const uint32_t m = qlen[q];
            const bool narrow = m <= 32u && !force64;
            if (narrow != (sizeof(W) == 4)) continue;
            const unsigned long long key = best[q];
            const uint32_t D = (uint32_t)(key >> 56), h = (uint32_t)(key >> 32) & 0xFFFFFFu, e = (uint32_t)key;
            const W p0 = (W)near_reverse(peq[q], m), p1 = (W)near_reverse(peq[(size_t)n_all + q], m),
                    p2 = (W)near_reverse(peq[2 * (size_t)n_all + q], m), p3 = (W)near_reverse(peq[3 * (size_t)n_all + q], m);
            const uint32_t b = hoff[h];
            const uint32_t cols = e < m + D ? e : m + D;
            W Pv = (W)~(W)0, Mv = (W)0;
            uint32_t score = m;
            int32_t s = -1;
            for (uint32_t j = 1; j <= cols; j++) {
                const uint32_t c = codes[b + e - j];
                near_step<W, true>(near_eq<W>(p0, p1, p2, p3, c), Pv, Mv, score, m - 1u);
                if (score == D) { s = (int32_t)(e - j); break; }
            }
            start[q] = s;
        }
    }
}

// rep [n] -> row[x] = rows ? rows[rep[x]] : rep[x], key[x], s[x]
__global__ void k_near_gather(const uint32_t* __restrict__ rep, uint32_t n, const uint32_t* __restrict__ rows, const unsigned long long* __restrict__ best,
                              const int32_t* __restrict__ start, uint32_t* __restrict__ row, unsigned long long* __restrict__ key, int32_t* __restrict__ s) {
    NEAR_EACH_THREAD {
        for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x) {
            const uint32_t q = rep[x];
            row[x] = rows ? rows[q] : q;
            key[x] = best[q];
            s[x] = start[q];
        }
    }
}
