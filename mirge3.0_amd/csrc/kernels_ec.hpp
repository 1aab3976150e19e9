// kernels_ec.hpp -- part of mirge_kernels.hpp: k-mer spectrum error correction of one sample's distinct reads (--kmer-correct,
// mirge_kmer_correct; the published background is in PAPERS.md, the specification in the README section "`--kmer-correct`: sequencing errors in reads, by k-mer spectra").
//
// One ROUND at one k, over the dictionary the round before left:
//   ELIGIBLE  a read without N of k .. 256 letters (the five storage groups without an N; of the long class only its reads of 256 nt).
//   SPECTRUM  S(x) = sum of the counts of the eligible reads over every window that spells x (forward strand, 64-bit); x is weak iff
//             S(x) <= H.
//   SUSPECT   a read with a weak window; lo = its last weak start, hi = its first weak start + k - 1 (at most len - 1).  lo > hi: no
//             single letter lies in all weak windows (uncorrectable).
//   CANDIDATE (p, b), lo <= p <= hi, b != r[p]: valid iff every window of the changed read that covers p is solid; its score is the
//             smallest S among them.  The read is corrected iff exactly one valid candidate has the largest score.
// The kernels: k_ec_count (a thread walks a read's windows with a rolling 2-bit shift into an open-addressing table: compare-and-swap
// on the key, 64-bit atomic add on the sum), k_ec_classify (a thread per read, lookups only, four in flight; the suspect reads with
// lo <= hi go into a list), k_ec_correct (a WAVE per listed read: lanes take (candidate, window) pairs, a candidate's smallest sum is
// a segmented wave minimum, the unique maximum a wave reduction of (score, how many, which)), then the regrouping around the
// weighted collapse: k_ec_gather, k_ec_rep, k_ec_index, k_ec_find, k_ec_follow.
// With a ratio (--kmer-ratio, mirge_kmer_correct_ratio) k_ec_dominate and k_ec_fold run between k_ec_count and k_ec_classify: see there.
//
// A sum is complete before anything reads it (kernel boundary), a lookup compares the whole key, and a read's outcome goes to the
// read's own cell: nothing depends on where an insert landed, on the order of the list or on timing.
//
// No LDS and no barrier.  The wave kernel is written over "lane variables" (EC_LANES / EC_AT): on the device one element and the
// lane's own pass through the loop, with cross-lane steps by __shfl_xor; compiled for the host (MIRGE_EC_HOSTSIM,
// tests/hostsim/ec_sim.cpp) 64 elements, the loop over all lanes and the same butterflies over the array.
#pragma once

#define MIRGE_EC_NG 5  // the storage groups without an N
#define MIRGE_EC_MAXLEN 256
#define MIRGE_EC_MAXK 31
#define MIRGE_EC_EMPTY 0xFFFFFFFFFFFFFFFFull  // (a k-mer of at most 31 letters has its two top bits clear)
#define MIRGE_EC_NONE 0xFFFFFFFFu
#define MIRGE_EC_BATCH 4  // independent lookups a lane has in flight
// tally words of a round
#define MIRGE_EC_T_LIST 0
#define MIRGE_EC_T_ELIG 1
#define MIRGE_EC_T_SUSPECT 2
#define MIRGE_EC_T_CORRECTED 3
#define MIRGE_EC_T_UNCORRECTABLE 4
#define MIRGE_EC_T_UNSUPPORTED 5
#define MIRGE_EC_T_AMBIGUOUS 6
#define MIRGE_EC_T_WORDS 8

struct EcGroup {
    const uint64_t* seq;     // [W][n], word-major
    const uint8_t* len;      // [n]; len16: uint16 [n] behind the same pointer (the long class)
    const uint32_t* counts;  // [n]
    uint32_t base, n;        // handle index of the group's first read, reads
    uint32_t W;
    int32_t len16;
};
struct EcView {
    EcGroup g[MIRGE_EC_NG];
    uint32_t n_reads;  // reads of the whole set (handle indices 0 .. n_reads - 1), the ones with an N included
    int32_t k;
    uint64_t H;          // a window is weak iff its sum is <= H
    uint64_t hash_keep;  // MIRGE_TEST_EC_HASH_BITS: the bits of the hash that are kept (all: ~0)
    uint64_t tab_mask;   // slots - 1 (a power of two, at least twice the windows: a probe always ends)
};
struct alignas(16) EcSlot { uint64_t key, sum; };  // one 16-byte load answers a lookup

#ifdef MIRGE_EC_HOSTSIM
#define EC_NL 64
#define EC_LANES for (int lane = 0; lane < 64; lane++)
#define EC_AT lane
#else
#define EC_NL 1
#define EC_LANES for (int lane = (int)(threadIdx.x & 63u), once_ = 1; once_; once_ = 0)
#define EC_AT 0
#endif

__host__ __device__ __forceinline__ uint64_t ec_mix(uint64_t x) {  // splitmix64's finalizer
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__host__ __device__ __forceinline__ uint64_t ec_home(const EcView& v, uint64_t x) { return (ec_mix(x) & v.hash_keep) & v.tab_mask; }
__host__ __device__ __forceinline__ int ec_len(const EcGroup& g, uint32_t j) {
    return g.len16 ? (int)reinterpret_cast<const uint16_t*>(g.len)[j] : (int)g.len[j];
}
__host__ __device__ __forceinline__ int ec_locate(const EcView& v, uint32_t i, uint32_t& j) {
    for (int q = 0; q < MIRGE_EC_NG; q++)
        if (i - v.g[q].base < v.g[q].n) { j = i - v.g[q].base; return q; }
    return -1;
}
__host__ __device__ __forceinline__ bool ec_eligible(const EcView& v, int len) { return len >= v.k && len <= MIRGE_EC_MAXLEN; }

// the sum of k-mer x behind the slot `e` that was loaded from its home: 0 for a k-mer no eligible read holds
__host__ __device__ __forceinline__ uint64_t ec_sum(const EcView& v, const EcSlot* __restrict__ tab, uint64_t x, EcSlot e) {
    for (uint64_t s = ec_home(v, x);;) {
        if (e.key == x) return e.sum;
        if (e.key == MIRGE_EC_EMPTY) return 0;
        s = (s + 1) & v.tab_mask;
        e = tab[s];
    }
}

// the rolling walk over a read's letters: after step() number t (from 1) `x` holds the k-mer that ends with letter t - 1 (for t >= k)
struct EcWalk {
    const uint64_t* seq;  // the read's word 0; its words are `stride` apart
    size_t stride;
    uint64_t cur, x;
    int p, top;  // next letter; 2 (k - 1)
    __host__ __device__ __forceinline__ void step() {
        if ((p & 31) == 0) cur = seq[(size_t)(p >> 5) * stride];
        x = (x >> 2) | ((cur & 3ull) << top);
        cur >>= 2;
        p++;
    }
};
__host__ __device__ __forceinline__ EcWalk ec_walk(const EcGroup& g, uint32_t j, int k) {
    EcWalk w; w.seq = g.seq + j; w.stride = g.n; w.cur = 0; w.x = 0; w.p = 0; w.top = 2 * (k - 1);
    return w;
}

__global__ void __launch_bounds__(MIRGE_BLOCK) k_ec_clear(EcSlot* __restrict__ tab, uint64_t slots) {
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * blockDim.x) {
        EcSlot e; e.key = MIRGE_EC_EMPTY; e.sum = 0;
        tab[s] = e;
    }
}

// every window of every eligible read adds the read's count to its k-mer's sum
__global__ void __launch_bounds__(MIRGE_BLOCK) k_ec_count(EcView v, EcSlot* tab) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < v.n_reads; i += gridDim.x * blockDim.x) {
        uint32_t j;
        const int gi = ec_locate(v, i, j);
        if (gi < 0) continue;
        const EcGroup& g = v.g[gi];
        const int len = ec_len(g, j);
        if (!ec_eligible(v, len)) continue;
        const unsigned long long c = g.counts[j];
        EcWalk w = ec_walk(g, j, v.k);
        for (int t = 1; t < v.k; t++) w.step();
        for (int t = v.k; t <= len; t++) {
            w.step();
            for (uint64_t s = ec_home(v, w.x);; s = (s + 1) & v.tab_mask) {
                unsigned long long* const key = reinterpret_cast<unsigned long long*>(&tab[s].key);
                unsigned long long seen = *key;  // (a hot k-mer is there already: no compare-and-swap then)
                if (seen == MIRGE_EC_EMPTY) seen = atomicCAS(key, (unsigned long long)MIRGE_EC_EMPTY, (unsigned long long)w.x);
                if (seen == MIRGE_EC_EMPTY || seen == w.x) { atomicAdd(reinterpret_cast<unsigned long long*>(&tab[s].sum), c); break; }
            }
        }
    }
}

// ---- the relative threshold (--kmer-ratio R, mirge_kmer_correct_ratio) ---------------------------------------------------------------
// A k-mer x with S(x) > H is DOMINATED iff a k-mer y one letter from it has S(y) >= R S(x); a dominated k-mer is weak.  Two launches
// between k_ec_count and k_ec_classify: k_ec_dominate decides every slot's flag from the complete sums (the table is read-only in it),
// k_ec_fold then zeroes the flagged sums and keeps their keys (probe chains stay whole).  Behind them "S <= H" says "weak" for
// k_ec_classify and k_ec_correct as they stand: a valid candidate's windows are all solid, so no zeroed sum enters a score.
//
// A thread per slot.  R S(x) is formed once per slot, and only where it fits 64 bits (S(x) <= (2^64 - 1) / R): beyond that no sum
// reaches it.  The 3 k neighbours x ^ (d << 2 q), q < k, d = 1 .. 3, MIRGE_EC_BATCH home slots in flight together; the walk ends with the
// batch that holds the first dominating one.  tally2[0] = slots with S > H, tally2[1] = the dominated among them.
__global__ void __launch_bounds__(MIRGE_BLOCK) k_ec_dominate(EcView v, const EcSlot* __restrict__ tab, uint64_t slots, uint64_t ratio,
                                                             uint8_t* __restrict__ flag, unsigned long long* __restrict__ tally2) {
    unsigned long long n_above = 0, n_dom = 0;
    const int n_nb = 3 * v.k;
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * blockDim.x) {
        const EcSlot me = tab[s];
        uint8_t f = 0;
        if (me.key != MIRGE_EC_EMPTY && me.sum > v.H) {
            n_above++;
            if (me.sum <= ~0ull / ratio) {
                const uint64_t need = me.sum * ratio;  // (no wrap: checked above)
                for (int c0 = 0; c0 < n_nb && !f; c0 += MIRGE_EC_BATCH) {
                    uint64_t xs[MIRGE_EC_BATCH];
                    EcSlot e[MIRGE_EC_BATCH];
#pragma unroll
                    for (int u = 0; u < MIRGE_EC_BATCH; u++) {
                        const int c = c0 + u < n_nb ? c0 + u : n_nb - 1;  // (behind the last neighbour: that one once more, its answer unused)
                        xs[u] = me.key ^ ((uint64_t)(c % 3 + 1) << (2 * (c / 3)));
                    }
#pragma unroll
                    for (int u = 0; u < MIRGE_EC_BATCH; u++) e[u] = tab[ec_home(v, xs[u])];
#pragma unroll
                    for (int u = 0; u < MIRGE_EC_BATCH; u++)
                        if (c0 + u < n_nb && ec_sum(v, tab, xs[u], e[u]) >= need) f = 1;
                }
            }
            n_dom += f;
        }
        flag[s] = f;
    }
    if (n_above) atomicAdd(&tally2[0], n_above);
    if (n_dom) atomicAdd(&tally2[1], n_dom);
}

__global__ void __launch_bounds__(MIRGE_BLOCK) k_ec_fold(EcSlot* __restrict__ tab, uint64_t slots, const uint8_t* __restrict__ flag) {
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < slots; s += (uint64_t)gridDim.x * blockDim.x)
        if (flag[s]) tab[s].sum = 0;
}

// range[i] = lo | hi << 16, fix[i] = none; the reads with lo <= hi into list[] (in no order: every listed read's outcome goes
// to its own cell); tally[]: eligible, suspect, uncorrectable
__global__ void __launch_bounds__(MIRGE_BLOCK) k_ec_classify(EcView v, const EcSlot* __restrict__ tab, uint32_t* __restrict__ range,
                                                             uint32_t* __restrict__ fix,
                                                             uint32_t* __restrict__ list, uint32_t* __restrict__ tally) {
    uint32_t n_elig = 0, n_susp = 0, n_unc = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < v.n_reads; i += gridDim.x * blockDim.x) {
        range[i] = 0; fix[i] = MIRGE_EC_NONE;
        uint32_t j;
        const int gi = ec_locate(v, i, j);
        if (gi < 0) continue;
        const EcGroup& g = v.g[gi];
        const int len = ec_len(g, j);
        if (!ec_eligible(v, len)) continue;
        n_elig++;
        const int nwin = len - v.k + 1;
        int first_weak = -1, last_weak = -1;
        EcWalk w = ec_walk(g, j, v.k);
        for (int t = 1; t < v.k; t++) w.step();
        for (int i0 = 0; i0 < nwin; i0 += MIRGE_EC_BATCH) {
            uint64_t xs[MIRGE_EC_BATCH];
            EcSlot e[MIRGE_EC_BATCH];
#pragma unroll
            for (int u = 0; u < MIRGE_EC_BATCH; u++) {
                if (i0 + u < nwin) w.step();
                xs[u] = w.x;  // (behind the last window: that window once more, its answer unused)
            }
#pragma unroll
            for (int u = 0; u < MIRGE_EC_BATCH; u++) e[u] = tab[ec_home(v, xs[u])];
#pragma unroll
            for (int u = 0; u < MIRGE_EC_BATCH; u++) {
                if (i0 + u >= nwin) continue;
                if (ec_sum(v, tab, xs[u], e[u]) <= v.H) {
                    if (first_weak < 0) first_weak = i0 + u;
                    last_weak = i0 + u;
                }
            }
        }
        if (first_weak < 0) continue;
        n_susp++;
        const int lo = last_weak;
        int hi = first_weak + v.k - 1;
        hi = hi < len - 1 ? hi : len - 1;
        if (lo > hi) { n_unc++; continue; }
        range[i] = (uint32_t)lo | ((uint32_t)hi << 16);
        list[atomicAdd(&tally[MIRGE_EC_T_LIST], 1u)] = i;
    }
    if (n_elig) atomicAdd(&tally[MIRGE_EC_T_ELIG], n_elig);
    if (n_susp) atomicAdd(&tally[MIRGE_EC_T_SUSPECT], n_susp);
    if (n_unc) atomicAdd(&tally[MIRGE_EC_T_UNCORRECTABLE], n_unc);
}

// ---- wave steps over lane variables -------------------------------------------------------------------------------------------
struct EcBest { uint64_t score; uint32_t n, cand; };  // the largest score among valid candidates, how many have it, the first of them
__host__ __device__ __forceinline__ EcBest ec_better(const EcBest& a, const EcBest& b) {  // commutative and associative
    if (a.score != b.score) return a.score > b.score ? a : b;
    EcBest r; r.score = a.score; r.n = a.n + b.n; r.cand = a.cand < b.cand ? a.cand : b.cand;
    return r;
}
#ifndef MIRGE_EC_HOSTSIM
__device__ __forceinline__ uint64_t ec_shfl_xor64(uint64_t x, int o) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), o, 64);
    return ((uint64_t)hi << 32) | lo;
}
#endif
// every lane of a segment of `sw` lanes (a power of two) gets the segment's minimum
__host__ __device__ __forceinline__ void ec_seg_min(uint64_t (&s)[EC_NL], int sw) {
    for (int o = 1; o < sw; o <<= 1) {
#ifdef MIRGE_EC_HOSTSIM
        uint64_t t[EC_NL];
        for (int l = 0; l < EC_NL; l++) t[l] = s[l ^ o];
        for (int l = 0; l < EC_NL; l++) s[l] = t[l] < s[l] ? t[l] : s[l];
#else
        const uint64_t t = ec_shfl_xor64(s[0], o);
        s[0] = t < s[0] ? t : s[0];
#endif
    }
}
// every lane gets the wave's best
__host__ __device__ __forceinline__ void ec_wave_best(EcBest (&b)[EC_NL]) {
    for (int o = 1; o < 64; o <<= 1) {
#ifdef MIRGE_EC_HOSTSIM
        EcBest t[EC_NL];
        for (int l = 0; l < EC_NL; l++) t[l] = b[l ^ o];
        for (int l = 0; l < EC_NL; l++) b[l] = ec_better(b[l], t[l]);
#else
        EcBest t;
        t.score = ec_shfl_xor64(b[0].score, o);
        t.n = (uint32_t)__shfl_xor((int)b[0].n, o, 64);
        t.cand = (uint32_t)__shfl_xor((int)b[0].cand, o, 64);
        b[0] = ec_better(b[0], t);
#endif
    }
}

// the k letters of read j from `start`, letter p (start <= p < start + k) exchanged for b: from the packed words, no changed copy
__host__ __device__ __forceinline__ uint64_t ec_window(const EcGroup& g, uint32_t j, int len, int start, int k, int p, uint64_t b) {
    const int wi = start >> 5, off = 2 * (start & 31);
    uint64_t x = g.seq[(size_t)wi * g.n + j] >> off;
    if (off + 2 * k > 64 && wi + 1 < ((len + 31) >> 5)) x |= g.seq[(size_t)(wi + 1) * g.n + j] << (64 - off);  // (off > 0 here: 2 k <= 62)
    x &= (1ull << (2 * k)) - 1ull;
    const int sh = 2 * (p - start);
    return (x & ~(3ull << sh)) | (b << sh);
}

// One wave per listed read.  Candidate c = 3 (p - lo) + (rank of b among the three other letters); a candidate's windows start at
// max(0, p - k + 1) .. min(p, len - k): at most nw = min(k, len - k + 1), so segments of sw = nw rounded up to a power of two lanes
// hold one candidate each, 64 / sw candidates a step, MIRGE_EC_BATCH steps with their lookups in flight together.
// fix[i] = p << 2 | b for a corrected read; tally[]: corrected, unsupported, ambiguous.
__global__ void __launch_bounds__(MIRGE_BLOCK) k_ec_correct(EcView v, const EcSlot* __restrict__ tab, const uint32_t* __restrict__ list,
                                                            uint32_t n_list, const uint32_t* __restrict__ range, uint32_t* __restrict__ fix,
                                                            uint32_t* __restrict__ tally) {
#ifdef MIRGE_EC_HOSTSIM
    if (threadIdx.x & 63u) return;  // (the wave's first thread runs all its lanes)
#endif
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t t = wave; t < n_list; t += n_waves) {
        const uint32_t i = list[t];
        uint32_t j;
        const int gi = ec_locate(v, i, j);
        const EcGroup& g = v.g[gi];
        const int len = ec_len(g, j), k = v.k;
        const int lo = (int)(range[i] & 0xFFFFu), hi = (int)(range[i] >> 16);
        const int n_cand = 3 * (hi - lo + 1);
        const int nw = k < len - k + 1 ? k : len - k + 1;
        int sw = 1, sw_log = 0;
        while (sw < nw) { sw <<= 1; sw_log++; }
        const int per_step = 64 >> sw_log;
        EcBest best[EC_NL];
        EC_LANES { best[EC_AT].score = 0; best[EC_AT].n = 0; best[EC_AT].cand = MIRGE_EC_NONE; }
        for (int c0 = 0; c0 < n_cand; c0 += per_step * MIRGE_EC_BATCH) {
            uint64_t sc[MIRGE_EC_BATCH][EC_NL];
            EC_LANES {
                uint64_t xs[MIRGE_EC_BATCH];
                EcSlot e[MIRGE_EC_BATCH];
                bool on[MIRGE_EC_BATCH];
#pragma unroll
                for (int u = 0; u < MIRGE_EC_BATCH; u++) {
                    const int cand = c0 + u * per_step + (lane >> sw_log), win = lane & (sw - 1);
                    on[u] = false; xs[u] = 0;
                    if (cand < n_cand) {
                        const int p = lo + cand / 3;
                        const uint64_t mine = (g.seq[(size_t)(p >> 5) * g.n + j] >> (2 * (p & 31))) & 3ull;
                        uint64_t b = (uint64_t)(cand % 3);
                        b += b >= mine ? 1 : 0;
                        const int s0 = p - k + 1 > 0 ? p - k + 1 : 0, s1 = p < len - k ? p : len - k;
                        if (s0 + win <= s1) { on[u] = true; xs[u] = ec_window(g, j, len, s0 + win, k, p, b); }
                    }
                }
#pragma unroll
                for (int u = 0; u < MIRGE_EC_BATCH; u++) e[u] = tab[ec_home(v, xs[u])];  // (an idle lane reads k-mer 0's home: in bounds, unused)
#pragma unroll
                for (int u = 0; u < MIRGE_EC_BATCH; u++) sc[u][EC_AT] = on[u] ? ec_sum(v, tab, xs[u], e[u]) : MIRGE_EC_EMPTY;
            }
#pragma unroll
            for (int u = 0; u < MIRGE_EC_BATCH; u++) ec_seg_min(sc[u], sw);
            EC_LANES {
#pragma unroll
                for (int u = 0; u < MIRGE_EC_BATCH; u++) {
                    const int cand = c0 + u * per_step + (lane >> sw_log);
                    if (cand < n_cand && (lane & (sw - 1)) == 0 && sc[u][EC_AT] > v.H) {  // the segment's first lane speaks for the candidate
                        EcBest m; m.score = sc[u][EC_AT]; m.n = 1; m.cand = (uint32_t)cand;
                        best[EC_AT] = ec_better(best[EC_AT], m);
                    }
                }
            }
        }
        ec_wave_best(best);
        EC_LANES {
            if (lane == 0) {
                const EcBest& b = best[EC_AT];
                if (b.n == 1) {
                    const int p = lo + (int)b.cand / 3;
                    const uint32_t mine = (uint32_t)((g.seq[(size_t)(p >> 5) * g.n + j] >> (2 * (p & 31))) & 3ull);
                    uint32_t letter = b.cand % 3;
                    letter += letter >= mine ? 1 : 0;
                    fix[i] = ((uint32_t)p << 2) | letter;
                    atomicAdd(&tally[MIRGE_EC_T_CORRECTED], 1u);
                } else atomicAdd(&tally[b.n ? MIRGE_EC_T_AMBIGUOUS : MIRGE_EC_T_UNSUPPORTED], 1u);
            }
        }
    }
}

// ---- regrouping ---------------------------------------------------------------------------------------------------------------
// One storage group of the round's dictionary as "raw reads" for the weighted collapse, in the order of their first indices
// (perm[t] = the group's read that appeared t-th), the corrected ones with their letter exchanged; weight / ftrue / src are indexed
// by the raw read's handle index base + t: its count, its first index and the handle index it had in the dictionary.
struct EcGather {
    const uint64_t *seq, *nmask;
    const uint8_t* len;
    const uint32_t *counts, *first, *perm;
    uint64_t *oseq, *onmask;
    uint8_t* olen;
    uint32_t base, n, W;
    int32_t len_bytes;
};
__global__ void __launch_bounds__(MIRGE_BLOCK) k_ec_gather(EcGather a, const uint32_t* __restrict__ fix, uint32_t* __restrict__ weight,
                                                           uint32_t* __restrict__ ftrue, uint32_t* __restrict__ src) {
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < a.n; t += gridDim.x * blockDim.x) {
        const uint32_t j = a.perm[t], f = fix ? fix[a.base + j] : MIRGE_EC_NONE;
        for (uint32_t w = 0; w < a.W; w++) {
            uint64_t word = a.seq[(size_t)w * a.n + j];
            if (f != MIRGE_EC_NONE && (f >> 7) == w) {
                const int sh = 2 * (int)((f >> 2) & 31u);
                word = (word & ~(3ull << sh)) | ((uint64_t)(f & 3u) << sh);
            }
            a.oseq[(size_t)w * a.n + t] = word;
            if (a.onmask) a.onmask[(size_t)w * a.n + t] = a.nmask ? a.nmask[(size_t)w * a.n + j] : 0ull;
        }
        if (a.len_bytes == 2) reinterpret_cast<uint16_t*>(a.olen)[t] = reinterpret_cast<const uint16_t*>(a.len)[j];
        else a.olen[t] = a.len[j];
        weight[a.base + t] = a.counts[j];
        ftrue[a.base + t] = a.first[j];
        src[a.base + t] = a.base + j;
    }
}

__global__ void __launch_bounds__(MIRGE_BLOCK) k_ec_iota(uint32_t* __restrict__ out, uint32_t n) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) out[j] = j;
}

// A group of the collapse's result: its `first` names the earliest raw read of each new read.  That raw read's old handle index
// maps to the new one, and `first` becomes the true first index again.
__global__ void __launch_bounds__(MIRGE_BLOCK) k_ec_rep(uint32_t* __restrict__ ufirst, uint32_t n, uint32_t base, const uint32_t* __restrict__ ftrue,
                                                        const uint32_t* __restrict__ src, uint32_t n_raw, uint32_t* __restrict__ next) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
        const uint32_t q = ufirst[r];
        if (q >= n_raw) continue;
        next[src[q]] = base + r;
        ufirst[r] = ftrue[q];
    }
}

// the reads that merged into an earlier one find it by their letters: an index of the new dictionary's reads without N of up to 256 nt
__host__ __device__ __forceinline__ uint64_t ec_read_hash(const EcView& v, const EcGroup& g, uint32_t j, int len) {
    uint64_t h = (uint64_t)len * 0x9E3779B97F4A7C15ull;
    for (int w = 0; w < (len + 31) >> 5; w++) h = ec_mix(h ^ g.seq[(size_t)w * g.n + j]);
    return ec_mix(h) & v.hash_keep;
}
__global__ void __launch_bounds__(MIRGE_BLOCK) k_ec_index(EcView v, uint64_t* __restrict__ rtab) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < v.n_reads; i += gridDim.x * blockDim.x) {
        uint32_t j;
        const int gi = ec_locate(v, i, j);
        if (gi < 0) continue;
        const EcGroup& g = v.g[gi];
        const int len = ec_len(g, j);
        if (len > MIRGE_EC_MAXLEN) continue;
        const uint64_t h = ec_read_hash(v, g, j, len), e = (h & 0xFFFFFFFF00000000ull) | i;
        for (uint64_t s = h & v.tab_mask;; s = (s + 1) & v.tab_mask)
            if (atomicCAS((unsigned long long*)&rtab[s], (unsigned long long)MIRGE_EC_EMPTY, (unsigned long long)e) == MIRGE_EC_EMPTY) break;
    }
}
// raw: the raw reads (k_ec_gather) as a view whose handle indices are the raw ones; v: the new dictionary.  A raw read whose old
// handle index has no successor yet takes the new read with its length and words (there is exactly one).
__global__ void __launch_bounds__(MIRGE_BLOCK) k_ec_find(EcView raw, EcView v, const uint64_t* __restrict__ rtab, const uint32_t* __restrict__ src,
                                                         uint32_t* __restrict__ next) {
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < raw.n_reads; q += gridDim.x * blockDim.x) {
        uint32_t j;
        const int gi = ec_locate(raw, q, j);
        if (gi < 0 || next[src[q]] != MIRGE_EC_NONE) continue;
        const EcGroup &a = raw.g[gi], &g = v.g[gi];  // (a read keeps its length: the same storage group)
        const int len = ec_len(a, j), nw = (len + 31) >> 5;
        const uint64_t h = ec_read_hash(v, a, j, len);
        for (uint64_t s = h & v.tab_mask;; s = (s + 1) & v.tab_mask) {
            const uint64_t e = rtab[s];
            if (e == MIRGE_EC_EMPTY) break;  // (cannot be: the read's own letters are in the new dictionary)
            if ((e >> 32) != (h >> 32)) continue;
            const uint32_t r = (uint32_t)e - g.base;
            if (r >= g.n || ec_len(g, r) != len) continue;
            bool same = true;
            for (int w = 0; w < nw && same; w++) same = g.seq[(size_t)w * g.n + r] == a.seq[(size_t)w * a.n + j];
            if (same) { next[src[q]] = (uint32_t)e; break; }
        }
    }
}

// every ORIGINAL read follows its current read through the round: bit `bit` if that read was corrected, then its successor
__global__ void __launch_bounds__(MIRGE_BLOCK) k_ec_follow(uint32_t* __restrict__ cur, uint32_t* __restrict__ mask, uint32_t n,
                                                           const uint32_t* __restrict__ fix, const uint32_t* __restrict__ next, uint32_t n_round,
                                                           int32_t bit) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t c = cur[i];
        if (c >= n_round) continue;  // (a read without a successor: cannot be; the host sees MIRGE_EC_NONE in final_of)
        if (fix[c] != MIRGE_EC_NONE) mask[i] |= 1u << bit;
        cur[i] = next[c];
    }
}
