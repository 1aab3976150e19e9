// kernels_adapter.hpp -- part of mirge_kernels.hpp: a sample's 3' adapter from the distinct reads of its head (-a auto, mirge_adapter_infer;
// the specification is the README section "`-a auto`: the 3' adapter, inferred from the reads").
//
//   ELIGIBLE  a read without N of K .. 256 letters (the five storage groups without an N), as --kmer-correct.
//   SPECTRUM  for every K-mer x: C(x) = the sum of the counts of the eligible reads over every window start p <= P - 1 that spells x
//             (64-bit), M(x) = the mask of those p.  A direct-addressed table over all 4^K codes (first letter most significant: the
//             order of the codes is the order of the strings): no key, no probe chain, no collision.
//   SEED      the code with the largest C among those with three distinct letters, popcount(M) >= SPREAD and C >= max(32, ceil(T / 20));
//             among equal C the smallest code.
//   WALKS     left while a letter in front keeps 90 % of the sum and the spread, at most LEFT_MAX steps; then right from there while a
//             letter behind keeps half of the start's sum, up to LEN_MAX letters.
// The kernels: the table by one of two forms -- k_ad_count (a thread per read, a rolling 2-bit shift, per window one 64-bit atomic add
// and, where the bit is not there yet, one atomic or), or k_ad_nwin, a scan, k_ad_keys, one sort and k_ad_fold (store and sum: see
// there; the faster one on the adapter's hot codes, profiles/adapter_auto.md) --, k_ad_seed (grid-stride over the slots; the best
// (C, code) by wave shuffles, through LDS per workgroup, into one cell per workgroup) and k_ad_seed_last (one workgroup over those
// cells), k_ad_walk (one wave: lanes 0 .. 3 look up the four letters of a step together, a butterfly over them picks the letter),
// k_ad_probe (the slots of listed codes, for tests).
//
// Sums, ors and maxima of (C, code): nothing depends on thread order, grid size or timing.  Compiled for the host
// (MIRGE_AD_HOSTSIM, tests/hostsim/ad_sim.cpp) a launch's threads run one after the other: the reductions then go over arrays of the
// workgroup's values in the same butterfly order, and the four lanes of a step are a loop.
#pragma once

#define MIRGE_AD_K 12
#define MIRGE_AD_P 64
#define MIRGE_AD_SPREAD 6
#define MIRGE_AD_LEFT_MAX 64
#define MIRGE_AD_LEN_MAX 32
#define MIRGE_AD_SLOTS (1u << (2 * MIRGE_AD_K))
#define MIRGE_AD_CODE_MASK (MIRGE_AD_SLOTS - 1u)

struct alignas(16) AdSlot { uint64_t sum, mask; };
struct AdBest { uint64_t sum; uint32_t code, any; };  // any == 0: nothing yet
struct AdResult {  // the fields of mirge_adapter (include/mirge_native.h)
    char seq[40];
    int32_t len, left_steps, spread, pad;
    uint64_t support, eligible, seed_sum, candidates;
    uint32_t seed, start;
};

__host__ __device__ __forceinline__ AdBest ad_better(const AdBest& a, const AdBest& b) {  // commutative and associative
    const bool take_a = a.any && (!b.any || a.sum > b.sum || (a.sum == b.sum && a.code <= b.code));
    AdBest r;  // (field by field: a choice between two references would put them in scratch)
    r.sum = take_a ? a.sum : b.sum; r.code = take_a ? a.code : b.code; r.any = take_a ? a.any : b.any;
    return r;
}
__host__ __device__ __forceinline__ int ad_letters(uint32_t code) {  // distinct letters of a K-mer
    uint32_t seen = 0;
#pragma unroll
    for (int q = 0; q < MIRGE_AD_K; q++) seen |= 1u << ((code >> (2 * q)) & 3u);
    return __popc(seen);
}

// the windows of read j (eligible, `len` letters): f(code, p) for every start p <= P - 1, by a rolling 2-bit shift
template <class F>
__host__ __device__ __forceinline__ void ad_windows(const EcGroup& g, uint32_t j, int len, F f) {
    const int letters = (len - MIRGE_AD_K < MIRGE_AD_P - 1 ? len - MIRGE_AD_K : MIRGE_AD_P - 1) + MIRGE_AD_K;  // up to the last window's end
    uint32_t x = 0;
    uint64_t cur = 0;
    for (int t = 0; t < letters; t++) {
        if ((t & 31) == 0) cur = g.seq[(size_t)(t >> 5) * g.n + j];
        x = ((x << 2) | (uint32_t)(cur & 3ull)) & MIRGE_AD_CODE_MASK;
        cur >>= 2;
        if (t >= MIRGE_AD_K - 1) f(x, t - (MIRGE_AD_K - 1));
    }
}
__host__ __device__ __forceinline__ bool ad_eligible(int len) { return len >= MIRGE_AD_K && len <= MIRGE_EC_MAXLEN; }

// ---- the atomic form: every window start p <= P - 1 of every eligible read: sum += the read's count, mask |= 1 << p; total += the
// eligible reads' counts.  The adapter's codes are hot addresses: every distinct read adds to them.
__global__ void __launch_bounds__(MIRGE_BLOCK) k_ad_count(EcView v, AdSlot* tab, unsigned long long* total) {
    unsigned long long mine = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < v.n_reads; i += gridDim.x * blockDim.x) {
        uint32_t j;
        const int gi = ec_locate(v, i, j);
        if (gi < 0) continue;
        const EcGroup& g = v.g[gi];
        const int len = ec_len(g, j);
        if (!ad_eligible(len)) continue;
        const unsigned long long c = g.counts[j];
        mine += c;
        ad_windows(g, j, len, [&](uint32_t x, int p) {
            const unsigned long long bit = 1ull << p;
            atomicAdd(reinterpret_cast<unsigned long long*>(&tab[x].sum), c);
            // (once a start is known the or is skipped; a stale answer only repeats it)
            if (!(tab[x].mask & bit)) atomicOr(reinterpret_cast<unsigned long long*>(&tab[x].mask), bit);
        });
    }
    if (mine) atomicAdd(total, mine);
}

// ---- the store-and-sum form: every window stores its key code << 6 | p with the read's count, one sort by key brings a code's
// windows together, and a thread per MIRGE_AD_FOLD sorted entries sums its runs in registers: one add and one or per (thread, code)
// instead of one per window -- a hot code gets 1 / MIRGE_AD_FOLD of the atomics.  Integer sums and ors: the same table.
#define MIRGE_AD_FOLD 32
#define MIRGE_AD_NOKEY 0xFFFFFFFFu  // (a key has 30 bits: the unused tail of the key array sorts behind them)

// nwin[i] = the windows of read i (0: not eligible); total += the eligible reads' counts
__global__ void __launch_bounds__(MIRGE_BLOCK) k_ad_nwin(EcView v, uint32_t* __restrict__ nwin, unsigned long long* total) {
    unsigned long long mine = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < v.n_reads; i += gridDim.x * blockDim.x) {
        uint32_t j, w = 0;
        const int gi = ec_locate(v, i, j);
        if (gi >= 0) {
            const int len = ec_len(v.g[gi], j);
            if (ad_eligible(len)) {
                w = (uint32_t)(len - MIRGE_AD_K < MIRGE_AD_P - 1 ? len - MIRGE_AD_K : MIRGE_AD_P - 1) + 1u;
                mine += v.g[gi].counts[j];
            }
        }
        nwin[i] = w;
    }
    if (mine) atomicAdd(total, mine);
}
// off[i] = the exclusive sum of nwin: read i's windows go to keys[off[i] ..], weights[off[i] ..]
// (cap: the arrays' entries; a read whose windows would not fit writes none and raises *over -- the host's bound was wrong)
__global__ void __launch_bounds__(MIRGE_BLOCK) k_ad_keys(EcView v, const uint32_t* __restrict__ off, const uint32_t* __restrict__ nwin, uint32_t cap,
                                                         uint32_t* __restrict__ keys, uint32_t* __restrict__ weights, unsigned long long* over) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < v.n_reads; i += gridDim.x * blockDim.x) {
        uint32_t j;
        const int gi = ec_locate(v, i, j);
        if (gi < 0) continue;
        const EcGroup& g = v.g[gi];
        const int len = ec_len(g, j);
        if (!ad_eligible(len)) continue;
        const uint32_t c = g.counts[j], at = off[i];
        if (at > cap || nwin[i] > cap - at) { atomicOr(over, 1ull); continue; }
        ad_windows(g, j, len, [&](uint32_t x, int p) { keys[at + (uint32_t)p] = (x << 6) | (uint32_t)p; weights[at + (uint32_t)p] = c; });
    }
}
// keys sorted (the unused tail, MIRGE_AD_NOKEY, last): a thread per MIRGE_AD_FOLD entries
__global__ void __launch_bounds__(MIRGE_BLOCK) k_ad_fold(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ weights, uint32_t n, AdSlot* tab) {
    const uint32_t chunks = (n + MIRGE_AD_FOLD - 1) / MIRGE_AD_FOLD;
    for (uint32_t ch = blockIdx.x * blockDim.x + threadIdx.x; ch < chunks; ch += gridDim.x * blockDim.x) {
        const uint32_t e0 = ch * MIRGE_AD_FOLD, e1 = n - e0 < MIRGE_AD_FOLD ? n : e0 + MIRGE_AD_FOLD;
        uint32_t code = MIRGE_AD_NOKEY;
        unsigned long long sum = 0, mask = 0;
        for (uint32_t e = e0; e < e1; e++) {
            const uint32_t k = keys[e];
            if (k == MIRGE_AD_NOKEY) break;
            if ((k >> 6) != code) {
                if (code != MIRGE_AD_NOKEY) {
                    atomicAdd(reinterpret_cast<unsigned long long*>(&tab[code].sum), sum);
                    atomicOr(reinterpret_cast<unsigned long long*>(&tab[code].mask), mask);
                }
                code = k >> 6; sum = 0; mask = 0;
            }
            sum += weights[e];
            mask |= 1ull << (k & 63u);
        }
        if (code != MIRGE_AD_NOKEY) {
            atomicAdd(reinterpret_cast<unsigned long long*>(&tab[code].sum), sum);
            atomicOr(reinterpret_cast<unsigned long long*>(&tab[code].mask), mask);
        }
    }
}

// The workgroup's best and the sum of its n: true for the one thread that holds them.
#ifdef MIRGE_AD_HOSTSIM
static AdBest ad_sim_best[MIRGE_BLOCK];
static unsigned long long ad_sim_n[MIRGE_BLOCK];
static inline bool ad_block_reduce(AdBest& best, unsigned long long& n) {
    ad_sim_best[threadIdx.x] = best; ad_sim_n[threadIdx.x] = n;
    if (threadIdx.x != blockDim.x - 1) return false;  // (the last thread to run sees them all)
    bool some = false;
    for (unsigned l = 0; l < blockDim.x && !some; l++) some = ad_sim_best[l].any || ad_sim_n[l];
    if (!some) { best.sum = 0; best.code = 0; best.any = 0; n = 0; return true; }  // (nothing to reduce: most workgroups of a small case)
    for (unsigned o = 1; o < 64; o <<= 1)  // the wave butterflies: afterwards every lane of a wave holds the wave's
        for (unsigned w = 0; w < blockDim.x; w += 64) {
            AdBest tb[64]; unsigned long long tn[64];
            for (unsigned l = 0; l < 64; l++) { tb[l] = ad_sim_best[w + (l ^ o)]; tn[l] = ad_sim_n[w + (l ^ o)]; }
            for (unsigned l = 0; l < 64; l++) { ad_sim_best[w + l] = ad_better(ad_sim_best[w + l], tb[l]); ad_sim_n[w + l] += tn[l]; }
        }
    best = ad_sim_best[0]; n = ad_sim_n[0];
    for (unsigned w = 64; w < blockDim.x; w += 64) { best = ad_better(best, ad_sim_best[w]); n += ad_sim_n[w]; }
    return true;
}
#else
__device__ __forceinline__ AdBest ad_shfl_xor(const AdBest& b, int o) {
    AdBest t;
    t.sum = ec_shfl_xor64(b.sum, o);
    t.code = (uint32_t)__shfl_xor((int)b.code, o, 64);
    t.any = (uint32_t)__shfl_xor((int)b.any, o, 64);
    return t;
}
__device__ __forceinline__ bool ad_block_reduce(AdBest& best, unsigned long long& n) {
    __shared__ AdBest sb[MIRGE_BLOCK / 64];
    __shared__ unsigned long long sn[MIRGE_BLOCK / 64];
    for (int o = 1; o < 64; o <<= 1) {
        best = ad_better(best, ad_shfl_xor(best, o));
        n += ec_shfl_xor64(n, o);
    }
    if ((threadIdx.x & 63u) == 0) { sb[threadIdx.x >> 6] = best; sn[threadIdx.x >> 6] = n; }
    __syncthreads();
    if (threadIdx.x) return false;
    for (unsigned w = 1; w < blockDim.x >> 6; w++) { best = ad_better(best, sb[w]); n += sn[w]; }
    return true;
}
#endif

// part[workgroup] = its best seed candidate, part_n[workgroup] = its number of candidates
__global__ void __launch_bounds__(MIRGE_BLOCK) k_ad_seed(const AdSlot* __restrict__ tab, const unsigned long long* __restrict__ total,
                                                         AdBest* __restrict__ part, unsigned long long* __restrict__ part_n) {
    const unsigned long long T = *total;
    unsigned long long floor_c = T / 20 + (T % 20 ? 1 : 0);
    if (floor_c < 32) floor_c = 32;
    AdBest best; best.sum = 0; best.code = 0; best.any = 0;
    unsigned long long n = 0;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < MIRGE_AD_SLOTS; s += gridDim.x * blockDim.x) {
        const AdSlot e = tab[s];
        if (e.sum < floor_c || __popcll(e.mask) < MIRGE_AD_SPREAD || ad_letters(s) < 3) continue;
        AdBest m; m.sum = e.sum; m.code = s; m.any = 1;
        best = ad_better(best, m);
        n++;
    }
    if (ad_block_reduce(best, n)) { part[blockIdx.x] = best; part_n[blockIdx.x] = n; }
}

// one workgroup over the cells of k_ad_seed: the seed (any == 0: no candidate) and the number of candidates
__global__ void __launch_bounds__(MIRGE_BLOCK) k_ad_seed_last(const AdBest* __restrict__ part, const unsigned long long* __restrict__ part_n,
                                                              uint32_t n_part, AdBest* __restrict__ seed, unsigned long long* __restrict__ n_cand) {
    AdBest best; best.sum = 0; best.code = 0; best.any = 0;
    unsigned long long n = 0;
    for (uint32_t q = threadIdx.x; q < n_part; q += blockDim.x) { best = ad_better(best, part[q]); n += part_n[q]; }
    if (ad_block_reduce(best, n)) { *seed = best; *n_cand = n; }
}

// One step of a walk: the letter b whose code base | b << shift has the largest sum among those with sum >= need and
// popcount(mask) >= min_spread, among equal sums the smallest b; its slot -> pick.  -1: no letter qualifies.
__host__ __device__ __forceinline__ int ad_step(const AdSlot* __restrict__ tab, uint32_t base, int shift, uint64_t need, int min_spread, AdSlot& pick) {
    AdBest best; best.sum = 0; best.code = 0; best.any = 0;
#ifdef MIRGE_AD_HOSTSIM
    for (uint32_t b = 0; b < 4; b++) {
        const AdSlot e = tab[base | (b << shift)];
        AdBest m; m.sum = e.sum; m.code = b; m.any = (e.sum >= need && __popcll(e.mask) >= min_spread) ? 1u : 0u;
        best = ad_better(best, m);
    }
#else
    const uint32_t lane = threadIdx.x & 63u;
    if (lane < 4) {
        const AdSlot e = tab[base | (lane << shift)];
        best.sum = e.sum; best.code = lane;
        best.any = (e.sum >= need && __popcll(e.mask) >= min_spread) ? 1u : 0u;
    }
    best = ad_better(best, ad_shfl_xor(best, 1));
    best = ad_better(best, ad_shfl_xor(best, 2));
    // (lanes 0 .. 3 agree; the others take lane 0's)
    best.sum = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(best.sum >> 32), 0, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)best.sum, 0, 64);
    best.code = (uint32_t)__shfl((int)best.code, 0, 64);
    best.any = (uint32_t)__shfl((int)best.any, 0, 64);
#endif
    if (!best.any) return -1;
    pick = tab[base | (best.code << shift)];
    return (int)best.code;
}

// one wave: the left walk from the seed, the right walk from where it ended, the result (lane 0 writes it)
__global__ void __launch_bounds__(64) k_ad_walk(const AdSlot* __restrict__ tab, const AdBest* __restrict__ seed_in,
                                                const unsigned long long* __restrict__ n_cand, const unsigned long long* __restrict__ total,
                                                AdResult* __restrict__ out) {
#ifdef MIRGE_AD_HOSTSIM
    if (threadIdx.x) return;  // (the wave's first thread runs its lanes)
#endif
    const AdBest seed = *seed_in;
    uint32_t first = 0;
    AdSlot at; at.sum = 0; at.mask = 0;
    int32_t len = 0, left_steps = 0;
    uint64_t tail = 0;  // the letters behind the start, two bits each, the first one lowest (no array: nothing in scratch)
    if (seed.any) {
        first = seed.code;
        at = tab[first];
        for (int it = 0; it < MIRGE_AD_LEFT_MAX; it++) {
            AdSlot pick;
            const int b = ad_step(tab, first >> 2, 2 * (MIRGE_AD_K - 1), at.sum - at.sum / 10, MIRGE_AD_SPREAD, pick);  // 10 C(y) >= 9 C(first)
            if (b < 0) break;
            first = (first >> 2) | ((uint32_t)b << (2 * (MIRGE_AD_K - 1)));
            at = pick;
            left_steps++;
        }
        len = MIRGE_AD_K;
        const uint64_t need = at.sum - at.sum / 2;  // 2 C(z) >= C(start)
        uint32_t last = first;
        while (len < MIRGE_AD_LEN_MAX) {
            AdSlot pick;
            const int b = ad_step(tab, (last << 2) & MIRGE_AD_CODE_MASK, 0, need, 0, pick);
            if (b < 0) break;
            last = ((last << 2) & MIRGE_AD_CODE_MASK) | (uint32_t)b;
            tail |= (uint64_t)b << (2 * (len - MIRGE_AD_K));
            len++;
        }
    }
    if (threadIdx.x & 63u) return;
#pragma unroll
    for (int q = 0; q < 40; q++) {
        const uint32_t b = q < MIRGE_AD_K ? (first >> (2 * (MIRGE_AD_K - 1 - q))) & 3u : (uint32_t)(tail >> (2 * (q - MIRGE_AD_K))) & 3u;
        out->seq[q] = q < len ? (char)((0x54474341u >> (8 * b)) & 0xFFu) : (char)0;  // "ACGT"
    }
    out->len = len; out->left_steps = left_steps; out->spread = seed.any ? __popcll(at.mask) : 0; out->pad = 0;
    out->support = at.sum; out->eligible = *total; out->seed_sum = seed.any ? seed.sum : 0; out->candidates = *n_cand;
    out->seed = seed.any ? seed.code : 0; out->start = first;
}

// the slots of listed codes (a code past the table: zeros)
__global__ void __launch_bounds__(MIRGE_BLOCK) k_ad_probe(const AdSlot* __restrict__ tab, const uint32_t* __restrict__ codes, uint32_t n,
                                                          uint64_t* __restrict__ sum, uint64_t* __restrict__ mask) {
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) {
        const uint32_t x = codes[q];
        AdSlot e; e.sum = 0; e.mask = 0;
        if (x < MIRGE_AD_SLOTS) e = tab[x];
        sum[q] = e.sum; mask[q] = e.mask;
    }
}
