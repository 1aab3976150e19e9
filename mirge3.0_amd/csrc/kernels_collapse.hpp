// kernels_collapse.hpp -- part of mirge_kernels.hpp: collapse kernels (general hash path, partitioned key path, heads / scan / scatter).
#pragma once
// ------------------------------------------------------------------------------------------
// collapse (digest.py:141-163): open-addressing hash table of representative read indices.
//   insert : slot claimed by atomicCAS on rep[]; a later equal read finds the slot by comparing
//            its words with the representative's (the raw arrays are read-only during the kernel)
//            and adds 1 to cnt[slot][sample]; firstj[slot] = min index (first appearance).
//   heads  : read j is the head of its group iff firstj[slot_of[j]] == j; block sums of heads.
//   scatter: exclusive scan of heads = rank in order of first appearance; heads copy their read
//            and their slot's count row to the output.
// ------------------------------------------------------------------------------------------
template <int W>
__device__ __forceinline__ bool same_read(const GroupView<W>& g, uint32_t a, const MirgeRead<W>& r) {
    if (g.len[a] != (uint8_t)r.len) return false;
    bool eq = true;
#pragma unroll
    for (int w = 0; w < W; w++) {
        eq &= g.seq[(size_t)w * g.n + a] == r.w[w];
        if (g.nmask) eq &= g.nmask[(size_t)w * g.n + a] == r.nm[w];
    }
    return eq;
}

template <int W>
__global__ void k_collapse_insert(GroupView<W> g, uint32_t* __restrict__ rep, uint32_t* __restrict__ firstj,
                                  uint32_t* __restrict__ cnt, uint32_t* __restrict__ slot_of,
                                  uint32_t mask, const int32_t* __restrict__ sample_ids,
                                  const uint32_t* __restrict__ orig, uint32_t base, int32_t S, uint32_t j_lo, uint32_t j_hi,
                                  const uint32_t* __restrict__ weight) {
    __shared__ unsigned long long c_key[MIRGE_CELL_CACHE];
    __shared__ uint32_t c_min[MIRGE_CELL_CACHE];
    __shared__ uint32_t c_cnt[MIRGE_CELL_CACHE];
    for (uint32_t i = threadIdx.x; i < MIRGE_CELL_CACHE; i += blockDim.x) { c_key[i] = 0ull; c_min[i] = 0xFFFFFFFFu; c_cnt[i] = 0; }
    __syncthreads();
    for (uint32_t j = j_lo + blockIdx.x * blockDim.x + threadIdx.x; j < j_hi; j += gridDim.x * blockDim.x) {
        MirgeRead<W> r;
        load_read<W>(g, j, r);
        uint64_t h = mirge_mix64(r.w[0] ^ ((uint64_t)r.len << 56));
#pragma unroll
        for (int w = 1; w < W; w++) h = mirge_mix64(h ^ r.w[w]);
#pragma unroll
        for (int w = 0; w < W; w++) h ^= mirge_mix64(r.nm[w] + 0x9e3779b97f4a7c15ull * (w + 1));
        uint32_t s = (uint32_t)(h >> 20) & mask;
        while (true) {
            uint32_t cur = rep[s];
            if (cur == MIRGE_EMPTY) cur = atomicCAS(&rep[s], MIRGE_EMPTY, j);
            if (cur == MIRGE_EMPTY || cur == j || same_read<W>(g, cur, r)) break;
            s = (s + 1) & mask;
        }
        slot_of[j] = s;
        const uint32_t hidx = orig ? orig[j] : base + j;
        const int32_t sid = sample_ids ? sample_ids[hidx] : 0;
        const uint32_t wgt = weight ? weight[hidx] : 1u;  // a read that stands for `wgt` copies (mirge_collapse_weighted)
        // The slot now identifies the read's sequence.  Its (min index, count) update goes through a
        // workgroup cache in LDS keyed by the cell (slot, sample): a hot sequence -- adapter dimers
        // are millions of identical long reads -- then costs this workgroup one pair of global
        // atomics instead of one pair per copy (same-address device atomics run at ~90 per us).
        const unsigned long long cell = (unsigned long long)s * (unsigned)S + (unsigned)sid + 1ull;  // 0 = empty
        uint32_t cs = (uint32_t)(mirge_mix64(cell) >> 11) & (MIRGE_CELL_CACHE - 1);
        bool cached = false;
        for (int t = 0; t < 4; t++) {
            unsigned long long cur = c_key[cs];
            if (cur == 0ull) cur = atomicCAS(&c_key[cs], 0ull, cell);
            if (cur == 0ull || cur == cell) {
                atomicMin(&c_min[cs], j);
                atomicAdd(&c_cnt[cs], wgt);
                cached = true;
                break;
            }
            cs = (cs + 1) & (MIRGE_CELL_CACHE - 1);
        }
        if (!cached) {
            atomicMin(&firstj[s], j);
            atomicAdd(&cnt[(size_t)s * S + sid], wgt);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < MIRGE_CELL_CACHE; i += blockDim.x) {
        const unsigned long long cell = c_key[i];
        if (cell == 0ull) continue;
        const unsigned long long lin = cell - 1ull;
        atomicMin(&firstj[lin / (unsigned)S], c_min[i]);
        atomicAdd(&cnt[lin], c_cnt[i]);
    }
}

// Fast form for the <=31-nt group without ambiguous calls and one sample (the bulk of any run): the
// whole identity of a read -- its bits plus a length sentinel bit at 2*len -- fits one u64, so the
// table holds the key itself: a duplicate is recognised from the slot (no representative read to
// fetch), and key, first index and count share one 16-byte slot = one 64-byte sector per read
// instead of six.  first is kept as ~j under atomicMax so that a zero-filled table is "empty".
struct KeySlot {
    unsigned long long key;  // 0 = empty
    uint32_t first_inv;      // 0xFFFFFFFF - (smallest read index)
    uint32_t cnt;
};

__global__ void k_collapse_insert_key(GroupView<1> g, KeySlot* __restrict__ slots, uint32_t* __restrict__ slot_of,
                                      uint32_t mask) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < g.n; j += gridDim.x * blockDim.x) {
        const unsigned long long key = g.seq[j] | (1ull << (2 * g.len[j]));
        uint32_t s = (uint32_t)(mirge_mix64(key) >> 20) & mask;
        uint32_t seen_first = 0;
        while (true) {
            const uint4 v = *reinterpret_cast<const uint4*>(&slots[s]);  // key, first_inv, cnt in one load
            unsigned long long cur = ((unsigned long long)v.y << 32) | v.x;
            seen_first = v.z;
            if (cur == 0ull) { cur = atomicCAS(&slots[s].key, 0ull, key); seen_first = 0; }
            if (cur == 0ull || cur == key) break;
            s = (s + 1) & mask;
        }
        slot_of[j] = s;
        // first_inv only grows, so a (possibly stale) plain read that is already >= ours proves the
        // atomic would change nothing: most duplicates skip it (scattered atomics run at ~20 G/s
        // chip-wide and are what bounds this kernel)
        if (0xFFFFFFFFu - j > seen_first) atomicMax(&slots[s].first_inv, 0xFFFFFFFFu - j);
        atomicAdd(&slots[s].cnt, 1u);
    }
}

// rep[] / firstj[] = 0xFFFFFFFF, cnt[] = 0 in ONE launch (three hipMemsetAsync = six fill kernels per small group before)
__global__ void k_collapse_init(uint32_t* __restrict__ rep, uint32_t* __restrict__ firstj, uint32_t* __restrict__ cnt,
                                uint32_t tsize, uint64_t ncnt) {
    // ncnt = tsize * S cells of the count matrix: beyond 2^32 from ~24 samples x 4 M reads on, hence the 64-bit walk
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < ncnt; i += (uint64_t)gridDim.x * blockDim.x) {
        if (i < tsize) { rep[i] = MIRGE_EMPTY; firstj[i] = MIRGE_EMPTY; }
        cnt[i] = 0;
    }
}

// ------------------------------------------------------------------------------------------
// Partitioned collapse for the key path (<=31 nt, no N, one sample).  Scattered device-scope atomics
// run at ~20 G/s chip-wide, which is what bounds k_collapse_insert_key (2.4 atomics per read).  Here
// equal keys are first brought together: reads are partitioned by the top bits of their hash into
// buckets of ~1-2 k reads, then ONE workgroup de-duplicates a bucket entirely in LDS (ds_cmpst / ds_min /
// ds_add) and emits the bucket's distinct reads with their counts.
// The partition is a radix split in one or two levels whose writes are APPEND STREAMS: a writer workgroup appends
// 16-byte records to one stream per bin through an LDS cursor.  A workgroup keeps 64-512 such streams open, so a CU's
// open 128-byte lines (<= 64 KiB) stay in L2 until they are full and HBM sees whole lines -- round 1's one-level scatter
// had 256 workgroups x 8192 buckets = 2 M open streams, every 16-byte record its own sector write (the random-sector
// ceiling, 0.17-0.18 ms of the step), behind a column prefix over a 2 M-cell histogram and a scan.
//   k_part_agg   : per workgroup chunk g: LDS cache merges equal reads -> records {key, min j, count}, appended to the
//                  workgroup's region of the record's level-1 bin b1 (fixed capacity: mean x 1.25 + 8 sigma; the hash is
//                  uniform and the cache has taken the hot keys out; a region that would overflow raises the flag that
//                  already sends a call to the global-atomic path)              rec1[(b1 * G + g) * cap1 + i]
//                  and counted per FINAL bucket                                 hist[g][b]
//   k_part_split : (two levels, B > 64) workgroup (b1, w) owns G / W2 of bin b1's regions: their hist rows give the
//                  exact size of every bucket's share, so the records are appended at exact offsets inside the
//                  workgroup's slab -- no capacity to overflow, however many copies of a read there are
//                                                                               rec2[(b1 * W2 + w) * slab + off[b2] + i]
//   k_part_dedup : per bucket, LDS table (key -> min j, count) over the bucket's R shares (R = G regions of level 1, or W2
//                  slab ranges); the distinct reads of MIRGE_DEDUP_K buckets are written to the output at a range reserved with
//                  one global atomicAdd (so the order of the unique reads of this path is unspecified; first[] carries the
//                  first raw index); a workgroup walks several buckets, their global round trips overlapped (see the kernel)
// ------------------------------------------------------------------------------------------
#ifndef MIRGE_PART_CAP
#define MIRGE_PART_CAP 4096  // largest LDS table per bucket (16 B per slot = 64 KiB)
#endif
#ifndef MIRGE_PART_B1
#define MIRGE_PART_B1 64       // level-1 bins (and the largest one-level partition)
#endif
#ifndef MIRGE_PART_SMALL
#define MIRGE_DEDUP_SHARDS 8          // output cursors of k_part_dedup (shards of its staging area)
#define MIRGE_DEDUP_SHARD_STRIDE 1024  // words between two cursors: 4 KiB, a memory channel of its own each
#define MIRGE_PART_SMALL 1600  // reads per bucket up to which k_part_dedup uses its 2048-slot table
#endif
#ifndef MIRGE_PART_W2
#define MIRGE_PART_W2 4       // splitter workgroups per level-1 bin (64 x 4 = one per CU)
#endif
#define MIRGE_PART_MAXREG 256  // regions a consumer workgroup reads (G <= 256 writers, or W2 splitters)

__device__ __forceinline__ unsigned long long read_key64(const GroupView<1>& g, uint32_t j) {
    return g.seq[j] | (1ull << (2 * g.len[j]));
}

// item i of a list of regions whose fill counts have the inclusive prefix pre[0..R): region and offset inside it
__device__ __forceinline__ uint32_t region_of(const uint32_t* pre, uint32_t R, uint32_t i, uint32_t& within) {
    uint32_t lo = 0, hi = R;  // first r with pre[r] > i
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (pre[mid] > i) hi = mid; else lo = mid + 1;
    }
    within = i - (lo ? pre[lo - 1] : 0u);
    return lo;
}

// inclusive prefix of up to MIRGE_PART_MAXREG region counts (clamped to cap) into LDS, by the first wave(s); returns total
__device__ __forceinline__ uint32_t region_prefix(const uint32_t* __restrict__ cnt, uint32_t R, uint32_t cap, uint32_t* pre) {
    for (uint32_t r = threadIdx.x; r < R; r += blockDim.x) pre[r] = min(cnt[r], cap);
    __syncthreads();
    if (threadIdx.x == 0) {  // R <= 256: a serial pass over LDS costs less than the barriers of a block scan
        uint32_t run = 0;
        for (uint32_t r = 0; r < R; r++) { run += pre[r]; pre[r] = run; }
    }
    __syncthreads();
    return R ? pre[R - 1] : 0u;
}

// k_part_agg: a workgroup walks its chunk of reads through a small LDS cache (key -> min index,
// count) before anything is partitioned.  Real small-RNA samples are extremely skewed (one miRNA can be
// a third of all reads): without this the hot key's bucket holds millions of records for ONE workgroup
// and every LDS atomic on it is a 64-way conflict (measured on a Zipf sample: 10.9 ms per step against
// 2.8 ms on unskewed reads).  With it a key contributes at most one record per workgroup.  The cache is
// best effort: a read that finds no slot within 4 probes is emitted as a record of count 1.
// One workgroup per CU (the LDS cache takes a good part of a CU's LDS), so the workgroup itself must bring
// the waves that hide its load and LDS latencies: 1024 threads = 16 waves per CU (256 threads: 0.26 ms, 2x slower)
#ifndef MIRGE_PART_THREADS
#define MIRGE_PART_THREADS 1024
#endif
#ifndef MIRGE_AGG_BUCKET4
#define MIRGE_AGG_BUCKET4 1
#endif
#ifndef MIRGE_AGG_UNROLL
#define MIRGE_AGG_UNROLL 2  // (measured, round 5: 0.131 -> 0.122 ms per 9.6 M reads; 4 reads per trip: the same)
#endif
__global__ void __launch_bounds__(MIRGE_PART_THREADS)
k_part_agg(GroupView<1> g, const uint32_t* __restrict__ orig, uint32_t base, uint32_t chunk, uint32_t shift1, uint32_t NB1,
           uint32_t bshift, uint32_t B, uint32_t CS, uint32_t cap1, uint4* __restrict__ rec1, uint32_t* __restrict__ cnt1,
           uint32_t* __restrict__ hist, uint32_t* __restrict__ overflow, uint32_t* __restrict__ n_records, uint32_t* __restrict__ shard_cur) {
    if (shard_cur && blockIdx.x == 0 && threadIdx.x < MIRGE_DEDUP_SHARDS) shard_cur[threadIdx.x * MIRGE_DEDUP_SHARD_STRIDE] = 0u;  // k_part_dedup's cursors
    extern __shared__ __attribute__((aligned(16))) unsigned long long lds_a[];  // [CS] keys | [CS] minj | [CS] cnt | [NB1] cursors | [B] hist
    uint32_t* c_min = reinterpret_cast<uint32_t*>(lds_a + CS);
    uint32_t* c_cnt = c_min + CS;
    uint32_t* cur = c_cnt + CS;
    uint32_t* lds_h = cur + NB1;  // records per final bucket (two levels only: hist != nullptr)
    for (uint32_t i = threadIdx.x; i < CS; i += blockDim.x) { lds_a[i] = 0ull; c_min[i] = 0xFFFFFFFFu; c_cnt[i] = 0; }
    for (uint32_t b = threadIdx.x; b < NB1; b += blockDim.x) cur[b] = 0;
    if (hist) for (uint32_t b = threadIdx.x; b < B; b += blockDim.x) lds_h[b] = 0;
    __syncthreads();
    const uint32_t lo = blockIdx.x * chunk, hi = min(lo + chunk, g.n);
    const uint32_t G = gridDim.x;
    auto append = [&](unsigned long long key, uint64_t h, uint32_t jr, uint32_t count) {
        const uint32_t b1 = (uint32_t)(h >> shift1);
        const uint32_t p = atomicAdd(&cur[b1], 1u);
        if (p < cap1) {
            rec1[((size_t)b1 * G + blockIdx.x) * cap1 + p] = make_uint4((uint32_t)key, (uint32_t)(key >> 32), jr, count);
            if (hist) atomicAdd(&lds_h[(uint32_t)(h >> bshift)], 1u);
        }
    };
    // MIRGE_AGG_UNROLL reads per thread and trip, their loads (key, length, raw index) issued together: with one workgroup per CU
    // the kernel is a chain of load -> LDS-atomic latencies, and sixteen waves with one load each in flight do not cover HBM
    for (uint32_t j0 = lo; j0 < hi; j0 += blockDim.x * MIRGE_AGG_UNROLL) {
        unsigned long long keys[MIRGE_AGG_UNROLL];
        uint32_t jrs[MIRGE_AGG_UNROLL];
#pragma unroll
        for (int u = 0; u < MIRGE_AGG_UNROLL; u++) {
            const uint32_t j = j0 + u * blockDim.x + threadIdx.x;
            keys[u] = 0ull; jrs[u] = 0;
            if (j < hi) {
                keys[u] = read_key64(g, j);
                // index among ALL raw reads (orig[] ascends with j, so min commutes; read coalesced here
                // instead of gathered per unique read at the end)
                jrs[u] = orig ? orig[j] : base + j;
            }
        }
#pragma unroll
        for (int u = 0; u < MIRGE_AGG_UNROLL; u++) {
        const uint32_t j = j0 + u * blockDim.x + threadIdx.x;
        bool direct = false;
        unsigned long long key = keys[u];
        uint32_t jr = jrs[u];
        uint64_t h = 0;
        if (j < hi) {
            h = mirge_mix64(key);
            direct = true;
#if MIRGE_AGG_BUCKET4
            // the cache as 4-way buckets (round 5): the four keys of the read's home bucket come with ONE 32-byte read (two
            // ds_read_b128 issued together) instead of up to four dependent probes; a key lives in the first slot of its bucket
            // that was free when it arrived (slots never change once set, every inserter walks them in order and takes the
            // compare-and-swap's word for what a slot holds: no key can sit in two slots), so a later copy always finds it
            const uint32_t b0 = ((uint32_t)(h >> 9) & (CS / 4 - 1)) * 4;
            const ulonglong2 ka = *reinterpret_cast<const ulonglong2*>(&lds_a[b0]);
            const ulonglong2 kb = *reinterpret_cast<const ulonglong2*>(&lds_a[b0 + 2]);
            const unsigned long long k4[4] = {ka.x, ka.y, kb.x, kb.y};
            int slot = -1;
#pragma unroll
            for (int t = 0; t < 4; t++) if (slot < 0 && k4[t] == key) slot = t;
            if (slot < 0) {
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    if (slot >= 0 || k4[t] != 0ull) continue;  // (held by another key when read: it still is)
                    const unsigned long long c0 = atomicCAS(&lds_a[b0 + t], 0ull, key);
                    if (c0 == 0ull || c0 == key) slot = t;
                }
            }
            if (slot >= 0) {
                const uint32_t s = b0 + (uint32_t)slot;
                if (*(volatile uint32_t*)&c_min[s] > jr) atomicMin(&c_min[s], jr);
                atomicAdd(&c_cnt[s], 1u);
                direct = false;
            }
#else
            uint32_t s = (uint32_t)(h >> 9) & (CS - 1);
            // four probes, always: a hot key that was displaced from its home slot when it arrived must still be found by its
            // later copies (looking at the home slot only once the cache is full was 6 % faster on unskewed reads and sent
            // every copy of such a key to its bin as a record of its own on a Zipf sample)
            for (int t = 0; t < 4; t++) {
                unsigned long long c0 = lds_a[s];
                if (c0 == 0ull) c0 = atomicCAS(&lds_a[s], 0ull, key);
                if (c0 == 0ull || c0 == key) {
                    // the slot's minimum only falls: a plain read that is already below ours proves the atomic would
                    // change nothing (indices grow with the loop, so this skips it for every later copy of a read)
                    if (*(volatile uint32_t*)&c_min[s] > jr) atomicMin(&c_min[s], jr);
                    atomicAdd(&c_cnt[s], 1u);
                    direct = false;
                    break;
                }
                s = (s + 1) & (CS - 1);
            }
#endif
        }
        // cache full around this key: the read itself becomes a record.  Copies of ONE sequence that meet in a wave are
        // merged first (two rounds: the key of the first such lane, then of the first lane left) -- a burst of a sequence that
        // arrives after the cache has filled is then one record per wave, not 64 for one level-1 region
        uint32_t count = 1;
        bool open = direct;  // not yet looked at as a group's key
#pragma unroll
        for (int round = 0; round < 2; round++) {
            const unsigned long long ob = __ballot(open);
            if (!ob) break;
            const int lead = __ffsll(ob) - 1;
            const unsigned long long k0 = __shfl(key, lead, 64);
            const bool same = open && key == k0;
            const unsigned long long sb = __ballot(same);
            if (__popcll(sb) > 1) {
                uint32_t mn = same ? jr : 0xFFFFFFFFu;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) mn = min(mn, (uint32_t)__shfl_xor((int)mn, o, 64));
                if ((threadIdx.x & 63) == lead) { jr = mn; count = (uint32_t)__popcll(sb); }
                else if (same) direct = false;  // the leader carries the group
            }
            open = open && !same;
        }
        if (direct) append(key, h, jr, count);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < CS; i += blockDim.x) {  // flush the cache
        const unsigned long long key = lds_a[i];
        if (key != 0ull) append(key, mirge_mix64(key), c_min[i], c_cnt[i]);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < NB1; b += blockDim.x) {
        const uint32_t n = cur[b];
        cnt1[(size_t)b * G + blockIdx.x] = min(n, cap1);
        if (n > cap1) atomicOr(overflow, 1u);
    }
    // (round 6) the sample's record count: what k_part_dedup chooses its output mode from -- on the device, for THIS sample (until
    // round 5 the host chose from the context's previous sample).  ONE add per workgroup: an add per level-1 bin was 16 384 adds on one
    // address, served one after the other at 11.6 ns -- 0.19 ms of atomic traffic that was still draining under k_part_split and
    // k_part_dedup, whose own cursor adds queued behind it (k_part_dedup 0.116 -> 0.130 ms).
    if (threadIdx.x == 0) {
        uint32_t mine = 0;
        for (uint32_t b = 0; b < NB1; b++) mine += min(cur[b], cap1);
        atomicAdd(n_records, mine);
    }
    if (hist) for (uint32_t b = threadIdx.x; b < B; b += blockDim.x) hist[(size_t)blockIdx.x * B + b] = lds_h[b];
}

// k_part_split: second radix level.  Workgroup (b1 = blockIdx / W2, w = blockIdx % W2) takes the regions
// [w * RPW, (w + 1) * RPW) of level-1 bin b1 (coalesced reads of ~0.6 k records each).  The hist rows of those writers
// give the exact number of records per final bucket b1 * NB2 + b2, so every record is appended at an exact offset of
// the workgroup's slab; the bucket's share is published as (offset, count) for k_part_dedup.
__global__ void __launch_bounds__(MIRGE_PART_THREADS)
k_part_split(const uint4* __restrict__ rec1, const uint32_t* __restrict__ cnt1, const uint32_t* __restrict__ hist, uint32_t G,
             uint32_t B, uint32_t cap1, uint32_t W2, uint32_t RPW, uint32_t shift2, uint32_t NB2, uint64_t slab,
             uint4* __restrict__ rec2, uint32_t* __restrict__ off2, uint32_t* __restrict__ cnt2) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_s[];  // [MAXREG] prefix | [NB2] cursors (start at the bucket's offset)
    uint32_t* pre = lds_s;
    uint32_t* cur = lds_s + MIRGE_PART_MAXREG;
    __shared__ uint32_t scan_tmp[MIRGE_PART_THREADS / 64 + 1];
    const uint32_t b1 = blockIdx.x / W2, w = blockIdx.x % W2;
    const uint32_t r0 = w * RPW, R = r0 < G ? min(RPW, G - r0) : 0u;
    // this workgroup's records per bucket, then their exclusive prefix = the buckets' offsets in the slab (NB2 <= 512 <= threads)
    uint32_t mine = 0;
    if (threadIdx.x < NB2)
        for (uint32_t r = 0; r < R; r++) mine += hist[(size_t)(r0 + r) * B + (size_t)b1 * NB2 + threadIdx.x];
    uint32_t tot_all;
    const uint32_t off = block_excl_scan<MIRGE_PART_THREADS / 64>(mine, tot_all, scan_tmp);
    if (threadIdx.x < NB2) {
        cur[threadIdx.x] = off;
        const size_t cell = ((size_t)b1 * NB2 + threadIdx.x) * W2 + w;
        off2[cell] = off;
        cnt2[cell] = mine;
    }
    for (uint32_t r = threadIdx.x; r < R; r += blockDim.x) pre[r] = min(cnt1[(size_t)b1 * G + r0 + r], cap1);
    __syncthreads();  // publishes cur[] and the regions' fill counts
    const uint4* in = rec1 + ((size_t)b1 * G + r0) * cap1;
    uint4* out = rec2 + (size_t)blockIdx.x * slab;
    // a wave takes whole regions: 64 consecutive records per load, no search for the region of an item
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n_waves = blockDim.x >> 6;
    for (uint32_t r = wave; r < R; r += n_waves) {
        const uint32_t n = pre[r];
        const uint4* src = in + (size_t)r * cap1;
        // four loads in flight per lane: with 16 waves on a CU the kernel is a chain of load -> LDS atomic -> store
        // latencies, not bandwidth
        for (uint32_t i0 = lane; i0 < n; i0 += 256) {
            uint4 rec[4];
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (i0 + 64 * u < n) rec[u] = src[i0 + 64 * u];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (i0 + 64 * u >= n) continue;
                const unsigned long long key = ((unsigned long long)rec[u].y << 32) | rec[u].x;
                const uint32_t b2 = (uint32_t)(mirge_mix64(key) >> shift2) & (NB2 - 1);
                out[atomicAdd(&cur[b2], 1u)] = rec[u];
            }
        }
    }
}

// ---- k_part_dedup: persistent and software-pipelined over the buckets of a workgroup -------------------------------------------
// What the kernel used to spend its time on (profiles/README.md round 5, profiles/dedup_pipelined.md): a bucket was a chain of four
// DEPENDENT global round trips with barriers between them -- the shares' cnt / off words, the records, the returning add on the
// output cursor, the output stores -- ~12 us per bucket whether it held 150 or 1 000 records, 1 024 buckets resident on the chip,
// 8 192 buckets: 8 x 12 us.  Not the cursor (8 192 adds in 0.11 ms arrive 13.5 ns apart and are served in 11.6 ns), not the
// records (1.5 per thread).  Here a workgroup STAYS (grid = the resident workgroups) and walks buckets w, w + grid, w + 2 grid, ...
// with the round trips of consecutive buckets overlapped:
//   while bucket i is inserted into the LDS table    the cnt / off words of bucket i + 2 are in flight (lanes 0..7 of every wave,
//                                                    one register)
//   behind bucket i's insert                         the first MIRGE_DEDUP_DEPTH records per thread of bucket i + 1 are asked for --
//                                                    into the registers bucket i's were just taken from: a second set beside K
//                                                    read-outs does not fit 64 VGPRs -- and are in flight behind the barrier, the
//                                                    last group's stores, the read-out, the scan and the reservation
//   behind the barrier                               every thread reads its PER slots out into registers and clears them: the table
//                                                    is free for bucket i + 1 without waiting for anything global
//   one reservation per MIRGE_DEDUP_K buckets        the read-outs of K buckets stay in registers, ONE returning add reserves their
//                                                    output range, and the add is waited for -- and the stores are issued -- BEHIND
//                                                    the insert of the next bucket
// No workgroup waits for another one.  The one-level partition (R = G > 4 shares, samples of up to 131 072 reads) walks its
// buckets in the same loop with the plain chain (prefix and offsets through LDS, a search per record, nothing asked for ahead);
// its reservations are grouped and its stores deferred in the same way.
#ifndef MIRGE_DEDUP_K
#define MIRGE_DEDUP_K 2      // buckets per output reservation (the cursor's floor is 8 192 x 11.6 ns / K per 10 M reads)
#endif
#ifndef MIRGE_DEDUP_DEPTH
#define MIRGE_DEDUP_DEPTH 2  // records per thread that are loaded one bucket ahead (K and DEPTH: <= 64 VGPRs at CAP = 2048, no scratch)
#endif

// a bucket's (up to four) shares of the two-level partition: inclusive ends of shares 0..2, the total, where each share starts
// inside its slab, the first slab's record index -- wave-uniform, in scalar registers
struct DedupShares {
    uint32_t e0, e1, e2, total, o0, o1, o2, o3;
    size_t base;
};
// lanes 0..3 of every wave hold the count of share `lane`, lanes 4..7 the offset of share `lane - 4` (0 beyond R): ONE register
__device__ __forceinline__ DedupShares dedup_shares(uint32_t co, uint32_t cap32, size_t base) {
    DedupShares s;
    s.e0 = min((uint32_t)__builtin_amdgcn_readlane((int)co, 0), cap32);
    s.e1 = s.e0 + min((uint32_t)__builtin_amdgcn_readlane((int)co, 1), cap32);
    s.e2 = s.e1 + min((uint32_t)__builtin_amdgcn_readlane((int)co, 2), cap32);
    s.total = s.e2 + min((uint32_t)__builtin_amdgcn_readlane((int)co, 3), cap32);
    s.o0 = (uint32_t)__builtin_amdgcn_readlane((int)co, 4);
    s.o1 = (uint32_t)__builtin_amdgcn_readlane((int)co, 5);
    s.o2 = (uint32_t)__builtin_amdgcn_readlane((int)co, 6);
    s.o3 = (uint32_t)__builtin_amdgcn_readlane((int)co, 7);
    s.base = base;
    return s;
}
__device__ __forceinline__ size_t dedup_record_at(const DedupShares& s, uint64_t rcap, uint32_t i) {
    return s.base + (i < s.e0 ? (size_t)s.o0 + i : i < s.e1 ? rcap + s.o1 + (i - s.e0) : i < s.e2 ? 2 * rcap + s.o2 + (i - s.e1) : 3 * rcap + s.o3 + (i - s.e2));
}

// CAP = LDS table slots (16 B each): 2048 when the buckets hold <= 1024 records (4 workgroups per CU), else 4096
// The table takes 32-64 KiB of LDS, so only 2-4 workgroups fit a CU: 1024-thread workgroups bring the waves.
// The bucket's records lie in R shares: share r holds cnt[bucket * R + r] records (clamped to rcap) from
// rec[(bucket * R + r) * rcap]  (off == nullptr: level-1 regions), or from rec[((bucket / NB2) * R + r) * rcap + off[bucket * R + r]]
// (ranges inside the level-2 slabs of capacity rcap).
#ifndef MIRGE_DEDUP_THREADS
// 512 threads: four workgroups per CU are resident (a CU holds 2048 threads: with 1024 only two of the four the 2048-slot table
// leaves room for), their barrier phases overlap: 0.140 -> 0.126 ms per 9.6 M reads (256 threads: 0.132)
#define MIRGE_DEDUP_THREADS 512
#endif
// Grid: the resident workgroups (n_cu x 4 at CAP = 2048, x 2 at 4096), never more than the B buckets; any grid in 1..B is correct.
// (waves per SIMD: the residency the tables allow -- 4 x 512 threads per CU = 8 waves per SIMD = 64 VGPRs at CAP = 2048, half that at 4096 --
//  is the register budget the compiler is held to: the persistent grid is sized for exactly that residency)
// FEW: the bucket's records lie in R <= 4 shares (the two-level partition) -- an instance of its own, or the one-level partition's
// prefix, search and addresses sit in the pipelined loop's register budget
template <int CAP, bool FEW>
__global__ void __launch_bounds__(MIRGE_DEDUP_THREADS) __attribute__((amdgpu_waves_per_eu(CAP <= 2048 ? 8 : 4)))
k_part_dedup(const uint4* __restrict__ rec, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off, uint32_t R,
             uint64_t rcap, uint32_t NB2, uint32_t B, uint64_t* __restrict__ useq, uint8_t* __restrict__ ulen,
             uint32_t* __restrict__ ucnt, uint32_t* __restrict__ ufirst, uint32_t* __restrict__ cursor,
             uint32_t* __restrict__ hist, uint32_t* __restrict__ overflow, uint32_t* __restrict__ shard_cur_in, uint32_t shard_cap,
             const uint32_t* __restrict__ n_records, uint32_t rec_thresh, uint64_t* __restrict__ sseq, uint8_t* __restrict__ slen, uint32_t* __restrict__ scnt,
             uint32_t* __restrict__ sfirst) {
    constexpr int T = MIRGE_DEDUP_THREADS, PER = CAP / T, K = MIRGE_DEDUP_K, D = MIRGE_DEDUP_DEPTH;
    static_assert(PER % 4 == 0 && K >= 2 && D >= 1, "a thread reads its slots out with 16-byte LDS operations");
    // Output mode, chosen HERE from the sample's record count (*n_records, written by k_part_agg; a line of its own): few records =
    // few unique reads per bucket = short buckets, whose reservations then come faster than one cursor serves them (11.6 ns per
    // returning add) -> eight cursors into the staging arrays (s*), k_part_compact closes the gaps; many records -> the one cursor,
    // straight into the output arrays (and k_part_compact returns at once).  Uniform over the launch: every workgroup reads the same
    // word, ONCE, by ONE thread (every lane asking was 65 k requests for one address per launch: a hot spot on one L2 channel), with a
    // VECTOR load (an address the compiler cannot prove uniform: a scalar load would be waited for at the kernel's first
    // `s_waitcnt lgkmcnt(0)` -- scalar loads and LDS operations share that counter), looked at in front of the workgroup's first barrier (the first bucket's share words were asked for with it).
    uint32_t lane_zero = 0u;
    asm volatile("" : "+v"(lane_zero));  // (a zero in a vector register the compiler cannot see through)
    uint32_t n_rec_now = 0u;
    if (threadIdx.x == 0 && shard_cur_in) n_rec_now = n_records[lane_zero];
    extern __shared__ __attribute__((aligned(16))) unsigned long long lds_k[];  // [CAP] keys, then [CAP] minj, [CAP] cnt
    uint32_t* lds_min = reinterpret_cast<uint32_t*>(lds_k + CAP);
    uint32_t* lds_cnt = lds_min + CAP;
    uint32_t* lds_x = lds_cnt + CAP;  // [0] distinct keys, [1] output base, [2..17] scan scratch, [18] the mode, [32..63] lengths (<= 31 nt)
    uint32_t* pre = lds_x + 64;       // [MAXREG] inclusive prefix of the regions' fill counts (one-level partition)
    uint32_t* roff = pre + MIRGE_PART_MAXREG;  // where share r starts inside its region
    uint32_t& n_distinct = lds_x[0];
    {   // clear with 16-byte stores: keys and counts to 0, first indices to ~0.  Once per workgroup: afterwards the read-out clears
        uint4* k4 = reinterpret_cast<uint4*>(lds_k);
        for (uint32_t i = threadIdx.x; i < CAP / 2; i += T) k4[i] = make_uint4(0u, 0u, 0u, 0u);
        uint4* m4 = reinterpret_cast<uint4*>(lds_min);
        for (uint32_t i = threadIdx.x; i < CAP / 4; i += T) m4[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
        uint4* c4 = reinterpret_cast<uint4*>(lds_cnt);
        for (uint32_t i = threadIdx.x; i < CAP / 4; i += T) c4[i] = make_uint4(0u, 0u, 0u, 0u);
    }
    for (uint32_t i = threadIdx.x; i < 32 + 32; i += T)
        if (i != 18) lds_x[i] = 0;  // key-path reads are <= 31 nt; [18] is thread 0's to write in front of the first barrier
    const uint32_t cap32 = (uint32_t)min(rcap, (uint64_t)0xFFFFFFFFu);
    const uint32_t grid = gridDim.x;
    // the thread's index as the bucket loop sees it: made opaque once per trip (below), or the compiler hoists every predicate
    // of it (the scan's lane masks, `tid == 0`, `lane < R`, ...) out of the loop as scalar register pairs and then spills them
    uint32_t tid = threadIdx.x;

    // one record into the table (a record stands for rc.w identical reads of one k_part_agg chunk).  `counted`: a bucket with fewer
    // records than the table has slots cannot fill it: the distinct-key counter (one LDS atomic on a single address per new key,
    // serialised over the lanes) is kept for the oversized buckets only
    auto insert = [&](const uint4 rc, const bool counted) {
        const unsigned long long key = ((unsigned long long)rc.y << 32) | rc.x;
        const uint32_t j = rc.z;
        uint32_t s = (uint32_t)(mirge_mix64(key) >> 7) & (CAP - 1);
        while (true) {
            unsigned long long c0 = lds_k[s];
            if (c0 == 0ull) {
                c0 = atomicCAS(&lds_k[s], 0ull, key);
                if (counted && c0 == 0ull && atomicAdd(&n_distinct, 1u) >= CAP - 64) atomicOr(overflow, 1u);
            }
            if (c0 == 0ull || c0 == key) break;
            if (counted && *(volatile uint32_t*)&n_distinct >= CAP - 32) break;  // table full: flagged, results discarded
            s = (s + 1) & (CAP - 1);
        }
        if (*(volatile uint32_t*)&lds_min[s] > j) atomicMin(&lds_min[s], j);
        atomicAdd(&lds_cnt[s], rc.w);
    };
    // the read-out of a bucket: a thread's PER slots, in registers (PER x 4 dwords), and the table cleared behind them
    struct ReadOut {
        unsigned long long key[PER];
        uint32_t mn[PER], ct[PER];
    };
    ReadOut ro[K];
    static_assert(K * 16 <= 32 && CAP <= 65536, "a thread's K ranks share one register");
    uint32_t ranks = 0u, tot[K];  // a thread's rank among its bucket's distinct keys (16 bits each, ro[q]'s at 16 q); the bucket's distinct keys
    auto read_out = [&](ReadOut& o, uint32_t& rk, uint32_t& total) {
        const uint32_t s0 = tid * PER;
        uint32_t mine = 0, zero = 0u;
        asm volatile("" : "+v"(zero));  // (made HERE: the compiler kept eight registers of 0 and ~0 for these stores across the whole loop)
        const uint32_t ones = ~zero;
#pragma unroll
        for (int p = 0; p < PER; p += 2) {
            ulonglong2* at = reinterpret_cast<ulonglong2*>(&lds_k[s0 + p]);
            const ulonglong2 k2 = *at;
            *at = make_ulonglong2((unsigned long long)zero, (unsigned long long)zero);
            o.key[p] = k2.x; o.key[p + 1] = k2.y;
            mine += (k2.x != 0ull) + (k2.y != 0ull);
        }
#pragma unroll
        for (int p = 0; p < PER; p += 4) {
            uint4* am = reinterpret_cast<uint4*>(&lds_min[s0 + p]);
            uint4* ac = reinterpret_cast<uint4*>(&lds_cnt[s0 + p]);
            const uint4 m = *am, c = *ac;
            *am = make_uint4(ones, ones, ones, ones);
            *ac = make_uint4(zero, zero, zero, zero);
            o.mn[p] = m.x; o.mn[p + 1] = m.y; o.mn[p + 2] = m.z; o.mn[p + 3] = m.w;
            o.ct[p] = c.x; o.ct[p + 1] = c.y; o.ct[p + 2] = c.z; o.ct[p + 3] = c.w;
        }
        if (tid == 0) n_distinct = 0u;
        // (the scan's barriers stand between these clears and the next bucket's inserts)
        rk = block_excl_scan<T / 64>(mine, total, lds_x + 2, tid);
        total = (uint32_t)__builtin_amdgcn_readfirstlane((int)total);
    };
    // Where a group of buckets' unique reads go: one thread reserves their range with ONE returning add -- on the one global cursor
    // (served one after the other, 11.6 ns each: 8 192 / K adds per 10 M reads), or, with shards, on cursor x (each on a line and
    // channel of its own) for a range in that shard's stretch of the staging area; k_part_compact closes the gaps between the
    // stretches afterwards.  The add is ISSUED here and its answer LOOKED AT in publish_base, one insert later.
    const uint32_t* shard_cur = nullptr;  // (shard_cur_in or nullptr, the same in every thread: set by take_mode)
    // (by thread 8, into `res_o`: a lane of the register in which lanes 0..7 of every wave keep the next shares in flight -- a
    //  register of its own for one thread's answer did not fit 64 VGPRs)
    uint32_t res_total = 0u, res_x = 0u, n_groups = 0u;
    auto reserve = [&](uint32_t& res_o, uint32_t total) {
        res_total = total;
        res_x = (blockIdx.x + n_groups++) % MIRGE_DEDUP_SHARDS;
        if (tid == 8 && total) res_o = shard_cur ? atomicAdd(&shard_cur_in[res_x * MIRGE_DEDUP_SHARD_STRIDE], total) : atomicAdd(cursor, total);
    };
    auto publish_base = [&](uint32_t res_o) {  // (a barrier follows)
        if (tid == 8) {
            uint32_t at = 0;
            if (res_total) {
                if (shard_cur) {
                    if (res_o + res_total > shard_cap) { atomicOr(overflow, 1u); at = 0xFFFFFFFFu; }  // (no room: nothing is written, the call is redone)
                    else at = res_x * shard_cap + res_o;
                } else at = res_o;
            }
            lds_x[1] = at;
        }
    };
    // the mode, for the other threads: thread 0 writes it in front of the workgroup's first barrier, everyone reads it behind it and
    // takes the staging arrays for the output arrays from there on
    auto publish_mode = [&]() { if (tid == 0) lds_x[18] = (shard_cur_in && n_rec_now < rec_thresh) ? 1u : 0u; };
    auto take_mode = [&]() {
        if (__builtin_amdgcn_readfirstlane((int)lds_x[18])) { shard_cur = shard_cur_in; useq = sseq; ulen = slen; ucnt = scnt; ufirst = sfirst; }
    };
    auto emit = [&](const ReadOut& o, uint32_t r) {  // r: where this thread's first distinct key goes
#pragma unroll
        for (int p = 0; p < PER; p++) {
            const unsigned long long key = o.key[p];
            if (key == 0ull) continue;
            const int L = (63 - __clzll((long long)key)) >> 1;  // the sentinel bit sits at 2*len
            useq[r] = key ^ (1ull << (2 * L));
            ulen[r] = (uint8_t)L;
            ucnt[r] = o.ct[p];
            ufirst[r] = o.mn[p];
            if (hist) atomicAdd(&lds_x[32 + L], 1u);
            r++;
        }
    };
    auto emit_group = [&](uint32_t n) {  // the last n read-outs (the newest is ro[K - 1]), back to back from the published base
        const uint32_t at = lds_x[1];
        if (at == 0xFFFFFFFFu) return;
        uint32_t run = at;
#pragma unroll
        for (int q = 0; q < K; q++)
            if ((uint32_t)(K - q) <= n) { emit(ro[q], run + ((ranks >> (16 * q)) & 0xFFFFu)); run += tot[q]; }
    };

    // ---- the bucket loop.  FEW (R <= 4 shares per bucket, the two-level partition: every sample above 131 072 reads): the pipeline of
    // the header; otherwise the one-level partition's plain chain in the same loop ----
    constexpr bool few = FEW;
    const uint32_t m = (B - blockIdx.x + grid - 1) / grid;  // this workgroup's buckets: blockIdx.x + i * grid, i < m
    const uint32_t nb2_lg = off ? (uint32_t)__builtin_ctz(NB2) : 0u;  // (B and the level-1 bins are powers of two)
    auto bucket_base = [&](uint32_t i) { return (size_t)((blockIdx.x + i * grid) >> nb2_lg) * R * rcap; };
    // lanes 0..7 of every wave: the shares' counts and offsets.  Held across a bucket only while they are in flight (nco: the
    // bucket after the next); of the next bucket the record count alone is kept, in a scalar register -- a bucket with more
    // records than were asked for ahead asks for its shares again (the L2 has them)
    auto ask_shares = [&](uint32_t i, uint32_t& co) {  // (lanes 0..7 only: thread 8 keeps its reservation in the same register)
        const uint32_t lane = tid & 63u, r = lane & 3u;
        if (lane < 8u) {
            co = 0u;
            if (few && i < m && r < R && (lane < 4u || off)) {
                const size_t cell = (size_t)(blockIdx.x + i * grid) * R + r;
                co = (lane < 4u ? cnt : off)[cell];
            }
        }
    };
    uint4 pf[D];  // the first D records per thread of the next bucket, in flight
    auto ask_records = [&](uint32_t i, uint32_t co) {  // returns the bucket's records
        const DedupShares s = dedup_shares(co, cap32, bucket_base(i));
#pragma unroll
        for (int u = 0; u < D; u++) {
            const uint32_t j = tid + u * T;
            if (j < s.total) pf[u] = rec[dedup_record_at(s, rcap, j)];
        }
        return s.total;
    };
    uint32_t nco = 0u;  // lanes 0..7 of every wave: shares in flight; thread 8: the answer of the returning add in flight (res_o)
    ask_shares(0, nco);
    uint32_t total_next = ask_records(0, nco);  // (no share, no record: the one-level partition)
    ask_shares(1, nco);
    publish_mode();
    __syncthreads();  // the clears, the mode
    take_mode();
    uint32_t pend = 0u;            // buckets of the group whose range is reserved and whose read-outs wait in ro[]
    uint32_t held = 0u, gsum = 0u;  // buckets read out for the group that is being collected, their distinct keys
    // ONE loop for both partitions, and one more trip than the workgroup has buckets: the last group's stores
    for (uint32_t i = 0; i <= m; i++) {
        asm volatile("" : "+v"(tid));
        if (i < m) {
            uint32_t total_in = total_next;
            if (!few) {
                // the one-level partition (R = G > 4 regions per bucket, at most 64 buckets): prefix and offsets through LDS, a search
                // per record, nothing asked for ahead
                const uint32_t b = blockIdx.x + i * grid;
                for (uint32_t r = tid; r < R; r += T) {
                    pre[r] = min(cnt[(size_t)b * R + r], cap32);
                    roff[r] = off ? off[(size_t)b * R + r] : 0u;
                }
                __syncthreads();
                if (tid == 0) {  // (as region_prefix: R <= 256, a serial pass over LDS costs less than the barriers of a block scan)
                    uint32_t run = 0;
                    for (uint32_t r = 0; r < R; r++) { run += pre[r]; pre[r] = run; }
                }
                __syncthreads();
                total_in = (uint32_t)__builtin_amdgcn_readfirstlane((int)pre[R - 1]);
            }
            const bool counted = total_in >= (uint32_t)(CAP - 64);
            uint32_t co = 0u, u = 0;
            if (total_in > (uint32_t)(D * T)) ask_shares(i, co);  // (more records than were asked for ahead)
            for (uint32_t j = tid; j < total_in; j += T, u++) {
                uint4 rc;
                if (few && u < (uint32_t)D) {
                    // asked for one bucket ago (consumed before the next ones are asked for: a second set of these registers would
                    // not fit 64 VGPRs beside K read-outs)
                    rc = pf[0];
#pragma unroll
                    for (int q = 1; q < D; q++) if (u == (uint32_t)q) rc = pf[q];
                } else if (few) {
                    rc = rec[dedup_record_at(dedup_shares(co, cap32, bucket_base(i)), rcap, j)];
                } else {
                    uint32_t k;
                    const uint32_t r = region_of(pre, R, j, k);
                    rc = rec[bucket_base(i) + (size_t)r * rcap + roff[r] + k];
                }
                insert(rc, counted);
            }
            // bucket i + 1's shares have arrived (asked for one bucket ago): ask for its first records, and for bucket i + 2's
            // shares; both are in flight behind this bucket's barrier, read-out, scan and reservation and the last group's stores
            total_next = ask_records(i + 1, nco);
            ask_shares(i + 2, nco);
        }
        // the group reserved one bucket ago: its add has had an insert's time to come back
        if (pend) publish_base(nco);
        __syncthreads();
        if (pend) { emit_group(pend); pend = 0u; }
        if (i < m) {
#pragma unroll
            for (int q = 0; q + 1 < K; q++) { ro[q] = ro[q + 1]; tot[q] = tot[q + 1]; }
            uint32_t rk;
            read_out(ro[K - 1], rk, tot[K - 1]);
            ranks = (ranks >> 16) | (rk << (16 * (K - 1)));
            gsum += tot[K - 1];
            if (++held == (uint32_t)K || i == m - 1) { reserve(nco, gsum); pend = held; held = 0u; gsum = 0u; }
        }
    }
    if (!hist) return;  // (the histogram comes from k_len_hist on the side stream: see there)
    __syncthreads();
    asm volatile("" : "+v"(tid));  // (or the prologue's addresses are kept for this across the loop)
    for (uint32_t i = tid; i < 32; i += T)
        if (lds_x[32 + i]) atomicAdd(&hist[i], lds_x[32 + i]);
}

// The length histogram of the partitioned path's unique reads, by a kernel of its own on the side stream (round 5).  k_part_dedup
// counted it while it emitted: one LDS atomic per unique read on ~16 hot counters and ~16 global atomics per bucket on 16
// addresses -- 130 k of them per sample from 8192 workgroups.  Nothing on the GPU waits for the histogram (the host reads it
// with the counts), but the main stream waited for those atomics: k_part_dedup 0.126 -> 0.118 ms and the step -1.7 % without
// them (profiles/README.md, round 5).  len[0 .. *n_dev): 3.8 MB per 10 M-read sample.
// The shards' stretches of k_part_dedup's staging area, one behind the other: the group's unique reads, dense.  *n_out = their number.
__global__ void __launch_bounds__(256) k_part_compact(const uint32_t* __restrict__ shard_cur, uint32_t shard_cap,
                                                       const uint64_t* __restrict__ sseq, const uint8_t* __restrict__ slen,
                                                       const uint32_t* __restrict__ scnt, const uint32_t* __restrict__ sfirst,
                                                       uint64_t* __restrict__ useq, uint8_t* __restrict__ ulen, uint32_t* __restrict__ ucnt,
                                                       uint32_t* __restrict__ ufirst, uint32_t* __restrict__ n_out,
                                                       const uint32_t* __restrict__ n_rec, uint32_t rec_thresh) {
    if (!(*n_rec < rec_thresh)) return;  // k_part_dedup took the one cursor: the output is dense already, *n_out is that cursor
    uint32_t end[MIRGE_DEDUP_SHARDS];  // (compile-time indices only: registers)
    uint32_t run = 0;
    bool over = false;  // a shard that overflowed was left unwritten by some buckets (k_part_dedup set the overflow flag: the call is
                        // redone): the group is published EMPTY, so that the cascade queued behind never walks uninitialised records
#pragma unroll
    for (int x = 0; x < MIRGE_DEDUP_SHARDS; x++) {
        const uint32_t cx = shard_cur[x * MIRGE_DEDUP_SHARD_STRIDE];
        over |= cx > shard_cap;
        run += min(cx, shard_cap); end[x] = run;
    }
    if (over) run = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_out = run;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < run; e += gridDim.x * blockDim.x) {
        uint32_t x = 0, lo = 0;
#pragma unroll
        for (int y = 0; y < MIRGE_DEDUP_SHARDS - 1; y++) if (e >= end[y]) { x = (uint32_t)y + 1; lo = end[y]; }
        const size_t src = (size_t)x * shard_cap + (e - lo);
        useq[e] = sseq[src]; ulen[e] = slen[src]; ucnt[e] = scnt[src]; ufirst[e] = sfirst[src];
    }
}

__global__ void __launch_bounds__(256) k_len_hist(const uint8_t* __restrict__ len, const uint32_t* __restrict__ n_dev, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[64];
    if (threadIdx.x < 64) h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t n = *n_dev;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) atomicAdd(&h[len[i] & 63u], 1u);
    __syncthreads();
    if (threadIdx.x < 64 && h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

// heads: read j is the head of its group iff it is the group's smallest index.  `first` is addressed
// as first[slot * stride] (inv: stored as 0xFFFFFFFF - index).  Writes flag[j] and per-block sums.
#define MIRGE_SCAN_ITEMS 8  // per thread -> 2048 per block
__global__ void k_heads_blocksum(const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ first,
                                 uint32_t stride, uint32_t inv, uint32_t n, const uint8_t* __restrict__ len,
                                 uint8_t* __restrict__ flag, uint32_t* __restrict__ blocksum,
                                 uint32_t* __restrict__ hist) {
    __shared__ uint32_t lds4[4];
    __shared__ uint32_t h[MIRGE_MAX_READ_LEN + 1];  // lengths of the heads = lengths of the unique reads
    for (int i = threadIdx.x; i <= MIRGE_MAX_READ_LEN; i += blockDim.x) h[i] = 0;
    __syncthreads();
    const uint32_t b0 = blockIdx.x * (MIRGE_BLOCK * MIRGE_SCAN_ITEMS) + threadIdx.x * MIRGE_SCAN_ITEMS;
    uint32_t c = 0;
    uint8_t fl[MIRGE_SCAN_ITEMS];
#pragma unroll
    for (int i = 0; i < MIRGE_SCAN_ITEMS; i++) {
        const uint32_t j = b0 + i;
        fl[i] = 0;
        if (j < n) {
            const uint32_t f = first[(size_t)slot_of[j] * stride];
            fl[i] = (inv ? 0xFFFFFFFFu - f : f) == j;
            if (fl[i]) {
                c++;
                if (len) {  // (nullptr: the long class, whose lengths the histogram has no room for)
                    const uint32_t L = len[j];
                    atomicAdd(&h[L > MIRGE_MAX_READ_LEN ? MIRGE_MAX_READ_LEN : L], 1u);
                }
            }
        }
    }
    if (b0 + MIRGE_SCAN_ITEMS <= n) {
        uint64_t packed = 0;
#pragma unroll
        for (int i = 0; i < MIRGE_SCAN_ITEMS; i++) packed |= (uint64_t)fl[i] << (8 * i);
        *reinterpret_cast<uint64_t*>(flag + b0) = packed;
    } else {
#pragma unroll
        for (int i = 0; i < MIRGE_SCAN_ITEMS; i++) if (b0 + i < n) flag[b0 + i] = fl[i];
    }
    uint32_t total;
    block_excl_scan(c, total, lds4);  // two barriers: the LDS histogram is complete after it
    if (threadIdx.x == 0) blocksum[blockIdx.x] = total;
    for (int i = threadIdx.x; i <= MIRGE_MAX_READ_LEN; i += blockDim.x)
        if (h[i]) atomicAdd(&hist[i], h[i]);
}

// single block: exclusive scan of blocksum[0..nb) in place, total to *out_total
__global__ void k_scan_blocksums(uint32_t* __restrict__ blocksum, uint32_t nb, uint32_t* __restrict__ out_total) {
    __shared__ uint32_t lds4[4];
    uint32_t carry = 0;
    for (uint32_t b = 0; b < nb; b += MIRGE_BLOCK) {
        uint32_t i = b + threadIdx.x;
        uint32_t v = i < nb ? blocksum[i] : 0u;
        uint32_t total;
        uint32_t ex = block_excl_scan(v, total, lds4);
        if (i < nb) blocksum[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *out_total = carry;
}

template <int W>
__global__ void k_collapse_scatter(GroupView<W> g, const uint32_t* __restrict__ slot_of,
                                   const uint8_t* __restrict__ flag, const uint32_t* __restrict__ cnt,
                                   uint32_t cnt_stride, const uint32_t* __restrict__ blockoff,
                                   const uint32_t* __restrict__ n_uniq_ptr, const uint32_t* __restrict__ orig,
                                   uint32_t base, int32_t S, uint64_t* __restrict__ useq,
                                   uint8_t* __restrict__ ulen, uint64_t* __restrict__ unmask,
                                   uint32_t* __restrict__ ucnt, uint32_t* __restrict__ ufirst) {
    __shared__ uint32_t lds4[4];
    const uint32_t U = *n_uniq_ptr;
    const uint32_t b0 = blockIdx.x * (MIRGE_BLOCK * MIRGE_SCAN_ITEMS) + threadIdx.x * MIRGE_SCAN_ITEMS;
    uint32_t heads = 0, c = 0;
    if (b0 + MIRGE_SCAN_ITEMS <= g.n) {
        const uint64_t packed = *reinterpret_cast<const uint64_t*>(flag + b0);
#pragma unroll
        for (int i = 0; i < MIRGE_SCAN_ITEMS; i++) if ((packed >> (8 * i)) & 1ull) { heads |= 1u << i; c++; }
    } else {
#pragma unroll
        for (int i = 0; i < MIRGE_SCAN_ITEMS; i++) if (b0 + i < g.n && flag[b0 + i]) { heads |= 1u << i; c++; }
    }
    uint32_t total;
    uint32_t rank = blockoff[blockIdx.x] + block_excl_scan(c, total, lds4);
#pragma unroll
    for (int i = 0; i < MIRGE_SCAN_ITEMS; i++) {
        if (heads & (1u << i)) {
            const uint32_t j = b0 + i;
            const uint32_t s = slot_of ? slot_of[j] : j;  // partitioned path: counts are stored per head read
#pragma unroll
            for (int w = 0; w < W; w++) {
                useq[(size_t)w * U + rank] = g.seq[(size_t)w * g.n + j];
                if (unmask) unmask[(size_t)w * U + rank] = g.nmask ? g.nmask[(size_t)w * g.n + j] : 0ull;
            }
            ulen[rank] = g.len[j];
            for (int32_t q = 0; q < S; q++) ucnt[(size_t)rank * S + q] = cnt[(size_t)s * cnt_stride + q];
            ufirst[rank] = orig ? orig[j] : base + j;
            rank++;
        }
    }
}

// mirge_collapse_merge (round 6): entry j of a per-sample dictionary's group becomes "read" number at + j of the joint set with its
// sample's index and its count as the weight (what mirge_collapse_weighted takes from the host, built where the dictionaries lie)
__global__ void k_merge_fill(const uint32_t* __restrict__ counts, uint32_t n, uint32_t at, int32_t sample, int32_t* __restrict__ dsample,
                             uint32_t* __restrict__ dweight) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        dsample[at + j] = sample;
        dweight[at + j] = counts[j];
    }
}
