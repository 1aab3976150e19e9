// kernels_cov.hpp -- part of mirge_kernels.hpp: per-sample genome coverage as bedGraph (`--coverage`).  Every row of `<sample>.sam`
// is ONE weighted interval on one chromosome and strand (the lift is single-segment: `<len>M`), so depth is a sum of +w / -w events:
//   k_cov_intervals : kept row (k_sam_select / k_sam_rows) -> (chromosome rank, 0-based start, length, weight, minus), lifted with
//                     sam_lift_start; the first row on a chromosome without rank and the first row outside [1, 2^31 - 1] are recorded
//   k_cov_events    : interval -> two (key, delta) pairs, (start, +w) and (end, -w); key = strand | chromosome rank | position
//   (radix sort by key, inclusive sum of the deltas -- hipCUB; every (strand, chromosome) group sums to zero, so no segmentation)
//   k_cov_last      : flag the last event of every distinct key                  \  exclusive sum of the flags + k_cov_scatter:
//   k_cov_change    : on that list, flag entry j iff S_j != S_{j-1} (S_{-1} = 0)  } three compactions with one scatter kernel
//   k_cov_nonzero   : on that list, flag entry j iff S_j != 0 = a run            /
//   k_cov_runs      : flagged entry j -> the run [pos_j, pos_{j+1}) of depth S_j on j's strand and chromosome
//   k_cov_measure   : bytes of a run's line `chrom \t start \t end \t depth \n`  -> one 64-bit exclusive scan
//   k_cov_write     : OUTPUT-stationary like k_sam_write: a workgroup owns a tile of the text, finds the lines that touch it with two
//                     binary searches over the line offsets and formats them, clipped to the tile, in LDS; 16 bytes a lane leave.
// All sums are integer sums: nothing depends on the order the hardware takes.  Only k_cov_write has a barrier or LDS.
#pragma once

#define MIRGE_COV_MAX_TILE 16384
#define MIRGE_COV_POS_BITS 31                  // a position is at most 2^31 - 1
#define MIRGE_COV_MAX_END 0x7FFFFFFFll
#define MIRGE_COV_NONE 0xFFFFFFFFu

struct CovIntervals {  // structure of arrays, n entries
    const int32_t* rank;     // global chromosome rank, 0 .. n_rank-1
    const long long* start;  // 0-based
    const int32_t* len;      // >= 1
    const uint32_t* weight;  // >= 1
    const uint8_t* minus;
};
struct CovRuns {  // n_runs entries in file order: plus strand first, then chromosome rank, then start
    uint8_t* strand;
    int32_t* chrom;
    long long* start;
    long long* end;
    long long* depth;
};

// flags[0] |= 1: an interval outside the contract (rank, start, length, weight or end); sum[0] += the weights.
// The strand bit lies directly above the used rank bits (strand_shift = 31 + bits of n_rank - 1), so the sort covers used bits only.
__global__ void k_cov_events(CovIntervals iv, uint32_t n, uint32_t n_rank, int stranded, int strand_shift, unsigned long long* __restrict__ key,
                             long long* __restrict__ delta, uint32_t* __restrict__ flags, unsigned long long* __restrict__ sum) {
    unsigned long long mine = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const long long s = iv.start[i], L = iv.len[i], w = iv.weight[i];
        const int32_t r = iv.rank[i];
        unsigned long long k0 = 0, k1 = 0;
        long long d = 0;
        if (r < 0 || (uint32_t)r >= n_rank || s < 0 || L < 1 || w < 1 || s + L > MIRGE_COV_MAX_END) {
            atomicOr(&flags[0], 1u);  // (two events that cancel at key 0: the arrays stay defined)
        } else {
            const unsigned long long hi = ((stranded && iv.minus[i]) ? 1ull << strand_shift : 0ull) | (unsigned long long)r << MIRGE_COV_POS_BITS;
            k0 = hi | (unsigned long long)s;
            k1 = hi | (unsigned long long)(s + L);
            d = w;
            mine += (unsigned long long)w;
        }
        key[2 * (size_t)i] = k0; delta[2 * (size_t)i] = d;
        key[2 * (size_t)i + 1] = k1; delta[2 * (size_t)i + 1] = -d;
    }
    if (mine) atomicAdd(sum, mine);
}

__global__ void k_cov_last(const unsigned long long* __restrict__ key, uint32_t m, uint32_t* __restrict__ flag) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x)
        flag[i] = (i + 1 == m || key[i + 1] != key[i]) ? 1u : 0u;
}
__global__ void k_cov_change(const long long* __restrict__ S, uint32_t m, uint32_t* __restrict__ flag) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x)
        flag[j] = S[j] != (j ? S[j - 1] : 0ll) ? 1u : 0u;
}
// flags[0] |= 2: a negative sum, or a last entry that does not return to 0 (the call fails: the events were not what k_cov_events writes)
__global__ void k_cov_nonzero(const long long* __restrict__ S, uint32_t m, uint32_t* __restrict__ flag, uint32_t* __restrict__ flags) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x) {
        const long long s = S[j];
        if (s < 0 || (j + 1 == m && s != 0)) atomicOr(&flags[0], 2u);
        flag[j] = s != 0 ? 1u : 0u;
    }
}
// pos = exclusive sum of flag
__global__ void k_cov_scatter(const unsigned long long* __restrict__ key, const long long* __restrict__ S, const uint32_t* __restrict__ flag,
                              const uint32_t* __restrict__ pos, uint32_t m, unsigned long long* __restrict__ key_out, long long* __restrict__ S_out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x)
        if (flag[i]) { key_out[pos[i]] = key[i]; S_out[pos[i]] = S[i]; }
}
// entry j with S_j != 0 and its successor (same strand and chromosome: a group's last entry has S = 0) are one run; n_plus[0] += runs of
// the plus strand
__global__ void k_cov_runs(const unsigned long long* __restrict__ key, const long long* __restrict__ S, const uint32_t* __restrict__ flag,
                           const uint32_t* __restrict__ pos, uint32_t m, int strand_shift, CovRuns runs, uint32_t* __restrict__ n_plus) {
    uint32_t mine = 0;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j + 1 < m; j += gridDim.x * blockDim.x) {
        if (!flag[j]) continue;
        const unsigned long long k = key[j], pmask = (1ull << MIRGE_COV_POS_BITS) - 1;
        const uint32_t x = pos[j];
        const uint8_t st = (uint8_t)((k >> strand_shift) & 1ull);
        runs.strand[x] = st;
        runs.chrom[x] = (int32_t)((k >> MIRGE_COV_POS_BITS) & ((1ull << (strand_shift - MIRGE_COV_POS_BITS)) - 1));
        runs.start[x] = (long long)(k & pmask);
        runs.end[x] = (long long)(key[j + 1] & pmask);
        runs.depth[x] = S[j];
        mine += st ? 0u : 1u;
    }
    if (mine) atomicAdd(n_plus, mine);
}

__host__ __device__ __forceinline__ uint32_t cov_digits(unsigned long long v) {
    uint32_t nd = 1;
    for (; v >= 10ull; v /= 10ull) nd++;
    return nd;
}
// name_off[n_rank + 1] into name_data: the chromosome names in rank order
__global__ void k_cov_measure(CovRuns runs, uint32_t n_runs, const uint32_t* __restrict__ name_off, unsigned long long* __restrict__ bytes) {
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n_runs; x += gridDim.x * blockDim.x) {
        const int32_t ch = runs.chrom[x];
        bytes[x] = (unsigned long long)(name_off[ch + 1] - name_off[ch]) + cov_digits((unsigned long long)runs.start[x]) +
                   cov_digits((unsigned long long)runs.end[x]) + cov_digits((unsigned long long)runs.depth[x]) + 4ull;
    }
}

// writes the part of a line that falls into [0, tile_len) of `o`; rel = line start - tile start (SamOut<true> of kernels_sam.hpp)
struct CovOut {
    uint8_t* o;
    int32_t rel, tile_len;
    uint32_t n;
    __device__ __forceinline__ void ch(uint8_t c) {
        const int32_t x = rel + (int32_t)n;
        if ((uint32_t)x < (uint32_t)tile_len) o[x] = c;
        n++;
    }
    __device__ __forceinline__ void u64(unsigned long long v) {
        const uint32_t nd = cov_digits(v);
        for (int d = (int)nd - 1; d >= 0; d--) {
            const int32_t at = rel + (int32_t)n + d;
            if ((uint32_t)at < (uint32_t)tile_len) o[at] = (uint8_t)('0' + (int)(v % 10ull));
            v /= 10ull;
        }
        n += nd;
    }
};

// text [chunk_start, chunk_start + chunk_bytes) of the lines -> out[0 .. chunk_bytes); one workgroup per tile of tile_bytes (a multiple
// of 16, at most MIRGE_COV_MAX_TILE); line_off[n_runs + 1] = exclusive scan of k_cov_measure's bytes.  A line is at most 24 + 3 * 20 + 4
// bytes and at least 8, so |line start - tile start| stays far inside 32 bits.
__global__ void __launch_bounds__(MIRGE_BLOCK) k_cov_write(CovRuns runs, uint32_t n_runs, const uint32_t* __restrict__ name_off,
                                                           const uint8_t* __restrict__ name_data, const unsigned long long* __restrict__ line_off,
                                                           unsigned long long chunk_start, uint32_t chunk_bytes, uint32_t tile_bytes,
                                                           uint8_t* __restrict__ out) {
    __shared__ uint4 tile16[MIRGE_COV_MAX_TILE / 16];
    uint8_t* tile = reinterpret_cast<uint8_t*>(tile16);
    for (uint32_t tb = blockIdx.x; (unsigned long long)tb * tile_bytes < chunk_bytes; tb += gridDim.x) {
        const uint32_t in_chunk = tb * tile_bytes;
        const uint32_t tile_len = chunk_bytes - in_chunk < tile_bytes ? chunk_bytes - in_chunk : tile_bytes;
        const unsigned long long tile_start = chunk_start + in_chunk, tile_end = tile_start + tile_len;
        // first = the line that holds byte tile_start, last = the first line that starts at or behind the tile's end (the same in every lane)
        uint32_t lo = 0, hi = n_runs;
        while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (line_off[mid + 1] <= tile_start) lo = mid + 1; else hi = mid; }
        const uint32_t first = lo;
        hi = n_runs;
        while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (line_off[mid] < tile_end) lo = mid + 1; else hi = mid; }
        const uint32_t last = lo;
        for (uint32_t x = first + threadIdx.x; x < last; x += blockDim.x) {
            CovOut w{tile, (int32_t)((long long)line_off[x] - (long long)tile_start), (int32_t)tile_len, 0u};
            const int32_t ch = runs.chrom[x];
            for (uint32_t p = name_off[ch]; p < name_off[ch + 1]; p++) w.ch(name_data[p]);
            w.ch('\t'); w.u64((unsigned long long)runs.start[x]);
            w.ch('\t'); w.u64((unsigned long long)runs.end[x]);
            w.ch('\t'); w.u64((unsigned long long)runs.depth[x]);
            w.ch('\n');
        }
        __syncthreads();
        uint4* dst = reinterpret_cast<uint4*>(out + in_chunk);
        for (uint32_t x = threadIdx.x; x < tile_len / 16; x += blockDim.x) dst[x] = tile16[x];
        for (uint32_t x = (tile_len & ~15u) + threadIdx.x; x < tile_len; x += blockDim.x) out[in_chunk + x] = tile[x];
        __syncthreads();
    }
}

#ifndef MIRGE_COV_NO_SAM
// the interval of every kept row of one sample's file (rows[]: k_sam_rows).  rank_of + rank_off[p] .. : pass p's chromosome index ->
// global rank, -1 where the caller's chromosome order does not hold the name.  err[0] = the first row (by index) on such a chromosome,
// err[1] = the first row with START < 1 or an end beyond 2^31 - 1; both start at MIRGE_COV_NONE.
struct CovRankMap {
    const int32_t* rank_of;
    uint32_t rank_off[MIRGE_MAX_PASSES_K];
};
__global__ void k_cov_intervals(SamTables t, const uint32_t* __restrict__ rows, uint32_t n_rows, CovRankMap rm, int32_t* __restrict__ rank,
                                long long* __restrict__ start, int32_t* __restrict__ len, uint32_t* __restrict__ weight, uint8_t* __restrict__ minus_out,
                                uint32_t* __restrict__ err) {
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n_rows; x += gridDim.x * blockDim.x) {
        uint32_t j;
        const int gi = sam_locate(t, rows[x], j);
        const CsvGroup& g = t.g[gi];
        const int p = g.pass[j];
        const SamPass& sp = t.pass[p];
        const int32_t r = g.ref[j];
        const int Ls = csv_len(g, j) - sp.trim5 - sp.trim3;
        const bool minus = sp.minus[r] != 0;
        const long long s1 = sam_lift_start(sp, r, t.off[gi][j], Ls, minus);
        const int32_t rk = rm.rank_of[rm.rank_off[p] + (uint32_t)sp.chrom_of_ref[r]];
        bool ok = true;
        if (rk < 0) { atomicMin(&err[0], x); ok = false; }
        if (s1 < 1 || s1 - 1 + (long long)Ls > MIRGE_COV_MAX_END) { atomicMin(&err[1], x); ok = false; }
        rank[x] = ok ? rk : 0;
        start[x] = ok ? s1 - 1 : 0;
        len[x] = Ls;
        weight[x] = g.counts[(size_t)j * t.S + t.sample];
        minus_out[x] = minus ? 1 : 0;
    }
}
// what an error message names: out[0..3] = read (handle index), pass, reference, the pass's chromosome index of row x
__global__ void k_cov_describe(SamTables t, const uint32_t* __restrict__ rows, uint32_t x, int32_t* __restrict__ out) {
    if (blockIdx.x || threadIdx.x) return;
    uint32_t j;
    const int gi = sam_locate(t, rows[x], j);
    const int p = t.g[gi].pass[j];
    const int32_t r = t.g[gi].ref[j];
    out[0] = (int32_t)rows[x]; out[1] = p; out[2] = r; out[3] = t.pass[p].chrom_of_ref[r];
}
#endif
