// kernels_pileup.hpp -- the reads of a sample against the sequences of their clusters once more, for the cluster features
// (generate_featureFiles.py / readCluster.py of the reference): the best ungapped local diagonal of every (cluster, read) row
// (k_cluster_diagonals) and the count-weighted column tallies of every cluster's gapless pile-up (k_pileup_extent,
// k_pileup_tally).  Integer kernels, wave64; DESIGN.md 'Cluster features'.
#pragma once

#define MIRGE_PILEUP_MAXREAD 64      // as the genome calls: a read's overhang over its cluster is at most 63 columns
#define MIRGE_PILEUP_MAXCLUSTER 128  // a cluster sequence held in LDS per thread; longer clusters are the host's
#define MIRGE_PILEUP_BLOCK 128       // k_cluster_diagonals: threads = rows per workgroup
#define MIRGE_PILEUP_CHUNK 2048      // rows of one cluster per work item of the tally: a heavy cluster is many work items
#define MIRGE_PILEUP_COLS (MIRGE_PILEUP_MAXCLUSTER + 2 * MIRGE_PILEUP_MAXREAD)
#define MIRGE_PILEUP_FLAG_GAP 1u     // best <= 2 * min(L, C) - 20: a gapped alignment could tie or win
#define MIRGE_PILEUP_FLAG_NONE 2u    // no positive score: localms returns nothing

// the tally's symbol order is the reference's: A, T, C, G, anything else
__device__ __forceinline__ uint8_t pileup_code(uint8_t ch) {
    return ch == 'A' ? 0 : ch == 'T' ? 1 : ch == 'C' ? 2 : ch == 'G' ? 3 : 4;
}

// One thread per row.  The row's read and its cluster lie in LDS, one byte per base, base-major (s[k * BLOCK + thread]): the
// lanes of a wave walk their own rows in step and read neighbouring bytes.  Every diagonal d = cluster index - read index is
// walked with a running max-subarray (match +2, mismatch -1, floor 0); of equal best scores the one whose END cell comes
// first in the cluster, then first in the read, wins -- the order in which pairwise2's result list starts.
// Codes 0..3 match themselves, 4 ('other', an N) matches nothing; the host sends only clusters made of A/C/G/T.
__global__ void __launch_bounds__(MIRGE_PILEUP_BLOCK)
k_cluster_diagonals(uint32_t n_rows, const char* __restrict__ reads, const int64_t* __restrict__ r_off, const char* __restrict__ clusters,
                    const int64_t* __restrict__ c_off, const uint32_t* __restrict__ row_cluster, int32_t* __restrict__ diag,
                    int32_t* __restrict__ score, int32_t* __restrict__ identity, uint8_t* __restrict__ flag) {
    __shared__ uint8_t s_read[MIRGE_PILEUP_MAXREAD * MIRGE_PILEUP_BLOCK];
    __shared__ uint8_t s_clu[MIRGE_PILEUP_MAXCLUSTER * MIRGE_PILEUP_BLOCK];
    const uint32_t t = threadIdx.x;
    const uint32_t row = blockIdx.x * MIRGE_PILEUP_BLOCK + t;
    if (row >= n_rows) return;  // no barrier below: every thread reads only what it wrote
    const int64_t r0 = r_off[row], c0 = c_off[row_cluster[row]];
    int L = (int)(r_off[row + 1] - r0), C = (int)(c_off[row_cluster[row] + 1] - c0);
    if (L > MIRGE_PILEUP_MAXREAD) L = MIRGE_PILEUP_MAXREAD;  // refused on the host; never past the LDS rows
    if (C > MIRGE_PILEUP_MAXCLUSTER) C = MIRGE_PILEUP_MAXCLUSTER;
    for (int j = 0; j < L; j++) s_read[j * MIRGE_PILEUP_BLOCK + t] = pileup_code((uint8_t)reads[r0 + j]);
    for (int i = 0; i < C; i++) s_clu[i * MIRGE_PILEUP_BLOCK + t] = pileup_code((uint8_t)clusters[c0 + i]);
    int best = 0, best_d = 0, best_i = 0x7FFFFFFF, best_id = 0;
    for (int d = -(L - 1); d <= C - 1; d++) {
        const int i_lo = d > 0 ? d : 0, i_hi = (L + d < C) ? L + d : C;  // the overlap on this diagonal, cluster coordinates
        int h = 0, top = 0, top_i = 0, same = 0;
        for (int i = i_lo; i < i_hi; i++) {
            const uint8_t a = s_clu[i * MIRGE_PILEUP_BLOCK + t], b = s_read[(i - d) * MIRGE_PILEUP_BLOCK + t];
            const bool eq = (a == b) && a < 4;
            same += eq;
            h += eq ? 2 : -1;
            if (h < 0) h = 0;
            if (h > top) { top = h; top_i = i; }  // the first cell of this diagonal that reaches its best
        }
        // end cells compare by (cluster position, read position); on one cluster position the smaller read position is the
        // larger diagonal
        if (top > best || (top == best && top > 0 && (top_i < best_i || (top_i == best_i && d > best_d)))) {
            best = top; best_d = d; best_i = top_i; best_id = same;
        }
    }
    const int m = L < C ? L : C;
    diag[row] = best_d;
    score[row] = best;
    identity[row] = best_id;
    flag[row] = (uint8_t)((best > 2 * m - 20 ? 0u : MIRGE_PILEUP_FLAG_GAP) | (best > 0 ? 0u : MIRGE_PILEUP_FLAG_NONE));
}

struct PileupItem {  // rows [row0, row1) of one cluster
    uint32_t cluster, row0, row1, whole;  // whole: the cluster's only work item (its flush needs no atomics)
};

// the cluster's head / tail padding: the largest overhang of a read left / right of the cluster.  One wave per work item, the
// lanes stride over its rows, one atomicMax per wave and side.
__global__ void __launch_bounds__(64)
k_pileup_extent(uint32_t n_items, const PileupItem* __restrict__ items, const int64_t* __restrict__ r_off, const int64_t* __restrict__ c_off,
                const int32_t* __restrict__ diag, int32_t* __restrict__ head, int32_t* __restrict__ tail) {
    const uint32_t it = blockIdx.x;
    if (it >= n_items) return;
    const PileupItem w = items[it];
    const int C = (int)(c_off[w.cluster + 1] - c_off[w.cluster]);
    int hp = 0, tp = 0;
    for (uint32_t r = w.row0 + threadIdx.x; r < w.row1; r += 64) {
        const int d = diag[r], L = (int)(r_off[r + 1] - r_off[r]);
        hp = max(hp, -d);
        tp = max(tp, L + d - C);
    }
    for (int s = 32; s; s >>= 1) {
        hp = max(hp, __shfl_xor(hp, s));
        tp = max(tp, __shfl_xor(tp, s));
    }
    if (threadIdx.x == 0) {
        if (hp > 0) atomicMax(&head[w.cluster], hp);
        if (tp > 0) atomicMax(&tail[w.cluster], tp);
    }
}

// the tallies: one wave per work item, a histogram [column][A, T, C, G, other] of 64-bit counts in LDS in cluster coordinates
// shifted by MAXREAD (so every read base of a valid row has a column whatever the padding), lanes stride over the rows.  Flush:
// the columns [MAXREAD - head, MAXREAD + C + tail) to the cluster's stretch of `tally` -- plain vector stores when the cluster
// is this one work item, 64-bit atomic adds into the zeroed stretch when its rows were split (integer sums: any order, one
// result).
__global__ void __launch_bounds__(64)
k_pileup_tally(uint32_t n_items, const PileupItem* __restrict__ items, const char* __restrict__ reads, const int64_t* __restrict__ r_off,
               const int64_t* __restrict__ c_off, const int32_t* __restrict__ diag, const int64_t* __restrict__ count,
               const int32_t* __restrict__ head, const int32_t* __restrict__ tail, const int64_t* __restrict__ col_off,
               unsigned long long* __restrict__ tally) {
    __shared__ unsigned long long hist[MIRGE_PILEUP_COLS * 5];
    const uint32_t it = blockIdx.x;
    if (it >= n_items) return;
    const PileupItem w = items[it];
    const int C = (int)(c_off[w.cluster + 1] - c_off[w.cluster]);
    const int H = head[w.cluster], T = tail[w.cluster];
    if (H < 0 || H >= MIRGE_PILEUP_MAXREAD || T < 0 || T >= MIRGE_PILEUP_MAXREAD || C > MIRGE_PILEUP_MAXCLUSTER) return;  // whole workgroup
    const int lo = (MIRGE_PILEUP_MAXREAD - H) * 5, hi = (MIRGE_PILEUP_MAXREAD + C + T) * 5;  // 0 <= lo, hi <= COLS * 5: checked on the host
    for (int k = lo + (int)threadIdx.x; k < hi; k += 64) hist[k] = 0ull;
    __syncthreads();
    // a row per trip, a lane per base (a read has at most 64): the three rows of a small cluster are three trips of ~22 busy
    // lanes, and the lanes of a trip add to different columns, so a heavy cluster's rows do not queue on one LDS address
    for (uint32_t r = w.row0; r < w.row1; r++) {
        const int64_t r0 = r_off[r];
        const int d = diag[r], L = (int)(r_off[r + 1] - r0);
        if (L > MIRGE_PILEUP_MAXREAD || d < -H || L + d > C + T) continue;  // not a row of this extent: refused on the host
        const int j = (int)threadIdx.x;
        if (j < L) atomicAdd(&hist[(MIRGE_PILEUP_MAXREAD + d + j) * 5 + pileup_code((uint8_t)reads[r0 + j])], (unsigned long long)count[r]);
    }
    __syncthreads();
    unsigned long long* out = tally + col_off[w.cluster] * 5;
    if (w.whole) {
        for (int k = lo + (int)threadIdx.x; k < hi; k += 64) out[k - lo] = hist[k];
    } else {
        for (int k = lo + (int)threadIdx.x; k < hi; k += 64)
            if (hist[k]) atomicAdd(&out[k - lo], hist[k]);
    }
}
