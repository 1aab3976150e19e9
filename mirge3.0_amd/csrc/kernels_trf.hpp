// kernels_trf.hpp -- part of mirge_kernels.hpp: the sequence work behind the tRNA fragment report (the reference's `-trf`:
// summary.py:1060-1220, mirge2_tRF_a2i.py:22-62).
//   k_trf_hits    : EVERY best-stratum alignment of a tRNA read (bowtie `-a --best --strata` of passes 2 and 3, manifoldAlign.py:85), not
//                   the one the cascade kept.  The enumerating sibling of mirge_align_indexed (mirge_core.hpp): the same probes through
//                   the same tables, every candidate window verified in full, kept when its total mismatches equal the read's stratum
//                   (the cascade's mm).  A window that several probes reach is reported by the LOWEST probe whose blocks match the
//                   text there exactly: probes below the current one are rechecked against the text (two extracts each), so no window
//                   comes out twice and nothing is shared between threads.  Run twice: COUNT (windows per row) -> one exclusive scan ->
//                   WRITE (key = row << 32 | global position into the row's own stretch).  One radix sort of the keys is the
//                   (row, reference, offset) order.
//   k_trf_finish  : key -> (row, reference, offset, mismatches, class, type); type = trfTypes (summary.py:649-674).
//   k_trf_row_counts : the count matrix of the report's rows alone (the host sums and prints them).
//   k_trf_assign  : a report row against every predefined tRF of its reference: minimum of (getDistance2, rank of the cluster name).
// Read-to-lane mapping: one ROW per lane in all three.  A tRNA read's work is a handful of probes with a few candidates each (the
// libraries hold some hundred references of 70-95 nt), rows number in the hundred thousands, and neighbouring rows of mapped.csv differ
// in length and probe plan anyway, so there is no per-row loop long or regular enough to spread over a wave; not measured against a
// wave-per-row form.
#pragma once

#define MIRGE_TRF_MAXG 10  // read groups of a handle (native_reads.hpp: MIRGE_NGROUPS; the long class never holds a tRNA read)
#define MIRGE_TRF_WHOLE 0  // tRF-whole
#define MIRGE_TRF_5HALF 1  // 5'-half
#define MIRGE_TRF_5TRF 2   // 5'-tRF
#define MIRGE_TRF_3HALF 3  // 3'-half
#define MIRGE_TRF_3TRF 4   // 3'-tRF
#define MIRGE_TRF_ITRF 5   // i-tRF
#define MIRGE_TRF_1 6      // tRF-1 (every hit of the primary class)
#define MIRGE_TRF_NO_DIST 100  // assign_cluster's distance of a reference without predefined tRFs ('Dele')

struct TrfGroup {
    const uint64_t* seq;    // [W][n]
    const uint64_t* nmask;  // [W][n] or nullptr
    const uint8_t* len;     // [n]
    const int8_t* pass;     // the cascade's answer for the group
    const int8_t* mm;
    const uint32_t* counts; // [n][S] or nullptr
    uint32_t base, n;       // handle index = base + j
    int32_t W, pad;         // 0: the long class
};
struct TrfClass {           // 0: mature tRNA (-v 1), 1: primary tRNA (-v 0 on the read without its T{3,}$ run)
    MirgeLibView lib;
    MirgePolicy pol;
    int32_t pass, pad;
};
struct TrfTables {
    TrfGroup g[MIRGE_TRF_MAXG];
    TrfClass cls[2];
    const int32_t* anticodon;  // [mature references] 0-based start of the anticodon (stru.index('XXX'))
};

__host__ __device__ __forceinline__ int trf_locate(const TrfTables& t, uint32_t i, uint32_t& j) {
    int gi = 0;
#pragma unroll
    for (int k = 1; k < MIRGE_TRF_MAXG; k++)
        if (t.g[k].n && i >= t.g[k].base) gi = k;
    j = i - t.g[gi].base;
    return gi;
}

// k <= 32 bases of the text from global position g
__host__ __device__ __forceinline__ uint64_t trf_text_kmer(const uint64_t* __restrict__ T, uint64_t g, int k) {
    const uint64_t q = g >> 5;
    const int s = (int)(g & 31) * 2;
    uint64_t lo = T[q] >> s;
    if (s) lo |= T[q + 1] << (64 - s);
    return lo & mirge_lowmask2(k);
}

// does probe `pr` of the read reach the window at g?  (the read's blocks hold no N and equal the text's)
template <int W>
__host__ __device__ __forceinline__ bool trf_probe_reaches(const uint64_t* __restrict__ T, uint64_t g, const MirgeRead<W>& r, const MirgeProbe& pr) {
    uint64_t key;
    if (!mirge_probe_key<W>(r, pr, key)) return false;
    uint64_t tk = trf_text_kmer(T, g + (uint64_t)pr.a1, pr.k1);
    if (pr.k2 > 0) tk |= trf_text_kmer(T, g + (uint64_t)(pr.a1 + pr.k1 + pr.gap), pr.k2) << (2 * pr.k1);
    return tk == key;
}

// flags[0]: 1 = a row is not of the two classes, 2 = count and write pass disagree, 4 = a probe table is missing
template <int W, bool WRITE>
__global__ void k_trf_hits(TrfTables t, const uint32_t* __restrict__ rows, uint32_t n_rows, unsigned long long* __restrict__ cnt,
                           const unsigned long long* __restrict__ off, unsigned long long* __restrict__ keys, uint32_t* __restrict__ flags) {
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n_rows; x += gridDim.x * blockDim.x) {
        uint32_t j;
        const int gi = trf_locate(t, rows[x], j);
        const TrfGroup& g = t.g[gi];
        if (g.W != W) continue;  // (another width's launch; the long class: no launch, no hits)
        const int ps = g.pass[j];
        const int c = ps == t.cls[0].pass ? 0 : (ps == t.cls[1].pass ? 1 : -1);
        if (c < 0) { atomicOr(&flags[0], 1u); continue; }
        const MirgeLibView& lib = t.cls[c].lib;
        const MirgePolicy& p = t.cls[c].pol;
        MirgeRead<W> r;
#pragma unroll
        for (int w = 0; w < W; w++) {
            r.w[w] = g.seq[(size_t)w * g.n + j];
            r.nm[w] = g.nmask ? g.nmask[(size_t)w * g.n + j] : 0ull;
        }
        r.len = g.len[j];
        unsigned long long n = 0;
        const unsigned long long room = WRITE ? off[x + 1] - off[x] : 0ull;
        if (mirge_effective_read<W>(r, p)) {
            const int stratum = g.mm[j];
            const int L = r.len;
            const int np = mirge_probe_count(p, L, lib.kmax, lib.total);
            for (int q = 0; q < np; q++) {
                MirgeProbe pr;
                mirge_probe_at(p, L, lib.kmax, lib.total, q, pr);
                uint64_t key;
                if (!mirge_probe_key<W>(r, pr, key)) continue;
                const MirgeKTable tb = lib.tables[mirge_shape_id(pr.k1, pr.gap, pr.k2)];
                if (!tb.bucket) { atomicOr(&flags[0], 4u); continue; }
                // (bits may carry the "entries behind a filter" mark of a MIRGE_PRESENCE_FILTER build in its lowest bit)
                const bool entries = !tb.bits || ((uintptr_t)tb.bits & 1u);
                const uint32_t* bits = reinterpret_cast<const uint32_t*>((uintptr_t)tb.bits & ~(uintptr_t)1);
                if (bits && !((bits[key >> 5] >> (key & 31)) & 1u)) continue;
                uint32_t n_cand, lo;
                bool inl = false;
                if (!entries) {
                    const uint32_t* b = static_cast<const uint32_t*>(tb.bucket);
                    lo = b[key]; n_cand = b[key + 1] - lo;
                } else {
                    const uint64_t e = static_cast<const uint64_t*>(tb.bucket)[key];
                    n_cand = (uint32_t)(e >> 32); lo = (uint32_t)e; inl = n_cand == 1;
                }
                for (uint32_t k = 0; k < n_cand; k++) {
                    const uint32_t pz = inl ? lo : tb.pos[lo + k];
                    if (pz < (uint32_t)pr.a1) continue;
                    const uint64_t gpos = (uint64_t)pz - (uint64_t)pr.a1;
                    if (mirge_window_mm<W>(lib.T, gpos, r, p) != stratum) continue;
                    if (mirge_window_invalid(lib.inv, gpos, L)) continue;
                    bool earlier = false;  // a probe below q reports this window
                    for (int q2 = 0; q2 < q && !earlier; q2++) {
                        MirgeProbe p2;
                        mirge_probe_at(p, L, lib.kmax, lib.total, q2, p2);
                        earlier = trf_probe_reaches<W>(lib.T, gpos, r, p2);
                    }
                    if (earlier) continue;
                    if (WRITE && n < room) keys[off[x] + n] = ((unsigned long long)x << 32) | (unsigned long long)gpos;
                    n++;
                }
            }
        }
        if (!WRITE) cnt[x] = n;
        else if (n != room) atomicOr(&flags[0], 2u);
    }
}

// trfTypes (summary.py:649-674) of a mature hit: start = 0-based offset, L = the whole read, tlen = the tRNA, ac = 0-based anticodon start
__host__ __device__ __forceinline__ int trf_type(int start, int L, int tlen, int ac) {
    const int last = start + L - 1;
    if (start == 0) {
        if (start + L == tlen) return MIRGE_TRF_WHOLE;
        if (last >= ac - 2 && last <= ac + 1) return MIRGE_TRF_5HALF;
        return MIRGE_TRF_5TRF;
    }
    if (last >= tlen - 1 - 2 && last <= tlen - 1) return (start >= ac - 1 && start <= ac + 2) ? MIRGE_TRF_3HALF : MIRGE_TRF_3TRF;
    return MIRGE_TRF_ITRF;
}

__global__ void k_trf_finish(TrfTables t, const uint32_t* __restrict__ rows, const unsigned long long* __restrict__ keys, uint32_t n_rec,
                             uint32_t* __restrict__ o_row, uint32_t* __restrict__ o_ref, int32_t* __restrict__ o_off, uint8_t* __restrict__ o_mm,
                             uint8_t* __restrict__ o_cls, uint8_t* __restrict__ o_type) {
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n_rec; k += gridDim.x * blockDim.x) {
        const uint32_t x = (uint32_t)(keys[k] >> 32), gpos = (uint32_t)keys[k];
        uint32_t j;
        const int gi = trf_locate(t, rows[x], j);
        const TrfGroup& g = t.g[gi];
        const int c = g.pass[j] == t.cls[0].pass ? 0 : 1;
        const MirgeLibView& lib = t.cls[c].lib;
        uint32_t lo = 0, hi = lib.n_refs;  // the reference with ref_start[lo] <= gpos < ref_start[lo + 1]
        while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (lib.ref_start[mid] <= gpos) lo = mid; else hi = mid; }
        const int start = (int)(gpos - lib.ref_start[lo]);
        const int tlen = (int)(lib.ref_start[lo + 1] - lib.ref_start[lo]) - 1;  // (one separator behind every reference)
        o_row[k] = x; o_ref[k] = lo; o_off[k] = start;
        o_mm[k] = (uint8_t)(c == 0 ? g.mm[j] : 0);
        o_cls[k] = (uint8_t)c;
        o_type[k] = (uint8_t)(c == 0 ? trf_type(start, (int)g.len[j], tlen, t.anticodon[lo]) : MIRGE_TRF_1);
    }
}

// the count matrix of the report's rows alone: out[x][s] = counts of read rows[x] in sample s
__global__ void k_trf_row_counts(TrfTables t, const uint32_t* __restrict__ rows, uint32_t n_rows, int32_t S, uint32_t* __restrict__ out) {
    const size_t total = (size_t)n_rows * (size_t)S;
    for (size_t x = blockIdx.x * (size_t)blockDim.x + threadIdx.x; x < total; x += (size_t)gridDim.x * blockDim.x) {
        uint32_t j;
        const int gi = trf_locate(t, rows[x / (size_t)S], j);
        const TrfGroup& g = t.g[gi];
        out[x] = g.counts ? g.counts[(size_t)j * (size_t)S + x % (size_t)S] : 0u;
    }
}

// ---- assignment to a predefined tRF (assign_cluster / getDistance2, mirge2_tRF_a2i.py:22-62)
struct TrfInfor {
    const uint32_t* ref_ptr;   // [n_tref + 1] CSR: the predefined tRFs of a reference
    const uint32_t* str_off;   // [n_trf + 1] into str: a tRF's dashed string (addDashNew), as text
    const uint8_t* str;
    const int32_t* c_start;    // [n_trf] coordinate(): 1-based first and last position that is no dash
    const int32_t* c_end;
    const int32_t* rank;       // [n_trf] rank of the cluster name in string order
    uint32_t n_tref, n_trf;
};

// per row: read = handle index, tref = index into ref_ptr (-1: the reference has no tRF), start = 1-based start in the reference.  The
// row's dashed string is '-' * (start - 1) + read + dashes: its coordinates are (start, start - 1 + len(read)) and its letters are the
// read's, T run included; the dashes behind them add nothing to the distance, so the row's `end` is not needed.
__global__ void k_trf_assign(TrfTables t, TrfInfor f, const uint32_t* __restrict__ read, const int32_t* __restrict__ tref,
                             const int32_t* __restrict__ start, uint32_t n_rows, int32_t* __restrict__ o_dist, int32_t* __restrict__ o_trf) {
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n_rows; x += gridDim.x * blockDim.x) {
        int best_d = MIRGE_TRF_NO_DIST, best_rank = 0, best = -1;
        const int32_t tr = tref[x];
        if (tr >= 0 && (uint32_t)tr < f.n_tref) {
            uint32_t j;
            const int gi = trf_locate(t, read[x], j);
            const TrfGroup& g = t.g[gi];
            const int L = g.W ? (int)g.len[j] : 0;
            const int s0 = start[x] - 1;  // 0-based position of the read's first letter in the dashed string
            for (uint32_t k = f.ref_ptr[tr]; k < f.ref_ptr[tr + 1]; k++) {
                const uint8_t* s2 = f.str + f.str_off[k];
                const int len2 = (int)(f.str_off[k + 1] - f.str_off[k]);
                int ds = (s0 + 1) - f.c_start[k], de = (s0 + L) - f.c_end[k];
                int d = (ds < 0 ? -ds : ds) + (de < 0 ? -de : de);
                uint64_t bits = 0, nm = 0;
                for (int p = 0; p < L; p++) {
                    if ((p & 31) == 0) {
                        bits = g.seq[(size_t)(p >> 5) * g.n + j];
                        nm = g.nmask ? g.nmask[(size_t)(p >> 5) * g.n + j] : 0ull;
                    }
                    const int sh = 2 * (p & 31);
                    const uint8_t a = ((nm >> sh) & 1ull) ? (uint8_t)'N' : (uint8_t)"ACGT"[(bits >> sh) & 3ull];
                    const int at = s0 + p;
                    if (at >= len2) d++;  // (the reference's IndexError branch)
                    else if (at >= 0) { const uint8_t b = s2[at]; d += (b != (uint8_t)'-' && b != a) ? 1 : 0; }
                }
                const int rk = f.rank[k];
                if (best < 0 || d < best_d || (d == best_d && rk < best_rank)) { best_d = d; best_rank = rk; best = (int)k; }
            }
            if (best < 0) best_d = MIRGE_TRF_NO_DIST;
        }
        o_dist[x] = best_d;
        o_trf[x] = best;
    }
}

// ---- density-peak clustering of the reads stacked on one tRNA (--trf-clusters: getDistance / local_density / min_distance and the
// border loop of trna_deliverables, mirge2_tRF_a2i.py:122-207, 776-839)
// A POINT is a row of <sample>.aligned_tRFs.report: a read at a 0-based offset of its template, with its RP100K as a double.  A GROUP is
// the points of one (sample, tRNA).  k_trf_cluster_pack shifts every point's packed words to the template's columns once: S = 2-bit
// codes, F = per column bit 0 'the letter is N' and bit 1 'there is a letter'.  The distance of two points of a group is then
// |start difference| + |end difference| + popcount over the words of (letters differ) & (both have a letter): XOR and popcount, no
// text and no per-pair shift.  It is recomputed wherever it is needed; no n x n matrix exists.
//   k_trf_density : rho.  One lane per point i, a serial loop over j = first .. last of the group, the j side staged in LDS tiles of
//                   MIRGE_TRF_TJ points (every lane of a wave reads the same j: a broadcast).  rho[i] = sum of gauss[d(i, j)] * rp[j] over
//                   j != i in ascending j, then + rp[i], in doubles with the product and the sum rounded separately (trf_mul_add), then
//                   rounded to float32: the order and the roundings of the reference's double loop.  gauss[] comes from the host.
//   k_trf_nearest : over the points ahead of i in the order ascending (-rho as float32, index): how many there are (= i's position in
//                   sort_rho_idx) and the nearest of them, among equal distances the LAST in that order (the reference's `<=`).
//   k_trf_border  : per point the largest (rho[i] + rho[j]) / 2 in float32 over the j of other clusters within distance 3 (the host
//                   takes the maximum per cluster), and the distance to the centre of its own cluster.
// Grid: one workgroup per TILE = (group, MIRGE_BLOCK consecutive points of it) of a host-built list, so that a group of 20 000 points
// spreads over 79 workgroups and a group of one costs one.  NW = 64-bit words per template (4: up to 128 columns, 8: up to 256); the
// i side stays in 4 * NW VGPRs.  The O(n) steps between the launches (the first point's delta, centres, the chain cl[i] =
// cl[nneigh[i]], halo) are the host's (csrc/native_trf.hpp).
// (tests/hostsim/trf_sim.cpp compiles the kernels above for the host one thread after the other; the ones below need a barrier and LDS,
// which a host build gets from tests/hostsim/trf_cluster_sim.cpp)
#if defined(__HIPCC__) || defined(MIRGE_TRF_CLUSTER_SIM)
#define MIRGE_TRF_TJ 128            // points of the j side per LDS tile
#define MIRGE_TRF_CL_MAXW 8         // words per template at most
#define MIRGE_TRF_CL_MAXCOL 256     // ... = columns: a longer template is refused by mirge_trf_cluster
#define MIRGE_TRF_CL_MAXG (2 * MIRGE_TRF_CL_MAXCOL + 1)  // distances 0 .. 2 * columns

struct TrfClusterView {
    const uint64_t* words;       // [n_pts][2 * MIRGE_TRF_CL_MAXW]: S words, then F words
    const int32_t* start;        // [n_pts] first column with a letter (0-based)
    const int32_t* end;          // [n_pts] one past the last
    const double* rp;            // [n_pts]
    const uint32_t* grp_ptr;     // [n_grp + 1]
    const uint32_t* tile_grp;    // [n_tile]
    const uint32_t* tile_first;  // [n_tile] first point of the tile (index into the points)
    const double* gauss;         // [n_gauss] exp(-(d / 3) ** 2) as the host's math.exp gives it
    int32_t n_gauss, pad;
};

// product and sum rounded one after the other, never fused, whatever the build's -ffp-contract says
__host__ __device__ __forceinline__ double trf_mul_add(double acc, double a, double b) {
#pragma clang fp contract(off)
    const double p = a * b;
    return acc + p;
}
__host__ __device__ __forceinline__ float trf_half_sum(float a, float b) {
#pragma clang fp contract(off)
    const float s = a + b;
    return s * 0.5f;
}

template <int NW>
__host__ __device__ __forceinline__ int trf_pair_dist(const uint64_t* Si, const uint64_t* Fi, int sti, int eni, const uint64_t* Sj,
                                                      const uint64_t* Fj, int stj, int enj) {
    const uint64_t M = 0x5555555555555555ull;
    int d = (sti < stj ? stj - sti : sti - stj) + (eni < enj ? enj - eni : eni - enj);
#pragma unroll
    for (int w = 0; w < NW; w++) {
        const uint64_t x = Si[w] ^ Sj[w], fi = Fi[w], fj = Fj[w];
        const uint64_t differ = ((fi ^ fj) & M) | (((x | (x >> 1)) & M) & ~(fi | fj));  // N against a base | two bases that differ
        d += __popcll(differ & ((fi & fj) >> 1));
    }
    return d;
}

// flags[0]: 1 = a point's read is of the long class, 2 = a point does not fit its template or the template is too long
__global__ void k_trf_cluster_pack(TrfTables t, const uint32_t* __restrict__ read, const int32_t* __restrict__ off, const int32_t* __restrict__ tlen,
                                   uint32_t n_pts, uint64_t* __restrict__ words, int32_t* __restrict__ o_start, int32_t* __restrict__ o_end,
                                   uint32_t* __restrict__ flags) {
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n_pts; x += gridDim.x * blockDim.x) {
        uint32_t j;
        const int gi = trf_locate(t, read[x], j);
        const TrfGroup& g = t.g[gi];
        uint64_t* S = words + (size_t)x * (2 * MIRGE_TRF_CL_MAXW);
        uint64_t* F = S + MIRGE_TRF_CL_MAXW;
        for (int w = 0; w < 2 * MIRGE_TRF_CL_MAXW; w++) S[w] = 0ull;
        o_start[x] = 0; o_end[x] = 0;
        if (!g.W) { atomicOr(&flags[0], 1u); continue; }
        const int L = (int)g.len[j], o = off[x];
        if (o < 0 || L < 1 || tlen[x] > MIRGE_TRF_CL_MAXCOL || o + L > tlen[x]) { atomicOr(&flags[0], 2u); continue; }
        o_start[x] = o; o_end[x] = o + L;
        for (int w = 0; 32 * w < L; w++) {
            const int nb = L - 32 * w < 32 ? L - 32 * w : 32;
            const uint64_t lm = mirge_lowmask2(nb);
            const uint64_t nm = (g.nmask ? g.nmask[(size_t)w * g.n + j] : 0ull) & lm & 0x5555555555555555ull;
            const uint64_t s = g.seq[(size_t)w * g.n + j] & lm & ~(nm | (nm << 1));
            const uint64_t f = nm | (lm & 0xAAAAAAAAAAAAAAAAull);
            const int c0 = o + 32 * w, wi = c0 >> 5, sh = 2 * (c0 & 31);
            S[wi] |= s << sh; F[wi] |= f << sh;
            if (sh && wi + 1 < MIRGE_TRF_CL_MAXW) { S[wi + 1] |= s >> (64 - sh); F[wi + 1] |= f >> (64 - sh); }
        }
    }
}

// the j side of a tile in LDS; every thread of the workgroup takes part
template <int NW>
__device__ __forceinline__ void trf_stage_tile(const TrfClusterView& v, uint32_t j0, uint32_t nj, uint64_t* sS, uint64_t* sF, int* sSt, int* sEn) {
    for (uint32_t k = threadIdx.x; k < nj * NW; k += blockDim.x) {
        const uint32_t jj = k / NW, w = k % NW;
        const uint64_t* src = v.words + (size_t)(j0 + jj) * (2 * MIRGE_TRF_CL_MAXW);
        sS[k] = src[w]; sF[k] = src[MIRGE_TRF_CL_MAXW + w];
    }
    for (uint32_t k = threadIdx.x; k < nj; k += blockDim.x) { sSt[k] = v.start[j0 + k]; sEn[k] = v.end[j0 + k]; }
}

template <int NW>
__global__ void __launch_bounds__(MIRGE_BLOCK) k_trf_density(TrfClusterView v, uint32_t tile0, float* __restrict__ rho) {
    __shared__ uint64_t sS[MIRGE_TRF_TJ * NW], sF[MIRGE_TRF_TJ * NW];
    __shared__ int sSt[MIRGE_TRF_TJ], sEn[MIRGE_TRF_TJ];
    __shared__ double sRp[MIRGE_TRF_TJ], sG[MIRGE_TRF_CL_MAXG];
    const uint32_t tile = tile0 + blockIdx.x, grp = v.tile_grp[tile], lo = v.grp_ptr[grp], hi = v.grp_ptr[grp + 1];
    const uint32_t i = v.tile_first[tile] + threadIdx.x;
    const bool active = i < hi;
    const int ng = v.n_gauss < MIRGE_TRF_CL_MAXG ? v.n_gauss : MIRGE_TRF_CL_MAXG;
    for (int k = (int)threadIdx.x; k < ng; k += (int)blockDim.x) sG[k] = v.gauss[k];
    uint64_t Si[NW], Fi[NW];
    int sti = 0, eni = 0;
    if (active) {
        const uint64_t* src = v.words + (size_t)i * (2 * MIRGE_TRF_CL_MAXW);
#pragma unroll
        for (int w = 0; w < NW; w++) { Si[w] = src[w]; Fi[w] = src[MIRGE_TRF_CL_MAXW + w]; }
        sti = v.start[i]; eni = v.end[i];
    } else {
#pragma unroll
        for (int w = 0; w < NW; w++) { Si[w] = 0ull; Fi[w] = 0ull; }
    }
    double acc = 0.0;
    for (uint32_t j0 = lo; j0 < hi; j0 += MIRGE_TRF_TJ) {
        const uint32_t nj = hi - j0 < MIRGE_TRF_TJ ? hi - j0 : MIRGE_TRF_TJ;
        __syncthreads();  // (the tile before is read to its end; sG is written)
        trf_stage_tile<NW>(v, j0, nj, sS, sF, sSt, sEn);
        for (uint32_t k = threadIdx.x; k < nj; k += blockDim.x) sRp[k] = v.rp[j0 + k];
        __syncthreads();
        if (active)
            for (uint32_t jj = 0; jj < nj; jj++) {
                if (j0 + jj == i) continue;
                int d = trf_pair_dist<NW>(Si, Fi, sti, eni, sS + jj * NW, sF + jj * NW, sSt[jj], sEn[jj]);
                d = d < ng ? d : ng - 1;  // (never: the host's table reaches 2 * the longest template)
                acc = trf_mul_add(acc, sG[d], sRp[jj]);
            }
    }
    if (active) rho[i] = (float)trf_mul_add(acc, 1.0, v.rp[i]);
}

// is point a (density ra, index ia) ahead of point b in the order ascending (-rho, index)?
__host__ __device__ __forceinline__ bool trf_ahead(float ra, uint32_t ia, float rb, uint32_t ib) { return ra > rb || (ra == rb && ia < ib); }

// o_delta: the smallest distance (the first point of the order gets 0 here and its value from the host), o_nneigh: 1-based, 0 = none
template <int NW>
__global__ void __launch_bounds__(MIRGE_BLOCK) k_trf_nearest(TrfClusterView v, uint32_t tile0, const float* __restrict__ rho, float* __restrict__ o_delta,
                                                             int32_t* __restrict__ o_nneigh, int32_t* __restrict__ o_order) {
    __shared__ uint64_t sS[MIRGE_TRF_TJ * NW], sF[MIRGE_TRF_TJ * NW];
    __shared__ int sSt[MIRGE_TRF_TJ], sEn[MIRGE_TRF_TJ];
    __shared__ float sRho[MIRGE_TRF_TJ];
    const uint32_t tile = tile0 + blockIdx.x, grp = v.tile_grp[tile], lo = v.grp_ptr[grp], hi = v.grp_ptr[grp + 1];
    const uint32_t i = v.tile_first[tile] + threadIdx.x;
    const bool active = i < hi;
    uint64_t Si[NW], Fi[NW];
    int sti = 0, eni = 0;
    float ri = 0.0f;
    if (active) {
        const uint64_t* src = v.words + (size_t)i * (2 * MIRGE_TRF_CL_MAXW);
#pragma unroll
        for (int w = 0; w < NW; w++) { Si[w] = src[w]; Fi[w] = src[MIRGE_TRF_CL_MAXW + w]; }
        sti = v.start[i]; eni = v.end[i]; ri = rho[i];
    } else {
#pragma unroll
        for (int w = 0; w < NW; w++) { Si[w] = 0ull; Fi[w] = 0ull; }
    }
    int best_d = 0x7FFFFFFF, n_ahead = 0;
    uint32_t best_j = 0;
    float best_r = 0.0f;
    bool have = false;
    for (uint32_t j0 = lo; j0 < hi; j0 += MIRGE_TRF_TJ) {
        const uint32_t nj = hi - j0 < MIRGE_TRF_TJ ? hi - j0 : MIRGE_TRF_TJ;
        __syncthreads();
        trf_stage_tile<NW>(v, j0, nj, sS, sF, sSt, sEn);
        for (uint32_t k = threadIdx.x; k < nj; k += blockDim.x) sRho[k] = rho[j0 + k];
        __syncthreads();
        if (active)
            for (uint32_t jj = 0; jj < nj; jj++) {
                const uint32_t j = j0 + jj;
                const float rj = sRho[jj];
                if (j == i || !trf_ahead(rj, j, ri, i)) continue;
                n_ahead++;
                const int d = trf_pair_dist<NW>(Si, Fi, sti, eni, sS + jj * NW, sF + jj * NW, sSt[jj], sEn[jj]);
                if (!have || d < best_d || (d == best_d && trf_ahead(best_r, best_j, rj, j))) { have = true; best_d = d; best_j = j; best_r = rj; }
            }
    }
    if (active) {
        o_delta[i] = have ? (float)best_d : 0.0f;
        o_nneigh[i] = have ? (int32_t)(best_j - lo) + 1 : 0;
        o_order[i] = n_ahead;
    }
}

// cl: the point's cluster (1-based; <= 0: none), cen: the point index of its cluster's centre (or -1), grp_nclust: clusters of the group
template <int NW>
__global__ void __launch_bounds__(MIRGE_BLOCK) k_trf_border(TrfClusterView v, uint32_t tile0, const float* __restrict__ rho, const int32_t* __restrict__ cl,
                                                            const int32_t* __restrict__ cen, const int32_t* __restrict__ grp_nclust,
                                                            float* __restrict__ o_bmax, int32_t* __restrict__ o_dcen) {
    __shared__ uint64_t sS[MIRGE_TRF_TJ * NW], sF[MIRGE_TRF_TJ * NW];
    __shared__ int sSt[MIRGE_TRF_TJ], sEn[MIRGE_TRF_TJ], sCl[MIRGE_TRF_TJ];
    __shared__ float sRho[MIRGE_TRF_TJ];
    const uint32_t tile = tile0 + blockIdx.x, grp = v.tile_grp[tile], lo = v.grp_ptr[grp], hi = v.grp_ptr[grp + 1];
    const uint32_t i = v.tile_first[tile] + threadIdx.x;
    const bool active = i < hi;
    const int nclust = grp_nclust[grp];  // (the same for the whole workgroup: the branches below do not split a barrier)
    uint64_t Si[NW], Fi[NW];
    int sti = 0, eni = 0, ci = 0;
    float ri = 0.0f;
    if (active) {
        const uint64_t* src = v.words + (size_t)i * (2 * MIRGE_TRF_CL_MAXW);
#pragma unroll
        for (int w = 0; w < NW; w++) { Si[w] = src[w]; Fi[w] = src[MIRGE_TRF_CL_MAXW + w]; }
        sti = v.start[i]; eni = v.end[i]; ri = rho[i]; ci = cl[i];
    } else {
#pragma unroll
        for (int w = 0; w < NW; w++) { Si[w] = 0ull; Fi[w] = 0ull; }
    }
    float bmax = 0.0f;
    if (nclust > 1)
        for (uint32_t j0 = lo; j0 < hi; j0 += MIRGE_TRF_TJ) {
            const uint32_t nj = hi - j0 < MIRGE_TRF_TJ ? hi - j0 : MIRGE_TRF_TJ;
            __syncthreads();
            trf_stage_tile<NW>(v, j0, nj, sS, sF, sSt, sEn);
            for (uint32_t k = threadIdx.x; k < nj; k += blockDim.x) { sRho[k] = rho[j0 + k]; sCl[k] = cl[j0 + k]; }
            __syncthreads();
            if (active)
                for (uint32_t jj = 0; jj < nj; jj++) {
                    if (sCl[jj] == ci) continue;  // (also j == i)
                    const int d = trf_pair_dist<NW>(Si, Fi, sti, eni, sS + jj * NW, sF + jj * NW, sSt[jj], sEn[jj]);
                    if (d > 3) continue;
                    const float a = trf_half_sum(ri, sRho[jj]);
                    bmax = a > bmax ? a : bmax;
                }
        }
    if (active) {
        int dc = -1;
        const int32_t c = cen[i];
        if (c >= (int32_t)lo && c < (int32_t)hi) {
            const uint64_t* src = v.words + (size_t)c * (2 * MIRGE_TRF_CL_MAXW);
            uint64_t Sc[NW], Fc[NW];
#pragma unroll
            for (int w = 0; w < NW; w++) { Sc[w] = src[w]; Fc[w] = src[MIRGE_TRF_CL_MAXW + w]; }
            dc = trf_pair_dist<NW>(Si, Fi, sti, eni, Sc, Fc, v.start[c], v.end[c]);
        }
        o_bmax[i] = bmax;
        o_dcen[i] = dc;
    }
}

// ---- the O(n) steps between the launches, on the host (shared by csrc/native_trf.hpp and the host simulation)
// behind k_trf_nearest: the first point's delta (mirge2_tRF_a2i.py:206), the centres and the one-cluster fallback (:776-800), the chain
// cl[i] = cl[nneigh[i]] in density order (:802-804).  cen[p] = the point index of the centre of p's cluster, or -1.  -> 0, or -1 when
// `order` is no permutation of a group's positions
inline int trf_cluster_assign(int64_t n_grp, const int64_t* grp_ptr, const float* rho, float* delta, const int32_t* nneigh, const int32_t* order,
                              int32_t* cl, int32_t* centre, int32_t* nclust, int32_t* cen) {
    std::vector<int32_t> by_order;
    for (int64_t g = 0; g < n_grp; g++) {
        const size_t lo = (size_t)grp_ptr[g], m = (size_t)(grp_ptr[g + 1] - grp_ptr[g]);
        nclust[g] = 0;
        if (!m) continue;
        by_order.assign(m, -1);
        for (size_t k = 0; k < m; k++) {
            const int32_t o = order[lo + k];
            if (o < 0 || (size_t)o >= m || by_order[(size_t)o] >= 0) return -1;
            by_order[(size_t)o] = (int32_t)k;
        }
        const size_t top = lo + (size_t)by_order[0];
        float dmax = 0.0f;  // (max(delta) runs over the list's unused slot 0 too, which holds 0.0)
        for (size_t k = 0; k < m; k++)
            if (lo + k != top && delta[lo + k] > dmax) dmax = delta[lo + k];
        delta[top] = dmax;
        int nc = 0;
        for (size_t k = 0; k < m; k++) {
            cl[lo + k] = -1; centre[lo + k] = 0;
        }
        for (size_t k = 0; k < m; k++)
            if ((double)rho[lo + k] >= 5.0 && (double)delta[lo + k] >= 8.0) { cl[lo + k] = ++nc; centre[lo + (size_t)nc - 1] = (int32_t)k + 1; }
        // all of the reads in one cluster: .index(max(...)) is the first of the densest points, the first of the order
        if (nc == 0 && (double)dmax <= 8.0 && (double)rho[top] >= 5.0) { nc = 1; cl[top] = 1; centre[lo] = (int32_t)(top - lo) + 1; }
        for (size_t o = 0; o < m; o++) {
            const size_t k = lo + (size_t)by_order[o];
            if (cl[k] == -1 && nneigh[k] > 0 && (size_t)nneigh[k] <= m) cl[k] = cl[lo + (size_t)nneigh[k] - 1];
        }
        nclust[g] = nc;
        for (size_t k = 0; k < m; k++) cen[lo + k] = cl[lo + k] >= 1 ? (int32_t)lo + centre[lo + (size_t)cl[lo + k] - 1] - 1 : -1;
    }
    return 0;
}

// behind k_trf_border (:808-839): a cluster's border density is the largest of its points' bmax; a point is halo (0) when its density
// is below that or its centre is farther than 8 away; without a cluster everything is 0
inline void trf_cluster_halo(int64_t n_grp, const int64_t* grp_ptr, const float* rho, const int32_t* cl, const int32_t* nclust, const float* bmax,
                             const int32_t* dcen, int32_t* halo) {
    std::vector<float> bord;
    for (int64_t g = 0; g < n_grp; g++) {
        const size_t lo = (size_t)grp_ptr[g], hi = (size_t)grp_ptr[g + 1];
        const int nc = nclust[g];
        bord.assign((size_t)(nc > 0 ? nc : 0) + 1, 0.0f);
        if (nc > 1)
            for (size_t k = lo; k < hi; k++)
                if (cl[k] >= 1 && cl[k] <= nc && bmax[k] > bord[(size_t)cl[k]]) bord[(size_t)cl[k]] = bmax[k];
        for (size_t k = lo; k < hi; k++) {
            halo[k] = 0;
            if (nc < 1 || cl[k] < 1 || cl[k] > nc) continue;
            halo[k] = cl[k];
            if (nc > 1 && rho[k] < bord[(size_t)cl[k]]) halo[k] = 0;
            if (dcen[k] > 8) halo[k] = 0;
        }
    }
}
#endif  // __HIPCC__ || MIRGE_TRF_CLUSTER_SIM
