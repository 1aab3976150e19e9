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
