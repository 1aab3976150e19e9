// kernels_qc.hpp -- part of mirge_kernels.hpp: --read-qc (mirge3_amd/readqc.py holds the specification): histograms over the text of a parsed chunk
// and a weighted histogram over the dictionary.
//   k_qc_pos    : the `base` and `qual` tables, a lane per position, a wave taking four reads per step one after the other: the lanes of a step differ in row and never
//                 share an LDS word, whatever the qualities are.  32-bit counters for positions 0 .. 255 in LDS (a cell grows by at most one per
//                 read, and a chunk holds fewer than 2^32 reads), flushed to the 64-bit global tables once per workgroup; positions of 256 and
//                 more -- the overflow row -- go to the global table directly.  One launch per view: a view's tables take 99 KiB of LDS.
//   k_qc_read   : the per-read figures (length, quality mean, G + C, first letter, the scalars), a lane per read over the same, L2-warm text.
//                 TABLES = true is the other form of the text histogram (MIRGE_QC_FORM=read, the default): the lane adds its read's positions to
//                 `base` and `qual` as it walks them, so that the 64 lanes of a step add to the row of one position.  Measured on 10 M reads with a
//                 sequencer's qualities (profiles/read_qc.md) this form is the faster one: the same-address adds cost less than k_qc_pos's waits.
//   k_qc_class  : per unique read of the dictionary the class (res_pass, or n_pass: unmapped), the length and the first letter from the packed
//                 word and nmask; count[s] and (count[s] > 0) into a per-workgroup LDS tile of the lengths below 64, then into the 64-bit global
//                 cells [S][n_pass + 1][257][5][2].  blockIdx.y = the sample.
// All sums are integers: the tables are a function of the input alone.
// Compiled for the host too (tests/hostsim/qc_sim.cpp, MIRGE_QC_HOSTSIM): a workgroup's threads then run one after the other between its barriers.
#pragma once

#define MIRGE_QC_P 256          // positions and lengths of 256 and more share key 256
#define MIRGE_QC_NQ 94          // qualities 0 .. 93
#define MIRGE_QC_NL 5           // letters A C G T N
#define MIRGE_QC_LEN_MAX 65535  // the `length` table is exact up to here
// one view's tables, in 64-bit words (mirge_qc_fetch hands out two views back to back: raw, trimmed)
#define MIRGE_QC_SCALARS 0      // [8]: reads, bases, reads_with_N, empty_reads, qual_clamped, qual_length_mismatch, 0, 0
#define MIRGE_QC_LENGTH 8       // [65536]
#define MIRGE_QC_BASE (MIRGE_QC_LENGTH + MIRGE_QC_LEN_MAX + 1)            // [257][5]
#define MIRGE_QC_QUAL (MIRGE_QC_BASE + (MIRGE_QC_P + 1) * MIRGE_QC_NL)    // [257][94]
#define MIRGE_QC_MEANQ (MIRGE_QC_QUAL + (MIRGE_QC_P + 1) * MIRGE_QC_NQ)   // [94]
#define MIRGE_QC_GC (MIRGE_QC_MEANQ + MIRGE_QC_NQ)                        // [101]
#define MIRGE_QC_FIRST (MIRGE_QC_GC + 101)                                // [257][5]
#define MIRGE_QC_VIEW_WORDS (MIRGE_QC_FIRST + (MIRGE_QC_P + 1) * MIRGE_QC_NL)
#define MIRGE_QC_POS_THREADS 1024
#define MIRGE_QC_POS_BATCH 4     // records a wave of k_qc_pos takes per step
#define MIRGE_QC_POS_LDS_WORDS (MIRGE_QC_P * MIRGE_QC_NL + MIRGE_QC_P * MIRGE_QC_NQ)  // 32-bit words: base, then qual
#define MIRGE_QC_CLASS_TILE 64  // lengths below this are summed in LDS by k_qc_class

#ifdef MIRGE_QC_HOSTSIM
#define QC_EACH_THREAD for (threadIdx.x = 0; threadIdx.x < blockDim.x; threadIdx.x++)
#define QC_BARRIER
#define QC_SHARED static
#define QC_UNIFORM(x) (x)
static unsigned long long qc_dyn_host[1 << 15];
#define QC_DYN(T, name) T* const name = reinterpret_cast<T*>(qc_dyn_host)
#else
#define QC_EACH_THREAD
#define QC_BARRIER __syncthreads()
#define QC_SHARED __shared__
#define QC_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)
#define QC_DYN(T, name) extern __shared__ __attribute__((aligned(16))) unsigned char qc_dyn_raw[]; T* const name = reinterpret_cast<T*>(qc_dyn_raw)
#endif

// what a launch looks at: the sequence line of every record, its quality line (FASTQ) or null, and for the trimmed view the bounds the modifier
// chain left (vstart[r * vstride + voff]; null: the line itself)
struct QcJob {
    const uint8_t* text;
    const int64_t *lstart, *lend, *qstart, *qend, *vstart, *vend;
    uint32_t n, vstride, voff;
    int32_t view;     // 0 raw, 1 trimmed
    int32_t min_len;  // the trimmed view holds the reads of at least this length
    int32_t base;     // phred base
};
struct QcRec {
    int64_t b, qb;
    uint32_t len;
    bool exists, has_q, mismatch;
};

__device__ __forceinline__ uint32_t qc_letter(uint8_t c) {
    const uint8_t u = c & 0xDF;
    return u == 'A' ? 0u : (u == 'C' ? 1u : (u == 'G' ? 2u : ((u == 'T' || u == 'U') ? 3u : 4u)));
}

__device__ __forceinline__ QcRec qc_rec(const QcJob& j, uint32_t r) {
    QcRec x;
    int64_t b = j.lstart[r], e = j.lend[r];
    if (e > b && j.text[e - 1] == 13) e--;
    x.qb = 0; x.has_q = false; x.mismatch = false;
    if (j.qstart) {
        const int64_t qb = j.qstart[r];
        int64_t qe = j.qend[r];
        if (qe > qb && j.text[qe - 1] == 13) qe--;
        if (qe - qb != e - b) x.mismatch = true;
        else { x.has_q = true; x.qb = qb; }
    }
    if (j.view == 1 && j.vstart) {
        const int64_t vb = j.vstart[(size_t)r * j.vstride + j.voff], ve = j.vend[(size_t)r * j.vstride + j.voff];
        x.qb += vb - b;
        b = vb; e = ve;
    }
    const int64_t L = e > b ? e - b : 0;
    x.b = b;
    x.len = (uint32_t)(L > 0x7FFFFFFF ? 0x7FFFFFFF : L);
    x.exists = j.view == 0 || L >= (int64_t)j.min_len;
    return x;
}

// quality of a byte, clamped to [0, 93]; `clamped` counts the bytes that needed it
__device__ __forceinline__ uint32_t qc_quality(uint8_t byte, int32_t base, uint32_t& clamped) {
    int q = (int)byte - base;
    if (q < 0) { q = 0; clamped++; }
    if (q > MIRGE_QC_NQ - 1) { q = MIRGE_QC_NQ - 1; clamped++; }
    return (uint32_t)q;
}

__global__ void __launch_bounds__(MIRGE_QC_POS_THREADS) k_qc_pos(QcJob j, unsigned long long* __restrict__ tab) {
    QC_DYN(uint32_t, s_tab);  // [256][5] base, then [256][94] qual when the text has qualities
    uint32_t* const s_base = s_tab;
    uint32_t* const s_qual = s_tab + MIRGE_QC_P * MIRGE_QC_NL;
    const uint32_t words = j.qstart ? MIRGE_QC_POS_LDS_WORDS : MIRGE_QC_P * MIRGE_QC_NL;
    QC_EACH_THREAD {
        for (uint32_t i = threadIdx.x; i < words; i += blockDim.x) s_tab[i] = 0u;
    }
    QC_BARRIER;
    QC_EACH_THREAD {
        // a wave takes MIRGE_QC_POS_BATCH records per step: their bounds, then their first 64 letters and qualities, are loaded together (one
        // record per step left a wave waiting out three dependent loads per record); what lies beyond position 63 follows record by record
        const uint32_t lane = threadIdx.x & 63u, wave = QC_UNIFORM(threadIdx.x >> 6), per_block = blockDim.x >> 6;
        for (uint32_t r0 = (blockIdx.x * per_block + wave) * MIRGE_QC_POS_BATCH; r0 < j.n; r0 += gridDim.x * per_block * MIRGE_QC_POS_BATCH) {
            QcRec x[MIRGE_QC_POS_BATCH];
#pragma unroll
            for (int u = 0; u < MIRGE_QC_POS_BATCH; u++) {
                x[u].b = x[u].qb = 0; x[u].len = 0; x[u].exists = x[u].has_q = x[u].mismatch = false;
                if (r0 + u < j.n) x[u] = qc_rec(j, r0 + u);
                if (!x[u].exists) x[u].len = 0;
            }
            uint8_t c[MIRGE_QC_POS_BATCH], qv[MIRGE_QC_POS_BATCH];
#pragma unroll
            for (int u = 0; u < MIRGE_QC_POS_BATCH; u++) {
                const bool in = lane < x[u].len;
                c[u] = in ? j.text[x[u].b + lane] : (uint8_t)0;
                qv[u] = in && x[u].has_q ? j.text[x[u].qb + lane] : (uint8_t)0;
            }
#pragma unroll
            for (int u = 0; u < MIRGE_QC_POS_BATCH; u++) {
                if (lane >= x[u].len) continue;
                atomicAdd(&s_base[lane * MIRGE_QC_NL + qc_letter(c[u])], 1u);
                if (x[u].has_q) {
                    uint32_t unused = 0;
                    atomicAdd(&s_qual[lane * MIRGE_QC_NQ + qc_quality(qv[u], j.base, unused)], 1u);
                }
            }
#pragma unroll
            for (int u = 0; u < MIRGE_QC_POS_BATCH; u++)
                for (uint32_t p = lane + 64u; p < x[u].len; p += 64u) {
                    const uint32_t l = qc_letter(j.text[x[u].b + p]);
                    if (p < MIRGE_QC_P) atomicAdd(&s_base[p * MIRGE_QC_NL + l], 1u);
                    else atomicAdd(&tab[MIRGE_QC_BASE + MIRGE_QC_P * MIRGE_QC_NL + l], 1ull);
                    if (x[u].has_q) {
                        uint32_t unused = 0;
                        const uint32_t q = qc_quality(j.text[x[u].qb + p], j.base, unused);
                        if (p < MIRGE_QC_P) atomicAdd(&s_qual[p * MIRGE_QC_NQ + q], 1u);
                        else atomicAdd(&tab[MIRGE_QC_QUAL + MIRGE_QC_P * MIRGE_QC_NQ + q], 1ull);
                    }
                }
        }
    }
    QC_BARRIER;
    QC_EACH_THREAD {
        for (uint32_t i = threadIdx.x; i < words; i += blockDim.x) {
            const uint32_t v = s_tab[i];
            if (!v) continue;
            const uint32_t at = i < MIRGE_QC_P * MIRGE_QC_NL ? MIRGE_QC_BASE + i : MIRGE_QC_QUAL + (i - MIRGE_QC_P * MIRGE_QC_NL);
            atomicAdd(&tab[at], (unsigned long long)v);
        }
    }
}

// (launched as one workgroup of 256 threads per CU at most.  More workgroups: every one ends with a global atomic per cell it touched, on the same
//  few hundred addresses -- with 2 048 workgroups that flush was most of the kernel's 8 ms on 10 M reads.  More threads: a lane walks its own read
//  byte by byte, so the lines of all resident lanes must stay cached while they are walked -- 1 024 threads per CU took 28 ms where 256 take 11 on
//  3.5 M reads of 150 nt, whose lanes share no line)
template <bool TABLES>
__global__ void __launch_bounds__(MIRGE_BLOCK) k_qc_read(QcJob j, unsigned long long* __restrict__ tab) {
    QC_SHARED uint32_t s_len[MIRGE_QC_P + 1];
    QC_SHARED uint32_t s_meanq[MIRGE_QC_NQ];
    QC_SHARED uint32_t s_gc[101];
    QC_SHARED uint32_t s_first[(MIRGE_QC_P + 1) * MIRGE_QC_NL];
    QC_SHARED unsigned long long s_sc[8];
    QC_DYN(uint32_t, s_tab);  // TABLES: as in k_qc_pos
    uint32_t* const s_base = s_tab;
    uint32_t* const s_qual = s_tab + MIRGE_QC_P * MIRGE_QC_NL;
    const uint32_t words = !TABLES ? 0u : (j.qstart ? MIRGE_QC_POS_LDS_WORDS : MIRGE_QC_P * MIRGE_QC_NL);
    QC_EACH_THREAD {
        for (uint32_t i = threadIdx.x; i <= MIRGE_QC_P; i += blockDim.x) s_len[i] = 0u;
        for (uint32_t i = threadIdx.x; i < MIRGE_QC_NQ; i += blockDim.x) s_meanq[i] = 0u;
        for (uint32_t i = threadIdx.x; i < 101; i += blockDim.x) s_gc[i] = 0u;
        for (uint32_t i = threadIdx.x; i < (MIRGE_QC_P + 1) * MIRGE_QC_NL; i += blockDim.x) s_first[i] = 0u;
        if (threadIdx.x < 8) s_sc[threadIdx.x] = 0ull;
        for (uint32_t i = threadIdx.x; i < words; i += blockDim.x) s_tab[i] = 0u;
    }
    QC_BARRIER;
    QC_EACH_THREAD {
        unsigned long long reads = 0, bases = 0, with_n = 0, empty = 0, clamped_all = 0, mismatch = 0;
        for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < j.n; r += gridDim.x * blockDim.x) {
            const QcRec x = qc_rec(j, r);
            if (!x.exists) continue;
            reads++; bases += x.len; mismatch += x.mismatch ? 1u : 0u;
            const uint32_t lk = x.len < MIRGE_QC_LEN_MAX ? x.len : MIRGE_QC_LEN_MAX;
            if (lk <= MIRGE_QC_P) atomicAdd(&s_len[lk], 1u);
            else atomicAdd(&tab[MIRGE_QC_LENGTH + lk], 1ull);
            if (!x.len) { empty++; continue; }
            uint32_t gc = 0, n_n = 0, qsum = 0, clamped = 0, first = 0;
            for (uint32_t p = 0; p < x.len; p++) {
                const uint32_t l = qc_letter(j.text[x.b + p]);
                gc += (l == 1u || l == 2u) ? 1u : 0u;
                n_n += l == 4u ? 1u : 0u;
                if (p == 0) first = l;
                uint32_t q = 0;
                if (x.has_q) { q = qc_quality(j.text[x.qb + p], j.base, clamped); qsum += q; }
                if (TABLES) {
                    if (p < MIRGE_QC_P) atomicAdd(&s_base[p * MIRGE_QC_NL + l], 1u);
                    else atomicAdd(&tab[MIRGE_QC_BASE + MIRGE_QC_P * MIRGE_QC_NL + l], 1ull);
                    if (x.has_q) {
                        if (p < MIRGE_QC_P) atomicAdd(&s_qual[p * MIRGE_QC_NQ + q], 1u);
                        else atomicAdd(&tab[MIRGE_QC_QUAL + MIRGE_QC_P * MIRGE_QC_NQ + q], 1ull);
                    }
                }
            }
            with_n += n_n ? 1u : 0u;
            clamped_all += clamped;
            if (x.has_q) atomicAdd(&s_meanq[qsum / x.len], 1u);
            atomicAdd(&s_gc[(uint32_t)((100ull * gc) / x.len)], 1u);
            atomicAdd(&s_first[(x.len < MIRGE_QC_P ? x.len : MIRGE_QC_P) * MIRGE_QC_NL + first], 1u);
        }
        if (reads) atomicAdd(&s_sc[0], reads);
        if (bases) atomicAdd(&s_sc[1], bases);
        if (with_n) atomicAdd(&s_sc[2], with_n);
        if (empty) atomicAdd(&s_sc[3], empty);
        if (clamped_all) atomicAdd(&s_sc[4], clamped_all);
        if (mismatch) atomicAdd(&s_sc[5], mismatch);
    }
    QC_BARRIER;
    QC_EACH_THREAD {
        for (uint32_t i = threadIdx.x; i <= MIRGE_QC_P; i += blockDim.x)
            if (s_len[i]) atomicAdd(&tab[MIRGE_QC_LENGTH + i], (unsigned long long)s_len[i]);
        for (uint32_t i = threadIdx.x; i < MIRGE_QC_NQ; i += blockDim.x)
            if (s_meanq[i]) atomicAdd(&tab[MIRGE_QC_MEANQ + i], (unsigned long long)s_meanq[i]);
        for (uint32_t i = threadIdx.x; i < 101; i += blockDim.x)
            if (s_gc[i]) atomicAdd(&tab[MIRGE_QC_GC + i], (unsigned long long)s_gc[i]);
        for (uint32_t i = threadIdx.x; i < (MIRGE_QC_P + 1) * MIRGE_QC_NL; i += blockDim.x)
            if (s_first[i]) atomicAdd(&tab[MIRGE_QC_FIRST + i], (unsigned long long)s_first[i]);
        if (threadIdx.x < 8 && s_sc[threadIdx.x]) atomicAdd(&tab[MIRGE_QC_SCALARS + threadIdx.x], s_sc[threadIdx.x]);
        for (uint32_t i = threadIdx.x; i < words; i += blockDim.x) {
            const uint32_t v = s_tab[i];
            if (!v) continue;
            const uint32_t at = i < MIRGE_QC_P * MIRGE_QC_NL ? MIRGE_QC_BASE + i : MIRGE_QC_QUAL + (i - MIRGE_QC_P * MIRGE_QC_NL);
            atomicAdd(&tab[at], (unsigned long long)v);
        }
    }
}

// the groups of a dictionary, back to back (as JoinGroups): the first packed word and nmask word of every read, its length, its pass, its counts
#define MIRGE_QC_NGROUPS 10
struct QcClassGroups {
    const int8_t* pass[MIRGE_QC_NGROUPS];
    const uint64_t* seq[MIRGE_QC_NGROUPS];
    const uint64_t* nmask[MIRGE_QC_NGROUPS];  // or nullptr
    const uint8_t* len[MIRGE_QC_NGROUPS];     // uint16 behind the pointer where len16 is set
    const uint32_t* counts[MIRGE_QC_NGROUPS];
    uint8_t len16[MIRGE_QC_NGROUPS];
    uint32_t start[MIRGE_QC_NGROUPS + 1];
    int32_t n_groups;
};

// out: [S][n_pass + 1][257][5][2] (raw reads, unique reads).  use_lds: the dynamic LDS holds (n_pass + 1) * 64 * 5 * 2 64-bit cells.
__global__ void __launch_bounds__(MIRGE_BLOCK) k_qc_class(QcClassGroups gs, int32_t S, int32_t n_pass, int32_t use_lds, unsigned long long* __restrict__ out) {
    QC_DYN(unsigned long long, s_tile);
    const uint32_t s = blockIdx.y;
    const uint32_t tile_cells = use_lds ? (uint32_t)(n_pass + 1) * MIRGE_QC_CLASS_TILE * MIRGE_QC_NL * 2u : 0u;
    unsigned long long* const mine = out + (size_t)s * (size_t)(n_pass + 1) * (MIRGE_QC_P + 1) * MIRGE_QC_NL * 2;
    QC_EACH_THREAD {
        for (uint32_t i = threadIdx.x; i < tile_cells; i += blockDim.x) s_tile[i] = 0ull;
    }
    QC_BARRIER;
    QC_EACH_THREAD {
        const uint32_t total = gs.start[gs.n_groups];
        for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
            int k = 0;
            for (int q = 1; q < MIRGE_QC_NGROUPS; q++) if (q < gs.n_groups && t >= gs.start[q]) k = q;
            const uint32_t i = t - gs.start[k];
            const unsigned long long c = gs.counts[k][(size_t)i * S + s];
            if (!c) continue;
            const int p = gs.pass[k][i];
            const uint32_t cls = p >= 0 && p < n_pass ? (uint32_t)p : (uint32_t)n_pass;
            const uint32_t L = gs.len16[k] ? (uint32_t)reinterpret_cast<const uint16_t*>(gs.len[k])[i] : (uint32_t)gs.len[k][i];
            uint32_t l = 4u;  // N; also what an empty read is filed under
            if (L && !(gs.nmask[k] && (gs.nmask[k][i] & 1ull))) l = (uint32_t)(gs.seq[k][i] & 3ull);
            const uint32_t lk = L < MIRGE_QC_P ? L : MIRGE_QC_P;
            if (use_lds && lk < MIRGE_QC_CLASS_TILE) {
                unsigned long long* const cell = s_tile + ((size_t)(cls * MIRGE_QC_CLASS_TILE + lk) * MIRGE_QC_NL + l) * 2;
                atomicAdd(cell, c);
                atomicAdd(cell + 1, 1ull);
            } else {
                unsigned long long* const cell = mine + ((size_t)(cls * (MIRGE_QC_P + 1) + lk) * MIRGE_QC_NL + l) * 2;
                atomicAdd(cell, c);
                atomicAdd(cell + 1, 1ull);
            }
        }
    }
    QC_BARRIER;
    QC_EACH_THREAD {
        for (uint32_t i = threadIdx.x; i < tile_cells; i += blockDim.x) {
            const unsigned long long v = s_tile[i];
            if (!v) continue;
            const uint32_t which = i & 1u, l = (i >> 1) % MIRGE_QC_NL, lk = ((i >> 1) / MIRGE_QC_NL) % MIRGE_QC_CLASS_TILE,
                           cls = ((i >> 1) / MIRGE_QC_NL) / MIRGE_QC_CLASS_TILE;
            atomicAdd(mine + ((size_t)(cls * (MIRGE_QC_P + 1) + lk) * MIRGE_QC_NL + l) * 2 + which, v);
        }
    }
}
