// kernels_genome.hpp -- part of mirge_kernels.hpp: the A-to-I report's whole-genome filter (rows a16 / N1), i.e. the two
// `bowtie <org>_genome -n N -f -a -3 2` runs of mirge2_tRF_a2i.py:1056-1096,1297-1316 as one streamed pass of the genome.
//
// The genome on the device is bowtie's own reference stream (.4.ebwt): the unambiguous stretches back to back, 2 bits per base,
// base i at bits 2*(i & 31) of little-endian word i >> 5 (A0 C1 G2 T3), plus the stream positions where its stretches start.
// A window is valid iff it lies inside one stretch (no N, no reference boundary).  The queries are few (10^3..10^5); each one's
// seed is cut into n_mm + 1 pieces on both strands (pigeonhole: a window with <= n_mm seed mismatches has one exact piece), the
// pieces' leading bases are sorted into small tables, and every genome position probes those tables with its own k-mers.
#pragma once

#define MIRGE_GENOME_MAXLEN 64    // trimmed query length held in two words
#define MIRGE_GENOME_MAXPIECES 3  // n_mm <= 2
#define MIRGE_GENOME_MINSEED 5    // bowtie's floor for -l; every one of the <= 3 pieces of a seed holds a base
#define MIRGE_GENOME_MAXK 13      // longest table key (a 4^13-bit = 8 MiB presence bitmap)
#define MIRGE_GENOME_STRIP 32     // genome positions per thread and loop trip: one text word

struct GenomeQS {  // one query on one strand, laid on the forward text ('-': the reverse complement; its seed is the END)
    uint64_t q[2];     // bases, 2 bits at bit 2t (N -> 0)
    uint64_t nm[2];    // bit 2t: base t is N (mismatches everything)
    uint64_t seed[2];  // bit 2t: base t lies in the seed
    uint32_t query;
    uint8_t len;       // trimmed length; 0: the query has no alignment (L < 1 or L <= n_mm)
    uint8_t npieces;
    uint8_t poff[MIRGE_GENOME_MAXPIECES], plen[MIRGE_GENOME_MAXPIECES];
};

struct GenomeQueryArgs {
    const char* ascii;
    const int64_t* off;
    uint32_t n;
    int32_t n_mm, seedlen, trim5, trim3, kmax;
    int32_t norc;  // forward strand only: the '-' entries stay empty (len 0, no key)
};

#define MIRGE_GENOME_NOKEY 0xFFFFFFFFFFFFFFFFull

// even-bit mask of positions [lo, hi) of a 64-base word (0 <= lo <= hi <= 32 per word after clamping)
__device__ __forceinline__ uint64_t genome_range_mask(int lo, int hi) {
    lo = lo < 0 ? 0 : (lo > 32 ? 32 : lo);
    hi = hi < 0 ? 0 : (hi > 32 ? 32 : hi);
    if (hi <= lo) return 0ull;
    const uint64_t up = hi >= 32 ? ~0ull : ((1ull << (2 * hi)) - 1ull);
    const uint64_t dn = (1ull << (2 * lo)) - 1ull;
    return (up & ~dn) & 0x5555555555555555ull;
}

// one thread per query: both strands encoded, pieces cut, one sort key per indexable piece (table kk = min(piece, kmax) in the
// bits above 32, the piece's first kk bases below; a piece holding an N can never be exact and gets MIRGE_GENOME_NOKEY)
__global__ void k_genome_queries(GenomeQueryArgs a, GenomeQS* __restrict__ qs, uint64_t* __restrict__ keys,
                                 uint32_t* __restrict__ vals) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int P = a.n_mm + 1;
    const int64_t b = a.off[i], e = a.off[i + 1];
    const int L = (int)(e - b) - a.trim5 - a.trim3;
    for (int s = 0; s < 2; s++) {
        GenomeQS g;
        g.q[0] = g.q[1] = g.nm[0] = g.nm[1] = g.seed[0] = g.seed[1] = 0ull;
        g.query = i;
        g.len = 0;
        g.npieces = 0;
        for (int j = 0; j < MIRGE_GENOME_MAXPIECES; j++) g.poff[j] = g.plen[j] = 0;
        const uint32_t slot = 2 * i + s;
        for (int j = 0; j < P; j++) {
            keys[(size_t)slot * P + j] = MIRGE_GENOME_NOKEY;
            vals[(size_t)slot * P + j] = slot * 4u + j;
        }
        if (L >= 1 && L > a.n_mm && L <= MIRGE_GENOME_MAXLEN && !(s == 1 && a.norc)) {
            for (int t = 0; t < L; t++) {
                const char ch = a.ascii[b + a.trim5 + (s == 0 ? t : L - 1 - t)];
                int c = -1;
                if (ch == 'A' || ch == 'a') c = 0;
                else if (ch == 'C' || ch == 'c') c = 1;
                else if (ch == 'G' || ch == 'g') c = 2;
                else if (ch == 'T' || ch == 't') c = 3;
                if (c >= 0 && s == 1) c = 3 - c;
                if (c < 0) g.nm[t >> 5] |= 1ull << (2 * (t & 31));
                else g.q[t >> 5] |= (uint64_t)c << (2 * (t & 31));
            }
            const int sl = a.seedlen < L ? a.seedlen : L;
            const int s0 = s == 0 ? 0 : L - sl;  // '-': the read's 5' end is the end of its reverse complement
            g.seed[0] = genome_range_mask(s0, s0 + sl);
            g.seed[1] = genome_range_mask(s0 - 32, s0 + sl - 32);
            g.len = (uint8_t)L;
            g.npieces = (uint8_t)P;
            for (int j = 0; j < P; j++) {
                const int lo = s0 + (j * sl) / P, hi = s0 + ((j + 1) * sl) / P;
                g.poff[j] = (uint8_t)lo;
                g.plen[j] = (uint8_t)(hi - lo);
                const uint64_t pm0 = genome_range_mask(lo, hi), pm1 = genome_range_mask(lo - 32, hi - 32);
                if ((g.nm[0] & pm0) | (g.nm[1] & pm1)) continue;
                const int kk = (hi - lo) < a.kmax ? (hi - lo) : a.kmax;
                // the piece's first kk bases: bits [2 lo, 2 (lo + kk)) of the 128-bit pattern
                uint64_t v;
                if (lo >= 32) v = g.q[1] >> (2 * (lo - 32));
                else if (lo == 0) v = g.q[0];
                else v = (g.q[0] >> (2 * lo)) | (g.q[1] << (64 - 2 * lo));
                v &= (1ull << (2 * kk)) - 1ull;
                keys[(size_t)slot * P + j] = ((uint64_t)kk << 32) | v;
            }
        }
        qs[slot] = g;
    }
}

// one thread per sorted key: the presence bit of the key in its table's bitmap, the table's [begin, end) in the sorted arrays
__global__ void k_genome_index(const uint64_t* __restrict__ skeys, uint32_t n, const uint64_t* __restrict__ bm_word_off,
                               uint32_t* __restrict__ bitmap, uint32_t* __restrict__ tab_b, uint32_t* __restrict__ tab_e) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = skeys[i];
    if (k == MIRGE_GENOME_NOKEY) return;
    const uint32_t t = (uint32_t)(k >> 32), v = (uint32_t)k;
    atomicOr(&bitmap[bm_word_off[t] + (v >> 5)], 1u << (v & 31));
    if (i == 0 || (uint32_t)(skeys[i - 1] >> 32) != t) tab_b[t] = i;
    if (i + 1 == n || skeys[i + 1] == MIRGE_GENOME_NOKEY || (uint32_t)(skeys[i + 1] >> 32) != t) tab_e[t] = i + 1;
}

struct GenomeScanArgs {
    const uint64_t* text;      // the packed stream, padded by >= 3 words
    uint64_t n_bases;
    const uint64_t* s_start;   // [n_str + 1] stream positions where the stretches start (s_start[n_str] = n_bases)
    uint32_t n_str;
    const uint32_t* bitmap;
    const uint64_t* skeys;
    const uint32_t* svals;
    const GenomeQS* qs;
    unsigned long long* counts;  // [n queries][3]: alignments with 0, 1, 2 mismatches -- in the seed when strata, else in all
    int32_t n_mm, maxtotal;
    int32_t ntab;                // tables present (key length tab_k[t], words at tab_bm[t], sorted slice [tab_b, tab_e))
    int32_t tab_k[MIRGE_GENOME_MAXK];
    uint64_t tab_bm[MIRGE_GENOME_MAXK];
    uint32_t tab_b[MIRGE_GENOME_MAXK], tab_e[MIRGE_GENOME_MAXK];
    // the fill pass (k_genome_scan<true>, mirge_genome_align_loci): query q's records go to [range[q], range[q + 1]) -- empty for
    // a query that reports nothing -- at the place its cursor hands out
    const uint64_t* range;       // [n queries + 1]
    uint32_t* cursor;            // [n queries], zeroed
    uint64_t* rec_pos;           // stream position of the window's first base
    uint32_t* rec_meta;          // (query_base + query) << 3 | strand << 2 | mismatches
    uint32_t* overflow;          // set when a cursor leaves its range (the two passes disagree: a bug, reported by the host)
    uint32_t query_base;
    // --best --strata (mirge_genome_align_loci_strata): a query's stratum is its fewest SEED mismatches.  The count pass then
    // counts by seed mismatches, so that the host reads the best stratum and its size from the same [n][3]; the fill pass drops
    // every candidate whose seed mismatches are not best[query]
    int32_t strata;
    const uint8_t* best;         // [n queries], fill pass under strata
};

#define MIRGE_GENOME_STASH 4  // hits a lane keeps per trip for the wave's merged flush (more go out one atomic each)

__device__ __forceinline__ void genome_window(const uint64_t* __restrict__ text, uint64_t ws, uint64_t& w0, uint64_t& w1) {
    const uint64_t i = ws >> 5;
    const uint32_t sh = (uint32_t)(ws & 31) * 2;
    const uint64_t a = text[i], b = text[i + 1], c = text[i + 2];
    if (sh) { w0 = (a >> sh) | (b << (64 - sh)); w1 = (b >> sh) | (c << (64 - sh)); }
    else { w0 = a; w1 = b; }
}

// The scan.  Thread = one strip of 32 stream positions per trip (one text word plus the next for keys that reach across it);
// the trip count is uniform over the wave, so that the wave can merge its lanes' hits at the end of every trip: lanes that hit
// the same (query, mismatches) add their counts into one atomic (a query with 10^5..10^6 repeat copies does not serialise on
// one address).  Per position: every present table is probed with the position's own k-mer through its presence bitmap; a
// set bit is looked up in the sorted keys, and every (query, strand, piece) under it is verified in full.  An alignment is
// counted by its OWNER only -- the first piece of its (query, strand) that is exact in the window -- so that it is counted
// once however many of its pieces are exact.
// FILL: the same scan writes every alignment it would count as a record.  A lane keeps its trip's hits in LDS; at the end of the
// trip the wave hands them out query by query: one atomic on the query's cursor per distinct query of the wave, every lane
// taking its rank under it (a query planted 10^5 times costs one atomic per wave and trip, as in the count pass).
template <bool FILL>
__global__ void __launch_bounds__(256) k_genome_scan(GenomeScanArgs a) {
    __shared__ uint64_t st_pos[FILL ? 256 * MIRGE_GENOME_STASH : 1];
    __shared__ uint32_t st_meta[FILL ? 256 * MIRGE_GENOME_STASH : 1];
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t n_strips = (a.n_bases + MIRGE_GENOME_STRIP - 1) / MIRGE_GENOME_STRIP;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint64_t sb = 1, se = 0;  // the stretch of the last candidate: [sb, se) (empty until looked up)
    for (uint64_t w0s = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); w0s < n_strips; w0s += stride) {
        const uint64_t strip = w0s + lane;
        uint32_t acc_key = 0xFFFFFFFFu;
        unsigned long long acc_n = 0;
        int n_st = 0;
        if (strip < n_strips) {
            const uint64_t wa = a.text[strip], wb = a.text[strip + 1];
            for (int i = 0; i < MIRGE_GENOME_STRIP; i++) {
                const uint64_t p = strip * MIRGE_GENOME_STRIP + i;
                if (p >= a.n_bases) break;
                const uint64_t kw = i ? ((wa >> (2 * i)) | (wb << (64 - 2 * i))) : wa;
                for (int t = 0; t < a.ntab; t++) {
                    const int kk = a.tab_k[t];
                    const uint32_t key = (uint32_t)(kw & ((1ull << (2 * kk)) - 1ull));
                    if (!((a.bitmap[a.tab_bm[t] + (key >> 5)] >> (key & 31)) & 1u)) continue;
                    const uint64_t fk = ((uint64_t)kk << 32) | key;
                    uint32_t lo = a.tab_b[t], hi = a.tab_e[t];
                    while (lo < hi) {
                        const uint32_t mid = (lo + hi) >> 1;
                        if (a.skeys[mid] < fk) lo = mid + 1; else hi = mid;
                    }
                    if (p < sb || p >= se) {  // the stretch that holds p
                        uint32_t l = 0, h = a.n_str;  // largest s with s_start[s] <= p
                        while (h - l > 1) {
                            const uint32_t m = (l + h) >> 1;
                            if (a.s_start[m] <= p) l = m; else h = m;
                        }
                        sb = a.s_start[l];
                        se = a.s_start[l + 1];
                    }
                    for (uint32_t j = lo; j < a.tab_e[t] && a.skeys[j] == fk; j++) {
                        const uint32_t v = a.svals[j];
                        const GenomeQS& g = a.qs[v >> 2];
                        const uint32_t piece = v & 3u;
                        const uint64_t po = g.poff[piece];
                        if (p < sb + po) continue;
                        const uint64_t ws = p - po;
                        if (ws + g.len > se) continue;
                        uint64_t x0, x1;
                        genome_window(a.text, ws, x0, x1);
                        x0 ^= g.q[0];
                        x1 ^= g.q[1];
                        const uint64_t lm0 = genome_range_mask(0, g.len), lm1 = genome_range_mask(-32, (int)g.len - 32);
                        const uint64_t d0 = (((x0 | (x0 >> 1)) & 0x5555555555555555ull) | g.nm[0]) & lm0;
                        const uint64_t d1 = (((x1 | (x1 >> 1)) & 0x5555555555555555ull) | g.nm[1]) & lm1;
                        const int tot = __popcll(d0) + __popcll(d1);
                        if (tot > a.maxtotal) continue;
                        const int sd = __popcll(d0 & g.seed[0]) + __popcll(d1 & g.seed[1]);
                        if (sd > a.n_mm) continue;
                        int owner = -1;
                        for (int q = 0; q < g.npieces && owner < 0; q++) {
                            const int plo = g.poff[q], phi = plo + g.plen[q];
                            if (!((d0 & genome_range_mask(plo, phi)) | (d1 & genome_range_mask(plo - 32, phi - 32)))) owner = q;
                        }
                        if (owner != (int)piece) continue;
                        if constexpr (FILL) {
                            const uint64_t rs = a.range[g.query], len = a.range[g.query + 1] - rs;
                            if (!len) continue;  // capped by max_loci
                            if (a.strata && sd != (int)a.best[g.query]) continue;  // a worse stratum takes no slot
                            const uint32_t meta = ((a.query_base + g.query) << 3) | (((v >> 2) & 1u) << 2) | (uint32_t)tot;
                            if (n_st < MIRGE_GENOME_STASH) {
                                st_pos[n_st * 256 + threadIdx.x] = ws;
                                st_meta[n_st * 256 + threadIdx.x] = meta;
                                n_st++;
                            } else {
                                const uint32_t idx = atomicAdd(&a.cursor[g.query], 1u);
                                if (idx < len) { a.rec_pos[rs + idx] = ws; a.rec_meta[rs + idx] = meta; }
                                else atomicOr(a.overflow, 1u);
                            }
                            continue;
                        }
                        const uint32_t hk = g.query * 3u + (uint32_t)(a.strata ? sd : tot);
                        if (acc_n && hk != acc_key) atomicAdd(&a.counts[acc_key], acc_n);
                        if (hk != acc_key) { acc_key = hk; acc_n = 0; }
                        acc_n++;
                    }
                }
            }
        }
        if constexpr (FILL) {
            for (int e = 0; e < MIRGE_GENOME_STASH; e++) {
                bool pending = e < n_st;
                unsigned long long m = __ballot(pending);
                if (!m) break;
                const uint64_t pos = pending ? st_pos[e * 256 + threadIdx.x] : 0ull;
                const uint32_t meta = pending ? st_meta[e * 256 + threadIdx.x] : 0u;
                const uint32_t ql = (meta >> 3) - a.query_base;
                while (m) {
                    const int leader = __ffsll((long long)m) - 1;
                    const uint32_t lq = (uint32_t)__shfl((int)ql, leader, 64);
                    const bool same = pending && ql == lq;
                    const unsigned long long sm = __ballot(same);
                    uint32_t base = 0;
                    if ((int)lane == leader) base = atomicAdd(&a.cursor[lq], (uint32_t)__popcll(sm));
                    base = (uint32_t)__shfl((int)base, leader, 64);
                    if (same) {
                        const uint32_t idx = base + (uint32_t)__popcll(sm & ((1ull << lane) - 1ull));
                        const uint64_t rs = a.range[lq], len = a.range[lq + 1] - rs;
                        if (idx < len) { a.rec_pos[rs + idx] = pos; a.rec_meta[rs + idx] = meta; }
                        else atomicOr(a.overflow, 1u);
                        pending = false;
                    }
                    m = __ballot(pending);
                }
            }
            continue;
        }
        // wave-level merge of the lanes' pending counts: one atomic per distinct (query, mismatches) of the wave
        bool pending = acc_n != 0;
        unsigned long long m = __ballot(pending);
        while (m) {
            const int leader = __ffsll((long long)m) - 1;
            const uint32_t lk = (uint32_t)__shfl((int)acc_key, leader, 64);
            const bool same = pending && acc_key == lk;
            unsigned long long s = same ? acc_n : 0ull;
            for (int o = 32; o > 0; o >>= 1) {
                const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(s >> 32), o, 64);
                const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)s, o, 64);
                s += ((unsigned long long)hi << 32) | lo;
            }
            if ((int)lane == leader) atomicAdd(&a.counts[lk], s);
            if (same) pending = false;
            m = __ballot(pending);
        }
    }
}

// ---- loci: a record's stream position -> (reference, offset inside it as bowtie counts it, ambiguous stretches included)
__global__ void k_genome_loci_finish(uint32_t n, const uint64_t* __restrict__ pos, const uint32_t* __restrict__ meta,
                                     const uint64_t* __restrict__ s_start, uint32_t n_str, const uint32_t* __restrict__ str_ref,
                                     const uint64_t* __restrict__ str_off, uint32_t* __restrict__ query, uint32_t* __restrict__ ref,
                                     uint64_t* __restrict__ off, uint8_t* __restrict__ strand, uint8_t* __restrict__ mm) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t p = pos[i];
    uint32_t l = 0, h = n_str;  // largest s with s_start[s] <= p
    while (h - l > 1) {
        const uint32_t m = (l + h) >> 1;
        if (s_start[m] <= p) l = m; else h = m;
    }
    const uint32_t v = meta[i];
    query[i] = v >> 3;
    ref[i] = str_ref[l];
    off[i] = str_off[l] + (p - s_start[l]);
    strand[i] = (uint8_t)((v >> 2) & 1u);
    mm[i] = (uint8_t)(v & 3u);
}

// ---- clustering of coordinate-sorted records (novel_mir.py:98-132 as a segmented running maximum)
struct ClusterItem {  // the scan's element over the records in (reference, strand, input order)
    uint64_t seg;     // reference << 1 | strand
    int64_t maxend;   // max over the segment so far of offset + length (0-based exclusive = the reference's 1-based endPos)
    uint32_t first;   // where the segment starts
    uint32_t pad;
};

struct ClusterScanOp {
    __host__ __device__ ClusterItem operator()(const ClusterItem& a, const ClusterItem& b) const {
        if (a.seg != b.seg) return b;
        ClusterItem r = b;
        r.maxend = a.maxend > b.maxend ? a.maxend : b.maxend;
        r.first = a.first;
        return r;
    }
};

__global__ void k_cluster_keys(uint32_t n, const uint32_t* __restrict__ ref, const uint8_t* __restrict__ strand,
                               uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = ((uint64_t)ref[i] << 1) | (strand[i] & 1u);
    vals[i] = i;
}

__global__ void k_cluster_items(uint32_t n, const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ perm,
                                const uint64_t* __restrict__ off, const uint32_t* __restrict__ query, const int32_t* __restrict__ qlen,
                                ClusterItem* __restrict__ items) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t i = perm[j];
    ClusterItem it;
    it.seg = skeys[j];
    it.maxend = (int64_t)off[i] + qlen[query[i]];
    it.first = j;
    it.pad = 0;
    items[j] = it;
}

// flag[j] = 1: record j (sorted order) does not join what is before it in its segment.  It joins iff
// startPos <= E and E - startPos + 1 >= threshold with E the running maximum of endPos, i.e. offset + max(threshold, 1) <= E.
__global__ void k_cluster_flags(uint32_t n, const ClusterItem* __restrict__ scanned, const uint32_t* __restrict__ perm,
                                const uint64_t* __restrict__ off, int32_t threshold, uint32_t* __restrict__ flag) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    uint32_t f = 1;
    if (scanned[j].first != j) {
        const int64_t need = (int64_t)off[perm[j]] + (threshold > 1 ? threshold : 1);
        f = need <= scanned[j - 1].maxend ? 0u : 1u;
    }
    flag[j] = f;
}

// kept[j] = 1: record j starts a cluster that is written.  first_only (the reference's minus strand): a segment on
// the minus strand keeps its first cluster only; a record after that cluster's end is dropped.  skip[ref]: the reference's name
// holds no 'chr'.
__global__ void k_cluster_kept(uint32_t n, const ClusterItem* __restrict__ scanned, const uint32_t* __restrict__ flag,
                               const uint32_t* __restrict__ fsum, const uint8_t* __restrict__ skip, int32_t minus_first_only,
                               uint32_t* __restrict__ kept, uint8_t* __restrict__ dropped) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const ClusterItem it = scanned[j];
    const bool minus = it.seg & 1u;
    const uint32_t ordinal = fsum[j] - fsum[it.first];  // clusters opened in the segment before this record's
    const bool drop = skip[it.seg >> 1] || (minus && minus_first_only && ordinal > 0);
    dropped[j] = drop ? 1 : 0;
    kept[j] = (!drop && flag[j]) ? 1u : 0u;
}

struct ClusterTable {
    uint32_t* ref; uint8_t* strand; uint64_t* start; unsigned long long* end; unsigned long long* reads; uint32_t* members;
};

__global__ void k_cluster_assign(uint32_t n, const ClusterItem* __restrict__ scanned, const uint32_t* __restrict__ perm,
                                 const uint32_t* __restrict__ kept, const uint32_t* __restrict__ ksum, const uint8_t* __restrict__ dropped,
                                 const uint64_t* __restrict__ off, const uint32_t* __restrict__ query, const int32_t* __restrict__ qlen,
                                 const int64_t* __restrict__ qcount, int32_t* __restrict__ cluster, ClusterTable t) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t i = perm[j];
    if (dropped[j]) { cluster[i] = -1; return; }
    const uint32_t c = ksum[j] - 1;
    cluster[i] = (int32_t)c;
    const uint32_t q = query[i];
    if (kept[j]) {
        t.ref[c] = (uint32_t)(scanned[j].seg >> 1);
        t.strand[c] = (uint8_t)(scanned[j].seg & 1u);
        t.start[c] = off[i];
    }
    atomicMax(&t.end[c], (unsigned long long)(off[i] + (uint64_t)qlen[q]));
    atomicAdd(&t.reads[c], (unsigned long long)qcount[q]);
    atomicAdd(&t.members[c], 1u);
}

// ---- windows of the resident genome as text (mirge_genome_fetch): one wave per window, a lane per output byte.  Output byte i
// of a window is reference position start + i ('+') or start + len - 1 - i, complemented ('-'); a position inside no stretch (an
// ambiguous character, or past what the genome holds of the reference) is 'N'.  The stretch of a position: the last one whose
// (reference, first position) is not past it -- the stretches lie in that order.
struct GenomeWindow {
    uint64_t start;    // 0-based in the reference
    uint64_t out_off;  // where the window's bytes start in the output
    uint32_t ref, len;
    uint8_t minus, rna, pad[6];
};

__global__ void __launch_bounds__(64)
k_genome_fetch(uint32_t n_win, const GenomeWindow* __restrict__ win, const uint64_t* __restrict__ text, const uint64_t* __restrict__ s_start,
               uint32_t n_str, const uint32_t* __restrict__ str_ref, const uint64_t* __restrict__ str_off, char* __restrict__ out) {
    if (blockIdx.x >= n_win) return;
    const GenomeWindow w = win[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < w.len; i += 64) {
        const uint64_t p = w.start + (w.minus ? (uint64_t)(w.len - 1 - i) : (uint64_t)i);
        char ch = 'N';
        if (n_str) {
            uint32_t l = 0, h = n_str;  // the largest s with (str_ref[s], str_off[s]) <= (ref, p), if stretch 0 is
            while (h - l > 1) {
                const uint32_t m = (l + h) >> 1;
                if (str_ref[m] < w.ref || (str_ref[m] == w.ref && str_off[m] <= p)) l = m; else h = m;
            }
            if (str_ref[l] == w.ref && str_off[l] <= p && p - str_off[l] < s_start[l + 1] - s_start[l]) {
                const uint64_t q = s_start[l] + (p - str_off[l]);
                uint32_t c = (uint32_t)(text[q >> 5] >> (2 * (q & 31))) & 3u;
                if (w.minus) c = 3u - c;
                ch = c == 0 ? 'A' : c == 1 ? 'C' : c == 2 ? 'G' : (w.rna ? 'U' : 'T');
            }
        }
        out[w.out_off + i] = ch;
    }
}
