// kernels_bam.hpp -- part of mirge_kernels.hpp: `<sample>_sorted.bam` of `--sorted-bam` (what the reference's createBAM gets from
// `samtools view -bS | sort | index`, bamFmt.py:173-205): the records of `<sample>.sam` (kernels_sam.hpp: same rows, same lift) as BAM v1,
// coordinate-sorted and BGZF-compressed where the reads, the counts and the cascade's result already lie.
//   k_bam_measure : per ROW (a unique read kept by k_sam_select) the sort key (refID, pos, reverse), the bytes of a record without the
//                   digits of its copy number k, the bytes of all its c copies (sam_digit_total)       -> radix sort, one 64-bit scan
//   k_bam_gather  : the per-row arrays in sorted order
//   k_bam_blocks  : OUTPUT-stationary, like k_sam_write.  A workgroup owns one BGZF block's stretch of the uncompressed stream (BAM
//                   header and reference list in front, then the records); every 32 bytes are a probe point whose thread finds the
//                   (row, k) of the record that holds it and writes that record, clipped to the block, into LDS.  The block is then
//                   deflated where it lies:
//                     - hash of every 4 bytes -> FIRST position of the block (of its 32 KiB half: a distance fits 15 bits) with that
//                       hash (LDS atomicMin): the candidate of every later position; copies of a row lie one record apart, so the
//                       first copy in the block serves all the others.  A second candidate is the byte in front (runs: QUAL).
//                     - every thread owns one segment of the block (a 256th), walks it greedily (a match ends with the segment)
//                       and counts its bits; one exclusive sum gives every segment its bit offset; the same walk then emits
//                       fixed-Huffman codes (BTYPE 01) into LDS words.  A block that does not shrink is stored (BTYPE 00).
//                     - CRC-32: every thread's table CRC of its segment, times x^(8 * bytes behind the segment) mod P, XOR-ed.
//                   and written as one BGZF member into the block's slot; k_bam_compact closes the gaps between the slots.
//                   deflate = 0: the uncompressed block goes out instead (MIRGE_BAM_DEFLATE=host: zlib on the host).
//                   deflate = 2 (MIRGE_BAM_DEFLATE=dynamic; on the device the kernel k_bam_blocks_dynamic): the same parse, and a
//                   third form to choose from: a Huffman code of the
//                   block's own (BTYPE 10).  The counting walk also adds its symbols to LDS histograms (one pair per wave) and leaves
//                   every match at its own bytes of the still empty output words; bam_huff_lengths makes the code lengths (at most
//                   15 bits; 7 for the code of the lengths themselves), a walk over the staged matches -- no match search -- gives
//                   every segment its bits under that code, and the form goes out when its bytes are fewer than those of the better
//                   of the other two: no member is larger than under deflate = 1.  k_bam_huff_probe: bam_huff_lengths alone.
//                   deflate = 3 (MIRGE_BAM_DEFLATE=tight; on the device the kernel k_bam_blocks_tight): the blocks, the CRC, the code
//                   builder, the header and the choice of the form of deflate = 2, on the tokens of another parse:
//                     - a match may run on behind its thread's segment, to the block's end or 258 bytes.  e_t = where thread t's
//                       last token ends; E_t = the maximum of e_j over j < t (one prefix maximum): thread t drops its tokens that
//                       end at or in front of E_t, trims the one across E_t to its suffix (same distance; a suffix shorter than
//                       the minimum match becomes literals) and emits [E_t, E_t+1).  The first search leaves a match that ends
//                       inside its segment at its own bytes of the output words, as deflate = 2 does, and keeps the last one, which
//                       may start in the segment's last bytes, in registers: nothing is staged in another thread's bytes.  Counts,
//                       histograms and bit offsets are taken from the trimmed tokens, behind the prefix maximum; the output words
//                       hold the staged matches until then, so the emitting walk searches a second time (same tokens: the search
//                       is a function of the block's bytes).
//                     - candidates: the byte in front; the distance of the thread's last match; the same offset in the previous
//                       record and the same distance from the record's end (distances: the previous and this record's length --
//                       the thread finds the record at its segment's start as a probe point does and walks on by the block_size
//                       words); per 4 KiB region of the block the FIRST position with the hash, 16 x 512 entries of 16 bits in
//                       head's 16 KB: the entry of the position's own region and of the MIRGE_BAM_TIGHT_LOOKBACK regions in front.
//                       The longest wins, of equally long ones the nearest.
//                     - one step of lazy matching: a match shorter than MIRGE_BAM_TIGHT_LAZY_BELOW gives way to a literal when the
//                       match one byte on is longer by more than one, or as long and nearer; a longer match from a region table
//                       gives way when one of the table-free candidates one byte on is as long and nearer.
//                   No promise per member against the other routes: another greedy parse can lose on a single block.
// No wave intrinsics: the same source runs on the host (tests/hostsim/bam_sim.cpp).
#pragma once

#define MIRGE_BAM_MAX_BLOCK 65280  // uncompressed bytes of a BGZF block (bgzf.h's BGZF_BLOCK_SIZE 0xff00)
#define MIRGE_BAM_PROBE 32         // bytes between two probe points; every record is longer (36 fixed bytes + name + cigar + ...)
#define MIRGE_BAM_HASH_BITS 11     // per 32 KiB half of the block
#define MIRGE_BAM_MIN_MATCH 4
#define MIRGE_BAM_MAX_MATCH 258
#define MIRGE_BAM_MAXP 16
#define MIRGE_BAM_MAX_POS (1ll << 29)  // the binning index ends here (SAM specification 5.1.1)

struct BamTables {
    const int32_t* refid[MIRGE_BAM_MAXP];  // per pass: chromosome index -> refID (the @SQ order), -1: no @SQ names it
    const uint8_t* header;                 // magic, l_text, text, n_ref, the references: the front of the uncompressed stream
    unsigned long long header_len;
};

__host__ __device__ __forceinline__ uint32_t bam_reg2bin(long long beg, long long end) {  // SAM specification 5.3
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0u;
}
__host__ __device__ __forceinline__ int bam_digits(unsigned long long v) { int nd = 1; for (; v >= 10ull; v /= 10ull) nd++; return nd; }

template <bool WRITE> __device__ __forceinline__ void bam_le16(SamOut<WRITE>& w, uint32_t v) { w.ch((char)(v & 255u)); w.ch((char)((v >> 8) & 255u)); }
template <bool WRITE> __device__ __forceinline__ void bam_le32(SamOut<WRITE>& w, uint32_t v) { bam_le16(w, v & 0xFFFFu); bam_le16(w, v >> 16); }
__device__ __forceinline__ uint32_t bam_base_code(char c) { return c == 'A' ? 1u : c == 'C' ? 2u : c == 'G' ? 4u : c == 'T' ? 8u : 15u; }

// what a row's records share: set by bam_row, read by bam_record
struct BamRow {
    uint32_t j; int gi, p; int32_t r, o; int L, Ls; bool minus; int32_t ci, refid; long long pos; unsigned long long c;
};
__device__ __forceinline__ void bam_row(const SamTables& t, const BamTables& bt, uint32_t read, BamRow& b) {
    b.gi = sam_locate(t, read, b.j);
    const CsvGroup& g = t.g[b.gi];
    b.p = g.pass[b.j];
    const SamPass& sp = t.pass[b.p];
    b.r = g.ref[b.j]; b.o = t.off[b.gi][b.j];
    b.L = csv_len(g, b.j); b.Ls = b.L - sp.trim5 - sp.trim3;
    b.minus = sp.minus[b.r] != 0;
    b.ci = sp.chrom_of_ref[b.r];
    b.refid = bt.refid[b.p][b.ci];
    b.pos = sam_lift_start(sp, b.r, b.o, b.Ls, b.minus) - 1;
    b.c = g.counts[(size_t)b.j * t.S + t.sample];
}

// copy k of a row's records; F = the row's bytes of a record without the digits of k (what block_size is computed from)
template <bool WRITE>
__device__ __forceinline__ void bam_record(const SamTables& t, const BamRow& b, uint32_t F, uint32_t k, SamOut<WRITE>& w) {
    const CsvGroup& g = t.g[b.gi];
    const SamPass& sp = t.pass[b.p];
    const int nd = bam_digits(k), Ls = b.Ls;
    SamRead rd(g, b.j);
    bam_le32(w, F - 4u + (uint32_t)nd);                      // block_size: the record behind this word
    bam_le32(w, (uint32_t)b.refid);
    bam_le32(w, (uint32_t)b.pos);
    w.ch((char)(b.L + 1 + nd + 1));                          // l_read_name with the NUL
    w.ch((char)255);                                         // mapq
    bam_le16(w, bam_reg2bin(b.pos, b.pos + Ls));
    bam_le16(w, 1u);                                         // n_cigar_op
    bam_le16(w, b.minus ? 16u : 0u);
    bam_le32(w, (uint32_t)Ls);
    bam_le32(w, 0xFFFFFFFFu); bam_le32(w, 0xFFFFFFFFu); bam_le32(w, 0u);  // next_refID, next_pos, tlen
    for (int p = 0; p < b.L; p++) w.ch(rd.at(p));            // QNAME: the whole read, untrimmed
    w.ch('_'); w.u64(k); w.ch('\0');
    bam_le32(w, (uint32_t)Ls << 4);                          // <Ls>M
    for (int q = 0; q < Ls; q += 2) {                        // SEQ as the SAM line has it: reverse-complemented on the minus strand
        const char hi = b.minus ? sam_complement(rd.at(sp.trim5 + Ls - 1 - q)) : rd.at(sp.trim5 + q);
        const char lo = q + 1 < Ls ? (b.minus ? sam_complement(rd.at(sp.trim5 + Ls - 2 - q)) : rd.at(sp.trim5 + q + 1)) : '\0';
        w.ch((char)((bam_base_code(hi) << 4) | (lo ? bam_base_code(lo) : 0u)));
    }
    for (int p = 0; p < Ls; p++) w.ch((char)40);             // QUAL 'I'
    const uint32_t mmv = (uint32_t)(t.mm[b.gi][b.j] < 0 ? 0 : t.mm[b.gi][b.j]);
    w.ch('X'); w.ch('A'); w.ch('C'); w.ch((char)mmv);
    w.ch('M'); w.ch('D'); w.ch('Z');
    const unsigned long long g0 = (unsigned long long)sp.ref_start[b.r] + (unsigned long long)b.o;
    unsigned long long run = 0;
    for (int p = 0; p < Ls; p++) {
        const char a = rd.at(sp.trim5 + p), c = sam_text_at(sp, g0 + (unsigned long long)p);
        if (a == c) run++;
        else { w.u64(run); w.ch(c); run = 0; }
    }
    w.u64(run); w.ch('\0');
    w.ch('N'); w.ch('M'); w.ch('C'); w.ch((char)mmv);
}

// flags[0] |= 2: a row's chromosome has no refID (flags[1] = pass, flags[2] = chromosome index of one such row); |= 4: a position
// outside [0, 2^29); |= 8: a QNAME longer than 254 characters (flags[3] = the longest such read)
__global__ void k_bam_measure(SamTables t, BamTables bt, const uint32_t* __restrict__ rows, uint32_t n_rows, unsigned long long* __restrict__ key,
                              uint32_t* __restrict__ fixed, unsigned long long* __restrict__ total, unsigned long long* __restrict__ n_records,
                              uint32_t* __restrict__ flags) {
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n_rows; x += gridDim.x * blockDim.x) {
        BamRow b;
        bam_row(t, bt, rows[x], b);
        key[x] = 0ull; fixed[x] = 0u; total[x] = 0ull;
        if (b.refid < 0) {
            atomicOr(&flags[0], 2u);
            if (atomicCAS(&flags[4], 0u, 1u) == 0u) { flags[1] = (uint32_t)b.p; flags[2] = (uint32_t)b.ci; }
            continue;
        }
        if (b.pos < 0 || b.pos + b.Ls > MIRGE_BAM_MAX_POS) { atomicOr(&flags[0], 4u); continue; }
        if (b.L + 1 + bam_digits(b.c - 1ull) > 254) { atomicOr(&flags[0], 8u); atomicMax(&flags[3], (uint32_t)b.L); continue; }
        SamOut<false> w{nullptr, 0, 0, 0u};
        bam_record<false>(t, b, 0u, 0u, w);
        const uint32_t F = w.n - 1u;  // (copy 0 printed one digit)
        key[x] = ((unsigned long long)(uint32_t)b.refid << 32) | ((unsigned long long)b.pos << 1) | (b.minus ? 1ull : 0ull);
        fixed[x] = F;
        total[x] = b.c * (unsigned long long)F + sam_digit_total(b.c);
        atomicAdd(n_records, b.c);
    }
}

__global__ void k_bam_gather(const uint32_t* __restrict__ perm, uint32_t n_rows, const uint32_t* __restrict__ rows, const uint32_t* __restrict__ fixed,
                             const unsigned long long* __restrict__ total, uint32_t* __restrict__ s_rows, uint32_t* __restrict__ s_fixed,
                             unsigned long long* __restrict__ s_total) {
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n_rows; x += gridDim.x * blockDim.x) {
        const uint32_t y = perm[x];
        s_rows[x] = rows[y]; s_fixed[x] = fixed[y]; s_total[x] = total[y];
    }
}

// per sorted row what the index needs: begin, end, count (the key holds refID and begin)
__global__ void k_bam_row_table(SamTables t, BamTables bt, const uint32_t* __restrict__ s_rows, uint32_t n_rows, uint32_t* __restrict__ span,
                                unsigned long long* __restrict__ count) {
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n_rows; x += gridDim.x * blockDim.x) {
        BamRow b;
        bam_row(t, bt, s_rows[x], b);
        span[x] = (uint32_t)b.Ls; count[x] = b.c;
    }
}

// ---- deflate (RFC 1951) with the fixed code
__device__ __forceinline__ int bam_log2(uint32_t x) { int lg = 0; while (x >> (lg + 1)) lg++; return lg; }
__device__ __forceinline__ uint32_t bam_bitrev(uint32_t code, int n) { uint32_t r = 0; for (int b = 0; b < n; b++) r |= ((code >> b) & 1u) << (n - 1 - b); return r; }
__device__ __forceinline__ uint32_t bam_crc_mul(uint32_t a, uint32_t b) {  // a * b mod P, reflected (zlib's multmodp)
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) { p ^= b; if ((a & (m - 1u)) == 0u) break; }
        m >>= 1;
        b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}
__device__ __forceinline__ uint32_t bam_crc_x8n(uint32_t n) {  // x^(8n) mod P
    uint32_t p = 1u << 31, base = 1u << 23;
    for (; n; n >>= 1) { if (n & 1u) p = bam_crc_mul(base, p); base = bam_crc_mul(base, base); }
    return p;
}

// bits of a segment, counted (WRITE = false) or OR-ed into the block's words from bit `at` on
template <bool WRITE>
struct BamBits {
    uint32_t* out;
    uint32_t at;               // next bit
    unsigned long long acc;    // bits not yet flushed, from bit (at & ~31) - ... of word `word` on
    uint32_t word; int fill;
    __device__ __forceinline__ void start(uint32_t* o, uint32_t bit) { out = o; at = bit; word = bit >> 5; fill = (int)(bit & 31u); acc = 0ull; }
    __device__ __forceinline__ void put(uint32_t v, int n) {
        if (WRITE) {
            acc |= (unsigned long long)v << fill;
            fill += n;
            if (fill >= 32) { atomicOr(&out[word], (uint32_t)acc); word++; acc >>= 32; fill -= 32; }
        }
        at += (uint32_t)n;
    }
    __device__ __forceinline__ void finish() { if (WRITE && fill > 0) atomicOr(&out[word], (uint32_t)acc); }
};
template <bool WRITE> __device__ __forceinline__ void bam_put_literal(BamBits<WRITE>& w, uint32_t b) {
    if (b < 144u) w.put(bam_bitrev(0x30u + b, 8), 8); else w.put(bam_bitrev(0x190u + (b - 144u), 9), 9);
}
// a match's length code 257 + idx and distance code dc with their extra bits (RFC 1951, 3.2.5)
struct BamMatchCode { uint32_t idx, xb, xv, dc, db, dv; };
__device__ __forceinline__ BamMatchCode bam_match_code(uint32_t len, uint32_t dist) {
    BamMatchCode m{0u, 0u, 0u, 0u, 0u, 0u};
    if (len <= 10u) m.idx = len - 3u;
    else if (len == 258u) m.idx = 28u;
    else { const uint32_t l = len - 3u; const int e = bam_log2(l) - 2; m.idx = 4u * (uint32_t)(e + 1) + ((l >> e) & 3u); m.xb = (uint32_t)e; m.xv = l & ((1u << e) - 1u); }
    if (dist <= 4u) m.dc = dist - 1u;
    else { const uint32_t d = dist - 1u; const int e = bam_log2(d) - 1; m.dc = 2u * (uint32_t)(e + 1) + ((d >> e) & 1u); m.db = (uint32_t)e; m.dv = d & ((1u << e) - 1u); }
    return m;
}
template <bool WRITE> __device__ __forceinline__ void bam_put_match(BamBits<WRITE>& w, uint32_t len, uint32_t dist) {
    const BamMatchCode m = bam_match_code(len, dist);
    const uint32_t sym = 257u + m.idx;
    if (sym <= 279u) w.put(bam_bitrev(sym - 256u, 7), 7); else w.put(bam_bitrev(0xC0u + (sym - 280u), 8), 8);
    if (m.xb) w.put(m.xv, (int)m.xb);
    w.put(bam_bitrev(m.dc, 5), 5);
    if (m.db) w.put(m.dv, (int)m.db);
}
__device__ __forceinline__ uint32_t bam_ld32(const uint8_t* d, uint32_t i) {
    return (uint32_t)d[i] | ((uint32_t)d[i + 1] << 8) | ((uint32_t)d[i + 2] << 16) | ((uint32_t)d[i + 3] << 24);
}
__device__ __forceinline__ uint32_t bam_hash(uint32_t v, uint32_t i) {
    return ((i >> 15) << MIRGE_BAM_HASH_BITS) | ((v * 2654435761u) >> (32 - MIRGE_BAM_HASH_BITS));
}
// the greedy parse of segment [s0, s1) of the block's n bytes into a sink W: bam_put_literal(w, byte), bam_put_match(w, length, distance)
template <class W>
__device__ __forceinline__ void bam_parse(const uint8_t* d, const uint32_t* head, uint32_t s0, uint32_t s1, W& w) {
    uint32_t i = s0;
    while (i < s1) {
        uint32_t best = 0, dist = 0;
        if (i + MIRGE_BAM_MIN_MATCH <= s1) {
            const uint32_t lim = s1 - i < MIRGE_BAM_MAX_MATCH ? s1 - i : MIRGE_BAM_MAX_MATCH;
            if (i > 0) {
                const uint8_t b = d[i - 1];
                uint32_t k = 0;
                while (k < lim && d[i + k] == b) k++;
                if (k >= MIRGE_BAM_MIN_MATCH) { best = k; dist = 1; }
            }
            const uint32_t cand = head[bam_hash(bam_ld32(d, i), i)];
            if (cand < i && best < lim) {
                uint32_t k = 0;
                while (k < lim && d[cand + k] == d[i + k]) k++;
                if (k >= MIRGE_BAM_MIN_MATCH && k > best) { best = k; dist = i - cand; }
            }
        }
        if (best) { bam_put_match(w, best, dist); i += best; }
        else { bam_put_literal(w, d[i]); i++; }
    }
}

// ---- deflate with a code of the block's own (RFC 1951, 3.2.7)
#define MIRGE_BAM_NLL 286          // literal/length symbols
#define MIRGE_BAM_ND 30            // distance symbols
#define MIRGE_BAM_NCL 19           // symbols of the code that the header spells the other two codes' lengths in
#define MIRGE_BAM_HUFF_MAX 288     // symbols bam_huff_lengths takes
#define MIRGE_BAM_HIST_COPIES 4    // one pair of histograms per wave of 64 threads: a hot literal's atomics stay inside its wave's copy

struct BamHuffWork { uint32_t a[MIRGE_BAM_HUFF_MAX]; uint32_t bl[16]; uint16_t order[MIRGE_BAM_HUFF_MAX]; };  // bam_huff_lengths' LDS

// Lengths len[0 .. n) of a prefix code for the counts cnt[0 .. n), n <= MIRGE_BAM_HUFF_MAX <= 2^max_bits, max_bits <= 15: 0 where the
// count is 0, none above max_bits, and sum count * length the Huffman optimum whenever an optimal tree fits max_bits.  Two or more used
// symbols give a complete code (Kraft sum 1); ONE used symbol gets length 1, which inflate takes for the distance code alone.
// cnt, len and w lie in LDS; all the workgroup's threads call, behind a barrier that made cnt visible, and leave through a barrier.
//   - bam_huff_rank, all threads: the used symbols sorted by (count, symbol), a rank each;
//   - bam_huff_tree, ONE thread behind a barrier: Moffat and Katajainen's in-place pass over the sorted counts (a tie takes the
//     leaf, not the inner node: of the optimal trees the one of least depth); where that is still deeper than max_bits, the deeper leaves come up to max_bits and, as long as
//     the Kraft sum is above 1, a leaf of the greatest length below max_bits moves one level down with a leaf of max_bits as its
//     sibling (each step takes 2^-max_bits off the sum); the lengths go out longest first to the rarest symbols.
// k_bam_blocks calls the two steps itself: two codes at a time, their trees on two threads of different waves.
// OWN: k_bam_blocks_tight's copies of what takes pointers into the block's BamDynamic.  While k_bam_blocks_dynamic is the only caller the
// compiler folds its one LDS block's addresses into these functions before it inlines them; a second caller's other block ends that, and
// the dynamic kernel then compiles to other code (same registers and LDS, another schedule).  With copies of its own it stays what it was.
// OWN is a number: 1 is the tight route's set of copies, 2 that of k_bgzf_text (kernels_bgzf.hpp).
template <int OWN = 0>
__device__ __forceinline__ void bam_huff_rank(const uint32_t* cnt, uint32_t n, uint8_t* len, BamHuffWork& w, uint32_t tid, uint32_t nth) {
    for (uint32_t s = tid; s < n; s += nth) {
        const uint32_t c = cnt[s];
        len[s] = 0;
        if (!c) continue;
        uint32_t rank = 0;
        for (uint32_t x = 0; x < n; x++) { const uint32_t cx = cnt[x]; rank += (cx != 0u && (cx < c || (cx == c && x < s))) ? 1u : 0u; }
        w.order[rank] = (uint16_t)s; w.a[rank] = c;
    }
}
template <int OWN = 0>
__device__ __forceinline__ void bam_huff_tree(const uint32_t* cnt, uint32_t n, uint32_t max_bits, uint8_t* len, BamHuffWork& w) {
    uint32_t* A = w.a;
    uint32_t m = 0;
    for (uint32_t x = 0; x < n; x++) m += cnt[x] != 0u ? 1u : 0u;
    if (m == 1u) len[w.order[0]] = 1;
    if (m >= 2u) {
        A[0] += A[1];
        uint32_t root = 0, leaf = 2;
        for (uint32_t next = 1; next + 1 < m; next++) {  // A[root .. next): weights of inner nodes; A[.. root): their parents
            if (leaf >= m || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = next; } else A[next] = A[leaf++];
            if (leaf >= m || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = next; } else A[next] += A[leaf++];
        }
        A[m - 2] = 0;
        for (int next = (int)m - 3; next >= 0; next--) A[next] = A[A[next]] + 1u;  // depths of the inner nodes
        int avbl = 1, used = 0, rt = (int)m - 2, nx = (int)m - 1;
        for (uint32_t depth = 0; avbl > 0; depth++) {  // depths of the leaves: A[0] the rarest symbol's, the greatest
            while (rt >= 0 && A[rt] == depth) { used++; rt--; }
            while (avbl > used) { A[nx--] = depth; avbl--; }
            avbl = 2 * used; used = 0;
        }
        for (uint32_t b = 0; b < 16u; b++) w.bl[b] = 0u;
        for (uint32_t x = 0; x < m; x++) w.bl[A[x] < max_bits ? A[x] : max_bits]++;
        if (A[0] > max_bits) {
            uint32_t total = 0;
            for (uint32_t b = 1; b <= max_bits; b++) total += w.bl[b] << (max_bits - b);
            for (; total > (1u << max_bits); total--) {
                w.bl[max_bits]--;
                for (uint32_t b = max_bits - 1u; b >= 1u; b--)
                    if (w.bl[b]) { w.bl[b]--; w.bl[b + 1u] += 2u; break; }
            }
        }
        uint32_t x = 0;
        for (uint32_t b = max_bits; b >= 1u; b--)
            for (uint32_t k = w.bl[b]; k; k--) len[w.order[x++]] = (uint8_t)b;
    }
}
__device__ __forceinline__ void bam_huff_lengths(const uint32_t* cnt, uint32_t n, uint32_t max_bits, uint8_t* len, BamHuffWork& w, uint32_t tid, uint32_t nth) {
    bam_huff_rank(cnt, n, len, w, tid, nth);
    __syncthreads();
    if (tid == 0) bam_huff_tree(cnt, n, max_bits, len, w);
    __syncthreads();
}
// two codes at once: the second one's tree is thread nth / 2's
template <int OWN = 0>
__device__ __forceinline__ void bam_huff_lengths2(const uint32_t* cnt0, uint32_t n0, uint8_t* len0, BamHuffWork& w0, const uint32_t* cnt1, uint32_t n1, uint8_t* len1,
                                                  BamHuffWork& w1, uint32_t max_bits, uint32_t tid, uint32_t nth) {
    bam_huff_rank<OWN>(cnt0, n0, len0, w0, tid, nth);
    bam_huff_rank<OWN>(cnt1, n1, len1, w1, tid, nth);
    __syncthreads();
    if (tid == 0) bam_huff_tree<OWN>(cnt0, n0, max_bits, len0, w0);
    if (tid == nth / 2u) bam_huff_tree<OWN>(cnt1, n1, max_bits, len1, w1);
    __syncthreads();
}
// the canonical code of lengths len[0 .. n) (RFC 1951, 3.2.2), bit-reversed for the LSB-first stream: code[s] = bits | length << 16.
// A symbol's code is the number of codes in front of it: 2^(L - l) per shorter code of length l, one per earlier symbol of its own length.
__device__ __forceinline__ void bam_huff_codes(const uint8_t* len, uint32_t n, uint32_t* code, uint32_t tid, uint32_t nth) {
    for (uint32_t s = tid; s < n; s += nth) {
        const uint32_t L = len[s];
        uint32_t c = 0;
        for (uint32_t x = 0; x < n && L; x++) {
            const uint32_t lx = len[x];
            if (lx && lx < L) c += 1u << (L - lx);
            else if (lx == L && x < s) c++;
        }
        code[s] = bam_bitrev(c, (int)L) | (L << 16);
    }
}
__device__ __forceinline__ uint32_t bam_cl_order(uint32_t k) {  // 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15: five bits each
    return (uint32_t)((k < 12u ? 0x22caa324e804a30ull >> (5u * k) : 0x3c2e1346cull >> (5u * (k - 12u))) & 31ull);
}

// the block's state of deflate == 2
struct BamDynamic {
    uint32_t hist_ll[MIRGE_BAM_HIST_COPIES][MIRGE_BAM_HUFF_MAX], hist_d[MIRGE_BAM_HIST_COPIES][32];  // [0]: the sums, the counts of the block
    uint32_t code_ll[MIRGE_BAM_HUFF_MAX], code_d[32], code_cl[32];
    uint32_t cnt_cl[2][32];            // [0]: of the header with run symbols (16, 17, 18), [1]: of the plain one
    uint32_t seg[MIRGE_BLOCK + 1];     // the segments' bits, then bit offsets, under the block's own code
    uint32_t hlit, hdist, hclen, n_tok, plain, header_bits;
    BamHuffWork work[2];
    uint16_t tok[MIRGE_BAM_NLL + MIRGE_BAM_ND + 4];  // the header with run symbols: symbol | extra bits' value << 8
    uint8_t len_ll[MIRGE_BAM_HUFF_MAX], len_d[32], len_cl[2][32];
};
// length k of the HLIT + HDIST lengths the header spells, as one sequence
template <int OWN = 0>
__device__ __forceinline__ uint32_t bam_dyn_seq(const BamDynamic& y, uint32_t k) { return k < y.hlit ? y.len_ll[k] : y.len_d[k - y.hlit]; }

// the counting walk of deflate == 2: the segment's bits under the fixed code, as BamBits<false> counts them; its symbols into the wave's
// histograms; every match at the first three of its own bytes of tok (the output words, all zero: a zero byte is a literal), bit 7 of the
// first one set, then length - 3 (8 bits) and distance - 1 (15 bits).  A match has MIRGE_BAM_MIN_MATCH >= 4 bytes and ends with its segment.
struct BamCount { uint32_t at, pos; uint32_t* ll; uint32_t* dd; uint8_t* tok; };
__device__ __forceinline__ void bam_put_literal(BamCount& w, uint32_t b) {
    w.at += b < 144u ? 8u : 9u;
    atomicAdd(&w.ll[b], 1u);
    w.pos++;
}
__device__ __forceinline__ void bam_put_match(BamCount& w, uint32_t len, uint32_t dist) {
    const BamMatchCode m = bam_match_code(len, dist);
    w.at += (m.idx <= 22u ? 7u : 8u) + m.xb + 5u + m.db;
    atomicAdd(&w.ll[257u + m.idx], 1u);
    atomicAdd(&w.dd[m.dc], 1u);
    const uint32_t v = (len - 3u) | ((dist - 1u) << 8);
    w.tok[w.pos] = (uint8_t)(0x80u | (v & 0x7Fu)); w.tok[w.pos + 1u] = (uint8_t)(v >> 7); w.tok[w.pos + 2u] = (uint8_t)(v >> 15);
    w.pos += len;
}
// the bits of segment [s0, s1) under the block's own code, from the staged matches
__device__ __forceinline__ uint32_t bam_dyn_bits(const BamDynamic& y, const uint8_t* d, const uint8_t* tok, uint32_t s0, uint32_t s1) {
    uint32_t bits = 0;
    for (uint32_t i = s0; i < s1;) {
        const uint32_t t0 = tok[i];
        if (!(t0 & 0x80u)) { bits += y.len_ll[d[i]]; i++; continue; }
        const uint32_t v = (t0 & 0x7Fu) | ((uint32_t)tok[i + 1u] << 7) | ((uint32_t)tok[i + 2u] << 15), len = (v & 255u) + 3u;
        const BamMatchCode m = bam_match_code(len, (v >> 8) + 1u);
        bits += y.len_ll[257u + m.idx] + m.xb + y.len_d[m.dc] + m.db;
        i += len;
    }
    return bits;
}
// the emitting walk with the block's own code
struct BamDynBits { BamBits<true> b; const uint32_t* ll; const uint32_t* dd; };
__device__ __forceinline__ void bam_put_code(BamBits<true>& b, uint32_t c) { b.put(c & 0xFFFFu, (int)(c >> 16)); }
__device__ __forceinline__ void bam_put_literal(BamDynBits& w, uint32_t b) { bam_put_code(w.b, w.ll[b]); }
__device__ __forceinline__ void bam_put_match(BamDynBits& w, uint32_t len, uint32_t dist) {
    const BamMatchCode m = bam_match_code(len, dist);
    bam_put_code(w.b, w.ll[257u + m.idx]);
    if (m.xb) w.b.put(m.xv, (int)m.xb);
    bam_put_code(w.b, w.dd[m.dc]);
    if (m.db) w.b.put(m.dv, (int)m.db);
}

// thread 0, the lengths of both codes known: HLIT, HDIST, and the sequence of their lengths in the symbols 0 .. 18 twice -- with the
// run symbols (16: the length in front 3 to 6 times more, 17: 3 to 10 zeros, 18: 11 to 138 zeros; greedy, a run may cross from one code
// into the other) into tok, and plain, a symbol per length -- and either form's counts
template <int OWN = 0>
__device__ __forceinline__ void bam_dyn_header_tokens(BamDynamic& y) {
    uint32_t hlit = MIRGE_BAM_NLL, hdist = MIRGE_BAM_ND, any = 0;
    for (uint32_t x = 0; x < MIRGE_BAM_ND; x++) any |= y.len_d[x];
    if (!any) y.len_d[0] = 1;  // a block without a match: inflate wants one distance code, of length 1 (no walk reads it: no match)
    while (hlit > 257u && !y.len_ll[hlit - 1u]) hlit--;
    while (hdist > 1u && !y.len_d[hdist - 1u]) hdist--;
    y.hlit = hlit; y.hdist = hdist;
    for (uint32_t x = 0; x < 32u; x++) { y.cnt_cl[0][x] = 0u; y.cnt_cl[1][x] = 0u; }
    const uint32_t N = hlit + hdist;
    uint32_t nt = 0;
    for (uint32_t k = 0; k < N;) {
        const uint32_t v = bam_dyn_seq<OWN>(y, k);
        uint32_t run = 1;
        while (k + run < N && bam_dyn_seq<OWN>(y, k + run) == v) run++;
        k += run;
        y.cnt_cl[1][v] += run;
        if (v) { y.tok[nt++] = (uint16_t)v; y.cnt_cl[0][v]++; run--; }
        while (run >= (v ? 3u : 11u)) {
            const uint32_t r = run < (v ? 6u : 138u) ? run : (v ? 6u : 138u), sym = v ? 16u : 18u;
            y.tok[nt++] = (uint16_t)(sym | ((r - (v ? 3u : 11u)) << 8)); y.cnt_cl[0][sym]++; run -= r;
        }
        if (!v && run >= 3u) { y.tok[nt++] = (uint16_t)(17u | ((run - 3u) << 8)); y.cnt_cl[0][17]++; run = 0; }
        for (; run; run--) { y.tok[nt++] = (uint16_t)v; y.cnt_cl[0][v]++; }
    }
    y.n_tok = nt;
}
// thread 0, the lengths of the code of either form known: the shorter header (a tie: the one with run symbols), HCLEN, its bits with BFINAL and BTYPE
template <int OWN = 0>
__device__ __forceinline__ void bam_dyn_header_choice(BamDynamic& y) {
    uint32_t bits[2], hclen[2];
    for (uint32_t f = 0; f < 2u; f++) {
        uint32_t h = MIRGE_BAM_NCL, sum = 0;
        while (h > 4u && !y.len_cl[f][bam_cl_order(h - 1u)]) h--;
        for (uint32_t x = 0; x < MIRGE_BAM_NCL; x++) sum += y.cnt_cl[f][x] * ((uint32_t)y.len_cl[f][x] + (x == 16u ? 2u : x == 17u ? 3u : x == 18u ? 7u : 0u));
        bits[f] = 3u + 5u + 5u + 4u + 3u * h + sum; hclen[f] = h;
    }
    y.plain = bits[1] < bits[0] ? 1u : 0u;
    y.header_bits = y.plain ? bits[1] : bits[0];
    y.hclen = y.plain ? hclen[1] : hclen[0];
}
// thread 0: the header into the output words
template <int OWN = 0>
__device__ __forceinline__ void bam_dyn_put_header(const BamDynamic& y, BamBits<true>& b) {
    b.put(5u, 3);  // BFINAL = 1, BTYPE = 10
    b.put(y.hlit - 257u, 5); b.put(y.hdist - 1u, 5); b.put(y.hclen - 4u, 4);
    const uint8_t* cl = y.len_cl[y.plain];
    for (uint32_t k = 0; k < y.hclen; k++) b.put(cl[bam_cl_order(k)], 3);
    if (y.plain)
        for (uint32_t k = 0; k < y.hlit + y.hdist; k++) bam_put_code(b, y.code_cl[bam_dyn_seq<OWN>(y, k)]);
    else
        for (uint32_t k = 0; k < y.n_tok; k++) {
            const uint32_t sym = y.tok[k] & 255u;
            bam_put_code(b, y.code_cl[sym]);
            if (sym >= 16u) b.put((uint32_t)y.tok[k] >> 8, sym == 16u ? 2 : sym == 17u ? 3 : 7);
        }
}

// ---- the parse of deflate == 3.  Build knobs (-D): MIRGE_BAM_TIGHT_LAZY (0: no lazy step), MIRGE_BAM_TIGHT_LAZY_BELOW (a match of
// this length or longer is taken at once), MIRGE_BAM_TIGHT_LOOKBACK (regions in front of the position's own whose entry is tried),
// and, for tools/bam_parse_sizes.py's table of what each ingredient buys, MIRGE_BAM_TIGHT_RECORD, MIRGE_BAM_TIGHT_REPEAT (0: without
// that candidate) and MIRGE_BAM_TIGHT_REGIONS (0: the other routes' two first-position tables instead of the region tables).
#ifndef MIRGE_BAM_TIGHT_LAZY
#define MIRGE_BAM_TIGHT_LAZY 1
#endif
#ifndef MIRGE_BAM_TIGHT_LAZY_BELOW
#define MIRGE_BAM_TIGHT_LAZY_BELOW 32
#endif
#ifndef MIRGE_BAM_TIGHT_LOOKBACK
#define MIRGE_BAM_TIGHT_LOOKBACK 2
#endif
#ifndef MIRGE_BAM_TIGHT_RECORD
#define MIRGE_BAM_TIGHT_RECORD 1
#endif
#ifndef MIRGE_BAM_TIGHT_REPEAT
#define MIRGE_BAM_TIGHT_REPEAT 1
#endif
#ifndef MIRGE_BAM_TIGHT_REGIONS
#define MIRGE_BAM_TIGHT_REGIONS 1
#endif
#define MIRGE_BAM_REGION_BITS 12       // a region: 4 KiB of the block
#define MIRGE_BAM_REGION_HASH_BITS 9   // its buckets
#define MIRGE_BAM_MAX_DIST 32768u
static_assert((((MIRGE_BAM_MAX_BLOCK - 1) >> MIRGE_BAM_REGION_BITS) + 1) << MIRGE_BAM_REGION_HASH_BITS <= (4u << MIRGE_BAM_HASH_BITS),
              "the region tables' 16-bit entries lie in head's words");
static_assert((MIRGE_BAM_TIGHT_LOOKBACK + 1) << MIRGE_BAM_REGION_BITS <= MIRGE_BAM_MAX_DIST, "a region candidate's distance fits the window");

__device__ __forceinline__ uint32_t bam_region_slot(uint32_t v, uint32_t region) {
    return (region << MIRGE_BAM_REGION_HASH_BITS) | ((v * 2654435761u) >> (32 - MIRGE_BAM_REGION_HASH_BITS));
}
__device__ __forceinline__ uint32_t bam_region_get(const uint32_t* tab, uint32_t slot) { return (tab[slot >> 1] >> ((slot & 1u) * 16u)) & 0xFFFFu; }
// entry `slot` = min(entry, v), v < 0xFFFF (an empty entry): the minimum does not depend on the order of the calls
__device__ __forceinline__ void bam_region_min(uint32_t* tab, uint32_t slot, uint32_t v) {
    uint32_t* w = &tab[slot >> 1];
    const uint32_t sh = (slot & 1u) * 16u;
    uint32_t old = *w;
    while (((old >> sh) & 0xFFFFu) > v) {
        const uint32_t got = atomicCAS(w, old, (old & ~(0xFFFFu << sh)) | (v << sh));
        if (got == old) break;
        old = got;
    }
}

// a thread's search state: the record that holds the position (start rs in block coordinates, possibly in front of the block; rl
// bytes; pl: the bytes of the record in front, a guess at the segment's start) and the distance of its last match
struct BamTight { const uint8_t* d; const uint32_t* tab; uint32_t n; long long rs; uint32_t rl, pl, rep; };
// the state at block byte s0 (stream byte ustart + s0): the header counts as one record without a neighbour
__device__ __forceinline__ void bam_tight_start(const SamTables& t, const BamTables& bt, const uint32_t* __restrict__ rows, uint32_t n_rows,
                                                const uint32_t* __restrict__ fixed, const unsigned long long* __restrict__ row_off,
                                                unsigned long long ustart, uint32_t s0, BamTight& c) {
    const unsigned long long H = bt.header_len, S = ustart + s0, far = 1ull << 30;
    c.rs = (long long)s0; c.rl = (uint32_t)far; c.pl = 0u; c.rep = 0u;
    if (S < H) { c.rl = (uint32_t)(H - S < far ? H - S : far); return; }
    const unsigned long long P = S - H;
    uint32_t lo = 0, hi = n_rows;  // the row with row_off[row] <= P < row_off[row + 1]
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (row_off[mid + 1] <= P) lo = mid + 1; else hi = mid; }
    if (lo >= n_rows) return;
    BamRow br;
    bam_row(t, bt, rows[lo], br);
    const unsigned long long F = fixed[lo];
    unsigned long long q = P - row_off[lo], rec_start = row_off[lo], b_lo = 0, b_hi = 10, len = F + 1ull;
    for (int d = 1; d <= 10; d++) {  // the digit band of k that holds byte q of the row
        const unsigned long long nk = (br.c < b_hi ? br.c : b_hi) - b_lo, ll = F + (unsigned long long)d;
        if (q < nk * ll) { rec_start += (q / ll) * ll; len = ll; break; }
        q -= nk * ll; rec_start += nk * ll;
        b_lo = b_hi; b_hi *= 10;
    }
    c.rs = (long long)(rec_start + H) - (long long)ustart; c.rl = c.pl = (uint32_t)len;
}
// on to the record that holds block byte i: a record's first word is the bytes behind it (a match is shorter than eight records)
__device__ __forceinline__ void bam_tight_record(BamTight& c, uint32_t i) {
    for (int g = 0; g < 8 && (long long)i >= c.rs + (long long)c.rl; g++) {
        c.rs += (long long)c.rl; c.pl = c.rl;
        if (c.rs + 4 <= (long long)c.n) c.rl = (bam_ld32(c.d, (uint32_t)c.rs) & 0xFFFFFu) + 4u;
    }
}
// the candidate `dist` bytes in front of i: taken when it is longer than the best so far, or as long and nearer
__device__ __forceinline__ void bam_tight_try(const uint8_t* d, uint32_t i, uint32_t dist, uint32_t lim, uint32_t& best, uint32_t& bdist) {
    if (dist - 1u >= MIRGE_BAM_MAX_DIST || dist > i || dist == bdist) return;
    const uint8_t* a = d + i;
    const uint8_t* b = a - dist;
    if (best && b[best - 1u] != a[best - 1u]) return;
    uint32_t k = 0;
    while (k < lim && b[k] == a[k]) k++;
    if (k >= MIRGE_BAM_MIN_MATCH && (k > best || (k == best && dist < bdist))) { best = k; bdist = dist; }
}
// the best match at i; near: of the candidates that cost no table look-up alone
__device__ __forceinline__ void bam_tight_find(const BamTight& c, uint32_t i, uint32_t& best, uint32_t& bdist, bool near = false) {
    best = 0u; bdist = 0u;
    if (i + MIRGE_BAM_MIN_MATCH > c.n) return;
    const uint32_t lim = c.n - i < MIRGE_BAM_MAX_MATCH ? c.n - i : MIRGE_BAM_MAX_MATCH;
    bam_tight_try(c.d, i, 1u, lim, best, bdist);
    if (MIRGE_BAM_TIGHT_REPEAT) bam_tight_try(c.d, i, c.rep, lim, best, bdist);
    if (MIRGE_BAM_TIGHT_RECORD) { bam_tight_try(c.d, i, c.pl, lim, best, bdist); bam_tight_try(c.d, i, c.rl, lim, best, bdist); }
    if (best >= lim || near) return;
    const uint32_t v = bam_ld32(c.d, i);
    if (MIRGE_BAM_TIGHT_REGIONS) {
        const uint32_t r = i >> MIRGE_BAM_REGION_BITS;
        for (uint32_t back = 0; back <= (uint32_t)MIRGE_BAM_TIGHT_LOOKBACK && back <= r; back++) {
            const uint32_t e = bam_region_get(c.tab, bam_region_slot(v, r - back));
            if (e == 0xFFFFu) continue;
            const uint32_t at = ((r - back) << MIRGE_BAM_REGION_BITS) | e;
            if (at < i) bam_tight_try(c.d, i, i - at, lim, best, bdist);
        }
    } else {
        const uint32_t at = c.tab[bam_hash(v, i)];
        if (at < i) bam_tight_try(c.d, i, i - at, lim, best, bdist);
    }
}
// segment [s0, s1) into a sink S: literal(position), match(position, length, distance); a match may end behind s1.  Returns the end of
// the last token.
template <class S>
__device__ __forceinline__ uint32_t bam_tight_parse(BamTight c, uint32_t s0, uint32_t s1, S& sink) {
    uint32_t i = s0;
    while (i < s1) {
        uint32_t len, dist;
        bam_tight_record(c, i);
        bam_tight_find(c, i, len, dist);
        if (MIRGE_BAM_TIGHT_LAZY && len && i + 1u < s1) {
            // a short match: everything one byte on; a long one from a table: only what is nearer (copy k of a row finds copy k - 10 at
            // its last digit, one byte in front of where copy k - 1 starts to match, for four more distance bits per record)
            const bool shortm = len < (uint32_t)MIRGE_BAM_TIGHT_LAZY_BELOW;
            if (shortm || (dist != 1u && dist != c.rep && dist != c.pl && dist != c.rl)) {
                uint32_t len1, dist1;
                bam_tight_find(c, i + 1u, len1, dist1, !shortm);
                if (len1 > len + 1u || (len1 >= len && dist1 < dist)) { sink.literal(i); i++; len = len1; dist = dist1; }
            }
        }
        if (len) { sink.match(i, len, dist); c.rep = dist; i += len; }
        else { sink.literal(i); i++; }
    }
    return i;
}
// the first search's sink: a match that ends inside the segment in the form of BamCount at its own bytes of tok; the last token, if it
// is a match that reaches the segment's end or runs on behind it, in fin_pos and fin_v (its first three bytes may be another thread's)
struct BamStage {
    uint8_t* tok; uint32_t s1, fin_pos, fin_v;
    __device__ __forceinline__ void literal(uint32_t) {}
    __device__ __forceinline__ void match(uint32_t i, uint32_t len, uint32_t dist) {
        const uint32_t v = (len - 3u) | ((dist - 1u) << 8);
        if (i + len >= s1) { fin_pos = i; fin_v = v; return; }
        tok[i] = (uint8_t)(0x80u | (v & 0x7Fu)); tok[i + 1u] = (uint8_t)(v >> 7); tok[i + 2u] = (uint8_t)(v >> 15);
    }
};
// the tokens of segment [s0, s1) again, from what BamStage left
template <class S>
__device__ __forceinline__ void bam_tight_walk(const uint8_t* tok, uint32_t s0, uint32_t s1, uint32_t fin_pos, uint32_t fin_v, S& sink) {
    for (uint32_t i = s0; i < s1;) {
        uint32_t v;
        if (i == fin_pos) v = fin_v;
        else if (tok[i] & 0x80u) v = (tok[i] & 0x7Fu) | ((uint32_t)tok[i + 1u] << 7) | ((uint32_t)tok[i + 2u] << 15);
        else { sink.literal(i); i++; continue; }
        sink.match(i, (v & 255u) + 3u, (v >> 8) + 1u);
        i += (v & 255u) + 3u;
    }
}
// a thread's tokens from E on into W (bam_put_literal, bam_put_match): those in front are dropped, the one across E is cut to its suffix
template <class W>
struct BamTrim {
    W& w; const uint8_t* d; uint32_t E;
    __device__ __forceinline__ void literal(uint32_t i) { if (i >= E) bam_put_literal(w, d[i]); }
    __device__ __forceinline__ void match(uint32_t i, uint32_t len, uint32_t dist) {
        const uint32_t end = i + len;
        if (end <= E) return;
        if (i < E) {
            len = end - E;
            if (len < MIRGE_BAM_MIN_MATCH) { for (uint32_t k = E; k < end; k++) bam_put_literal(w, d[k]); return; }
        }
        bam_put_match(w, len, dist);
    }
};
// BamTrim's W of the counting walk: the bits under the fixed code, the symbols into the wave's histograms
struct BamTally { uint32_t at; uint32_t* ll; uint32_t* dd; };
__device__ __forceinline__ void bam_put_literal(BamTally& w, uint32_t b) { w.at += b < 144u ? 8u : 9u; atomicAdd(&w.ll[b], 1u); }
__device__ __forceinline__ void bam_put_match(BamTally& w, uint32_t len, uint32_t dist) {
    const BamMatchCode m = bam_match_code(len, dist);
    w.at += (m.idx <= 22u ? 7u : 8u) + m.xb + 5u + m.db;
    atomicAdd(&w.ll[257u + m.idx], 1u);
    atomicAdd(&w.dd[m.dc], 1u);
}
// and of the walk that sizes the segments under the block's own code
struct BamDynTally { uint32_t bits; const BamDynamic* y; };
__device__ __forceinline__ void bam_put_literal(BamDynTally& w, uint32_t b) { w.bits += w.y->len_ll[b]; }
__device__ __forceinline__ void bam_put_match(BamDynTally& w, uint32_t len, uint32_t dist) {
    const BamMatchCode m = bam_match_code(len, dist);
    w.bits += w.y->len_ll[257u + m.idx] + m.xb + w.y->len_d[m.dc] + m.db;
}

// bam_huff_lengths alone, one workgroup (mirge_bam_huffman_probe: a payload that drives the real parse into the 15-bit limit cannot
// be built -- bytes skewed enough always match)
__global__ void __launch_bounds__(MIRGE_BLOCK) k_bam_huff_probe(const uint32_t* __restrict__ counts, uint32_t n, uint32_t max_bits, uint8_t* __restrict__ lengths) {
    __shared__ uint32_t cnt[MIRGE_BAM_HUFF_MAX];
    __shared__ uint8_t len[MIRGE_BAM_HUFF_MAX];
    __shared__ BamHuffWork work;
    if (blockIdx.x != 0 || n > MIRGE_BAM_HUFF_MAX) return;
    for (uint32_t x = threadIdx.x; x < n; x += blockDim.x) cnt[x] = counts[x];
    __syncthreads();
    bam_huff_lengths(cnt, n, max_bits, len, work, threadIdx.x, blockDim.x);
    for (uint32_t x = threadIdx.x; x < n; x += blockDim.x) lengths[x] = len[x];
}

// blocks first_block .. first_block + n_blocks - 1 of the uncompressed stream (stream_bytes = header + records; row_off[n_rows + 1] =
// exclusive scan of the sorted rows' bytes, without the header).  deflate != 0: block b -> one BGZF member at out + b * slot_stride,
// sizes[b] = its bytes.  deflate == 0: its uncompressed bytes at out + b * block_bytes.  DYN: deflate != 0 is deflate == 2, or, with
// TIGHT, deflate == 3.
template <bool DYN> struct BamDynSlot { BamDynamic v; };
template <> struct BamDynSlot<false> {};
// deflate == 3, per thread: the search state at its segment's start, what it emits ([E0, E1)), its last match
template <bool TIGHT> struct BamTightRegs { BamTight c; uint32_t E0, E1, fin_pos, fin_v; };
template <> struct BamTightRegs<false> {};
template <bool DYN, bool TIGHT = false>
__device__ __forceinline__ void bam_blocks_body(const SamTables& t, const BamTables& bt, const uint32_t* __restrict__ rows, uint32_t n_rows,
                                                const uint32_t* __restrict__ fixed, const unsigned long long* __restrict__ row_off,
                                                unsigned long long stream_bytes, unsigned long long first_block, uint32_t n_blocks,
                                                uint32_t block_bytes, int deflate, uint32_t slot_stride, uint8_t* __restrict__ out,
                                                uint32_t* __restrict__ sizes) {
    __shared__ uint32_t data32[(MIRGE_BAM_MAX_BLOCK + 256) / 4];
    __shared__ uint32_t out32[(MIRGE_BAM_MAX_BLOCK + 256) / 4];
    __shared__ uint32_t head[2u << MIRGE_BAM_HASH_BITS];
    __shared__ uint32_t crc_table[256];
    __shared__ uint32_t seg_bits[MIRGE_BLOCK + 1];
    __shared__ uint32_t s_crc;
    __shared__ BamDynSlot<DYN> slot;
    static_assert(DYN || !TIGHT, "the tight parse goes with the block's own code");
    uint8_t* data = reinterpret_cast<uint8_t*>(data32);
    const unsigned long long H = bt.header_len, body = row_off[n_rows];
    const uint32_t tid = threadIdx.x, nth = blockDim.x;
    for (uint32_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const unsigned long long ustart = (first_block + b) * (unsigned long long)block_bytes;
        const uint32_t n = (uint32_t)(stream_bytes - ustart < block_bytes ? stream_bytes - ustart : block_bytes);
        // ---- the block's bytes
        for (uint32_t x = tid; x < n && ustart + x < H; x += nth) data[x] = bt.header[ustart + x];
        const uint32_t n_probe = (n + MIRGE_BAM_PROBE - 1) / MIRGE_BAM_PROBE + 1;  // the last one lies at or behind the block's end
        for (uint32_t i = tid; i < n_probe; i += nth) {
            const unsigned long long S = ustart + (unsigned long long)i * MIRGE_BAM_PROBE;
            if (S < H || S - H >= body) continue;
            const unsigned long long P = S - H;
            uint32_t lo = 0, hi = n_rows;  // the row with row_off[row] <= P < row_off[row + 1]
            while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (row_off[mid + 1] <= P) lo = mid + 1; else hi = mid; }
            if (lo >= n_rows) continue;
            const uint32_t row = lo;
            BamRow br;
            bam_row(t, bt, rows[row], br);
            const unsigned long long F = fixed[row];
            unsigned long long q = P - row_off[row], rec_start = row_off[row], k = 0, b_lo = 0, b_hi = 10;
            for (int d = 1; d <= 10; d++) {  // the digit band of k that holds byte q of the row
                const unsigned long long nk = (br.c < b_hi ? br.c : b_hi) - b_lo, ll = F + (unsigned long long)d;
                if (q < nk * ll) { const unsigned long long kk = q / ll; k = b_lo + kk; rec_start += kk * ll; break; }
                q -= nk * ll; rec_start += nk * ll;
                b_lo = b_hi; b_hi *= 10;
            }
            // the record's owner: the first probe at or behind its start; probe 0 (or the first behind the header) for the one that
            // crosses the block's start (or starts inside the probe's stretch behind the header)
            const bool first_probe = i == 0 || S - MIRGE_BAM_PROBE < H;
            if (!first_probe && rec_start + MIRGE_BAM_PROBE <= P) continue;
            if (rec_start + H >= ustart + n) continue;
            SamOut<true> w{data, (int32_t)((long long)(rec_start + H) - (long long)ustart), (int32_t)n, 0u};
            bam_record<true>(t, br, (uint32_t)F, (uint32_t)k, w);
        }
        __syncthreads();
        if (!deflate) {
            uint8_t* dst = out + (size_t)b * block_bytes;
            if ((block_bytes & 3u) == 0u) {
                uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);
                for (uint32_t x = tid; x < n / 4; x += nth) d4[x] = data32[x];
                for (uint32_t x = (n & ~3u) + tid; x < n; x += nth) dst[x] = data[x];
            } else
                for (uint32_t x = tid; x < n; x += nth) dst[x] = data[x];
            __syncthreads();
            continue;
        }
        // ---- deflate
        for (uint32_t x = tid; x < (2u << MIRGE_BAM_HASH_BITS); x += nth) head[x] = 0xFFFFFFFFu;
        for (uint32_t x = tid; x < (n + 16) / 4 + 1; x += nth) out32[x] = 0u;
        for (uint32_t x = tid; x < 256u; x += nth) {
            uint32_t c = x;
            for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            crc_table[x] = c;
        }
        if (tid == 0) s_crc = 0u;
        if constexpr (DYN) {
            BamDynamic& dyn = slot.v;
            for (uint32_t x = tid; x < MIRGE_BAM_HIST_COPIES * MIRGE_BAM_HUFF_MAX; x += nth) (&dyn.hist_ll[0][0])[x] = 0u;
            for (uint32_t x = tid; x < MIRGE_BAM_HIST_COPIES * 32u; x += nth) (&dyn.hist_d[0][0])[x] = 0u;
        }
        __syncthreads();
        if constexpr (TIGHT && MIRGE_BAM_TIGHT_REGIONS) {
            for (uint32_t i = tid; i + MIRGE_BAM_MIN_MATCH <= n; i += nth)
                bam_region_min(head, bam_region_slot(bam_ld32(data, i), i >> MIRGE_BAM_REGION_BITS), i & ((1u << MIRGE_BAM_REGION_BITS) - 1u));
        } else
            for (uint32_t i = tid; i + MIRGE_BAM_MIN_MATCH <= n; i += nth) atomicMin(&head[bam_hash(bam_ld32(data, i), i)], i);
        __syncthreads();
        const uint32_t seg = (n + nth - 1) / nth;
        const uint32_t s0 = tid * seg < n ? tid * seg : n, s1 = s0 + seg < n ? s0 + seg : n;
        BamTightRegs<TIGHT> tr;
        {
            if constexpr (TIGHT) {
                BamDynamic& dyn = slot.v;
                BamStage st{reinterpret_cast<uint8_t*>(out32), s1, 0xFFFFFFFFu, 0u};
                tr.c = BamTight{data, head, n, 0ll, 0u, 0u, 0u};
                if (s0 < s1) bam_tight_start(t, bt, rows, n_rows, fixed, row_off, ustart, s0, tr.c);
                seg_bits[tid] = bam_tight_parse(tr.c, s0, s1, st);
                tr.fin_pos = st.fin_pos; tr.fin_v = st.fin_v;
                __syncthreads();
                if (tid == 0) {  // E_t: where the tokens of the threads in front end
                    uint32_t run = 0u;
                    for (uint32_t x = 0; x < nth; x++) { const uint32_t v = seg_bits[x]; seg_bits[x] = run; run = v > run ? v : run; }
                    seg_bits[nth] = run;
                }
                __syncthreads();
                tr.E0 = seg_bits[tid]; tr.E1 = seg_bits[tid + 1u];
                __syncthreads();
                const uint32_t copy = (tid >> 6) % MIRGE_BAM_HIST_COPIES;
                BamTally cw{0u, dyn.hist_ll[copy], dyn.hist_d[copy]};
                BamTrim<BamTally> tw{cw, data, tr.E0};
                if (tr.E1 > tr.E0) bam_tight_walk(reinterpret_cast<const uint8_t*>(out32), s0, s1, tr.fin_pos, tr.fin_v, tw);
                seg_bits[tid] = cw.at;
            } else if constexpr (DYN) {
                BamDynamic& dyn = slot.v;
                const uint32_t copy = (tid >> 6) % MIRGE_BAM_HIST_COPIES;
                BamCount cw{0u, s0, dyn.hist_ll[copy], dyn.hist_d[copy], reinterpret_cast<uint8_t*>(out32)};
                bam_parse(data, head, s0, s1, cw);
                seg_bits[tid] = cw.at;
            } else {
                BamBits<false> cw;
                cw.start(nullptr, 0u);
                bam_parse(data, head, s0, s1, cw);
                seg_bits[tid] = cw.at;
            }
            uint32_t crc = 0xFFFFFFFFu;
            for (uint32_t x = s0; x < s1; x++) crc = crc_table[(crc ^ data[x]) & 255u] ^ (crc >> 8);
            if (s1 > s0) atomicXor(&s_crc, bam_crc_mul(bam_crc_x8n(n - s1), ~crc));
        }
        __syncthreads();
        if (tid == 0) {  // exclusive sum of the segments' bits behind the 3 bits of the block header
            uint32_t run = 3u;
            for (uint32_t x = 0; x < nth; x++) { const uint32_t v = seg_bits[x]; seg_bits[x] = run; run += v; }
            seg_bits[nth] = run;
        }
        __syncthreads();
        const uint32_t end_bit = seg_bits[nth] + 7u;  // (the end-of-block code: seven zeros)
        bool stored = (end_bit + 7u) / 8u >= n + 5u, dynamic = false;
        uint32_t clen = stored ? n + 5u : (end_bit + 7u) / 8u;
        if constexpr (DYN) {  // ---- the block's own code: its lengths, the header, every segment's bits; taken when it is the shortest form
            BamDynamic& dyn = slot.v;
            for (uint32_t x = tid; x < MIRGE_BAM_HUFF_MAX; x += nth)
                dyn.hist_ll[0][x] += dyn.hist_ll[1][x] + dyn.hist_ll[2][x] + dyn.hist_ll[3][x] + (x == 256u ? 1u : 0u);  // (the end-of-block code: once)
            for (uint32_t x = tid; x < 32u; x += nth) dyn.hist_d[0][x] += dyn.hist_d[1][x] + dyn.hist_d[2][x] + dyn.hist_d[3][x];
            __syncthreads();
            bam_huff_lengths2<TIGHT>(dyn.hist_ll[0], MIRGE_BAM_NLL, dyn.len_ll, dyn.work[0], dyn.hist_d[0], MIRGE_BAM_ND, dyn.len_d, dyn.work[1], 15u, tid, nth);
            if constexpr (TIGHT) {
                BamDynTally cw{0u, &dyn};
                BamTrim<BamDynTally> tw{cw, data, tr.E0};
                if (tr.E1 > tr.E0) bam_tight_walk(reinterpret_cast<const uint8_t*>(out32), s0, s1, tr.fin_pos, tr.fin_v, tw);
                dyn.seg[tid] = cw.bits;
            } else
                dyn.seg[tid] = bam_dyn_bits(dyn, data, reinterpret_cast<const uint8_t*>(out32), s0, s1);
            if (tid == 0) bam_dyn_header_tokens<TIGHT>(dyn);
            __syncthreads();
            bam_huff_lengths2<TIGHT>(dyn.cnt_cl[0], MIRGE_BAM_NCL, dyn.len_cl[0], dyn.work[0], dyn.cnt_cl[1], MIRGE_BAM_NCL, dyn.len_cl[1], dyn.work[1], 7u, tid, nth);
            if (tid == 0) {  // exclusive sum of the segments' bits behind the header's
                bam_dyn_header_choice<TIGHT>(dyn);
                uint32_t run = dyn.header_bits;
                for (uint32_t x = 0; x < nth; x++) { const uint32_t v = dyn.seg[x]; dyn.seg[x] = run; run += v; }
                dyn.seg[nth] = run + dyn.len_ll[256];
            }
            __syncthreads();
            dynamic = (dyn.seg[nth] + 7u) / 8u < clen;
            if (dynamic) { clen = (dyn.seg[nth] + 7u) / 8u; stored = false; }
            for (uint32_t x = tid; x < (n + 16) / 4 + 1; x += nth) out32[x] = 0u;  // (the staged matches)
            if (dynamic) {
                bam_huff_codes(dyn.len_ll, MIRGE_BAM_NLL, dyn.code_ll, tid, nth);
                bam_huff_codes(dyn.len_d, MIRGE_BAM_ND, dyn.code_d, tid, nth);
                bam_huff_codes(dyn.len_cl[dyn.plain], MIRGE_BAM_NCL, dyn.code_cl, tid, nth);
            }
            __syncthreads();
        }
        uint8_t* dst = out + (size_t)b * slot_stride;
        if (!stored) {
            if constexpr (DYN) if (dynamic) {
                BamDynamic& dyn = slot.v;
                BamDynBits ew;
                ew.ll = dyn.code_ll; ew.dd = dyn.code_d;
                ew.b.start(out32, dyn.seg[tid]);
                if (tid == 0) { ew.b.start(out32, 0u); bam_dyn_put_header<TIGHT>(dyn, ew.b); }
                if constexpr (TIGHT) {
                    BamTrim<BamDynBits> tw{ew, data, tr.E0};
                    if (tr.E1 > tr.E0) bam_tight_parse(tr.c, s0, s1, tw);
                } else
                    bam_parse(data, head, s0, s1, ew);
                if (tid == nth - 1u) bam_put_code(ew.b, dyn.code_ll[256]);  // (every segment behind the block's end is empty: the last thread ends the stream)
                ew.b.finish();
            }
            if (!dynamic) {
                BamBits<true> ew;
                ew.start(out32, seg_bits[tid]);
                if (tid == 0) { ew.start(out32, 0u); ew.put(3u, 3); }  // BFINAL = 1, BTYPE = 01
                if constexpr (TIGHT) {
                    BamTrim<BamBits<true>> tw{ew, data, tr.E0};
                    if (tr.E1 > tr.E0) bam_tight_parse(tr.c, s0, s1, tw);
                } else
                    bam_parse(data, head, s0, s1, ew);
                ew.finish();
            }
            __syncthreads();
            const uint8_t* ob = reinterpret_cast<const uint8_t*>(out32);
            for (uint32_t x = tid; x < clen; x += nth) dst[18 + x] = ob[x];
        } else {
            if (tid == 0) {
                dst[18] = 1u;  // BFINAL = 1, BTYPE = 00
                dst[19] = (uint8_t)(n & 255u); dst[20] = (uint8_t)(n >> 8);
                dst[21] = (uint8_t)(~n & 255u); dst[22] = (uint8_t)((~n >> 8) & 255u);
            }
            for (uint32_t x = tid; x < n; x += nth) dst[23 + x] = data[x];
        }
        if (tid == 0) {
            const uint32_t bsize = clen + 26u, crc = s_crc;
            const uint8_t hd[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)((bsize - 1u) & 255u), (uint8_t)((bsize - 1u) >> 8)};
            for (int x = 0; x < 18; x++) dst[x] = hd[x];
            uint8_t* tr = dst + 18 + clen;
            for (int x = 0; x < 4; x++) { tr[x] = (uint8_t)(crc >> (8 * x)); tr[4 + x] = (uint8_t)(n >> (8 * x)); }
            sizes[b] = bsize;
        }
        __syncthreads();
    }
}
// deflate == 2 is an instantiation of its own, so that the code and the registers of the other two stay what they are without it: on the
// device k_bam_blocks_dynamic is its kernel (native_bam.hpp launches it for MIRGE_BAM_DEFLATE=dynamic) and k_bam_blocks does not hold
// it; compiled for the host (tests/hostsim/bam_sim.cpp), where nothing is allocated, k_bam_blocks takes deflate == 2 as well.
// deflate == 3 likewise: k_bam_blocks_tight on the device (MIRGE_BAM_DEFLATE=tight), k_bam_blocks on the host.
__global__ void __launch_bounds__(MIRGE_BLOCK) k_bam_blocks(SamTables t, BamTables bt, const uint32_t* __restrict__ rows, uint32_t n_rows,
                                                            const uint32_t* __restrict__ fixed, const unsigned long long* __restrict__ row_off,
                                                            unsigned long long stream_bytes, unsigned long long first_block, uint32_t n_blocks,
                                                            uint32_t block_bytes, int deflate, uint32_t slot_stride, uint8_t* __restrict__ out,
                                                            uint32_t* __restrict__ sizes) {
#ifndef __HIP_DEVICE_COMPILE__
    if (deflate == 2) { bam_blocks_body<true>(t, bt, rows, n_rows, fixed, row_off, stream_bytes, first_block, n_blocks, block_bytes, deflate, slot_stride, out, sizes); return; }
    if (deflate == 3) { bam_blocks_body<true, true>(t, bt, rows, n_rows, fixed, row_off, stream_bytes, first_block, n_blocks, block_bytes, deflate, slot_stride, out, sizes); return; }
#endif
    bam_blocks_body<false>(t, bt, rows, n_rows, fixed, row_off, stream_bytes, first_block, n_blocks, block_bytes, deflate, slot_stride, out, sizes);
}
__global__ void __launch_bounds__(MIRGE_BLOCK) k_bam_blocks_dynamic(SamTables t, BamTables bt, const uint32_t* __restrict__ rows, uint32_t n_rows,
                                                                    const uint32_t* __restrict__ fixed, const unsigned long long* __restrict__ row_off,
                                                                    unsigned long long stream_bytes, unsigned long long first_block, uint32_t n_blocks,
                                                                    uint32_t block_bytes, uint32_t slot_stride, uint8_t* __restrict__ out,
                                                                    uint32_t* __restrict__ sizes) {
    bam_blocks_body<true>(t, bt, rows, n_rows, fixed, row_off, stream_bytes, first_block, n_blocks, block_bytes, 2, slot_stride, out, sizes);
}
__global__ void __launch_bounds__(MIRGE_BLOCK) k_bam_blocks_tight(SamTables t, BamTables bt, const uint32_t* __restrict__ rows, uint32_t n_rows,
                                                                  const uint32_t* __restrict__ fixed, const unsigned long long* __restrict__ row_off,
                                                                  unsigned long long stream_bytes, unsigned long long first_block, uint32_t n_blocks,
                                                                  uint32_t block_bytes, uint32_t slot_stride, uint8_t* __restrict__ out,
                                                                  uint32_t* __restrict__ sizes) {
    bam_blocks_body<true, true>(t, bt, rows, n_rows, fixed, row_off, stream_bytes, first_block, n_blocks, block_bytes, 3, slot_stride, out, sizes);
}

// member b of a chunk from its slot to its place: off[] = exclusive scan of sizes[]
__global__ void k_bam_compact(const uint8_t* __restrict__ slots, uint32_t slot_stride, const uint32_t* __restrict__ sizes, const uint32_t* __restrict__ off,
                              uint32_t n_blocks, uint8_t* __restrict__ out) {
    for (uint32_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const uint8_t* src = slots + (size_t)b * slot_stride;
        uint8_t* dst = out + off[b];
        for (uint32_t x = threadIdx.x; x < sizes[b]; x += blockDim.x) dst[x] = src[x];
    }
}
