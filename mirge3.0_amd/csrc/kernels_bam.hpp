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
template <bool WRITE> __device__ __forceinline__ void bam_put_match(BamBits<WRITE>& w, uint32_t len, uint32_t dist) {
    uint32_t idx, xb = 0, xv = 0;
    if (len <= 10u) idx = len - 3u;
    else if (len == 258u) idx = 28u;
    else { const uint32_t l = len - 3u; const int e = bam_log2(l) - 2; idx = 4u * (uint32_t)(e + 1) + ((l >> e) & 3u); xb = (uint32_t)e; xv = l & ((1u << e) - 1u); }
    const uint32_t sym = 257u + idx;
    if (sym <= 279u) w.put(bam_bitrev(sym - 256u, 7), 7); else w.put(bam_bitrev(0xC0u + (sym - 280u), 8), 8);
    if (xb) w.put(xv, (int)xb);
    uint32_t dc, db = 0, dv = 0;
    if (dist <= 4u) dc = dist - 1u;
    else { const uint32_t d = dist - 1u; const int e = bam_log2(d) - 1; dc = 2u * (uint32_t)(e + 1) + ((d >> e) & 1u); db = (uint32_t)e; dv = d & ((1u << e) - 1u); }
    w.put(bam_bitrev(dc, 5), 5);
    if (db) w.put(dv, (int)db);
}
__device__ __forceinline__ uint32_t bam_ld32(const uint8_t* d, uint32_t i) {
    return (uint32_t)d[i] | ((uint32_t)d[i + 1] << 8) | ((uint32_t)d[i + 2] << 16) | ((uint32_t)d[i + 3] << 24);
}
__device__ __forceinline__ uint32_t bam_hash(uint32_t v, uint32_t i) {
    return ((i >> 15) << MIRGE_BAM_HASH_BITS) | ((v * 2654435761u) >> (32 - MIRGE_BAM_HASH_BITS));
}
// the greedy parse of segment [s0, s1) of the block's n bytes
template <bool WRITE>
__device__ __forceinline__ void bam_parse(const uint8_t* d, const uint32_t* head, uint32_t s0, uint32_t s1, BamBits<WRITE>& w) {
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

// blocks first_block .. first_block + n_blocks - 1 of the uncompressed stream (stream_bytes = header + records; row_off[n_rows + 1] =
// exclusive scan of the sorted rows' bytes, without the header).  deflate != 0: block b -> one BGZF member at out + b * slot_stride,
// sizes[b] = its bytes.  deflate == 0: its uncompressed bytes at out + b * block_bytes.
__global__ void __launch_bounds__(MIRGE_BLOCK) k_bam_blocks(SamTables t, BamTables bt, const uint32_t* __restrict__ rows, uint32_t n_rows,
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
        __syncthreads();
        for (uint32_t i = tid; i + MIRGE_BAM_MIN_MATCH <= n; i += nth) atomicMin(&head[bam_hash(bam_ld32(data, i), i)], i);
        __syncthreads();
        const uint32_t seg = (n + nth - 1) / nth;
        const uint32_t s0 = tid * seg < n ? tid * seg : n, s1 = s0 + seg < n ? s0 + seg : n;
        {
            BamBits<false> cw;
            cw.start(nullptr, 0u);
            bam_parse<false>(data, head, s0, s1, cw);
            seg_bits[tid] = cw.at;
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
        const bool stored = (end_bit + 7u) / 8u >= n + 5u;
        const uint32_t clen = stored ? n + 5u : (end_bit + 7u) / 8u;
        uint8_t* dst = out + (size_t)b * slot_stride;
        if (!stored) {
            BamBits<true> ew;
            ew.start(out32, seg_bits[tid]);
            if (tid == 0) { ew.start(out32, 0u); ew.put(3u, 3); }  // BFINAL = 1, BTYPE = 01
            bam_parse<true>(data, head, s0, s1, ew);
            ew.finish();
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

// member b of a chunk from its slot to its place: off[] = exclusive scan of sizes[]
__global__ void k_bam_compact(const uint8_t* __restrict__ slots, uint32_t slot_stride, const uint32_t* __restrict__ sizes, const uint32_t* __restrict__ off,
                              uint32_t n_blocks, uint8_t* __restrict__ out) {
    for (uint32_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const uint8_t* src = slots + (size_t)b * slot_stride;
        uint8_t* dst = out + off[b];
        for (uint32_t x = threadIdx.x; x < sizes[b]; x += blockDim.x) dst[x] = src[x];
    }
}
