// kernels_sam.hpp -- part of mirge_kernels.hpp: the per-sample SAM text of `--sam-out` (what the reference's `-bam` route hands to
// `samtools view`: alignPlusParse's side files, manifoldAlign.py:12-64; bow2bam, bamFmt.py:115-170; the order of summary.py:841-880)
// formatted where the reads, the count matrix and the cascade's (pass, reference, offset, mismatches) already lie.
//   k_sam_select  : frame position k -> flag "writes lines into this sample's file" in its class's stretch of ONE flag array
//                   (class-major: snoRNA, rRNA, ncrna others, mRNA, exact miRNA, isomiR, hairpin); one exclusive scan of that array
//                   IS the file's row order.  Dropped: a count of 0 in this sample, a reference without lift entry, tRNA / spike-in.
//   k_sam_rows    : kept positions -> rows[] (handle indices)
//   k_sam_measure : per row, the bytes of a line without the digits of its copy number k, and the bytes of all its c copies
//                   (closed form over the decimal digit bands of k = 0 .. c-1)                       -> one 64-bit exclusive scan
//   k_sam_write   : OUTPUT-stationary.  A workgroup owns a fixed stretch (tile) of the file's text; every 32 bytes of it are a probe
//                   point whose thread finds the (row, k) of the line that holds the point (binary search over the row offsets,
//                   then the digit bands) and formats that line iff it is the first probe point at or behind the line's start (a
//                   line is longer than 32 bytes, so every line has exactly one such point per tile it touches).  Lines are clipped
//                   to the tile, built in LDS and stored 16 bytes a lane.  A row with 10^6 copies costs what 10^6 rows with one do.
// A line:  READ_k \t FLAG \t CHROM \t START \t 255 \t <len>M \t * \t 0 \t 0 \t SEQ \t I*len \t XA:i:n \t MD:Z:.. \t NM:i:n \n
#pragma once

#define MIRGE_SAM_NCLASS 7
#define MIRGE_SAM_PROBE 32       // bytes between two probe points; every line is longer (13 tabs + newline + 34 fixed characters)
#define MIRGE_SAM_MAX_TILE 16384

struct SamPass {
    const uint64_t* T;            // the pass's library: 2-bit text, invalid bitmap, reference starts (MirgeLibView)
    const uint64_t* inv;
    const uint32_t* ref_start;
    const int32_t* chrom_of_ref;  // [n_refs] index into the chromosome table, -1: no line for reads of this reference
    const uint8_t* minus;         // [n_refs] 1: the transcript lies on the minus strand
    const uint32_t* seg_ptr;      // [n_refs + 1] CSR into the four bound arrays
    const int32_t* seg_s;         // transcript coordinates of a segment, 1-based, both inclusive
    const int32_t* seg_e;
    const long long* cds_lo;      // the segment's first and second genome coordinate as the header writes them
    const long long* cds_hi;
    const uint8_t* chrom_data;
    const uint32_t* chrom_off;    // [n_chrom + 1]
    uint32_t n_refs, n_chrom;
    int32_t trim5, trim3;
    int32_t cls;                  // position of the pass in the file's class order, -1: writes nothing
    int32_t pad;
};
struct SamTables {
    CsvGroup g[MIRGE_CSV_MAXG];
    const int32_t* off[MIRGE_CSV_MAXG];
    const int8_t* mm[MIRGE_CSV_MAXG];
    const SamPass* pass;          // [n_pass], device memory
    int32_t n_pass, S, sample;
};

__device__ __forceinline__ int sam_locate(const SamTables& t, uint32_t i, uint32_t& j) {
    int gi = 0;
#pragma unroll
    for (int k = 1; k < MIRGE_CSV_MAXG; k++)
        if (t.g[k].n && i >= t.g[k].base) gi = k;
    j = i - t.g[gi].base;
    return gi;
}

// sum of the decimal digits' COUNT over k = 0 .. c-1 (k = 0 has one digit)
__host__ __device__ __forceinline__ unsigned long long sam_digit_total(unsigned long long c) {
    unsigned long long total = 0, lo = 0, hi = 10;
    for (int d = 1; d <= 20 && lo < c; d++) {
        total += (unsigned long long)d * ((c < hi ? c : hi) - lo);
        lo = hi; hi *= 10;
    }
    return total;
}

// flags[0] |= 1: pass / reference / offset out of range (the call fails)
__global__ void k_sam_select(SamTables t, const uint32_t* __restrict__ order, uint32_t n, uint32_t* __restrict__ keep, uint32_t* __restrict__ flags) {
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
        uint32_t j;
        const int gi = sam_locate(t, order[k], j);
        const CsvGroup& g = t.g[gi];
        const int p = g.pass[j];
        if (p < 0) continue;
        if (p >= t.n_pass) { atomicOr(&flags[0], 1u); continue; }
        const SamPass& sp = t.pass[p];
        if (sp.cls < 0 || g.counts[(size_t)j * t.S + t.sample] == 0u) continue;
        const int32_t r = g.ref[j];
        const int32_t o = t.off[gi][j];
        const int Ls = csv_len(g, j) - sp.trim5 - sp.trim3;
        if (!sp.T || r < 0 || (uint32_t)r >= sp.n_refs || o < 0 || Ls < 1 ||
            (unsigned long long)sp.ref_start[r] + (unsigned long long)o + (unsigned long long)Ls > (unsigned long long)sp.ref_start[r + 1]) {
            atomicOr(&flags[0], 1u);
            continue;
        }
        const int32_t ci = sp.chrom_of_ref[r];
        if (ci < 0) continue;
        if ((uint32_t)ci >= sp.n_chrom) { atomicOr(&flags[0], 1u); continue; }
        keep[(size_t)sp.cls * n + k] = 1u;
    }
}
__global__ void k_sam_rows(const uint32_t* __restrict__ order, uint32_t n, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ pos,
                           uint32_t* __restrict__ rows) {
    const size_t total = (size_t)n * MIRGE_SAM_NCLASS;
    for (size_t x = blockIdx.x * (size_t)blockDim.x + threadIdx.x; x < total; x += (size_t)gridDim.x * blockDim.x)
        if (keep[x]) rows[pos[x]] = order[x % n];
}

// a cursor that counts (WRITE = false) or writes the part of a line that falls into [0, tile_len) of `o`; rel = line start - tile start
template <bool WRITE>
struct SamOut {
    uint8_t* o;
    int32_t rel, tile_len;
    uint32_t n;
    __device__ __forceinline__ void ch(char c) {
        if (WRITE) { const int32_t x = rel + (int32_t)n; if ((uint32_t)x < (uint32_t)tile_len) o[x] = (uint8_t)c; }
        n++;
    }
    __device__ __forceinline__ void str(const char* s) { for (int k = 0; s[k]; k++) ch(s[k]); }
    __device__ __forceinline__ void u64(unsigned long long v) {
        int nd = 1;
        for (unsigned long long x = v; x >= 10ull; x /= 10ull) nd++;
        if (WRITE) {
            unsigned long long x = v;
            for (int d = nd - 1; d >= 0; d--) {
                const int32_t at = rel + (int32_t)n + d;
                if ((uint32_t)at < (uint32_t)tile_len) o[at] = (uint8_t)('0' + (int)(x % 10ull));
                x /= 10ull;
            }
        }
        n += (uint32_t)nd;
    }
    __device__ __forceinline__ void i64(long long v) { if (v < 0) { ch('-'); u64(0ull - (unsigned long long)v); } else u64((unsigned long long)v); }
};

// base p of a packed read, one load per 32 bases
struct SamRead {
    const CsvGroup& g;
    uint32_t j;
    int cur;
    uint64_t bits, nm;
    __device__ __forceinline__ SamRead(const CsvGroup& gg, uint32_t jj) : g(gg), j(jj), cur(-1), bits(0), nm(0) {}
    __device__ __forceinline__ char at(int p) {
        const int w = p >> 5;
        if (w != cur) { cur = w; bits = g.seq[(size_t)w * g.n + j]; nm = g.nmask ? g.nmask[(size_t)w * g.n + j] : 0ull; }
        const int s = 2 * (p & 31);
        return ((nm >> s) & 1ull) ? 'N' : "ACGT"[(bits >> s) & 3ull];
    }
};
__device__ __forceinline__ char sam_text_at(const SamPass& sp, unsigned long long gpos) {
    if ((sp.inv[gpos >> 6] >> (gpos & 63)) & 1ull) return 'N';
    return "ACGT"[(sp.T[gpos >> 5] >> (2 * (gpos & 31))) & 3ull];
}
__device__ __forceinline__ char sam_complement(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c; }

// START of a read of Ls bases at offset o of reference r, lifted to the genome: fetch_pos_coordinate / fetch_neg_coordinate
// (bamFmt.py:36-113): the FIRST segment that holds POS decides; none: POS itself
__device__ __forceinline__ long long sam_lift_start(const SamPass& sp, int32_t r, int32_t o, int Ls, bool minus) {
    const long long pos1 = (long long)o + 1;
    for (uint32_t s = sp.seg_ptr[r]; s < sp.seg_ptr[r + 1]; s++)
        if (pos1 >= (long long)sp.seg_s[s] && pos1 <= (long long)sp.seg_e[s])
            return minus ? sp.cds_hi[s] - (pos1 - (long long)sp.seg_s[s]) - (long long)Ls + 1 : sp.cds_lo[s] + (pos1 - (long long)sp.seg_s[s]);
    return pos1;
}

// copy k of the row of unique read `read` (a row k_sam_select kept)
template <bool WRITE>
__device__ __forceinline__ void sam_line(const SamTables& t, uint32_t read, uint32_t k, SamOut<WRITE>& w) {
    uint32_t j;
    const int gi = sam_locate(t, read, j);
    const CsvGroup& g = t.g[gi];
    const SamPass& sp = t.pass[g.pass[j]];
    const int32_t r = g.ref[j];
    const int32_t o = t.off[gi][j];
    const int L = csv_len(g, j);
    const int Ls = L - sp.trim5 - sp.trim3;
    const bool minus = sp.minus[r] != 0;
    SamRead rd(g, j);
    for (int p = 0; p < L; p++) w.ch(rd.at(p));  // QNAME: the whole read, untrimmed
    w.ch('_'); w.u64(k);
    w.str(minus ? "\t16\t" : "\t0\t");
    const int32_t ci = sp.chrom_of_ref[r];
    for (uint32_t x = sp.chrom_off[ci]; x < sp.chrom_off[ci + 1]; x++) w.ch((char)sp.chrom_data[x]);
    w.ch('\t');
    w.i64(sam_lift_start(sp, r, o, Ls, minus));
    w.str("\t255\t"); w.u64((unsigned long long)Ls); w.str("M\t*\t0\t0\t");
    if (minus) for (int p = Ls - 1; p >= 0; p--) w.ch(sam_complement(rd.at(sp.trim5 + p)));
    else for (int p = 0; p < Ls; p++) w.ch(rd.at(sp.trim5 + p));
    w.ch('\t');
    for (int p = 0; p < Ls; p++) w.ch('I');
    const unsigned long long mmv = (unsigned long long)(t.mm[gi][j] < 0 ? 0 : t.mm[gi][j]);
    w.str("\tXA:i:"); w.u64(mmv);
    w.str("\tMD:Z:");
    const unsigned long long g0 = (unsigned long long)sp.ref_start[r] + (unsigned long long)o;
    unsigned long long run = 0;
    for (int p = 0; p < Ls; p++) {  // matches, the reference's base at a mismatch, matches (the forward read, also on the minus strand)
        const char a = rd.at(sp.trim5 + p), b = sam_text_at(sp, g0 + (unsigned long long)p);
        if (a == b) run++;
        else { w.u64(run); w.ch(b); run = 0; }
    }
    w.u64(run);
    w.str("\tNM:i:"); w.u64(mmv);
    w.ch('\n');
}

__global__ void k_sam_measure(SamTables t, const uint32_t* __restrict__ rows, uint32_t n_rows, uint32_t* __restrict__ fixed,
                              unsigned long long* __restrict__ total, unsigned long long* __restrict__ n_lines) {
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n_rows; x += gridDim.x * blockDim.x) {
        SamOut<false> w{nullptr, 0, 0, 0u};
        sam_line<false>(t, rows[x], 0u, w);
        uint32_t j;
        const int gi = sam_locate(t, rows[x], j);
        const unsigned long long c = t.g[gi].counts[(size_t)j * t.S + t.sample];
        const uint32_t F = w.n - 1u;  // (copy 0 printed one digit)
        fixed[x] = F;
        total[x] = c * (unsigned long long)F + sam_digit_total(c);
        atomicAdd(n_lines, c);
    }
}

// text [chunk_start, chunk_start + chunk_bytes) of the file's body -> out[0 .. chunk_bytes); one workgroup per tile of tile_bytes
// (a multiple of 16, at most MIRGE_SAM_MAX_TILE); row_off[n_rows + 1] = exclusive scan of k_sam_measure's totals
__global__ void __launch_bounds__(MIRGE_BLOCK) k_sam_write(SamTables t, const uint32_t* __restrict__ rows, uint32_t n_rows,
                                                           const uint32_t* __restrict__ fixed, const unsigned long long* __restrict__ row_off,
                                                           unsigned long long chunk_start, uint32_t chunk_bytes, uint32_t tile_bytes,
                                                           uint8_t* __restrict__ out) {
    __shared__ uint4 tile16[MIRGE_SAM_MAX_TILE / 16];
    uint8_t* tile = reinterpret_cast<uint8_t*>(tile16);
    const unsigned long long body = row_off[n_rows];
    for (uint32_t tb = blockIdx.x; (unsigned long long)tb * tile_bytes < chunk_bytes; tb += gridDim.x) {
        const uint32_t in_chunk = tb * tile_bytes;
        const uint32_t tile_len = chunk_bytes - in_chunk < tile_bytes ? chunk_bytes - in_chunk : tile_bytes;
        const unsigned long long tile_start = chunk_start + in_chunk;
        const uint32_t n_probe = (tile_len + MIRGE_SAM_PROBE - 1) / MIRGE_SAM_PROBE + 1;  // the last one lies at or behind the tile's end
        for (uint32_t i = threadIdx.x; i < n_probe; i += blockDim.x) {
            const unsigned long long P = tile_start + (unsigned long long)i * MIRGE_SAM_PROBE;
            if (P >= body) continue;
            uint32_t lo = 0, hi = n_rows;  // the row with row_off[row] <= P < row_off[row + 1]
            while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (row_off[mid + 1] <= P) lo = mid + 1; else hi = mid; }
            if (lo >= n_rows) continue;
            const uint32_t row = lo, read = rows[row];
            uint32_t j;
            const int gi = sam_locate(t, read, j);
            const unsigned long long c = t.g[gi].counts[(size_t)j * t.S + t.sample];
            const unsigned long long F = fixed[row];
            unsigned long long q = P - row_off[row], line_start = row_off[row], k = 0, b_lo = 0, b_hi = 10;
            for (int d = 1; d <= 10; d++) {  // the digit band of k that holds byte q of the row
                const unsigned long long nk = (c < b_hi ? c : b_hi) - b_lo, ll = F + (unsigned long long)d;
                if (q < nk * ll) { const unsigned long long kk = q / ll; k = b_lo + kk; line_start += kk * ll; break; }
                q -= nk * ll; line_start += nk * ll;
                b_lo = b_hi; b_hi *= 10;
            }
            // the line's owner: probe 0 for the line that crosses the tile's start, else the first probe at or behind its start
            if (i != 0 && line_start + MIRGE_SAM_PROBE <= P) continue;
            if (line_start >= tile_start + tile_len) continue;
            SamOut<true> w{tile, (int32_t)((long long)line_start - (long long)tile_start), (int32_t)tile_len, 0u};
            sam_line<true>(t, read, (uint32_t)k, w);
        }
        __syncthreads();
        uint4* dst = reinterpret_cast<uint4*>(out + in_chunk);
        for (uint32_t x = threadIdx.x; x < tile_len / 16; x += blockDim.x) dst[x] = tile16[x];
        for (uint32_t x = (tile_len & ~15u) + threadIdx.x; x < tile_len; x += blockDim.x) out[in_chunk + x] = tile[x];
        __syncthreads();
    }
}
