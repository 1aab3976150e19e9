// kernels_bw.hpp -- part of mirge_kernels.hpp: the runs of `--coverage` (kernels_cov.hpp, CovRuns) as bigWig (`--coverage-bigwig`;
// mirge3_amd/bigwig.py holds the format).  The container's headers, trees and indexes are host work (bw_layout.hpp); here is what
// costs per run or per byte:
//   k_bw_ranges      : the first run of every (strand, chromosome rank), by binary search -- the runs are contiguous per rank, the
//                      host walks the ranks in the byte order of their names
//   k_bw_limits      : the first run that ends beyond its chromosome's LN; the largest depth per strand
//   k_bw_zoom_count  : per run, the bins of width R it opens = the bins it spans, minus the first one when the previous run of the same
//   k_bw_zoom_bins     strand and chromosome already ended in it (64-bit exclusive sum, hipCUB); every record keeps its first run
//   k_bw_pick        : where every rank's records start (the offsets at k_bw_ranges' runs)
//   k_bw_zoom_reduce : per record, forward from that run while the runs start before the bin's end: overlapped bases, min, max and the
//                      two sums in doubles, product and sum rounded one after the other
//   k_bw_summary     : per section, the same sums over its items in item order (the host adds the sections' partials)
//   k_bw_blocks<REC> : one workgroup per block (section: 24-byte header + items with the float conversion; or zoom records): the bytes
//                      in LDS, Adler-32 from per-lane partials, the fixed-code deflate of kernels_bam.hpp (bam_parse, BamBits) or the
//                      stored form when that is not larger, as one zlib stream into the block's slot; k_bam_compact packs the slots
// Integer work except the sums, which have one order.  LDS per instance: payload 12 312 B (sections) or 32 768 B (zoom blocks).
#pragma once

#define MIRGE_BW_MAX_SECTION 1024u
#define MIRGE_BW_MAX_LEVELS 8
#define MIRGE_BW_MAX_REDUCTION (1u << 20)
#define MIRGE_BW_NONE 0xFFFFFFFFu
#define MIRGE_BW_ADLER 65521u

struct BwRec { uint32_t chrom, start, end, valid; float vmin, vmax, sum, sq; };  // a zoom record as the file holds it
struct BwBlk { uint32_t first, count, chrom; };                                  // a block: items / records [first, first + count) of chromId chrom
struct BwPart { unsigned long long bases; double vmin, vmax, sum, sq; };          // a section's part of the total summary
static_assert(sizeof(BwRec) == 32, "a zoom record is 32 bytes");

// float32(depth), round to nearest even, in integer steps so that host and device agree bit for bit
__host__ __device__ __forceinline__ uint32_t bw_value_bits(long long depth) {
    unsigned long long d = (unsigned long long)depth;
    if (d == 0ull) return 0u;
    int top = 63;
    while (!((d >> top) & 1ull)) top--;
    if (top <= 23) return ((uint32_t)(127 + top) << 23) + (uint32_t)((d << (23 - top)) - (1ull << 23));
    const int sh = top - 23;
    unsigned long long m = d >> sh;
    const unsigned long long rem = d & ((1ull << sh) - 1ull), half = 1ull << (sh - 1);
    if (rem > half || (rem == half && (m & 1ull))) m++;  // (m = 2^24 carries into the exponent below)
    return ((uint32_t)(127 + top) << 23) + (uint32_t)(m - (1ull << 23));
}
__host__ __device__ __forceinline__ float bw_value(long long depth) {
    const uint32_t b = bw_value_bits(depth);
    float f;
    memcpy(&f, &b, 4);
    return f;
}
// acc + a * b with the product and the sum rounded one after the other, never fused
__host__ __device__ __forceinline__ double bw_mul(double a, double b) {
#pragma clang fp contract(off)
    const double p = a * b;
    return p;
}
__host__ __device__ __forceinline__ double bw_add(double a, double b) {
#pragma clang fp contract(off)
    const double s = a + b;
    return s;
}

// first[s * n_rank + r] = the first run at or behind (strand s, rank r); first[n_str * n_rank] = n_runs
__global__ void k_bw_ranges(CovRuns runs, uint32_t n_runs, uint32_t n_rank, uint32_t n_str, uint32_t* __restrict__ first) {
    const unsigned long long n_q = (unsigned long long)n_str * n_rank;
    for (unsigned long long q = blockIdx.x * blockDim.x + threadIdx.x; q <= n_q; q += (unsigned long long)gridDim.x * blockDim.x) {
        const uint32_t s = (uint32_t)(q / n_rank), r = (uint32_t)(q % n_rank);
        uint32_t lo = 0, hi = n_runs;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            const uint32_t ms = runs.strand[mid], mr = (uint32_t)runs.chrom[mid];
            if (ms < s || (ms == s && mr < r)) lo = mid + 1; else hi = mid;
        }
        first[q] = q == n_q ? n_runs : lo;
    }
}

// err[0] = the first run (by index) that ends beyond ln[its rank]; max_depth[strand]
__global__ void k_bw_limits(CovRuns runs, uint32_t n_runs, const uint32_t* __restrict__ ln, uint32_t* __restrict__ err,
                            unsigned long long* __restrict__ max_depth) {
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < n_runs; x += gridDim.x * blockDim.x) {
        if ((unsigned long long)runs.end[x] > (unsigned long long)ln[runs.chrom[x]]) atomicMin(&err[0], x);
        atomicMax(&max_depth[runs.strand[x] ? 1 : 0], (unsigned long long)runs.depth[x]);
    }
}

// runs [r0, r1) of one file.  The bins run x opens: [bw_first_bin, its last bin]
__device__ __forceinline__ uint32_t bw_first_bin(const CovRuns& runs, uint32_t r0, uint32_t x, uint32_t R, uint32_t& last) {
    uint32_t b0 = (uint32_t)((unsigned long long)runs.start[x] / R);
    last = (uint32_t)((unsigned long long)(runs.end[x] - 1) / R);
    if (x > r0 && runs.chrom[x - 1] == runs.chrom[x] && (uint32_t)((unsigned long long)(runs.end[x - 1] - 1) / R) == b0) b0++;
    return b0;
}
__global__ void k_bw_zoom_count(CovRuns runs, uint32_t r0, uint32_t r1, uint32_t R, unsigned long long* __restrict__ count) {
    for (uint32_t x = r0 + blockIdx.x * blockDim.x + threadIdx.x; x < r1; x += gridDim.x * blockDim.x) {
        uint32_t last;
        const uint32_t b0 = bw_first_bin(runs, r0, x, R, last);
        count[x - r0] = (unsigned long long)(last + 1u - b0);
    }
}
// off = exclusive sum of count; record off[x - r0] + k is bin b0 + k, first run x
__global__ void k_bw_zoom_bins(CovRuns runs, uint32_t r0, uint32_t r1, uint32_t R, const unsigned long long* __restrict__ off,
                               uint32_t* __restrict__ rec_run, uint32_t* __restrict__ rec_bin) {
    for (uint32_t x = r0 + blockIdx.x * blockDim.x + threadIdx.x; x < r1; x += gridDim.x * blockDim.x) {
        uint32_t last;
        const uint32_t b0 = bw_first_bin(runs, r0, x, R, last);
        const unsigned long long at = off[x - r0];
        for (uint32_t j = b0; j <= last; j++) { rec_run[at + (j - b0)] = x; rec_bin[at + (j - b0)] = j; }
    }
}
// out[q] = off[first[q] - r0]: where the records of every rank start (first: k_bw_ranges' entries of this file, n of them)
__global__ void k_bw_pick(const unsigned long long* __restrict__ off, const uint32_t* __restrict__ first, uint32_t n, uint32_t r0,
                          unsigned long long* __restrict__ out) {
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) out[q] = off[first[q] - r0];
}
// ln / cid: per chromosome rank.  r1 = the end of the file's runs.
__global__ void k_bw_zoom_reduce(CovRuns runs, uint32_t r1, const uint32_t* __restrict__ rec_run, const uint32_t* __restrict__ rec_bin, uint32_t n_rec,
                                 uint32_t R, const uint32_t* __restrict__ ln, const uint32_t* __restrict__ cid, BwRec* __restrict__ out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_rec; i += gridDim.x * blockDim.x) {
        const uint32_t x = rec_run[i];
        const int32_t ch = runs.chrom[x];
        const unsigned long long b0 = (unsigned long long)rec_bin[i] * R, lim = ln[ch];
        const unsigned long long b1 = b0 + R < lim ? b0 + R : lim;
        uint32_t valid = 0;
        float vmin = 0.f, vmax = 0.f;
        double sum = 0.0, sq = 0.0;
        for (uint32_t y = x; y < r1 && runs.chrom[y] == ch && (unsigned long long)runs.start[y] < b1; y++) {
            const unsigned long long s = (unsigned long long)runs.start[y], e = (unsigned long long)runs.end[y];
            const uint32_t ov = (uint32_t)((e < b1 ? e : b1) - (s > b0 ? s : b0));
            const float vf = bw_value(runs.depth[y]);
            const double v = (double)vf;
            if (y == x) { vmin = vf; vmax = vf; }
            vmin = vf < vmin ? vf : vmin; vmax = vf > vmax ? vf : vmax;
            valid += ov;
            sum = bw_add(sum, bw_mul((double)ov, v));
            sq = bw_add(sq, bw_mul((double)ov, bw_mul(v, v)));
        }
        out[i] = BwRec{cid[ch], (uint32_t)b0, (uint32_t)b1, valid, vmin, vmax, (float)sum, (float)sq};
    }
}

__global__ void k_bw_summary(CovRuns runs, const BwBlk* __restrict__ blk, uint32_t n_blocks, BwPart* __restrict__ out) {
    for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < n_blocks; b += gridDim.x * blockDim.x) {
        const BwBlk k = blk[b];
        BwPart p{0ull, 0.0, 0.0, 0.0, 0.0};
        for (uint32_t x = k.first; x < k.first + k.count; x++) {
            const unsigned long long len = (unsigned long long)(runs.end[x] - runs.start[x]);
            const double v = (double)bw_value(runs.depth[x]);
            if (x == k.first) { p.vmin = v; p.vmax = v; }
            p.vmin = v < p.vmin ? v : p.vmin; p.vmax = v > p.vmax ? v : p.vmax;
            p.bases += len;
            p.sum = bw_add(p.sum, bw_mul((double)len, v));
            p.sq = bw_add(p.sq, bw_mul((double)len, bw_mul(v, v)));
        }
        out[b] = p;
    }
}

// Block b of blk[0 .. n_blocks) -> slots + b * slot_stride, sizes[b] = its bytes in the file, bounds[3 b ..] = chromId, start, end.
// deflate != 0: one zlib stream (0x78 0x01, one deflate block, Adler-32 big-endian); deflate == 0: the block's bytes as they are.
// slot_stride >= payload + 11 (the stored form: 2 + 5 + n + 4).  blockDim.x = MIRGE_BLOCK.
template <bool RECORDS>
__global__ void __launch_bounds__(MIRGE_BLOCK) k_bw_blocks(CovRuns runs, const BwRec* __restrict__ recs, const BwBlk* __restrict__ blk, uint32_t n_blocks,
                                                           int deflate, uint32_t slot_stride, uint8_t* __restrict__ slots, uint32_t* __restrict__ sizes,
                                                           uint32_t* __restrict__ bounds) {
    constexpr uint32_t P = RECORDS ? MIRGE_BW_MAX_SECTION * 32u : 24u + MIRGE_BW_MAX_SECTION * 12u;  // the largest payload
    __shared__ uint32_t data32[(P + 16) / 4];
    __shared__ uint32_t out32[(P + 16) / 4 + 2];
    __shared__ uint32_t head[1u << MIRGE_BAM_HASH_BITS];  // (a payload stays below 32 KiB + 1: bam_hash's upper half is never reached)
    __shared__ uint32_t seg_bits[MIRGE_BLOCK + 1];
    __shared__ uint32_t s_adler[2];
    static_assert(P <= (1u << 15), "bam_hash keeps to its first half");
    uint8_t* data = reinterpret_cast<uint8_t*>(data32);
    const uint32_t tid = threadIdx.x, nth = blockDim.x;
    for (uint32_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const BwBlk k = blk[b];
        const uint32_t cnt = k.count < MIRGE_BW_MAX_SECTION ? k.count : MIRGE_BW_MAX_SECTION;
        const uint32_t n = RECORDS ? cnt * 32u : 24u + cnt * 12u;
        // ---- the block's bytes
        if constexpr (RECORDS) {
            const uint32_t* src = reinterpret_cast<const uint32_t*>(recs + k.first);
            for (uint32_t x = tid; x < cnt * 8u; x += nth) data32[x] = src[x];
            if (tid == 0) { bounds[3 * b] = k.chrom; bounds[3 * b + 1] = recs[k.first].start; bounds[3 * b + 2] = recs[k.first + cnt - 1].end; }
        } else {
            if (tid == 0) {
                const uint32_t s = (uint32_t)runs.start[k.first], e = (uint32_t)runs.end[k.first + cnt - 1];
                data32[0] = k.chrom; data32[1] = s; data32[2] = e; data32[3] = 0u; data32[4] = 0u; data32[5] = 1u | (cnt << 16);
                bounds[3 * b] = k.chrom; bounds[3 * b + 1] = s; bounds[3 * b + 2] = e;
            }
            for (uint32_t x = tid; x < cnt; x += nth) {
                data32[6 + 3 * x] = (uint32_t)runs.start[k.first + x];
                data32[7 + 3 * x] = (uint32_t)runs.end[k.first + x];
                data32[8 + 3 * x] = bw_value_bits(runs.depth[k.first + x]);
            }
        }
        __syncthreads();
        uint8_t* dst = slots + (size_t)b * slot_stride;
        if (!deflate) {
            uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);  // (slot_stride is a multiple of 16, n of 4)
            for (uint32_t x = tid; x < n / 4; x += nth) d4[x] = data32[x];
            if (tid == 0) sizes[b] = n;
            __syncthreads();
            continue;
        }
        // ---- deflate with the fixed code, a segment per lane
        for (uint32_t x = tid; x < (1u << MIRGE_BAM_HASH_BITS); x += nth) head[x] = 0xFFFFFFFFu;
        for (uint32_t x = tid; x < (n + 16) / 4 + 1; x += nth) out32[x] = 0u;
        if (tid < 2) s_adler[tid] = 0u;
        __syncthreads();
        for (uint32_t i = tid; i + MIRGE_BAM_MIN_MATCH <= n; i += nth) atomicMin(&head[bam_hash(bam_ld32(data, i), i)], i);
        __syncthreads();
        const uint32_t seg = (n + nth - 1) / nth;
        const uint32_t s0 = tid * seg < n ? tid * seg : n, s1 = s0 + seg < n ? s0 + seg : n;
        {
            BamBits<false> cw;
            cw.start(nullptr, 0u);
            bam_parse(data, head, s0, s1, cw);
            seg_bits[tid] = cw.at;
            // Adler-32: A = 1 + sum d_i, B = n + sum (n - i) d_i (mod 65521); a lane's part stays below 2^32 (at most 128 bytes a lane)
            uint32_t a = 0u, bb = 0u;
            for (uint32_t x = s0; x < s1; x++) { a += data[x]; bb += (n - x) * data[x]; }
            if (s1 > s0) { atomicAdd(&s_adler[0], a % MIRGE_BW_ADLER); atomicAdd(&s_adler[1], bb % MIRGE_BW_ADLER); }
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
        if (!stored) {
            BamBits<true> ew;
            ew.start(out32, seg_bits[tid]);
            if (tid == 0) { ew.start(out32, 0u); ew.put(3u, 3); }  // BFINAL = 1, BTYPE = 01
            bam_parse(data, head, s0, s1, ew);
            ew.finish();
            __syncthreads();
            const uint8_t* ob = reinterpret_cast<const uint8_t*>(out32);
            for (uint32_t x = tid; x < clen; x += nth) dst[2 + x] = ob[x];
        } else {
            if (tid == 0) {
                dst[2] = 1u;  // BFINAL = 1, BTYPE = 00
                dst[3] = (uint8_t)(n & 255u); dst[4] = (uint8_t)(n >> 8);
                dst[5] = (uint8_t)(~n & 255u); dst[6] = (uint8_t)((~n >> 8) & 255u);
            }
            for (uint32_t x = tid; x < n; x += nth) dst[7 + x] = data[x];
        }
        if (tid == 0) {
            const uint32_t A = (1u + s_adler[0]) % MIRGE_BW_ADLER, B = (n % MIRGE_BW_ADLER + s_adler[1]) % MIRGE_BW_ADLER;
            dst[0] = 0x78; dst[1] = 0x01;
            uint8_t* tr = dst + 2 + clen;
            tr[0] = (uint8_t)(B >> 8); tr[1] = (uint8_t)B; tr[2] = (uint8_t)(A >> 8); tr[3] = (uint8_t)A;
            sizes[b] = clen + 6u;
        }
        __syncthreads();
    }
}
