// kernels_fq.hpp -- part of mirge_kernels.hpp: --trimmed-out (mirge3_amd/trimmed_out.py holds the specification): the records of a parsed piece,
// with the bounds the modifier chain left, as FASTQ / FASTA / one-sequence-per-line text.  The piece's output S never exists whole.
//   k_fq_measure : a lane per record: where its header, its read and its quality slice lie in the text (FqRec -- k_seq_class writes the sliced
//                  bounds back over the parser's arrays later, so the writer keeps what it measured), and the bytes the record adds to S: 0 when
//                  the read after the LAST modifier is shorter than min_len, else  H \n S \n + \n Q \n  (format 1),  H \n S \n  (2),  S \n  (3).
//                  The header line needs no array of its own: it starts one byte behind the previous record's last line end (0 for the first
//                  record) and ends one byte before the sequence line, less a '\r'.  counts[0] += written, [1] += too short, [2] |= a quality
//                  line that is not as long as its sequence line.  One 64-bit exclusive scan of bytes[] gives rec_off[n + 1].
//   k_fq_write   : output-stationary, as k_sam_write / k_cov_write: a workgroup owns a tile of S (tile_bytes, a multiple of 16, at most
//                  MIRGE_FQ_MAX_TILE), finds the records that touch it with two binary searches over rec_off, its waves take records and their
//                  lanes bytes: every record is copied clipped to the tile into LDS -- a record of 65 535 nt spans many tiles, a tile may hold
//                  thousands of one-byte records, and dropped records (no bytes) sit between kept ones -- and the tile leaves 16 bytes a lane.
// No byte of S depends on chunk or tile sizes.  No wave intrinsics: the same source runs on the host (tests/hostsim/fq_sim.cpp, MIRGE_FQ_HOSTSIM),
// a workgroup's threads then one after the other between its barriers.
#pragma once

#define MIRGE_FQ_MAX_TILE 16384

#ifdef MIRGE_FQ_HOSTSIM
#define FQ_EACH_THREAD for (threadIdx.x = 0; threadIdx.x < blockDim.x; threadIdx.x++)
#define FQ_BARRIER
#define FQ_SHARED static
#else
#define FQ_EACH_THREAD
#define FQ_BARRIER __syncthreads()
#define FQ_SHARED __shared__
#endif

// one record of the piece as the writer takes it: byte offsets into the piece's text
struct FqRec {
    int64_t hs, ss, qs;   // header line, read, quality slice
    uint32_t hlen, slen;  // bytes of the header line (format 3: 0) and of the read (= of the quality slice)
};
static_assert(sizeof(FqRec) == 32, "FqRec");

// what k_fq_measure looks at: the parser's line bounds, and the bounds after the last modifier (vstart[r * vstride + voff]; null: the line itself)
struct FqJob {
    const uint8_t* text;
    const int64_t *lstart, *lend, *qstart, *qend, *vstart, *vend;
    uint32_t n, vstride, voff;
    int32_t format;   // 1 FASTQ, 2 FASTA, 3 one sequence per line
    int32_t min_len;
};

__global__ void __launch_bounds__(MIRGE_BLOCK) k_fq_measure(FqJob j, FqRec* __restrict__ recs, unsigned long long* __restrict__ bytes,
                                                            unsigned long long* __restrict__ counts) {
    FQ_SHARED uint32_t s_cnt[3];
    FQ_EACH_THREAD { if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0u; }
    FQ_BARRIER;
    FQ_EACH_THREAD {
        for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < j.n; r += gridDim.x * blockDim.x) {
            const int64_t ls = j.lstart[r];
            int64_t le = j.lend[r];
            if (le > ls && j.text[le - 1] == 13) le--;
            FqRec k;
            k.hs = 0; k.hlen = 0; k.qs = 0;
            if (j.format != 3) {
                const int64_t hs = r == 0 ? 0 : (j.format == 1 ? j.qend[r - 1] : j.lend[r - 1]) + 1;
                int64_t he = ls - 1;  // (the header's line end)
                if (he > hs && j.text[he - 1] == 13) he--;
                k.hs = hs;
                k.hlen = (uint32_t)(he > hs ? he - hs : 0);
            }
            int64_t ts = ls, te = le;
            if (j.vstart) { ts = j.vstart[(size_t)r * j.vstride + j.voff]; te = j.vend[(size_t)r * j.vstride + j.voff]; }
            if (ts < ls) ts = ls;  // (never outside the line, whatever the bounds say)
            if (te > le) te = le;
            if (te < ts) te = ts;
            k.ss = ts; k.slen = (uint32_t)(te - ts);
            if (j.format == 1) {
                const int64_t qs = j.qstart[r];
                int64_t qe = j.qend[r];
                if (qe > qs && j.text[qe - 1] == 13) qe--;
                if (qe - qs != le - ls) atomicAdd(&s_cnt[2], 1u);
                k.qs = qs + (ts - ls);
            }
            unsigned long long b = 0;
            if ((int64_t)k.slen >= (int64_t)j.min_len) {
                b = j.format == 1 ? (unsigned long long)k.hlen + 2ull * k.slen + 5ull : (j.format == 2 ? (unsigned long long)k.hlen + k.slen + 2ull : k.slen + 1ull);
                atomicAdd(&s_cnt[0], 1u);
            } else {
                atomicAdd(&s_cnt[1], 1u);
            }
            recs[r] = k;
            bytes[r] = b;
        }
    }
    FQ_BARRIER;
    FQ_EACH_THREAD {
        if (threadIdx.x < 3 && s_cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
    }
}

// byte x of a written record
__device__ __forceinline__ uint8_t fq_byte(const uint8_t* __restrict__ text, const FqRec& k, int32_t format, unsigned long long x) {
    if (format != 3) {
        if (x < k.hlen) return text[k.hs + (int64_t)x];
        x -= k.hlen;
        if (x == 0) return (uint8_t)'\n';
        x -= 1;
    }
    if (x < k.slen) return text[k.ss + (int64_t)x];
    x -= k.slen;
    if (format != 1) return (uint8_t)'\n';
    if (x < 3) return x == 1 ? (uint8_t)'+' : (uint8_t)'\n';
    x -= 3;
    if (x < k.slen) return text[k.qs + (int64_t)x];
    return (uint8_t)'\n';
}

// S[chunk_start, chunk_start + chunk_bytes) -> out[0 .. chunk_bytes) (out 16-byte aligned); rec_off[n + 1] = exclusive scan of k_fq_measure's bytes
__global__ void __launch_bounds__(MIRGE_BLOCK) k_fq_write(const uint8_t* __restrict__ text, const FqRec* __restrict__ recs,
                                                          const unsigned long long* __restrict__ rec_off, uint32_t n, int32_t format,
                                                          unsigned long long chunk_start, uint32_t chunk_bytes, uint32_t tile_bytes,
                                                          uint8_t* __restrict__ out) {
    FQ_SHARED uint4 tile16[MIRGE_FQ_MAX_TILE / 16];
    uint8_t* const tile = reinterpret_cast<uint8_t*>(tile16);
    if (tile_bytes > MIRGE_FQ_MAX_TILE || tile_bytes < 16u || (tile_bytes & 15u)) return;  // (uniform: the launch is the host's mistake)
    for (uint32_t tb = blockIdx.x; (unsigned long long)tb * tile_bytes < chunk_bytes; tb += gridDim.x) {
        const uint32_t in_chunk = tb * tile_bytes;
        const uint32_t tile_len = chunk_bytes - in_chunk < tile_bytes ? chunk_bytes - in_chunk : tile_bytes;
        const unsigned long long tile_start = chunk_start + in_chunk, tile_end = tile_start + tile_len;
        // r0: the first record that ends behind the tile's start; r1: the first record that starts at or behind the tile's end
        uint32_t r0, r1;
        {
            uint32_t lo = 0, hi = n;
            while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (rec_off[mid + 1] <= tile_start) lo = mid + 1; else hi = mid; }
            r0 = lo;
            hi = n;
            while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (rec_off[mid] < tile_end) lo = mid + 1; else hi = mid; }
            r1 = lo;
        }
        FQ_EACH_THREAD {
            const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, n_waves = (blockDim.x + 63u) >> 6;
            for (uint32_t r = r0 + wave; r < r1; r += n_waves) {
                const unsigned long long a = rec_off[r], b = rec_off[r + 1];
                if (a == b) continue;  // a dropped record
                const unsigned long long lo = a > tile_start ? a : tile_start, hi = b < tile_end ? b : tile_end;
                const FqRec k = recs[r];
                for (unsigned long long p = lo + lane; p < hi; p += 64u) tile[(uint32_t)(p - tile_start)] = fq_byte(text, k, format, p - a);
            }
        }
        FQ_BARRIER;
        FQ_EACH_THREAD {
            uint4* dst = reinterpret_cast<uint4*>(out + in_chunk);
            for (uint32_t x = threadIdx.x; x < tile_len / 16u; x += blockDim.x) dst[x] = tile16[x];
            for (uint32_t x = (tile_len & ~15u) + threadIdx.x; x < tile_len; x += blockDim.x) out[in_chunk + x] = tile[x];
        }
        FQ_BARRIER;
    }
}
