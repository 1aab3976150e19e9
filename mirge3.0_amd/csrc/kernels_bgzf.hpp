// kernels_bgzf.hpp -- part of mirge_kernels.hpp: any byte stream as BGZF members (`--bgzf-out`: the text of `--sam-out` and `--coverage`;
// mirge_bgzf_write: bytes from the host).  The stream lies in a device buffer; nothing here knows what the bytes are.
//   k_bgzf_text : a workgroup owns one block (block_bytes, at most MIRGE_BAM_MAX_BLOCK) of the buffer: it loads the block into LDS --
//                 16 bytes a lane where the source is aligned, single bytes in front of and behind that stretch, never a byte outside
//                 the block -- and deflates it where it lies with the stage of kernels_bam.hpp's deflate == 2: the first-position hash,
//                 every thread's greedy parse of its segment into per-wave histograms, the CRC-32 from per-segment partials, both
//                 Huffman trees (bam_huff_lengths2), the two candidate headers, and the form: dynamic if and only if its bytes are
//                 strictly fewer than those of the better of stored and fixed.  So a member is never longer than n + 31 bytes (18 of
//                 header, 5 + n stored, 8 of trailer).  The member goes into the block's slot, its size into sizes[b]; k_bam_compact
//                 closes the gaps as it does for BAM.
// The helpers that take pointers into the block's BamDynamic are instantiated a third time (<2>: kernels_bam.hpp says why the
// tight route has copies of its own), and bgzf_dyn_bits is this kernel's copy of bam_dyn_bits: k_bam_blocks_dynamic stays the only
// caller of its own.  No wave intrinsics: the same source runs on the host (tests/hostsim/bgzf_sim.cpp).
#pragma once

#define MIRGE_BGZF_OWN 2

__device__ __forceinline__ uint32_t bgzf_dyn_bits(const BamDynamic& y, const uint8_t* d, const uint8_t* tok, uint32_t s0, uint32_t s1) {
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

// blocks first_block .. first_block + n_blocks - 1 of text[0 .. text_bytes): block b -> one BGZF member at out + b * slot_stride
// (slot_stride >= block_bytes + 31), sizes[b] = its bytes.  Every block asked for starts inside the text.
__global__ void __launch_bounds__(MIRGE_BLOCK) k_bgzf_text(const uint8_t* __restrict__ text, unsigned long long text_bytes, unsigned long long first_block,
                                                           uint32_t n_blocks, uint32_t block_bytes, uint32_t slot_stride, uint8_t* __restrict__ out,
                                                           uint32_t* __restrict__ sizes) {
    __shared__ uint4 data16[(MIRGE_BAM_MAX_BLOCK + 256) / 16];
    __shared__ uint32_t out32[(MIRGE_BAM_MAX_BLOCK + 256) / 4];
    __shared__ uint32_t head[2u << MIRGE_BAM_HASH_BITS];
    __shared__ uint32_t crc_table[256];
    __shared__ uint32_t seg_bits[MIRGE_BLOCK + 1];
    __shared__ uint32_t s_crc;
    __shared__ BamDynamic dyn;
    const uint32_t tid = threadIdx.x, nth = blockDim.x;
    for (uint32_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const unsigned long long ustart = (first_block + b) * (unsigned long long)block_bytes;
        if (ustart >= text_bytes || block_bytes > MIRGE_BAM_MAX_BLOCK) { if (tid == 0) sizes[b] = 0u; continue; }  // (uniform: no barrier is skipped by a part of the group)
        const uint32_t n = (uint32_t)(text_bytes - ustart < block_bytes ? text_bytes - ustart : block_bytes);
        // ---- the block's bytes: LDS byte a + x holds text byte ustart + x, a = the source's offset in its 16 bytes
        const uint8_t* src = text + ustart;
        const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15u);
        uint8_t* data = reinterpret_cast<uint8_t*>(data16) + a;
        const uint32_t lead = ((16u - a) & 15u) < n ? ((16u - a) & 15u) : n, wide = (n - lead) / 16u;
        if (tid < lead) data[tid] = src[tid];
        {
            const uint4* s16 = reinterpret_cast<const uint4*>(src + lead);
            uint4* d16 = reinterpret_cast<uint4*>(data + lead);
            for (uint32_t x = tid; x < wide; x += nth) d16[x] = s16[x];
        }
        for (uint32_t x = lead + wide * 16u + tid; x < n; x += nth) data[x] = src[x];
        // ---- deflate
        for (uint32_t x = tid; x < (2u << MIRGE_BAM_HASH_BITS); x += nth) head[x] = 0xFFFFFFFFu;
        for (uint32_t x = tid; x < (n + 16) / 4 + 1; x += nth) out32[x] = 0u;
        for (uint32_t x = tid; x < 256u; x += nth) {
            uint32_t c = x;
            for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            crc_table[x] = c;
        }
        if (tid == 0) s_crc = 0u;
        for (uint32_t x = tid; x < MIRGE_BAM_HIST_COPIES * MIRGE_BAM_HUFF_MAX; x += nth) (&dyn.hist_ll[0][0])[x] = 0u;
        for (uint32_t x = tid; x < MIRGE_BAM_HIST_COPIES * 32u; x += nth) (&dyn.hist_d[0][0])[x] = 0u;
        __syncthreads();
        for (uint32_t i = tid; i + MIRGE_BAM_MIN_MATCH <= n; i += nth) atomicMin(&head[bam_hash(bam_ld32(data, i), i)], i);
        __syncthreads();
        const uint32_t seg = (n + nth - 1) / nth;
        const uint32_t s0 = tid * seg < n ? tid * seg : n, s1 = s0 + seg < n ? s0 + seg : n;
        {
            const uint32_t copy = (tid >> 6) % MIRGE_BAM_HIST_COPIES;
            BamCount cw{0u, s0, dyn.hist_ll[copy], dyn.hist_d[copy], reinterpret_cast<uint8_t*>(out32)};
            bam_parse(data, head, s0, s1, cw);
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
        bool stored = (end_bit + 7u) / 8u >= n + 5u;
        uint32_t clen = stored ? n + 5u : (end_bit + 7u) / 8u;
        // ---- the block's own code: its lengths, the header, every segment's bits
        for (uint32_t x = tid; x < MIRGE_BAM_HUFF_MAX; x += nth)
            dyn.hist_ll[0][x] += dyn.hist_ll[1][x] + dyn.hist_ll[2][x] + dyn.hist_ll[3][x] + (x == 256u ? 1u : 0u);  // (the end-of-block code: once)
        for (uint32_t x = tid; x < 32u; x += nth) dyn.hist_d[0][x] += dyn.hist_d[1][x] + dyn.hist_d[2][x] + dyn.hist_d[3][x];
        __syncthreads();
        bam_huff_lengths2<MIRGE_BGZF_OWN>(dyn.hist_ll[0], MIRGE_BAM_NLL, dyn.len_ll, dyn.work[0], dyn.hist_d[0], MIRGE_BAM_ND, dyn.len_d, dyn.work[1], 15u, tid, nth);
        dyn.seg[tid] = bgzf_dyn_bits(dyn, data, reinterpret_cast<const uint8_t*>(out32), s0, s1);
        if (tid == 0) bam_dyn_header_tokens<MIRGE_BGZF_OWN>(dyn);
        __syncthreads();
        bam_huff_lengths2<MIRGE_BGZF_OWN>(dyn.cnt_cl[0], MIRGE_BAM_NCL, dyn.len_cl[0], dyn.work[0], dyn.cnt_cl[1], MIRGE_BAM_NCL, dyn.len_cl[1], dyn.work[1], 7u, tid, nth);
        if (tid == 0) {  // exclusive sum of the segments' bits behind the header's
            bam_dyn_header_choice<MIRGE_BGZF_OWN>(dyn);
            uint32_t run = dyn.header_bits;
            for (uint32_t x = 0; x < nth; x++) { const uint32_t v = dyn.seg[x]; dyn.seg[x] = run; run += v; }
            dyn.seg[nth] = run + dyn.len_ll[256];
        }
        __syncthreads();
        const bool dynamic = (dyn.seg[nth] + 7u) / 8u < clen;
        if (dynamic) { clen = (dyn.seg[nth] + 7u) / 8u; stored = false; }
        for (uint32_t x = tid; x < (n + 16) / 4 + 1; x += nth) out32[x] = 0u;  // (the staged matches)
        if (dynamic) {
            bam_huff_codes(dyn.len_ll, MIRGE_BAM_NLL, dyn.code_ll, tid, nth);
            bam_huff_codes(dyn.len_d, MIRGE_BAM_ND, dyn.code_d, tid, nth);
            bam_huff_codes(dyn.len_cl[dyn.plain], MIRGE_BAM_NCL, dyn.code_cl, tid, nth);
        }
        __syncthreads();
        uint8_t* dst = out + (size_t)b * slot_stride;
        if (!stored) {
            if (dynamic) {
                BamDynBits ew;
                ew.ll = dyn.code_ll; ew.dd = dyn.code_d;
                ew.b.start(out32, dyn.seg[tid]);
                if (tid == 0) { ew.b.start(out32, 0u); bam_dyn_put_header<MIRGE_BGZF_OWN>(dyn, ew.b); }
                bam_parse(data, head, s0, s1, ew);
                if (tid == nth - 1u) bam_put_code(ew.b, dyn.code_ll[256]);  // (every segment behind the block's end is empty: the last thread ends the stream)
                ew.b.finish();
            } else {
                BamBits<true> ew;
                ew.start(out32, seg_bits[tid]);
                if (tid == 0) { ew.start(out32, 0u); ew.put(3u, 3); }  // BFINAL = 1, BTYPE = 01
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
