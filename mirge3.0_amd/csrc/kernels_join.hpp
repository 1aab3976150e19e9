// kernels_join.hpp -- part of mirge_kernels.hpp: k_join, k_member_list (k_tally: kernels_tally.hpp).
#pragma once
// ------------------------------------------------------------------------------------------
// k_join: count join (summary.py:686-698,749-752): class_sums[pass][s] += counts[i][s],
// exact/iso[ref][s] += counts[i][s] for the two miRNA passes.  Class sums are accumulated in LDS
// per workgroup and flushed with one atomic per (pass, sample) cell.
// ------------------------------------------------------------------------------------------
#define MIRGE_JOIN_LDS 2048
__global__ void k_join(const int8_t* __restrict__ res_pass, const int32_t* __restrict__ res_ref,
                       const uint32_t* __restrict__ counts, uint32_t n, int32_t S, int32_t n_pass,
                       int32_t exact_pass, int32_t iso_pass, unsigned long long* __restrict__ class_sums,
                       unsigned long long* __restrict__ exact, unsigned long long* __restrict__ iso) {
    __shared__ unsigned long long acc[MIRGE_JOIN_LDS];
    const int cells = n_pass * S;
    const bool use_lds = cells <= MIRGE_JOIN_LDS;
    if (use_lds) {
        for (int c = threadIdx.x; c < cells; c += blockDim.x) acc[c] = 0ull;
        __syncthreads();
    }
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int p = res_pass[i];
        if (p < 0) continue;
        const int32_t ref = res_ref[i];
        for (int32_t s = 0; s < S; s++) {
            const unsigned long long c = counts[(size_t)i * S + s];
            if (!c) continue;
            if (use_lds) atomicAdd(&acc[p * S + s], c);
            else atomicAdd(&class_sums[p * S + s], c);
            if (p == exact_pass) atomicAdd(&exact[(size_t)ref * S + s], c);
            else if (p == iso_pass) atomicAdd(&iso[(size_t)ref * S + s], c);
        }
    }
    if (use_lds) {
        __syncthreads();
        for (int c = threadIdx.x; c < cells; c += blockDim.x)
            if (acc[c]) atomicAdd(&class_sums[c], acc[c]);
    }
}

// the small read groups of a result in ONE launch (each its own launch was 4-5 us of a step's tail, four times)
// The reference of a miRNA read (exact_pass / iso_pass: the only reads whose reference the tables need) comes from its POSITION: one
// granule entry of that pass's library (ResolveTable's row, handed over by value: `mi[0]` exact_pass, `mi[1]` iso_pass) through
// resolve_entry -- the device function k_resolve answers with, so the same reference by construction.  The miRNA library's granule
// table is a few tens of KB and stays in cache; the join then needs nothing of k_resolve, whose look-ups for every OTHER annotated
// read (one random granule entry each, out of tables as large as the mRNA library's) run behind the join (native_join.hpp).
// from_pos == 0: the references are read from `ref` (a result whose positions or granule tables this context cannot vouch for).
struct JoinResolveRow { const uint32_t* ref_start; const uint32_t* coarse; uint32_t n_refs; };
struct JoinGroups {
    const int8_t* pass[MIRGE_NCLS];
    const int32_t* ref[MIRGE_NCLS];
    const uint32_t* pos[MIRGE_NCLS];
    const uint32_t* counts[MIRGE_NCLS];
    uint32_t start[MIRGE_NCLS + 1];  // group k holds the items [start[k], start[k + 1]) of the launch
    int32_t n_groups;
    int32_t from_pos;
    JoinResolveRow mi[2];
};
__device__ __forceinline__ PairU32 join_granule(const JoinResolveRow& t, uint32_t g) {
    return load_pair32((gptr_u32)t.coarse + 2 * (size_t)(g >> MIRGE_COARSE_SHIFT));
}
__device__ __forceinline__ uint32_t join_ref_at(const JoinResolveRow& t, const PairU32 e, uint32_t g) {
    int32_t ref, off;
    resolve_entry(e, t.ref_start, t.n_refs, g, ref, off);
    return (uint32_t)ref;
}
// the reference of read i of a group, annotated by pass p (one of the two miRNA passes)
__device__ __forceinline__ uint32_t join_ref(const JoinGroups& gs, bool is_iso, const int32_t* gr, const uint32_t* gq, uint32_t i) {
    if (!gs.from_pos) return (uint32_t)gr[i];
    const JoinResolveRow t = is_iso ? gs.mi[1] : gs.mi[0];
    const uint32_t g = gq[i];
    return join_ref_at(t, join_granule(t, g), g);
}
__global__ void k_join_multi(JoinGroups gs, int32_t S, int32_t n_pass, int32_t exact_pass, int32_t iso_pass,
                             unsigned long long* __restrict__ class_sums, unsigned long long* __restrict__ exact,
                             unsigned long long* __restrict__ iso) {
    __shared__ unsigned long long acc[MIRGE_JOIN_LDS];
    const int cells = n_pass * S;
    const bool use_lds = cells <= MIRGE_JOIN_LDS;
    if (use_lds) {
        for (int c = threadIdx.x; c < cells; c += blockDim.x) acc[c] = 0ull;
        __syncthreads();
    }
    const uint32_t total = gs.start[gs.n_groups];
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
        int k = 0;
#pragma unroll
        for (int q = 1; q < MIRGE_NCLS; q++) if (q < gs.n_groups && t >= gs.start[q]) k = q;
        const uint32_t i = t - gs.start[k];
        const int8_t* gp = nullptr; const int32_t* gr = nullptr; const uint32_t* gq = nullptr; const uint32_t* gc = nullptr;
#pragma unroll
        for (int q = 0; q < MIRGE_NCLS; q++) if (q == k) { gp = gs.pass[q]; gr = gs.ref[q]; gq = gs.pos[q]; gc = gs.counts[q]; }
        const int p = gp[i];
        if (p < 0) continue;
        const bool mirna = p == exact_pass || p == iso_pass;
        const uint32_t ref = mirna ? join_ref(gs, p != exact_pass, gr, gq, i) : 0u;
        for (int32_t s = 0; s < S; s++) {
            const unsigned long long c = gc[(size_t)i * S + s];
            if (!c) continue;
            if (use_lds) atomicAdd(&acc[p * S + s], c);
            else atomicAdd(&class_sums[p * S + s], c);
            if (p == exact_pass) atomicAdd(&exact[(size_t)ref * S + s], c);
            else if (p == iso_pass) atomicAdd(&iso[(size_t)ref * S + s], c);
        }
    }
    if (use_lds) {
        __syncthreads();
        for (int c = threadIdx.x; c < cells; c += blockDim.x)
            if (acc[c]) atomicAdd(&class_sums[c], acc[c]);
    }
}

// k_join_rows / k_join_reduce (round 3): the same sums without a global atomic per read.  k_join's exact / isomiR tables take
// one device-scope atomic per miRNA read -- 2.5 M of them on 2.9 k hot addresses for a 10 M-read sample, 74 us at the
// chip's ~20-30 G scattered atomics/s: the last kernel of the step and 5 % of it.  Here a 1024-thread workgroup keeps ALL
// tables (class sums + exact + isomiR, 64-bit cells) in LDS while it walks its share of the reads, writes them out as
// one plain row of partial[workgroup][cell], and a second small kernel sums the rows column-wise into the ctx's tables.
// Used when the tables fit 48 KiB of LDS (one sample: up to ~3 000 miRNA references); otherwise k_join.
#define MIRGE_JOIN_ROWS_THREADS 1024
#define MIRGE_JOIN_ROWS_CELLS 6144  // 64-bit LDS cells
__global__ void __launch_bounds__(MIRGE_JOIN_ROWS_THREADS)
k_join_rows(JoinGroups gs, int32_t S, int32_t n_pass, int32_t exact_pass, int32_t iso_pass, uint32_t n_tab,
            unsigned long long* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long j_acc[];  // [n_pass * S] | [n_tab] exact | [n_tab] iso
    const uint32_t n_cls = (uint32_t)(n_pass * S), W = n_cls + 2 * n_tab;
    for (uint32_t c = threadIdx.x; c < W; c += blockDim.x) j_acc[c] = 0ull;
    __syncthreads();
    const uint32_t total = gs.start[gs.n_groups];
    if (gs.n_groups == 1 && S == 1) {
        // the bulk group of one sample: four reads per thread and sweep, their loads issued together (16 dependent
        // pass -> reference -> count walks per thread before: 23 us for 38 MB)
        const int8_t* __restrict__ gp = gs.pass[0]; const int32_t* __restrict__ gr = gs.ref[0]; const uint32_t* __restrict__ gc = gs.counts[0];
        const uint32_t* __restrict__ gq = gs.pos[0];
        const bool from_pos = gs.from_pos != 0;
        const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;  // 64-bit: t0 + 3 * stride passes 2^32 for a group near that size
        for (uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t0 < total; t0 += 4 * stride) {
            int p[4]; uint32_t r[4]; unsigned long long c[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint64_t i = t0 + (uint64_t)u * stride;
                const bool in = i < total;
                p[u] = in ? (int)gp[i] : -1;
                r[u] = in ? (from_pos ? gq[i] : (uint32_t)gr[i]) : 0u;  // the position, or the reference itself
                c[u] = in ? (unsigned long long)gc[i] : 0ull;
            }
            if (from_pos) {  // the granule entries of the up to four miRNA reads, their loads issued together
                PairU32 e[4]; bool m[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    m[u] = p[u] >= 0 && (p[u] == exact_pass || p[u] == iso_pass);
                    e[u] = m[u] ? join_granule(p[u] == exact_pass ? gs.mi[0] : gs.mi[1], r[u]) : PairU32{0u, 0u};
                }
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (m[u]) r[u] = join_ref_at(p[u] == exact_pass ? gs.mi[0] : gs.mi[1], e[u], r[u]);
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (p[u] < 0 || !c[u]) continue;
                atomicAdd(&j_acc[p[u]], c[u]);
                if (p[u] == exact_pass) atomicAdd(&j_acc[n_cls + r[u]], c[u]);
                else if (p[u] == iso_pass) atomicAdd(&j_acc[n_cls + n_tab + r[u]], c[u]);
            }
        }
    } else
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
        int k = 0;  // one group (the bulk) or the few small ones, back to back
#pragma unroll
        for (int q = 1; q < MIRGE_NCLS; q++) if (q < gs.n_groups && t >= gs.start[q]) k = q;
        const int8_t* gp = gs.pass[0]; const int32_t* gr = gs.ref[0]; const uint32_t* gq = gs.pos[0]; const uint32_t* gc = gs.counts[0];
#pragma unroll
        for (int q = 1; q < MIRGE_NCLS; q++) if (q == k) { gp = gs.pass[q]; gr = gs.ref[q]; gq = gs.pos[q]; gc = gs.counts[q]; }
        const uint32_t i = t - gs.start[k];
        const int p = gp[i];
        if (p < 0) continue;
        const bool mirna = p == exact_pass || p == iso_pass;
        const uint32_t ref = mirna ? join_ref(gs, p != exact_pass, gr, gq, i) : 0u;
        for (int32_t s = 0; s < S; s++) {
            const unsigned long long c = gc[(size_t)i * S + s];
            if (!c) continue;
            atomicAdd(&j_acc[p * S + s], c);
            if (p == exact_pass) atomicAdd(&j_acc[n_cls + (size_t)ref * S + s], c);
            else if (p == iso_pass) atomicAdd(&j_acc[n_cls + n_tab + (size_t)ref * S + s], c);
        }
    }
    __syncthreads();
    unsigned long long* row = partial + (size_t)blockIdx.x * W;
    for (uint32_t c = threadIdx.x; c < W; c += blockDim.x) row[c] = j_acc[c];
}
// tables[c] += sum over rows of partial[row][c].  A workgroup owns 64 consecutive cells; its 16 waves take every 16th row each
// (a wave's load of a row's 64 cells is one coalesced 512-byte access), then the waves' sums are added up through LDS.
// (One thread per cell walking all 256 rows by itself took 46 us for 5.9 k cells: a chain of 256 dependent-latency loads.)
// host_out != nullptr (page-locked host memory): the sums -- plus whatever `tables` already holds -- are written THERE and
// `tables` stays as it is: no device-to-host copy behind the kernel, and tables that were zero need no clearing afterwards.
__global__ void __launch_bounds__(1024)
k_join_reduce(const unsigned long long* __restrict__ partial, uint32_t rows, uint32_t W, unsigned long long* __restrict__ tables,
              unsigned long long* __restrict__ host_out) {
    __shared__ unsigned long long s_part[16][64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t c = blockIdx.x * 64 + lane;
    unsigned long long sum = 0ull;
    if (c < W)
        for (uint32_t r = wave; r < rows; r += 16) sum += partial[(size_t)r * W + c];
    s_part[wave][lane] = sum;
    __syncthreads();
    if (wave == 0 && c < W) {
        unsigned long long tot = 0ull;
#pragma unroll
        for (int w = 0; w < 16; w++) tot += s_part[w][lane];
        if (host_out) host_out[c] = tables[c] + tot;
        else if (tot) tables[c] += tot;
    }
}

// out[orig[j] or base+j] = in[j]
template <typename T>
__global__ void k_scatter_out(const T* __restrict__ in, uint32_t n, uint32_t base,
                              const uint32_t* __restrict__ orig, T* __restrict__ out) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x)
        out[orig ? orig[j] : base + j] = in[j];
}


// The reads a heavy per-read kernel works on, compacted.  k_tally and k_isotype run ~2 000 and more instructions of loops
// per read whose trip counts differ, on the minority of a sample's unique reads that are miRNA rows: a wave costs what
// its busiest lane costs, and skipping the other reads lane by lane left k_tally at 10 % lane utilisation with 66 % of its
// time in VALU issue.  Workgroup b compacts the reads [b * chunk, (b + 1) * chunk) that satisfy `pred` in place:
// list[b * chunk ...], n_list[b] of them -- no global cursor (one returning atomic per 256 reads on one address cost
// more than the work it saved); the consumer runs one workgroup per chunk.
// (TallyMember, k_tally's predicate: kernels_tally.hpp)
struct IsoMember {  // a miRNA row of the GFF: annotated by one of the two miRNA passes and given an output slot by the host
    const int8_t* res_pass; int32_t exact_pass, iso_pass; const uint32_t* orig; uint32_t base; const int32_t* slot_of_read;
    __device__ __forceinline__ bool operator()(uint32_t i) const {
        const int p = res_pass[i];
        return (p == exact_pass || p == iso_pass) && slot_of_read[orig ? orig[i] : base + i] >= 0;
    }
};

template <class Pred, int BLOCK>
__global__ void k_member_list(uint32_t n, uint32_t chunk, Pred pred, uint32_t* __restrict__ list, uint32_t* __restrict__ n_list) {
    __shared__ uint32_t s_wave[BLOCK / 64 + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t lo = blockIdx.x * chunk, hi = min(n, lo + chunk);
    uint32_t run = 0;
    for (uint32_t i0 = lo; i0 < hi; i0 += BLOCK) {
        const uint32_t i = i0 + threadIdx.x;
        const bool member = i < hi && pred(i);
        const unsigned long long bal = __ballot(member);
        if (lane == 0) s_wave[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t before = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < BLOCK / 64; w++) { const uint32_t c = s_wave[w]; if (w < wave) before += c; tot += c; }
        if (member) list[lo + run + before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = i;
        run += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) n_list[blockIdx.x] = run;
}
