// kernels_umi.hpp -- part of mirge_kernels.hpp: error-tolerant UMI deduplication, the "directional" network method of UMI-tools (Smith, Heger
// & Sudbery, Genome Research 2017) on the distinct UMI-tagged reads of one sample (--umi-cluster directional, mirge_umi_cluster).
//
// A node is a distinct tagged read (handle index of a one-column collapse result) with its count c.  ELIGIBLE: no N, at most 256 nt, at
// least f + b letters.  NEIGHBOURS: two eligible reads of one length that differ in exactly one letter, and that letter lies in the UMI
// region (the first f and the last b letters): the same insert, UMIs at Hamming distance 1.  Edge a -> v iff c(a) >= 2 c(v) - 1.  The
// number of breadth-first searches UMI-tools starts (nodes by descending count) is the number of strongly connected components without an
// edge from outside, and that is
//   (1) the nodes v with c(v) >= 2 that have no neighbour a with c(a) >= 2 c(v) - 1 (an equal count >= 2 is never enough, so such
//       components are single nodes), plus
//   (2) the connected components of the count-1 nodes (every neighbour of a count-1 node has an edge into it) none of whose members has a
//       neighbour of count >= 2.
// FOUNDERS: every ineligible read, every node of (1), and of every component of (2) the member that appeared first in the file.
//
// The kernels: k_umi_insert (an open-addressing table of the eligible reads, keyed by a hash of length and letters), k_umi_edges (every
// node looks its 3 (f + b) one-letter variants up: in-edge / big-neighbour / linked flags, and the count-1 nodes' first label),
// k_umi_round (minimum-label propagation over the count-1 nodes: one launch per round, until a round changes nothing), k_umi_comp_big and
// k_umi_founders.  A candidate the table gives is a neighbour only after its length and every packed word were compared, and every read is
// distinct, so a lookup has one answer whatever the hash does and wherever the inserts landed: flags are a function of the input alone.
// No LDS and no barrier: the kernels compile for the host as they are (tests/hostsim/umi_sim.cpp).
#pragma once

#define MIRGE_UMI_NG 5        // the storage groups without an N: the four templated widths and the long class (for its reads of 256 nt)
#define MIRGE_UMI_MAXLEN 256  // a longer read is a molecule of its own
#define MIRGE_UMI_MAXTAG 32   // f + b at most
#define MIRGE_UMI_NONE 0xFFFFFFFFu
#define MIRGE_UMI_EMPTY 0xFFFFFFFFFFFFFFFFull
// per-node state word
#define MIRGE_UMI_ELIG 1u      // eligible
#define MIRGE_UMI_INEDGE 2u    // c >= 2 and some neighbour a has c(a) >= 2 c - 1
#define MIRGE_UMI_HASBIG 4u    // c == 1 and some neighbour has c >= 2
#define MIRGE_UMI_LINK 8u      // c == 1 and some neighbour has c == 1: takes part in the propagation
#define MIRGE_UMI_COMPBIG 16u  // on a component's label node: some member has MIRGE_UMI_HASBIG

struct UmiGroup {
    const uint64_t* seq;     // [W][n], word-major
    const uint8_t* len;      // [n]; len16: uint16 [n] behind the same pointer (the long class)
    const uint32_t* counts;  // [n] (one sample column)
    const uint32_t* first;   // [n] raw index of the first copy
    uint32_t base, n;        // handle index of the group's first read, reads
    int32_t len16, pad;
};
struct UmiView {
    UmiGroup g[MIRGE_UMI_NG];
    int32_t front, back;
    uint32_t n_nodes, pad;  // reads of the whole set (handle indices 0 .. n_nodes - 1), ineligible ones included
    uint64_t hash_keep;     // MIRGE_TEST_UMI_HASH_BITS: the bits of the hash that are kept (all: ~0)
    uint64_t tab_mask;      // slots - 1 (a power of two, at least twice the eligible reads: a probe always ends at an empty slot)
};

__host__ __device__ __forceinline__ uint64_t umi_mix(uint64_t x) {  // splitmix64's finalizer
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// a word's share of a read's hash: the shares are XORed, so a variant's hash is the read's with one share exchanged
__host__ __device__ __forceinline__ uint64_t umi_share(uint64_t word, int w) { return umi_mix(word + 0x9E3779B97F4A7C15ull * (uint64_t)(w + 1)); }
__host__ __device__ __forceinline__ uint64_t umi_finish(const UmiView& v, uint64_t h, int len) {
    return umi_mix(h ^ ((uint64_t)len << 48)) & v.hash_keep;
}
__host__ __device__ __forceinline__ int umi_len(const UmiGroup& g, uint32_t j) {
    return g.len16 ? (int)reinterpret_cast<const uint16_t*>(g.len)[j] : (int)g.len[j];
}
__host__ __device__ __forceinline__ bool umi_eligible(const UmiView& v, int len) { return len <= MIRGE_UMI_MAXLEN && len >= v.front + v.back; }
// the group that holds handle index i, or -1 (a read with an N, or of the long class beyond its N-free group: not in the view)
__host__ __device__ __forceinline__ int umi_locate(const UmiView& v, uint32_t i, uint32_t& j) {
    for (int k = 0; k < MIRGE_UMI_NG; k++)
        if (i - v.g[k].base < v.g[k].n) { j = i - v.g[k].base; return k; }
    return -1;
}
__host__ __device__ __forceinline__ uint64_t umi_read_hash(const UmiGroup& g, uint32_t j, int len) {
    uint64_t h = 0;
    for (int w = 0; w < (len + 31) >> 5; w++) h ^= umi_share(g.seq[(size_t)w * g.n + j], w);
    return h;
}

// the read of group g that equals read j but for word `wi`, which is `word` there: its handle index, or MIRGE_UMI_NONE.  Equal lengths
// mean one storage group, so the candidates of other groups are passed over by their index alone.
__host__ __device__ __forceinline__ uint32_t umi_lookup(const UmiView& v, const uint64_t* __restrict__ tab, const UmiGroup& g, uint32_t j, int len,
                                                        int wi, uint64_t word, uint64_t h) {
    const int nw = (len + 31) >> 5;
    for (uint64_t s = h & v.tab_mask;; s = (s + 1) & v.tab_mask) {
        const uint64_t e = tab[s];
        if (e == MIRGE_UMI_EMPTY) return MIRGE_UMI_NONE;
        if ((e >> 32) != (h >> 32)) continue;
        const uint32_t k = (uint32_t)e - g.base;
        if (k >= g.n || umi_len(g, k) != len) continue;
        bool same = true;
        for (int w = 0; w < nw && same; w++) same = g.seq[(size_t)w * g.n + k] == (w == wi ? word : g.seq[(size_t)w * g.n + j]);
        if (same) return (uint32_t)e;
    }
}

// position of UMI letter k (0 .. f + b - 1) in a read of `len` letters
__host__ __device__ __forceinline__ int umi_pos(const UmiView& v, int len, int k) { return k < v.front ? k : len - v.back + (k - v.front); }

// state[i] = MIRGE_UMI_ELIG for every eligible read, which enters the table.  An entry is (upper half of the hash, handle index).
__global__ void __launch_bounds__(MIRGE_BLOCK) k_umi_insert(UmiView v, uint64_t* __restrict__ tab, uint32_t* __restrict__ state) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < v.n_nodes; i += gridDim.x * blockDim.x) {
        uint32_t j;
        const int gi = umi_locate(v, i, j);
        if (gi < 0) continue;
        const UmiGroup& g = v.g[gi];
        const int len = umi_len(g, j);
        if (!umi_eligible(v, len)) continue;
        state[i] = MIRGE_UMI_ELIG;
        const uint64_t h = umi_finish(v, umi_read_hash(g, j, len), len);
        const uint64_t e = (h & 0xFFFFFFFF00000000ull) | i;
        for (uint64_t s = h & v.tab_mask;; s = (s + 1) & v.tab_mask)
            if (atomicCAS((unsigned long long*)&tab[s], (unsigned long long)MIRGE_UMI_EMPTY, (unsigned long long)e) == MIRGE_UMI_EMPTY) break;
    }
}

// Every eligible node against its neighbours.  c >= 2: MIRGE_UMI_INEDGE; c == 1: MIRGE_UMI_HASBIG, MIRGE_UMI_LINK and the first label,
// (first index << 32) | handle index: first indices are distinct, so labels order nodes by first appearance and name the node.
// The comparison c(a) >= 2 c(v) - 1 is made in 64 bits (counts are 32-bit).
__global__ void __launch_bounds__(MIRGE_BLOCK) k_umi_edges(UmiView v, const uint64_t* __restrict__ tab, uint32_t* __restrict__ state,
                                                           uint64_t* __restrict__ label) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < v.n_nodes; i += gridDim.x * blockDim.x) {
        uint32_t j;
        const int gi = umi_locate(v, i, j);
        if (gi < 0) continue;
        const UmiGroup& g = v.g[gi];
        const int len = umi_len(g, j);
        if (!umi_eligible(v, len)) continue;
        const int64_t c = (int64_t)g.counts[j];
        const uint64_t h0 = umi_read_hash(g, j, len);
        uint32_t st = MIRGE_UMI_ELIG;
        for (int k = 0; k < v.front + v.back; k++) {
            const int p = umi_pos(v, len, k), wi = p >> 5, sh = 2 * (p & 31);
            const uint64_t mine = g.seq[(size_t)wi * g.n + j], hrest = h0 ^ umi_share(mine, wi);
            for (uint64_t x = 1; x < 4; x++) {
                const uint64_t word = mine ^ (x << sh);
                const uint32_t a = umi_lookup(v, tab, g, j, len, wi, word, umi_finish(v, hrest ^ umi_share(word, wi), len));
                if (a == MIRGE_UMI_NONE) continue;
                const int64_t ca = (int64_t)g.counts[a - g.base];
                if (c >= 2) { if (ca >= 2 * c - 1) st |= MIRGE_UMI_INEDGE; }
                else st |= ca >= 2 ? MIRGE_UMI_HASBIG : MIRGE_UMI_LINK;
            }
        }
        state[i] = st;
        label[i] = c >= 2 ? MIRGE_UMI_EMPTY : (((uint64_t)g.first[j] << 32) | i);
    }
}

// One round of minimum-label propagation over the linked count-1 nodes: a node takes the smallest label among its own, its count-1
// neighbours' and that label's node's (pointer jumping), and hands it to itself and to the node its old label names (hooking), both by
// atomicMin.  Labels only fall and always name a node of the same component, so a value another workgroup wrote in this launch, seen or
// not (a CU's L1 may hold the older one), changes how many rounds there are and nothing else: the host launches rounds until one sets
// `changed` nowhere, and in that round nothing was written, every load saw the previous launch's labels, and every node's label is
// its component's smallest.
__global__ void __launch_bounds__(MIRGE_BLOCK) k_umi_round(UmiView v, const uint64_t* __restrict__ tab, const uint32_t* __restrict__ state,
                                                           uint64_t* label, uint32_t* __restrict__ changed) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < v.n_nodes; i += gridDim.x * blockDim.x) {
        if (!(state[i] & MIRGE_UMI_LINK)) continue;
        uint32_t j;
        const int gi = umi_locate(v, i, j);
        const UmiGroup& g = v.g[gi];
        const int len = umi_len(g, j);
        const uint64_t h0 = umi_read_hash(g, j, len);
        const uint64_t old = label[i];
        uint64_t m = old;
        for (int k = 0; k < v.front + v.back; k++) {
            const int p = umi_pos(v, len, k), wi = p >> 5, sh = 2 * (p & 31);
            const uint64_t mine = g.seq[(size_t)wi * g.n + j], hrest = h0 ^ umi_share(mine, wi);
            for (uint64_t x = 1; x < 4; x++) {
                const uint64_t word = mine ^ (x << sh);
                const uint32_t a = umi_lookup(v, tab, g, j, len, wi, word, umi_finish(v, hrest ^ umi_share(word, wi), len));
                if (a == MIRGE_UMI_NONE || !(state[a] & MIRGE_UMI_LINK)) continue;
                const uint64_t la = label[a];
                m = la < m ? la : m;
            }
        }
        const uint64_t lm = label[(uint32_t)m];
        m = lm < m ? lm : m;
        if (m < old) {
            atomicMin((unsigned long long*)&label[i], (unsigned long long)m);
            atomicMin((unsigned long long*)&label[(uint32_t)old], (unsigned long long)m);
            *changed = 1u;
        }
    }
}

// a component's MIRGE_UMI_HASBIG, ORed into the state of the node its label names
__global__ void __launch_bounds__(MIRGE_BLOCK) k_umi_comp_big(UmiView v, uint32_t* __restrict__ state, const uint64_t* __restrict__ label) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < v.n_nodes; i += gridDim.x * blockDim.x) {
        const uint32_t st = state[i];
        if ((st & MIRGE_UMI_HASBIG) && label[i] != MIRGE_UMI_EMPTY) atomicOr(&state[(uint32_t)label[i]], MIRGE_UMI_COMPBIG);
    }
}

__global__ void __launch_bounds__(MIRGE_BLOCK) k_umi_founders(UmiView v, const uint32_t* __restrict__ state, const uint64_t* __restrict__ label,
                                                              uint8_t* __restrict__ founder, uint32_t* __restrict__ tally) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < v.n_nodes; i += gridDim.x * blockDim.x) {
        const uint32_t st = state[i];
        uint8_t f;
        if (!(st & MIRGE_UMI_ELIG)) f = 1;
        else if (label[i] == MIRGE_UMI_EMPTY) f = !(st & MIRGE_UMI_INEDGE);
        else f = (uint32_t)label[i] == i && !(st & MIRGE_UMI_COMPBIG);
        founder[i] = f;
        // tally[1..3]: founders, eligible reads, count-1 reads with a count-1 neighbour
        if (f) atomicAdd(&tally[1], 1u);
        if (st & MIRGE_UMI_ELIG) atomicAdd(&tally[2], 1u);
        if (st & MIRGE_UMI_LINK) atomicAdd(&tally[3], 1u);
    }
}

// (parse route) the first indices of the reads that are no founders leave the list: they sort behind every founder's
__global__ void __launch_bounds__(MIRGE_BLOCK) k_umi_mask_keys(const uint8_t* __restrict__ founder, uint32_t n, uint32_t* __restrict__ keys) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        if (!founder[i]) keys[i] = 0xFFFFFFFFu;
}
