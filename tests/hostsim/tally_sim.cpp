// tally_sim.cpp -- csrc/kernels_tally.hpp compiled for the HOST (tests/test_tally_hostsim.py): the same k_tally source and the same
// TallyMember predicate, every thread of every workgroup one after the other (k_tally has no barrier; its atomics are plain adds here).
// What the runtime (csrc/native_join.hpp, mirge_variant_tally) does around the kernel is restated: the canonical sequences packed
// into one word each with the same two refusals, the reads in width groups (<= 31 nt: one word, 32..64 nt: two words, each with and
// without an N mask), outputs preset to state -1 / diag 0, and the member predicate alone over the reads of more than 64 nt.
// k_member_list compacts with __ballot / __syncthreads; here the chunked list it produces (list[b * chunk + k], n_list[b]) is
// filled by a loop over the predicate.  (pass, ref) per read come from the caller: no cascade runs here.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __restrict__
struct D3 { unsigned x; };
static D3 threadIdx, blockIdx, blockDim, gridDim;
template <class T> T atomicAdd(T* p, T v) { T o = *p; *p += v; return o; }
using std::max;
using std::min;
#include "../../mirge3.0_amd/csrc/mirge_core.hpp"
#include "../../mirge3.0_amd/csrc/mirge_libbuild.hpp"  // mirge_base_code
template <int W>
struct GroupView {  // as in csrc/mirge_kernels.hpp
    const uint64_t* seq;    // [W][n]
    const uint8_t* len;     // [n]
    const uint64_t* nmask;  // [W][n] or nullptr
    uint32_t n;
};
#include "../../mirge3.0_amd/csrc/kernels_tally.hpp"

template <class F> static void launch(unsigned grid, unsigned block, F f) {
    gridDim.x = grid; blockDim.x = block;
    for (unsigned b = 0; b < grid; b++)
        for (unsigned t = 0; t < block; t++) { blockIdx.x = b; threadIdx.x = t; f(); }
}

struct SimGroup {
    int W = 1;
    bool has_n = false;
    std::vector<uint32_t> read;  // index of the caller's read
    std::vector<uint64_t> seq, nm;
    std::vector<uint8_t> len;
    std::vector<int8_t> pass;
    std::vector<int32_t> ref;
    std::vector<uint32_t> counts;
    uint32_t base = 0;
};

// -> 0, or the runtime's error code (-6: a canonical sequence of more than 32 nt, -7: one with another character).
// diag / state / fam_tables / census as mirge_variant_tally returns them, diag and state in the caller's read order;
// wide_members: reads of more than 64 nt that satisfy the member predicate (the runtime refuses the call when there is one);
// n_chunks[4]: member-list chunks of the four groups (one word, two words, one word with N, two words with N).
extern "C" int sim_tally(const char* reads, const int64_t* roff, int64_t n, const int8_t* pass, const int32_t* ref, const uint32_t* counts,
                         int32_t S, int32_t exact_pass, int32_t iso_pass, const int32_t* fam_of_ref, const char* target_ascii,
                         const int64_t* target_off, int64_t n_fam, const uint8_t* retained, const double* freq, uint32_t chunk,
                         uint32_t block, int64_t* fam_tables, int64_t* census, int8_t* diag_out, int8_t* state_out, int64_t* wide_members,
                         int32_t* n_chunks) {
    std::vector<uint64_t> tb((size_t)std::max<int64_t>(n_fam, 1), 0ull);
    std::vector<uint8_t> tl((size_t)std::max<int64_t>(n_fam, 1), 0);
    for (int64_t f = 0; f < n_fam; f++) {
        const int64_t L = target_off[f + 1] - target_off[f];
        if (L < 0 || L > MIRGE_TALLY_MAXPOS) return -6;
        for (int64_t k = 0; k < L; k++) {
            const int code = mirge_base_code(target_ascii[target_off[f] + k]);
            if (code < 0) return -7;
            tb[(size_t)f] |= (uint64_t)code << (2 * k);
        }
        tl[(size_t)f] = (uint8_t)L;
    }
    // ---- the reads in their groups; handle index = group base + j
    SimGroup G[4];
    for (int k = 0; k < 4; k++) { G[k].W = 1 + (k & 1); G[k].has_n = k >= 2; }
    std::vector<uint32_t> wide;
    std::vector<int> cls((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const int64_t L = roff[i + 1] - roff[i];
        if (L < 1) return -1;
        bool has_n = false;
        for (int64_t p = 0; p < L; p++) has_n |= mirge_base_code(reads[roff[i] + p]) < 0;
        cls[(size_t)i] = L > 64 ? -1 : (L <= 31 ? 0 : 1) + (has_n ? 2 : 0);
        if (cls[(size_t)i] < 0) wide.push_back((uint32_t)i); else G[cls[(size_t)i]].read.push_back((uint32_t)i);
    }
    std::vector<uint32_t> handle((size_t)n, 0);
    uint32_t base = 0;
    for (auto& g : G) {
        const size_t gn = g.read.size();
        g.base = base; base += (uint32_t)gn;
        g.seq.assign((size_t)g.W * gn + 1, 0ull); g.nm.assign((size_t)g.W * gn + 1, 0ull);
        g.len.assign(gn + 1, 0); g.pass.assign(gn + 1, -1); g.ref.assign(gn + 1, -1); g.counts.assign(gn * S + 1, 0u);
        for (size_t j = 0; j < gn; j++) {
            const uint32_t i = g.read[j];
            const int L = (int)(roff[i + 1] - roff[i]);
            for (int p = 0; p < L; p++) {
                const int code = mirge_base_code(reads[roff[i] + p]);
                const size_t w = (size_t)(p >> 5) * gn + j;
                if (code < 0) g.nm[w] |= 1ull << (2 * (p & 31));
                else g.seq[w] |= (uint64_t)code << (2 * (p & 31));
            }
            g.len[j] = (uint8_t)L; g.pass[j] = pass[i]; g.ref[j] = ref[i];
            for (int32_t s = 0; s < S; s++) g.counts[j * S + s] = counts[(size_t)i * S + s];
            handle[i] = g.base + (uint32_t)j;
        }
    }
    const size_t nh = (size_t)base + 1;
    std::vector<uint8_t> ret_h(nh, 0);
    if (retained) for (auto& g : G) for (size_t j = 0; j < g.read.size(); j++) ret_h[g.base + j] = retained[g.read[j]];
    std::vector<int8_t> diag_h(nh, 0), state_h(nh, -1);
    const size_t n_fs = (size_t)std::max<int64_t>(n_fam, 1) * S, n_cen = n_fs * MIRGE_TALLY_MAXPOS * 16 * 3;
    std::vector<unsigned long long> d(5 * n_fs + n_cen, 0ull);
    TallyOut o;
    o.n_seqs = d.data(); o.seq_true = d.data() + n_fs; o.count_true = d.data() + 2 * n_fs; o.canon = d.data() + 3 * n_fs;
    o.kept_exact = d.data() + 4 * n_fs; o.census = d.data() + 5 * n_fs; o.diag = diag_h.data(); o.state = state_h.data();
    for (int k = 0; k < 4; k++) {
        SimGroup& g = G[k];
        const uint32_t gn = (uint32_t)g.read.size();
        n_chunks[k] = 0;
        if (!gn) continue;
        const uint32_t grid = (gn + chunk - 1) / chunk;
        n_chunks[k] = (int32_t)grid;
        std::vector<uint32_t> list((size_t)grid * chunk + grid, 0xFFFFFFFFu);
        uint32_t* n_list = list.data() + (size_t)grid * chunk;
        const TallyMember pred{g.pass.data(), g.ref.data(), g.counts.data(), S, exact_pass, iso_pass, fam_of_ref, freq};
        for (uint32_t b = 0; b < grid; b++) {
            uint32_t run = 0;
            for (uint32_t i = b * chunk; i < std::min(gn, (b + 1) * chunk); i++)
                if (pred(i)) list[(size_t)b * chunk + run++] = i;
            n_list[b] = run;
        }
        const uint64_t* nmask = g.has_n ? g.nm.data() : nullptr;
        const uint8_t* ret = retained ? ret_h.data() : nullptr;
        if (g.W == 1) {
            const GroupView<1> v{g.seq.data(), g.len.data(), nmask, gn};
            launch(grid, block, [&] { k_tally<1>(v, g.base, nullptr, g.pass.data(), g.ref.data(), g.counts.data(), S, exact_pass, iso_pass, fam_of_ref,
                                                 tb.data(), tl.data(), ret, freq, o, list.data(), n_list, chunk); });
        } else {
            const GroupView<2> v{g.seq.data(), g.len.data(), nmask, gn};
            launch(grid, block, [&] { k_tally<2>(v, g.base, nullptr, g.pass.data(), g.ref.data(), g.counts.data(), S, exact_pass, iso_pass, fam_of_ref,
                                                 tb.data(), tl.data(), ret, freq, o, list.data(), n_list, chunk); });
        }
    }
    // ---- the reads no instance of k_tally takes: the member predicate alone
    {
        std::vector<int8_t> wp; std::vector<int32_t> wr; std::vector<uint32_t> wc;
        for (uint32_t i : wide) {
            wp.push_back(pass[i]); wr.push_back(ref[i]);
            for (int32_t s = 0; s < S; s++) wc.push_back(counts[(size_t)i * S + s]);
        }
        wp.push_back(-1); wr.push_back(-1); wc.push_back(0);
        const TallyMember pred{wp.data(), wr.data(), wc.data(), S, exact_pass, iso_pass, fam_of_ref, freq};
        *wide_members = 0;
        for (uint32_t j = 0; j < (uint32_t)wide.size(); j++) *wide_members += pred(j) ? 1 : 0;
    }
    for (size_t k = 0; k < 5 * (size_t)n_fam * S; k++) {
        const size_t t = k / ((size_t)n_fam * S), r = k % ((size_t)n_fam * S);
        fam_tables[k] = (int64_t)d[t * n_fs + r];
    }
    for (size_t k = 0; k < (size_t)n_fam * S * MIRGE_TALLY_MAXPOS * 16 * 3; k++) census[k] = (int64_t)d[5 * n_fs + k];
    for (int64_t i = 0; i < n; i++) {
        diag_out[i] = cls[(size_t)i] < 0 ? 0 : diag_h[handle[(size_t)i]];
        state_out[i] = cls[(size_t)i] < 0 ? -1 : state_h[handle[(size_t)i]];
    }
    return 0;
}
