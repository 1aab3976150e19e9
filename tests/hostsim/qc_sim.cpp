// qc_sim.cpp -- the kernels of csrc/kernels_qc.hpp compiled for the HOST (tests/test_read_qc_hostsim.py): the same kernel source, a workgroup's
// threads one after the other between its barriers (MIRGE_QC_HOSTSIM; an atomic is then a plain read-modify-write), the launches in the order
// of csrc/native_qc.hpp: per view k_qc_pos and k_qc_read<false>, or k_qc_read<true> alone; k_qc_class over two groups of a dictionary.
// With -DQC_SIM_MAIN a stand-alone program over generated texts, for a sanitizer build of this host code.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
#define MIRGE_BLOCK 256
#define MIRGE_QC_HOSTSIM 1
struct D3 { unsigned x, y; };
static D3 threadIdx, blockIdx, blockDim, gridDim;
template <class T> static T atomicAdd(T* p, T v) { const T o = *p; *p += v; return o; }
#include "../../mirge3.0_amd/csrc/kernels_qc.hpp"

template <class F> static void launch(unsigned grid, unsigned grid_y, unsigned block, F f) {
    gridDim.x = grid; gridDim.y = grid_y; blockDim.x = block; blockDim.y = 1;
    for (unsigned y = 0; y < grid_y; y++)
        for (unsigned b = 0; b < grid; b++) { blockIdx.x = b; blockIdx.y = y; threadIdx.x = 0; threadIdx.y = 0; f(); }
}

// The records [r0, r1) of a text added to tab[2][MIRGE_QC_VIEW_WORDS] (not cleared: a sample's pieces add up).  lstart / lend / qstart / qend:
// per record (q: null without qualities); vstart / vend [n][vstride] (null: nothing trims), the last column holds the trimmed bounds.
// form_pos: 1 the lane-per-position form, 0 the lane-per-read form.  pos_grid: workgroups of k_qc_pos (few: its grid stride runs).
extern "C" int sim_qc_accumulate(const uint8_t* text, const int64_t* lstart, const int64_t* lend, const int64_t* qstart, const int64_t* qend,
                                 const int64_t* vstart, const int64_t* vend, int32_t vstride, int64_t r0, int64_t r1, int32_t min_len, int32_t base,
                                 int32_t form_pos, int32_t pos_grid, unsigned long long* tab) {
    if (r1 <= r0) return 0;
    QcJob j;
    std::memset(&j, 0, sizeof(j));
    j.text = text;
    j.lstart = lstart + r0; j.lend = lend + r0;
    j.qstart = qstart ? qstart + r0 : nullptr; j.qend = qend ? qend + r0 : nullptr;
    j.n = (uint32_t)(r1 - r0);
    j.min_len = min_len; j.base = base;
    const unsigned read_grid = std::max(1u, std::min(3u, (j.n + MIRGE_BLOCK - 1) / MIRGE_BLOCK));
    for (int view = 0; view < 2; view++) {
        j.view = view;
        if (view == 1 && vstart) {
            j.vstart = vstart + r0 * vstride; j.vend = vend + r0 * vstride;
            j.vstride = (uint32_t)vstride; j.voff = (uint32_t)vstride - 1;
        }
        unsigned long long* const t = tab + (size_t)view * MIRGE_QC_VIEW_WORDS;
        if (form_pos) {
            launch((unsigned)std::max(1, pos_grid), 1, MIRGE_QC_POS_THREADS, [&] { k_qc_pos(j, t); });
            launch(read_grid, 1, MIRGE_BLOCK, [&] { k_qc_read<false>(j, t); });
        } else {
            launch(read_grid, 1, MIRGE_BLOCK, [&] { k_qc_read<true>(j, t); });
        }
    }
    return 0;
}

// two groups of a dictionary: A with 8-bit lengths, B with 16-bit lengths; nmask may be null; counts [n][S]; out [S][n_pass + 1][257][5][2], cleared here
extern "C" int sim_qc_class(int64_t n_a, const int8_t* pass_a, const uint64_t* seq_a, const uint64_t* nmask_a, const uint8_t* len_a, const uint32_t* counts_a,
                            int64_t n_b, const int8_t* pass_b, const uint64_t* seq_b, const uint64_t* nmask_b, const uint16_t* len_b, const uint32_t* counts_b,
                            int32_t S, int32_t n_pass, int32_t use_lds, int32_t grid, unsigned long long* out) {
    QcClassGroups gs;
    std::memset(&gs, 0, sizeof(gs));
    uint32_t total = 0;
    if (n_a) {
        const int k = gs.n_groups++;
        gs.pass[k] = pass_a; gs.seq[k] = seq_a; gs.nmask[k] = nmask_a; gs.len[k] = len_a; gs.counts[k] = counts_a; gs.len16[k] = 0; gs.start[k] = total;
        total += (uint32_t)n_a;
    }
    if (n_b) {
        const int k = gs.n_groups++;
        gs.pass[k] = pass_b; gs.seq[k] = seq_b; gs.nmask[k] = nmask_b; gs.len[k] = reinterpret_cast<const uint8_t*>(len_b); gs.counts[k] = counts_b; gs.len16[k] = 1;
        gs.start[k] = total;
        total += (uint32_t)n_b;
    }
    gs.start[gs.n_groups] = total;
    std::memset(out, 0, (size_t)S * (n_pass + 1) * (MIRGE_QC_P + 1) * MIRGE_QC_NL * 2 * 8);
    if ((size_t)(n_pass + 1) * MIRGE_QC_CLASS_TILE * MIRGE_QC_NL * 2 * 8 > sizeof(qc_dyn_host)) use_lds = 0;
    if (total) launch((unsigned)std::max(1, grid), (unsigned)S, MIRGE_BLOCK, [&] { k_qc_class(gs, S, n_pass, use_lds, out); });
    return 0;
}

#ifdef QC_SIM_MAIN
int main() {
    uint64_t state = 77, sum = 0;
    auto rnd = [&](uint64_t m) { state = state * 6364136223846793005ull + 1442695040888963407ull; return (state >> 33) % m; };
    for (int set = 0; set < 24; set++) {
        std::string text;
        std::vector<int64_t> ls, le, qs, qe, vs, ve;
        const int n = (int)rnd(600), stride = 1 + (int)rnd(3);
        const size_t lens[] = {0, 1, 22, 51, 63, 64, 65, 255, 256, 257, 300};
        for (int r = 0; r < n; r++) {
            const size_t L = rnd(8) ? 15 + rnd(40) : lens[rnd(11)];
            text += "@r\n";
            ls.push_back((int64_t)text.size());
            for (size_t p = 0; p < L; p++) text += "ACGTNacgu."[rnd(10)];
            const bool cr = rnd(5) == 0;
            if (cr) text += '\r';
            le.push_back((int64_t)text.size());
            text += "\n+\n";
            qs.push_back((int64_t)text.size());
            const size_t QL = rnd(20) ? L : L + 1;
            for (size_t p = 0; p < QL; p++) text += (char)(30 + rnd(98));
            if (cr) text += '\r';
            qe.push_back((int64_t)text.size());
            text += "\n";
            const int64_t a = (int64_t)rnd(L + 1), b = a + (int64_t)rnd(L - (size_t)a + 1);
            for (int s = 0; s < stride; s++) { vs.push_back(ls.back() + (s == stride - 1 ? a : 0)); ve.push_back(ls.back() + (s == stride - 1 ? b : (int64_t)L)); }
        }
        text += "\n\n\n\n\n\n\n\n";
        std::vector<unsigned long long> tab(2 * (size_t)MIRGE_QC_VIEW_WORDS, 0ull);
        const bool trim = set % 3 != 0, qual = set % 4 != 3;
        const int64_t cut = n / 3;
        for (const auto& piece : {std::pair<int64_t, int64_t>{0, cut}, {cut, n}})
            if (sim_qc_accumulate((const uint8_t*)text.data(), ls.data(), le.data(), qual ? qs.data() : nullptr, qual ? qe.data() : nullptr, trim ? vs.data() : nullptr,
                                  trim ? ve.data() : nullptr, stride, piece.first, piece.second, set % 2 ? 16 : 0, set % 5 ? 33 : 64, set % 2, 1 + set % 3, tab.data()))
                return 1;
        for (unsigned long long v : tab) sum += v;
        // the class profile of a made-up dictionary
        const int na = (int)rnd(700), nb = (int)rnd(50), S = 1 + set % 3, P = 9;
        std::vector<int8_t> pa(na + 1), pb(nb + 1);
        std::vector<uint64_t> sa(na + 1), ma(na + 1), sb(nb + 1), mb(nb + 1);
        std::vector<uint8_t> la(na + 1);
        std::vector<uint16_t> lb(nb + 1);
        std::vector<uint32_t> ca((size_t)na * S + 1), cb((size_t)nb * S + 1);
        for (int i = 0; i < na; i++) { pa[i] = (int8_t)((int)rnd(P + 1) - 1); sa[i] = rnd(1u << 30); ma[i] = rnd(9) ? 0 : 1; la[i] = (uint8_t)rnd(256); }
        for (int i = 0; i < nb; i++) { pb[i] = (int8_t)((int)rnd(P + 1) - 1); sb[i] = rnd(1u << 30); mb[i] = rnd(9) ? 0 : 1; lb[i] = (uint16_t)(256 + rnd(3000)); }
        for (auto& x : ca) x = (uint32_t)rnd(4) * (uint32_t)rnd(1000);
        for (auto& x : cb) x = (uint32_t)rnd(4) * (uint32_t)rnd(1000);
        std::vector<unsigned long long> out((size_t)S * (P + 1) * (MIRGE_QC_P + 1) * MIRGE_QC_NL * 2);
        if (sim_qc_class(na, pa.data(), sa.data(), set % 2 ? ma.data() : nullptr, la.data(), ca.data(), nb, pb.data(), sb.data(), mb.data(), lb.data(), cb.data(), S, P, set % 2,
                         1 + set % 4, out.data()))
            return 1;
        for (unsigned long long v : out) sum += v;
    }
    std::printf("qc_sim: 24 sets, checksum %llu\n", (unsigned long long)sum);
    return 0;
}
#endif
