// near_sim.cpp -- the kernels of csrc/kernels_nearest.hpp compiled for the HOST (tests/test_nearest_hostsim.py): the same kernel source, a workgroup's
// threads one after the other between its barriers (MIRGE_NEAR_HOSTSIM; an atomic is then a plain read-modify-write), the launches in the order of
// csrc/native_nearest.hpp: k_near_codes, k_near_masks_ascii (or k_near_flag, the selection and k_near_masks_packed over a made-up dictionary),
// k_near_width, the selection of each instance's queries, k_near_scan<uint32_t> and <uint64_t> over (chunks) x (query tiles), k_near_report, the
// selection of the kept queries, k_near_start in both instances, k_near_gather.  The chunk list is built as near_chunks builds it.
// With -DNEAR_SIM_MAIN a stand-alone program over generated libraries, for a sanitizer build of this host code.
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
#define MIRGE_NEAR_HOSTSIM 1
struct D3 { unsigned x, y; };
static D3 threadIdx, blockIdx, blockDim, gridDim;
template <class T> static T atomicAdd(T* p, T v) { const T o = *p; *p += v; return o; }
template <class T> static T atomicMin(T* p, T v) { const T o = *p; if (v < o) *p = v; return o; }
#include "../../mirge3.0_amd/csrc/kernels_nearest.hpp"

template <class F> static void launch(unsigned grid, unsigned grid_y, unsigned block, F f) {
    gridDim.x = grid; gridDim.y = grid_y; blockDim.x = block; blockDim.y = 1;
    for (unsigned y = 0; y < grid_y; y++)
        for (unsigned b = 0; b < grid; b++) { blockIdx.x = b; blockIdx.y = y; threadIdx.x = 0; threadIdx.y = 0; f(); }
}

// hipCUB's flagged selection of the indices [0, n)
static std::vector<uint32_t> select(const std::vector<uint8_t>& flags) {
    std::vector<uint32_t> out;
    for (size_t i = 0; i < flags.size(); i++) if (flags[i]) out.push_back((uint32_t)i);
    return out;
}

struct SimLib {
    std::vector<uint32_t> code_words;  // the codes, in words as the scan fetches them, with the device buffer's slack
    std::vector<uint32_t> hoff;
    std::vector<NearChunk> chunks;
    const uint8_t* codes() const { return reinterpret_cast<const uint8_t*>(code_words.data()); }
};

static SimLib sim_lib(const uint8_t* t_text, const int64_t* t_off, int64_t n_t, int32_t chunk_bases) {
    SimLib L;
    L.hoff.assign((size_t)n_t + 1, 0u);
    for (int64_t h = 0; h <= n_t && n_t; h++) L.hoff[(size_t)h] = (uint32_t)t_off[h];
    const uint32_t total = L.hoff[(size_t)n_t];
    L.code_words.assign(((size_t)total + 16) / 4 + 1, 0u);
    if (total) launch(2, 1, MIRGE_BLOCK, [&] { k_near_codes(t_text, total, reinterpret_cast<uint8_t*>(L.code_words.data())); });
    const uint32_t cap = (uint32_t)std::max(1, std::min(chunk_bases, MIRGE_NEAR_LDS_BASES)), n_h = (uint32_t)n_t;
    for (uint32_t h = 0; h < n_h;) {
        uint32_t h1 = h + 1;
        while (h1 < n_h && L.hoff[h1 + 1] - L.hoff[h] <= cap) h1++;
        if (L.hoff[h1] > L.hoff[h]) L.chunks.push_back(NearChunk{h, h1});
        h = h1;
    }
    return L;
}

// peq [4][n], qlen [n] -> best [n], start [n], the kept queries.  tile_grid: blockIdx.y of the scan (fewer than the tiles: its stride runs)
static std::vector<uint32_t> sim_pipeline(const SimLib& L, const std::vector<uint64_t>& peq, const std::vector<uint8_t>& qlen, int32_t K, int32_t force64,
                                          unsigned tile_grid, std::vector<unsigned long long>& best, std::vector<int32_t>& start) {
    const uint32_t n = (uint32_t)qlen.size();
    best.assign(n, MIRGE_NEAR_NO_KEY);
    start.assign(n, -1);
    if (L.chunks.empty() || !n) return {};
    std::vector<uint8_t> f32(n), f64(n), frep(n);
    launch(2, 1, MIRGE_BLOCK, [&] { k_near_width(qlen.data(), n, force64, f32.data(), f64.data()); });
    const std::vector<uint32_t> i32 = select(f32), i64 = select(f64);
    const unsigned n_chunk = (unsigned)L.chunks.size();
    auto tiles = [&](size_t nq) { return (unsigned)std::max<size_t>(1, std::min<size_t>(tile_grid, (nq + MIRGE_BLOCK - 1) / MIRGE_BLOCK)); };
    if (!i32.empty())
        launch(n_chunk, tiles(i32.size()), MIRGE_BLOCK, [&] {
            k_near_scan<uint32_t>(i32.data(), (uint32_t)i32.size(), n, peq.data(), qlen.data(), L.codes(), L.hoff.data(), L.chunks.data(), best.data());
        });
    if (!i64.empty())
        launch(n_chunk, tiles(i64.size()), MIRGE_BLOCK, [&] {
            k_near_scan<uint64_t>(i64.data(), (uint32_t)i64.size(), n, peq.data(), qlen.data(), L.codes(), L.hoff.data(), L.chunks.data(), best.data());
        });
    launch(2, 1, MIRGE_BLOCK, [&] { k_near_report(best.data(), qlen.data(), n, K, frep.data()); });
    const std::vector<uint32_t> rep = select(frep);
    if (rep.empty()) return rep;
    if (!i32.empty())
        launch(2, 1, MIRGE_BLOCK, [&] {
            k_near_start<uint32_t>(rep.data(), (uint32_t)rep.size(), n, peq.data(), qlen.data(), L.codes(), L.hoff.data(), best.data(), force64, start.data());
        });
    if (!i64.empty())
        launch(2, 1, MIRGE_BLOCK, [&] {
            k_near_start<uint64_t>(rep.data(), (uint32_t)rep.size(), n, peq.data(), qlen.data(), L.codes(), L.hoff.data(), best.data(), force64, start.data());
        });
    return rep;
}

// mirge_nearest_scan: -1 everywhere for a query without a hit.  -> 0, or 1 when an anchored scan did not reach its distance
extern "C" int sim_nearest_scan(const uint8_t* q_text, const int64_t* q_off, int64_t n_q, const uint8_t* t_text, const int64_t* t_off, int64_t n_t,
                                int32_t chunk_bases, int32_t force64, int32_t tile_grid, int32_t* dist, int32_t* hairpin, int32_t* start, int32_t* end) {
    for (int64_t i = 0; i < n_q; i++) dist[i] = hairpin[i] = start[i] = end[i] = -1;
    if (!n_q) return 0;
    const SimLib L = sim_lib(t_text, t_off, n_t, chunk_bases);
    const uint32_t n = (uint32_t)n_q;
    std::vector<uint64_t> peq((size_t)n * 4);
    std::vector<uint8_t> qlen(n);
    launch(2, 1, MIRGE_BLOCK, [&] { k_near_masks_ascii(q_text, q_off, n, peq.data(), qlen.data()); });
    std::vector<unsigned long long> best;
    std::vector<int32_t> st;
    sim_pipeline(L, peq, qlen, -1, force64, (unsigned)std::max(1, tile_grid), best, st);
    for (uint32_t i = 0; i < n; i++) {
        if (best[i] == MIRGE_NEAR_NO_KEY) continue;
        if (st[i] < 0) return 1;
        dist[i] = (int32_t)(best[i] >> 56); hairpin[i] = (int32_t)((best[i] >> 32) & 0xFFFFFFull); end[i] = (int32_t)(uint32_t)best[i]; start[i] = st[i];
    }
    return 0;
}

// mirge_nearest_unmapped over a dictionary of two groups: A one word per read (<= 31 nt), B two words (<= 64 nt); nmask may be null.
// out arrays: room for n_a + n_b rows; stats[5].  -> the number of kept rows, or -1
extern "C" int64_t sim_nearest_unmapped(int64_t n_a, const uint64_t* seq_a, const uint64_t* nmask_a, const uint8_t* len_a, const int8_t* pass_a, int64_t n_b,
                                        const uint64_t* seq_b, const uint64_t* nmask_b, const uint8_t* len_b, const int8_t* pass_b, const uint8_t* t_text,
                                        const int64_t* t_off, int64_t n_t, int32_t K, int32_t chunk_bases, uint32_t* row, int32_t* dist, int32_t* hairpin,
                                        int32_t* start, int32_t* end, int64_t* stats) {
    NearGroups t;
    std::memset(&t, 0, sizeof(t));
    t.g[0] = NearGroup{seq_a, nmask_a, len_a, pass_a, 0u, (uint32_t)n_a, 1, 0};
    t.g[1] = NearGroup{seq_b, nmask_b, len_b, pass_b, (uint32_t)n_a, (uint32_t)n_b, 2, 0};
    const uint32_t n_rows = (uint32_t)(n_a + n_b);
    for (int k = 0; k < 5; k++) stats[k] = 0;
    if (!n_rows) return 0;
    const SimLib L = sim_lib(t_text, t_off, n_t, chunk_bases);
    std::vector<uint8_t> flags(n_rows);
    unsigned long long st3[4] = {0, 0, 0, 0};
    launch(3, 1, MIRGE_BLOCK, [&] { k_near_flag(t, n_rows, flags.data(), st3); });
    const std::vector<uint32_t> sel = select(flags);
    stats[0] = (int64_t)st3[MIRGE_NEAR_ST_UNMAPPED]; stats[1] = (int64_t)st3[MIRGE_NEAR_ST_SHORT]; stats[2] = (int64_t)st3[MIRGE_NEAR_ST_LONG];
    stats[3] = (int64_t)sel.size();
    if (sel.empty()) return 0;
    const uint32_t n = (uint32_t)sel.size();
    std::vector<uint64_t> peq((size_t)n * 4);
    std::vector<uint8_t> qlen(n);
    launch(2, 1, MIRGE_BLOCK, [&] { k_near_masks_packed(t, sel.data(), n, peq.data(), qlen.data()); });
    std::vector<unsigned long long> best;
    std::vector<int32_t> st;
    const std::vector<uint32_t> rep = sim_pipeline(L, peq, qlen, K, 0, 2, best, st);
    stats[4] = (int64_t)rep.size();
    if (rep.empty()) return 0;
    std::vector<unsigned long long> key(rep.size());
    launch(2, 1, MIRGE_BLOCK, [&] { k_near_gather(rep.data(), (uint32_t)rep.size(), sel.data(), best.data(), st.data(), row, key.data(), start); });
    for (size_t i = 0; i < rep.size(); i++) {
        if (start[i] < 0) return -1;
        dist[i] = (int32_t)(key[i] >> 56); hairpin[i] = (int32_t)((key[i] >> 32) & 0xFFFFFFull); end[i] = (int32_t)(uint32_t)key[i];
    }
    return (int64_t)rep.size();
}

#ifdef NEAR_SIM_MAIN
int main() {
    uint64_t state = 99, sum = 0;
    auto rnd = [&](uint64_t m) { state = state * 6364136223846793005ull + 1442695040888963407ull; return (state >> 33) % m; };
    for (int set = 0; set < 40; set++) {
        std::string lib, qs;
        std::vector<int64_t> t_off{0}, q_off{0};
        const int n_t = set == 0 ? 0 : 1 + (int)rnd(8);
        for (int h = 0; h < n_t; h++) {
            const size_t L = rnd(6) ? rnd(130) : (rnd(2) ? 0 : 4097 + rnd(300));
            for (size_t p = 0; p < L; p++) lib += "ACGTN"[rnd(40) ? rnd(4) : 4];
            t_off.push_back((int64_t)lib.size());
        }
        const int n_q = (int)rnd(600);
        for (int i = 0; i < n_q; i++) {
            const size_t m = rnd(10) ? 12 + rnd(53) : rnd(80);
            if (lib.size() > m && rnd(4)) {
                const size_t at = rnd(lib.size() - m);
                for (size_t p = 0; p < m; p++) qs += rnd(12) ? lib[at + p] : "ACGTN"[rnd(5)];
            } else {
                for (size_t p = 0; p < m; p++) qs += "ACGT"[rnd(4)];
            }
            q_off.push_back((int64_t)qs.size());
        }
        lib += "\0\0\0\0";
        qs += "\0\0\0\0";
        std::vector<int32_t> d(n_q + 1), hp(n_q + 1), s(n_q + 1), e(n_q + 1);
        if (sim_nearest_scan((const uint8_t*)qs.data(), q_off.data(), n_q, (const uint8_t*)lib.data(), t_off.data(), n_t, set % 2 ? 64 : 4096, set % 3 == 0, 1 + set % 2,
                             d.data(), hp.data(), s.data(), e.data()))
            return 1;
        for (int i = 0; i < n_q; i++) sum += (uint64_t)(d[i] + 2) * 31u + (uint64_t)(hp[i] + 2) * 7u + (uint64_t)(s[i] + 2) + (uint64_t)(e[i] + 2) * 3u;
        // the same queries as a packed dictionary, every third one annotated
        std::vector<uint64_t> sa, ma, sb, mb;
        std::vector<uint8_t> la, lb;
        std::vector<int8_t> pa, pb;
        for (int i = 0; i < n_q; i++) {
            const size_t m = (size_t)(q_off[i + 1] - q_off[i]);
            if (m > 64) continue;
            uint64_t w[2] = {0, 0}, nm[2] = {0, 0};
            for (size_t p = 0; p < m; p++) {
                const uint8_t c = near_code((uint8_t)qs[(size_t)q_off[i] + p]);
                if (c > 3) nm[p >> 5] |= 1ull << (2 * (p & 31));
                else w[p >> 5] |= (uint64_t)c << (2 * (p & 31));
            }
            if (m <= 31) { sa.push_back(w[0]); ma.push_back(nm[0]); la.push_back((uint8_t)m); pa.push_back(i % 3 ? -1 : 2); }
            else { sb.push_back(w[0]); mb.push_back(nm[0]); lb.push_back((uint8_t)m); pb.push_back(i % 3 ? -1 : 0); }
        }
        const size_t na = la.size(), nb = lb.size();
        std::vector<uint64_t> sb2(2 * nb + 1), mb2(2 * nb + 1);  // [W][n]
        {
            size_t k = 0;
            for (int i = 0; i < n_q; i++) {
                const size_t m = (size_t)(q_off[i + 1] - q_off[i]);
                if (m <= 31 || m > 64) continue;
                uint64_t w1 = 0, n1 = 0;
                for (size_t p = 32; p < m; p++) {
                    const uint8_t c = near_code((uint8_t)qs[(size_t)q_off[i] + p]);
                    if (c > 3) n1 |= 1ull << (2 * (p & 31));
                    else w1 |= (uint64_t)c << (2 * (p & 31));
                }
                sb2[k] = sb[k]; mb2[k] = mb[k]; sb2[nb + k] = w1; mb2[nb + k] = n1;
                k++;
            }
        }
        sa.push_back(0); ma.push_back(0); la.push_back(0); pa.push_back(0); lb.push_back(0); pb.push_back(0);
        std::vector<uint32_t> row(na + nb + 1);
        std::vector<int32_t> d2(na + nb + 1), h2(na + nb + 1), s2(na + nb + 1), e2(na + nb + 1);
        int64_t stats[5];
        const int64_t kept = sim_nearest_unmapped((int64_t)na, sa.data(), set % 2 ? ma.data() : nullptr, la.data(), pa.data(), (int64_t)nb, sb2.data(), mb2.data(), lb.data(),
                                                  pb.data(), (const uint8_t*)lib.data(), t_off.data(), n_t, 1 + set % 8, set % 2 ? 64 : 4096, row.data(), d2.data(),
                                                  h2.data(), s2.data(), e2.data(), stats);
        if (kept < 0) return 1;
        for (int64_t i = 0; i < kept; i++) sum += row[i] + (uint64_t)d2[i] * 5u + (uint64_t)h2[i] + (uint64_t)s2[i] + (uint64_t)e2[i];
        for (int k = 0; k < 5; k++) sum += (uint64_t)stats[k];
    }
    std::printf("near_sim: 40 sets, checksum %llu\n", (unsigned long long)sum);
    return 0;
}
#endif
