// ec_ratio_sim.cpp -- csrc/kernels_ec.hpp compiled for the HOST with the relative threshold of --kmer-ratio (tests/test_kmer_ratio_hostsim.py):
// ec_sim.cpp's scheme (the same kernel source, a launch's threads one after the other, the wave kernel's lanes as a loop), the launches of
// a round in the order of csrc/native_ec.hpp's mirge_kmer_correct_ratio: k_ec_clear, k_ec_count, with a ratio k_ec_dominate and k_ec_fold,
// k_ec_classify, k_ec_correct.  The regrouping between two rounds is a std::map here.
// With -DEC_RATIO_SIM_MAIN a stand-alone program over named cases of its own, for a sanitizer build of this host code.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
#define MIRGE_BLOCK 256
#define MIRGE_EC_HOSTSIM 1
struct D3 { unsigned x; };
static D3 threadIdx, blockIdx, blockDim, gridDim;
template <class T> static T atomicCAS(T* p, T expect, T v) { const T o = *p; if (o == expect) *p = v; return o; }
template <class T> static T atomicAdd(T* p, T v) { const T o = *p; *p += v; return o; }
#include "../../mirge3.0_amd/csrc/kernels_ec.hpp"

template <class F> static void launch(unsigned grid, unsigned block, F f) {
    gridDim.x = grid; blockDim.x = block;
    for (unsigned b = 0; b < grid; b++)
        for (unsigned t = 0; t < block; t++) { blockIdx.x = b; threadIdx.x = t; f(); }
}

struct Entry { std::string read; uint32_t count, first; };

// one round over D (in any order): fix[i] = p << 2 | letter for a corrected read, MIRGE_EC_NONE otherwise; tally[] as the device's;
// ad[0..1] = k-mers above H, the dominated among them (zeros without a ratio)
static void sim_round(const std::vector<Entry>& D, int k, uint64_t H, uint64_t ratio, int hash_bits, std::vector<uint32_t>& fix_of, uint32_t* tally,
                      unsigned long long* ad) {
    const size_t n = D.size();
    std::vector<int> cls(n);
    std::vector<uint32_t> cnt(MIRGE_EC_NG + 1, 0), base(MIRGE_EC_NG + 1, 0), at(MIRGE_EC_NG + 1, 0), handle(n);
    size_t longest = 256;
    for (size_t i = 0; i < n; i++) {
        const std::string& r = D[i].read;
        const size_t L = r.size();
        const bool amb = r.find_first_not_of("ACGT") != std::string::npos;
        cls[i] = amb ? MIRGE_EC_NG : (L <= 31 ? 0 : (L <= 64 ? 1 : (L <= 128 ? 2 : (L <= 255 ? 3 : 4))));
        cnt[cls[i]]++;
        longest = std::max(longest, L);
    }
    for (int q = 1; q <= MIRGE_EC_NG; q++) base[q] = base[q - 1] + cnt[q - 1];
    const int Ws[MIRGE_EC_NG] = {1, 2, 4, 8, (int)((longest + 31) / 32)};
    std::vector<uint64_t> seq[MIRGE_EC_NG];
    std::vector<uint8_t> len8[MIRGE_EC_NG];
    std::vector<uint16_t> len16(cnt[4] + 1, 0);
    std::vector<uint32_t> gc[MIRGE_EC_NG];
    for (int q = 0; q < MIRGE_EC_NG; q++) { seq[q].assign((size_t)Ws[q] * cnt[q] + 1, 0ull); len8[q].assign(cnt[q] + 1, 0); gc[q].assign(cnt[q] + 1, 0); }
    uint64_t windows = 0;
    for (size_t i = 0; i < n; i++) {
        const int q = cls[i];
        const uint32_t j = at[q]++;
        handle[i] = base[q] + j;
        const std::string& r = D[i].read;
        if ((int)r.size() >= k) windows += std::min<size_t>(r.size(), 256) - k + 1;  // (from the lengths alone, as the device)
        if (q == MIRGE_EC_NG) continue;
        for (size_t p = 0; p < r.size(); p++) {
            const char ch = r[p];
            const uint64_t code = ch == 'A' ? 0 : (ch == 'C' ? 1 : (ch == 'G' ? 2 : 3));
            seq[q][(p >> 5) * cnt[q] + j] |= code << (2 * (p & 31));
        }
        if (q == 4) len16[j] = (uint16_t)r.size(); else len8[q][j] = (uint8_t)r.size();
        gc[q][j] = D[i].count;
    }
    EcView v;
    std::memset(&v, 0, sizeof(v));
    for (int q = 0; q < MIRGE_EC_NG; q++)
        if (cnt[q]) v.g[q] = EcGroup{seq[q].data(), q == 4 ? reinterpret_cast<const uint8_t*>(len16.data()) : len8[q].data(), gc[q].data(), base[q], cnt[q], (uint32_t)Ws[q], q == 4};
    v.n_reads = (uint32_t)n; v.k = k; v.H = H;
    v.hash_keep = hash_bits < 0 || hash_bits > 63 ? ~0ull : (1ull << hash_bits) - 1;
    uint64_t slots = 256;
    while (slots < 2 * windows) slots <<= 1;
    v.tab_mask = slots - 1;
    std::vector<EcSlot> tab((size_t)slots);
    std::vector<uint32_t> range(n + 1, 7), fix(n + 1, 7), list(n + 1, 0);
    for (int q = 0; q < MIRGE_EC_T_WORDS; q++) tally[q] = 0;
    const unsigned grid = (unsigned)std::min<size_t>((n + MIRGE_BLOCK - 1) / MIRGE_BLOCK, 3);  // (grid-stride loops: a few workgroups do)
    launch(2, MIRGE_BLOCK, [&] { k_ec_clear(tab.data(), slots); });
    launch(grid, MIRGE_BLOCK, [&] { k_ec_count(v, tab.data()); });
    ad[0] = ad[1] = 0;
    if (ratio) {
        std::vector<uint8_t> flag((size_t)slots, 7);
        const EcSlot* ctab = tab.data();  // (read-only in k_ec_dominate)
        launch(3, MIRGE_BLOCK, [&] { k_ec_dominate(v, ctab, slots, ratio, flag.data(), ad); });
        launch(2, MIRGE_BLOCK, [&] { k_ec_fold(tab.data(), slots, flag.data()); });
    }
    launch(grid, MIRGE_BLOCK, [&] { k_ec_classify(v, tab.data(), range.data(), fix.data(), list.data(), tally); });
    const uint32_t n_list = tally[MIRGE_EC_T_LIST];
    if (n_list) launch(2, MIRGE_BLOCK, [&] { k_ec_correct(v, tab.data(), list.data(), n_list, range.data(), fix.data(), tally); });
    fix_of.resize(n);
    for (size_t i = 0; i < n; i++) fix_of[i] = fix[handle[i]];
}

// reads: ASCII, roff[n + 1]; counts, first: per read.  final_out: ASCII over the same offsets (a read keeps its length); rounds_mask[n]: bit
// (k - ks); stats[7 r + 0..6] per round: eligible, suspect, corrected, uncorrectable, unsupported, ambiguous, distinct reads after.
// ad[2 r + 0..1]: k-mers above H, the dominated among them.  hash_bits < 0: the whole hash.  -> 0, -1 (a bad range or ratio)
extern "C" int sim_kmer_correct_ratio(const char* reads, const int64_t* roff, int64_t n_reads, const uint32_t* counts, const uint32_t* first, int32_t ks,
                                      int32_t ke, int32_t H, int32_t ratio, int32_t hash_bits, char* final_out, uint32_t* rounds_mask, int64_t* stats,
                                      int64_t* ad) {
    if (H < 1 || ks < 8 || ke > MIRGE_EC_MAXK || ks > ke || ratio == 1 || ratio < 0) return -1;
    const size_t n = (size_t)n_reads;
    std::vector<Entry> D(n);
    std::vector<std::string> now(n);
    for (size_t i = 0; i < n; i++) {
        D[i] = Entry{std::string(reads + roff[i], (size_t)(roff[i + 1] - roff[i])), counts[i], first[i]};
        now[i] = D[i].read;
        rounds_mask[i] = 0;
    }
    for (int k = ks; k <= ke; k++) {
        std::vector<uint32_t> fix;
        uint32_t tally[MIRGE_EC_T_WORDS];
        unsigned long long ad_round[2];
        sim_round(D, k, (uint64_t)H, (uint64_t)ratio, hash_bits, fix, tally, ad_round);
        ad[2 * (k - ks)] = (int64_t)ad_round[0]; ad[2 * (k - ks) + 1] = (int64_t)ad_round[1];
        std::map<std::string, std::pair<std::string, bool>> step;  // a read of D -> (what it becomes, corrected)
        std::map<std::string, std::pair<uint64_t, uint32_t>> merged;
        for (size_t i = 0; i < D.size(); i++) {
            std::string r = D[i].read;
            if (fix[i] != MIRGE_EC_NONE) r[fix[i] >> 2] = "ACGT"[fix[i] & 3u];
            step[D[i].read] = {r, fix[i] != MIRGE_EC_NONE};
            auto it = merged.find(r);
            if (it == merged.end()) merged[r] = {D[i].count, D[i].first};
            else { it->second.first += D[i].count; it->second.second = std::min(it->second.second, D[i].first); }
        }
        for (size_t i = 0; i < n; i++) {
            const auto& s = step[now[i]];
            if (s.second) rounds_mask[i] |= 1u << (k - ks);
            now[i] = s.first;
        }
        D.clear();
        for (const auto& m : merged) D.push_back(Entry{m.first, (uint32_t)m.second.first, m.second.second});
        int64_t* st = stats + 7 * (k - ks);
        st[0] = tally[MIRGE_EC_T_ELIG]; st[1] = tally[MIRGE_EC_T_SUSPECT]; st[2] = tally[MIRGE_EC_T_CORRECTED]; st[3] = tally[MIRGE_EC_T_UNCORRECTABLE];
        st[4] = tally[MIRGE_EC_T_UNSUPPORTED]; st[5] = tally[MIRGE_EC_T_AMBIGUOUS]; st[6] = (int64_t)D.size();
    }
    for (size_t i = 0; i < n; i++) std::memcpy(final_out + roff[i], now[i].data(), now[i].size());
    return 0;
}

#ifdef EC_RATIO_SIM_MAIN
// named cases: a deep template and its error, the edge of 2a (80 / 79 against 10), k = 31 with a neighbour at the first, the middle and the
// last letter of a word, sums beyond 2^33 against the largest ratio, an empty dictionary, nothing above H; whole and 4-bit hashes
struct Named { const char* name; std::vector<std::string> reads; std::vector<uint32_t> counts; int ks, ke, H, ratio; int64_t want_a, want_d; };
static std::string sub(std::string s, size_t p) { s[p] = s[p] == 'A' ? 'C' : 'A'; return s; }
int main() {
    const std::string t24 = "ACGTTGCAAGCTTAGGCTAACGTC", w10 = "GATTACAGTC";
    const std::string t65 = "ACGGTCATTGCAAGTCCGATAGGCTTAACGTGCATCGGATCTTAGCAAGTCGGATACCTGAATCG";
    const uint32_t big = 0xFFFFFFFFu;
    std::vector<Named> cases = {
        {"deep_template", {t24, sub(t24, 12)}, {1000, 20}, 10, 10, 5, 8, 25, 10},
        {"no_ratio", {t24, sub(t24, 12)}, {1000, 20}, 10, 10, 5, 0, 0, 0},
        {"edge_80", {w10, sub(w10, 3)}, {10, 80}, 10, 10, 5, 8, 2, 1},
        {"edge_79", {w10, sub(w10, 3)}, {10, 79}, 10, 10, 5, 8, 2, 0},
        {"k31", {t65, sub(t65, 0), sub(t65, 15), sub(t65, 30), sub(t65, 64)}, {1000, 20, 20, 20, 20}, 31, 31, 5, 8, 35 + 1 + 16 + 31 + 1, 1 + 16 + 31 + 1},
        {"wrap", {w10 + "A", w10 + "C", w10 + "G", sub(w10, 4) + "A", sub(w10, 4) + "C", sub(w10, 4) + "G"}, {2863311532u, 2863311532u, 2863311533u, big, big, big},
         10, 10, 5, 0x7FFFFFFF, 8, 0},
        {"empty", {}, {}, 10, 12, 5, 8, 0, 0},
        {"nothing_above_h", {w10, sub(w10, 2), "CCGTAGGTCA"}, {5, 2, 3}, 10, 10, 5, 2, 0, 0},
    };
    int bad = 0;
    for (const Named& c : cases)
        for (int bits : {-1, 4}) {
            std::string text;
            std::vector<int64_t> off{0};
            std::vector<uint32_t> first;
            for (const std::string& r : c.reads) { text += r; off.push_back((int64_t)text.size()); first.push_back((uint32_t)first.size()); }
            std::vector<char> fin(text.size() + 1);
            std::vector<uint32_t> mask(c.reads.size() + 1), counts(c.counts);
            counts.push_back(0);
            int64_t stats[7 * 24], ad[2 * 24];
            if (sim_kmer_correct_ratio(text.data(), off.data(), (int64_t)c.reads.size(), counts.data(), first.data(), c.ks, c.ke, c.H, c.ratio, bits, fin.data(),
                                       mask.data(), stats, ad)) { std::printf("%s: refused\n", c.name); bad++; continue; }
            const bool ok = ad[0] == c.want_a && ad[1] == c.want_d;
            std::printf("ec_ratio_sim %s (hash bits %d): above %lld dominated %lld corrected %lld%s\n", c.name, bits, (long long)ad[0], (long long)ad[1],
                        (long long)stats[2], ok ? "" : "  UNEXPECTED");
            bad += !ok;
        }
    return bad ? 1 : 0;
}
#endif
