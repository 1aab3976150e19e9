// trf_sim.cpp -- csrc/kernels_trf.hpp compiled for the HOST (tests/test_trf_hostsim.py): the same kernel source, every thread of every
// workgroup one after the other (the tRF kernels have no barrier).  The libraries are packed and their probe tables built by the host
// twins the cascade's simulation uses (mirge_libbuild.hpp); the exclusive scan and the key sort that the runtime (csrc/native_trf.hpp)
// does with hipCUB are a loop and std::sort here.  The runtime itself and the real device are the GPU tests' business.
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
template <class T> T atomicOr(T* p, T v) { T o = *p; *p |= v; return o; }
#include "../../mirge3.0_amd/csrc/mirge_core.hpp"
#include "../../mirge3.0_amd/csrc/mirge_libbuild.hpp"
#include "../../mirge3.0_amd/csrc/kernels_trf.hpp"

template <class F> static void launch(unsigned grid, unsigned block, F f) {
    gridDim.x = grid; blockDim.x = block;
    for (unsigned b = 0; b < grid; b++)
        for (unsigned t = 0; t < block; t++) { blockIdx.x = b; threadIdx.x = t; f(); }
}

struct SimLib {
    MirgeHostLib h;
    std::vector<std::vector<uint64_t>> entry;
    std::vector<std::vector<uint32_t>> bucket, pos, bits;
    std::vector<MirgeKTable> tables;
    SimLib() : entry(MIRGE_SHAPE_SLOTS), bucket(MIRGE_SHAPE_SLOTS), pos(MIRGE_SHAPE_SLOTS), bits(MIRGE_SHAPE_SLOTS), tables(MIRGE_SHAPE_SLOTS) {
        for (auto& t : tables) { t.bucket = nullptr; t.pos = nullptr; t.bits = nullptr; }
    }
    // every table a read of (trimmed) length l can ask for; entries_all: also the small tables as self-contained entries
    void prepare(const MirgePolicy& p, int l, bool entries_all) {
        if (l < 1 || l <= p.mm) return;
        const int np = mirge_probe_count(p, l, h.kmax, h.total);
        for (int q = 0; q < np; q++) {
            MirgeProbe pr;
            mirge_probe_at(p, l, h.kmax, h.total, q, pr);
            if (pr.k1 <= 0) continue;
            const int sid = mirge_shape_id(pr.k1, pr.gap, pr.k2);
            if (tables[sid].bucket) continue;
            mirge_hostlib_table(h, pr.k1, pr.gap, pr.k2, bucket[sid], entry[sid], pos[sid]);
            tables[sid].bucket = entry[sid].data();
            tables[sid].pos = pos[sid].data();
            if (pr.k1 + pr.k2 <= 10 && !entries_all) {
                const auto& bk = bucket[sid];
                auto& bt = bits[sid];
                bt.assign((bk.size() - 1 + 31) / 32, 0u);
                for (size_t b = 0; b + 1 < bk.size(); b++) if (bk[b + 1] > bk[b]) bt[b >> 5] |= 1u << (b & 31);
                tables[sid].bits = bt.data();
                tables[sid].bucket = bk.data();
            }
        }
    }
    MirgeLibView view() {
        MirgeLibView v;
        v.T = h.T.data(); v.inv = h.inv.data(); v.ref_start = h.ref_start.data(); v.tables = tables.data();
        v.total = h.total; v.n_refs = (uint32_t)h.n_refs; v.kmax = h.kmax;
        return v;
    }
};

// the reads as four width groups (up to 31, 64, 128, 255 nt), word-major; handle index = group base + j
struct SimReads {
    std::vector<uint64_t> seq[4], nm[4];
    std::vector<uint8_t> len[4];
    std::vector<int8_t> pass[4], mm[4];
    std::vector<uint32_t> handle;  // read -> handle index
    int fill(const char* reads, const int64_t* roff, int64_t n, const int8_t* ps, const int8_t* m, TrfTables& t) {
        static const int Ws[4] = {1, 2, 4, 8};
        std::vector<uint32_t> cnt(4, 0), at(4, 0), base(4, 0);
        std::vector<int> cls((size_t)n);
        for (int64_t i = 0; i < n; i++) {
            const int64_t L = roff[i + 1] - roff[i];
            if (L < 1 || L > MIRGE_MAX_READ_LEN) return -6;
            cls[(size_t)i] = L <= 31 ? 0 : (L <= 64 ? 1 : (L <= 128 ? 2 : 3));
            cnt[cls[(size_t)i]]++;
        }
        for (int k = 1; k < 4; k++) base[k] = base[k - 1] + cnt[k - 1];
        handle.resize((size_t)n);
        for (int k = 0; k < 4; k++) {
            seq[k].assign((size_t)Ws[k] * cnt[k] + 1, 0ull); nm[k].assign((size_t)Ws[k] * cnt[k] + 1, 0ull);
            len[k].assign(cnt[k] + 1, 0); pass[k].assign(cnt[k] + 1, -1); mm[k].assign(cnt[k] + 1, -1);
        }
        for (int64_t i = 0; i < n; i++) {
            const int k = cls[(size_t)i];
            const uint32_t j = at[k]++;
            const int L = (int)(roff[i + 1] - roff[i]);
            for (int p = 0; p < L; p++) {
                const int code = mirge_base_code(reads[roff[i] + p]);
                const size_t w = (size_t)(p >> 5) * cnt[k] + j;
                if (code < 0) nm[k][w] |= 1ull << (2 * (p & 31));
                else seq[k][w] |= (uint64_t)code << (2 * (p & 31));
            }
            len[k][j] = (uint8_t)L; pass[k][j] = ps[i]; mm[k][j] = m[i];
            handle[(size_t)i] = base[k] + j;
        }
        for (int k = 0; k < 4; k++)
            t.g[k] = TrfGroup{seq[k].data(), nm[k].data(), len[k].data(), pass[k].data(), mm[k].data(), nullptr, base[k], cnt[k], Ws[k], 0};
        return 0;
    }
};

// -> number of records, or < 0.  out arrays hold `cap` records.
extern "C" long long sim_trf_hits(const char* reads, const int64_t* roff, int64_t n, const int8_t* ps, const int8_t* mm,
                                  const char* const* lib_seq, const int64_t* const* lib_off, const int64_t* lib_n, const MirgePolicy* pol,
                                  const int32_t* cls_pass, const int32_t* anticodon, const int64_t* rows, int64_t n_rows, int32_t entries_all,
                                  long long cap, uint32_t* o_row, uint32_t* o_ref, int32_t* o_off, uint8_t* o_mm, uint8_t* o_cls, uint8_t* o_type) {
    TrfTables t;
    std::memset(&t, 0, sizeof(t));
    SimReads R;
    if (int rc = R.fill(reads, roff, n, ps, mm, t)) return rc;
    SimLib libs[2];
    for (int c = 0; c < 2; c++) {
        std::string err;
        if (mirge_hostlib_build(libs[c].h, lib_seq[c], lib_off[c], lib_n[c], err)) return -1;
        int max_len = 1;
        for (int64_t i = 0; i < n; i++) max_len = std::max(max_len, (int)(roff[i + 1] - roff[i]));
        for (int l = 1; l <= max_len; l++) libs[c].prepare(pol[c], l, entries_all != 0);
        t.cls[c].lib = libs[c].view(); t.cls[c].pol = pol[c]; t.cls[c].pass = cls_pass[c];
    }
    t.anticodon = anticodon;
    std::vector<uint32_t> r32((size_t)n_rows + 1);
    for (int64_t k = 0; k < n_rows; k++) r32[(size_t)k] = R.handle[(size_t)rows[k]];
    std::vector<unsigned long long> cnt((size_t)n_rows + 1, 0), off((size_t)n_rows + 1, 0);
    uint32_t flags[16] = {0};
    const uint32_t nr = (uint32_t)n_rows;
    launch(2, 64, [&] { k_trf_hits<1, false>(t, r32.data(), nr, cnt.data(), off.data(), nullptr, flags); });
    launch(2, 64, [&] { k_trf_hits<2, false>(t, r32.data(), nr, cnt.data(), off.data(), nullptr, flags); });
    launch(2, 64, [&] { k_trf_hits<4, false>(t, r32.data(), nr, cnt.data(), off.data(), nullptr, flags); });
    launch(2, 64, [&] { k_trf_hits<8, false>(t, r32.data(), nr, cnt.data(), off.data(), nullptr, flags); });
    if (flags[0]) return -100 - (long long)flags[0];
    for (int64_t k = 0; k < n_rows; k++) off[(size_t)k + 1] = off[(size_t)k] + cnt[(size_t)k];
    const unsigned long long n_rec = off[(size_t)n_rows];
    if ((long long)n_rec > cap) return -2;
    std::vector<unsigned long long> keys((size_t)n_rec + 1, ~0ull);
    launch(3, 32, [&] { k_trf_hits<1, true>(t, r32.data(), nr, cnt.data(), off.data(), keys.data(), flags); });
    launch(3, 32, [&] { k_trf_hits<2, true>(t, r32.data(), nr, cnt.data(), off.data(), keys.data(), flags); });
    launch(3, 32, [&] { k_trf_hits<4, true>(t, r32.data(), nr, cnt.data(), off.data(), keys.data(), flags); });
    launch(3, 32, [&] { k_trf_hits<8, true>(t, r32.data(), nr, cnt.data(), off.data(), keys.data(), flags); });
    if (flags[0]) return -100 - (long long)flags[0];
    std::sort(keys.begin(), keys.begin() + (size_t)n_rec);
    launch(2, 64, [&] { k_trf_finish(t, r32.data(), keys.data(), (uint32_t)n_rec, o_row, o_ref, o_off, o_mm, o_cls, o_type); });
    return (long long)n_rec;
}

extern "C" int sim_trf_assign(const char* reads, const int64_t* roff, int64_t n, int64_t n_rows, const int64_t* read, const int32_t* tref,
                              const int32_t* start, int64_t n_tref, const uint32_t* ref_ptr, int64_t n_trf, const uint32_t* str_off,
                              const uint8_t* str, const int32_t* c_start, const int32_t* c_end, const int32_t* rank, int32_t* dist, int32_t* trf) {
    TrfTables t;
    std::memset(&t, 0, sizeof(t));
    SimReads R;
    std::vector<int8_t> none((size_t)n + 1, -1);
    if (int rc = R.fill(reads, roff, n, none.data(), none.data(), t)) return rc;
    std::vector<uint32_t> r32((size_t)n_rows + 1);
    for (int64_t k = 0; k < n_rows; k++) r32[(size_t)k] = R.handle[(size_t)read[k]];
    TrfInfor f{ref_ptr, str_off, str, c_start, c_end, rank, (uint32_t)n_tref, (uint32_t)n_trf};
    launch(2, 64, [&] { k_trf_assign(t, f, r32.data(), tref, start, (uint32_t)n_rows, dist, trf); });
    return 0;
}
