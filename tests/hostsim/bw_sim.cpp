// bw_sim.cpp -- csrc/kernels_bw.hpp compiled for the HOST (tests/test_bigwig_hostsim.py): the same kernel source, the launches in the
// order of csrc/native_bw.hpp (BwJob::write / one_file / stream), the file put together by the same csrc/bw_layout.hpp.  The kernels
// without a barrier run a launch's threads one after the other; k_bw_blocks, which builds and deflates a block in LDS behind barriers,
// runs ONE workgroup of 256 std::threads that takes the blocks in turn (its own grid-stride loop), so that a lane's segment is what it
// is on the device.  hipCUB's scans are loops; all blocks of a stream go through one launch (the device's groups only bound memory).
// Built with -DBW_SIM_MAIN it is a program of its own (a fixed set of runs through both deflate routes) for an ASan / UBSan build.
#include <algorithm>
#include <atomic>
#include <climits>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <vector>
#include <linux/futex.h>
#include <sys/syscall.h>
#include <unistd.h>
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
#define __shared__ static
struct D3 { unsigned x; };
static thread_local D3 threadIdx;
static D3 blockIdx, blockDim, gridDim;
struct Barrier { int n = 0; std::atomic<int> count{0}; std::atomic<int> gen{0};
  void wait() {
    const int g = gen.load(std::memory_order_acquire);
    if (count.fetch_add(1, std::memory_order_acq_rel) + 1 == n) {
      count.store(0, std::memory_order_relaxed); gen.store(g + 1, std::memory_order_release);
      syscall(SYS_futex, reinterpret_cast<int*>(&gen), FUTEX_WAKE_PRIVATE, INT32_MAX, nullptr, nullptr, 0);
    } else
      while (gen.load(std::memory_order_acquire) == g) syscall(SYS_futex, reinterpret_cast<int*>(&gen), FUTEX_WAIT_PRIVATE, g, nullptr, nullptr, 0);
  } };
static Barrier* g_bar;
static void __syncthreads() { g_bar->wait(); }
struct uint4 { uint32_t x, y, z, w; };
static std::mutex g_am;
template <class T> T atomicOr(T* p, T v) { std::lock_guard<std::mutex> l(g_am); T o = *p; *p |= v; return o; }
template <class T> T atomicXor(T* p, T v) { std::lock_guard<std::mutex> l(g_am); T o = *p; *p ^= v; return o; }
template <class T> T atomicAdd(T* p, T v) { std::lock_guard<std::mutex> l(g_am); T o = *p; *p += v; return o; }
template <class T> T atomicMin(T* p, T v) { std::lock_guard<std::mutex> l(g_am); T o = *p; if (v < o) *p = v; return o; }
template <class T> T atomicMax(T* p, T v) { std::lock_guard<std::mutex> l(g_am); T o = *p; if (v > o) *p = v; return o; }
template <class T> T atomicCAS(T* p, T c, T v) { std::lock_guard<std::mutex> l(g_am); T o = *p; if (o == c) *p = v; return o; }
#define MIRGE_BLOCK 256
#define MIRGE_CSV_MAXG 10
#define MIRGE_COV_NO_SAM
struct CsvGroup { const uint64_t* seq; const uint64_t* nmask; const uint8_t* len; const uint32_t* counts; const int8_t* pass; const int32_t* ref; uint32_t base, n; int32_t W; int32_t len16; };
static inline int csv_len(const CsvGroup& g, uint32_t j) { return g.len16 ? (int)reinterpret_cast<const uint16_t*>(g.len)[j] : (int)g.len[j]; }
#include "../../mirge3.0_amd/csrc/kernels_sam.hpp"
#include "../../mirge3.0_amd/csrc/kernels_bam.hpp"
#include "../../mirge3.0_amd/csrc/kernels_cov.hpp"
#include "../../mirge3.0_amd/csrc/kernels_bw.hpp"
#include "../../mirge3.0_amd/csrc/bw_layout.hpp"

template <class F> static void launch(unsigned grid, unsigned block, F f) {  // kernels without a barrier
    gridDim.x = grid; blockDim.x = block;
    for (unsigned b = 0; b < grid; b++)
        for (unsigned t = 0; t < block; t++) { blockIdx.x = b; threadIdx.x = t; f(); }
}
template <class F> static void launch_group(unsigned block, F f) {  // one workgroup, its threads together
    gridDim.x = 1; blockDim.x = block; blockIdx.x = 0;
    Barrier bar; bar.n = (int)block; g_bar = &bar;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < block; t++) th.emplace_back([&, t] { threadIdx.x = t; f(); });
    for (auto& x : th) x.join();
}
static unsigned grid_of(size_t n) { return (unsigned)std::min<size_t>((n + MIRGE_BLOCK - 1) / MIRGE_BLOCK, 3); }

struct Sim {
    CovRuns r;
    uint32_t n_runs, n_rank, S, base;
    int deflate;
    std::vector<std::string> keys;
    std::vector<uint32_t> size_by_cid, rank_of_cid, cid, ln, first;
    std::vector<uint8_t> file;

    void put(const std::vector<uint8_t>& b, uint64_t at) {
        if (file.size() < at + b.size()) file.resize(at + b.size(), 0);
        std::copy(b.begin(), b.end(), file.begin() + at);
    }
    void cut(std::vector<BwBlk>& blk, uint64_t lo, uint64_t hi, uint32_t c) const {
        for (uint64_t a = lo; a < hi; a += S) blk.push_back(BwBlk{(uint32_t)a, (uint32_t)std::min<uint64_t>(S, hi - a), c});
    }
    int stream(bool records, const BwRec* recs, const std::vector<BwBlk>& blk, uint64_t& pos, std::vector<BwPlaced>& placed, uint32_t& largest) {
        const size_t nb = blk.size();
        if (!nb) return 0;
        const uint32_t payload = records ? S * 32u : 24u + S * 12u, stride = (payload + 11u + 15u) & ~15u;
        std::vector<uint8_t> slots(nb * stride + 16, 0xEE), out(nb * stride + 16, 0xEE);
        std::vector<uint32_t> sizes(nb + 1, 0), off(nb + 1, 0), bounds(3 * nb, 0);
        if (records) launch_group(MIRGE_BLOCK, [&] { k_bw_blocks<true>(r, recs, blk.data(), (uint32_t)nb, deflate, stride, slots.data(), sizes.data(), bounds.data()); });
        else launch_group(MIRGE_BLOCK, [&] { k_bw_blocks<false>(r, recs, blk.data(), (uint32_t)nb, deflate, stride, slots.data(), sizes.data(), bounds.data()); });
        for (size_t b = 0; b < nb; b++) {
            if (sizes[b] == 0 || sizes[b] > stride) return -3;
            for (uint32_t x = sizes[b]; x < stride; x++) if (slots[b * stride + x] != 0xEE) return -4;  // (nothing behind the block in its slot)
            off[b + 1] = off[b] + sizes[b];
        }
        launch(std::min<unsigned>((unsigned)nb, 3), 8, [&] { k_bam_compact(slots.data(), stride, sizes.data(), off.data(), (uint32_t)nb, out.data()); });
        for (size_t b = 0; b < nb; b++) {
            placed.push_back(BwPlaced{bounds[3 * b], bounds[3 * b + 1], bounds[3 * b + 2], pos + off[b], sizes[b]});
            largest = std::max(largest, records ? blk[b].count * 32u : 24u + blk[b].count * 12u);
        }
        put(std::vector<uint8_t>(out.begin(), out.begin() + off[nb]), pos);
        pos += off[nb];
        return 0;
    }
    int one_file(int f, int64_t* stats) {
        const uint32_t* fr = first.data() + (size_t)f * n_rank;
        const uint32_t r0 = n_runs ? fr[0] : 0, r1 = n_runs ? fr[n_rank] : 0, n = r1 - r0;
        std::vector<BwBlk> secs;
        for (uint32_t k = 0; k < n_rank && n; k++) cut(secs, fr[rank_of_cid[k]], fr[rank_of_cid[k] + 1], k);
        std::vector<BwZoomHead> zoom;
        std::vector<std::vector<BwBlk>> zblk;
        std::vector<std::vector<BwRec>> zrec;
        unsigned long long prev = n;
        for (int k = 0; k < MIRGE_BW_MAX_LEVELS && n; k++) {
            const unsigned long long R64 = (unsigned long long)base << (2 * k);
            if (R64 > MIRGE_BW_MAX_REDUCTION) break;
            const uint32_t R = (uint32_t)R64;
            std::vector<unsigned long long> cnt(n + 1, 0), off(n + 1, 0), pick((size_t)n_rank + 1, 0);
            launch(grid_of(n), MIRGE_BLOCK, [&] { k_bw_zoom_count(r, r0, r1, R, cnt.data()); });
            for (uint32_t x = 0; x < n; x++) off[x + 1] = off[x] + cnt[x];
            const unsigned long long n_k = off[n];
            if (2 * n_k > prev) break;
            std::vector<uint32_t> rec_run(n_k), rec_bin(n_k);
            zrec.emplace_back(n_k);
            launch(grid_of(n), MIRGE_BLOCK, [&] { k_bw_zoom_bins(r, r0, r1, R, off.data(), rec_run.data(), rec_bin.data()); });
            launch(grid_of(n_k), MIRGE_BLOCK, [&] { k_bw_zoom_reduce(r, r1, rec_run.data(), rec_bin.data(), (uint32_t)n_k, R, ln.data(), cid.data(), zrec.back().data()); });
            launch(grid_of(n_rank + 1), MIRGE_BLOCK, [&] { k_bw_pick(off.data(), fr, n_rank + 1u, r0, pick.data()); });
            zblk.emplace_back();
            for (uint32_t cx = 0; cx < n_rank; cx++) cut(zblk.back(), pick[rank_of_cid[cx]], pick[rank_of_cid[cx] + 1], cx);
            zoom.push_back(BwZoomHead{R, 0, 0});
            prev = n_k;
        }
        BwTotals tot;
        if (!secs.empty()) {
            std::vector<BwPart> part(secs.size());
            launch(grid_of(secs.size()), MIRGE_BLOCK, [&] { k_bw_summary(r, secs.data(), (uint32_t)secs.size(), part.data()); });
            tot.vmin = part[0].vmin; tot.vmax = part[0].vmax;
            for (const BwPart& p : part) {
                tot.bases += p.bases; tot.vmin = std::min(tot.vmin, p.vmin); tot.vmax = std::max(tot.vmax, p.vmax);
                tot.sum = bw_add(tot.sum, p.sum); tot.sq = bw_add(tot.sq, p.sq);
            }
        }
        const uint64_t data_at = bw_front_bytes(keys, zoom.size());
        uint64_t pos = data_at + 8;
        uint32_t largest = 0;
        std::vector<BwPlaced> placed;
        file.clear();
        int rc = stream(false, nullptr, secs, pos, placed, largest);
        if (rc) return rc;
        BwBytes o;
        o.u64(secs.size()); put(o.b, data_at);
        const uint64_t index_at = pos;
        o.b.clear(); bw_rtree(placed, index_at, index_at, o); put(o.b, pos); pos += o.b.size();
        for (size_t k = 0; k < zoom.size(); k++) {
            zoom[k].data_at = pos;
            o.b.clear(); o.u32((uint32_t)zrec[k].size()); put(o.b, pos); pos += 4;
            placed.clear();
            if ((rc = stream(true, zrec[k].data(), zblk[k], pos, placed, largest))) return rc;
            zoom[k].index_at = pos;
            o.b.clear(); bw_rtree(placed, pos, pos, o); put(o.b, pos); pos += o.b.size();
        }
        o.b.clear(); o.u32(MIRGE_BW_MAGIC); put(o.b, pos); pos += 4;
        o.b.clear(); bw_front(keys, size_by_cid, zoom, index_at, tot, deflate ? largest : 0u, o);
        if (o.b.size() != data_at) return -5;
        put(o.b, 0);
        stats[0] = (int64_t)secs.size(); stats[1] = n; stats[2] = (int64_t)zoom.size(); stats[3] = (int64_t)pos;
        for (size_t k = 0; k < zoom.size(); k++) stats[5 + k] = (int64_t)zrec[k].size();
        return 0;
    }
};

// The runs (file order: plus strand first, then rank, then start) -> file f of n_str.  Returns the file's bytes in out, -1: a run beyond
// its chromosome's LN (err = rank, end, LN), -2: out too small, -3 .. -5: an inconsistency of the simulation.  stats[16] as the device's.
extern "C" long long sim_bigwig(uint32_t n_runs, uint8_t* strand, int32_t* chrom, int64_t* start, int64_t* end, int64_t* depth, int32_t n_rank,
                                const char* name_data, const int64_t* name_off, const int64_t* ln, const int32_t* cid, int32_t n_str, int32_t f,
                                uint32_t S, uint32_t base, int32_t deflate, uint8_t* out, long long out_cap, int64_t* stats, int64_t* err) {
    for (int k = 0; k < 16; k++) stats[k] = 0;
    Sim s;
    std::vector<long long> st(start, start + n_runs), en(end, end + n_runs), dp(depth, depth + n_runs);
    s.r = CovRuns{strand, chrom, st.data(), en.data(), dp.data()};
    s.n_runs = n_runs; s.n_rank = (uint32_t)n_rank; s.S = S; s.base = base; s.deflate = deflate;
    s.keys.assign(n_rank, std::string()); s.size_by_cid.assign(n_rank, 0); s.rank_of_cid.assign(n_rank, 0); s.cid.resize(n_rank); s.ln.resize(n_rank);
    for (int32_t r = 0; r < n_rank; r++) {
        s.rank_of_cid[cid[r]] = (uint32_t)r;
        s.keys[cid[r]].assign(name_data + name_off[r], name_data + name_off[r + 1]);
        s.size_by_cid[cid[r]] = (uint32_t)ln[r]; s.cid[r] = (uint32_t)cid[r]; s.ln[r] = (uint32_t)ln[r];
    }
    const size_t nq = (size_t)n_str * n_rank + 1;
    s.first.assign(nq, 0);
    if (n_runs) {
        uint32_t herr = MIRGE_BW_NONE;
        unsigned long long maxd[2] = {0, 0};
        launch(grid_of(n_runs), MIRGE_BLOCK, [&] { k_bw_limits(s.r, n_runs, s.ln.data(), &herr, maxd); });
        launch(grid_of(nq), MIRGE_BLOCK, [&] { k_bw_ranges(s.r, n_runs, (uint32_t)n_rank, (uint32_t)n_str, s.first.data()); });
        if (herr != MIRGE_BW_NONE) { err[0] = chrom[herr]; err[1] = end[herr]; err[2] = ln[chrom[herr]]; return -1; }
        stats[4] = (int64_t)maxd[f];
    }
    const int rc = s.one_file(f, stats);
    if (rc) return rc;
    if ((long long)s.file.size() > out_cap) return -2;
    std::memcpy(out, s.file.data(), s.file.size());
    return (long long)s.file.size();
}

#ifdef BW_SIM_MAIN
int main() {
    // two strands, three chromosomes (rank order c, a, b: ids 2, 0, 1), one without a run; a run over many bins, abutting runs, a depth
    // beyond 2^24, a run that ends at its chromosome's LN
    std::vector<uint8_t> strand;
    std::vector<int32_t> chrom;
    std::vector<int64_t> start, end, depth;
    auto add = [&](int st, int ch, int64_t a, int64_t b, int64_t d) { strand.push_back((uint8_t)st); chrom.push_back(ch); start.push_back(a); end.push_back(b); depth.push_back(d); };
    for (int x = 0; x < 256; x++) add(0, 0, x, x + 1, 1 + x % 2);  // (dense enough for zoom levels to be kept)
    add(0, 0, 300, 460, 5); add(0, 2, 5, 9, 16777217); add(0, 2, 9, 10, 3); add(1, 0, 7, 8, 12884901886ll); add(1, 2, 990, 999, 0x4D4D4E);
    const uint32_t n_runs = (uint32_t)strand.size();
    const char names[] = "cab";
    const int64_t name_off[] = {0, 1, 2, 3}, ln[] = {1000, 50, 999};
    const int32_t cid[] = {2, 0, 1};
    int bad = 0;
    for (int deflate = 0; deflate < 2; deflate++)
        for (int f = 0; f < 2; f++)
            for (uint32_t S : {1u, 3u, 1024u}) {
                std::vector<uint8_t> out(1 << 20);
                int64_t stats[16], err[4] = {0, 0, 0, 0};
                const long long n = sim_bigwig(n_runs, strand.data(), chrom.data(), start.data(), end.data(), depth.data(), 3, names, name_off, ln, cid, 2, f, S, 4, deflate, out.data(), (long long)out.size(), stats, err);
                std::printf("deflate %d file %d S %u: %lld bytes, %lld sections, %lld items, %lld levels\n", deflate, f, S, n, (long long)stats[0], (long long)stats[1], (long long)stats[2]);
                bad |= n <= 0;
            }
    return bad;
}
#endif
