// fq_sim.cpp -- the kernels of csrc/kernels_fq.hpp compiled for the HOST (tests/test_trimmed_out_hostsim.py): the same kernel source, a workgroup's
// threads one after the other between its barriers (MIRGE_FQ_HOSTSIM; an atomic is then a plain read-modify-write), the launches in the order of
// csrc/native_fq.hpp: k_fq_measure, the exclusive scan, then k_fq_write chunk by chunk into a 16-byte aligned buffer of the chunk's size.
// With -DFQ_SIM_MAIN a stand-alone program over generated texts that also holds every stream against a plain construction, for a sanitizer
// build of this host code.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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
#define MIRGE_FQ_HOSTSIM 1
struct D3 { unsigned x, y; };
static D3 threadIdx, blockIdx, blockDim, gridDim;
struct alignas(16) uint4 { uint32_t x, y, z, w; };
template <class T> static T atomicAdd(T* p, T v) { const T o = *p; *p += v; return o; }
#include "../../mirge3.0_amd/csrc/kernels_fq.hpp"

template <class F> static void launch(unsigned grid, unsigned block, F f) {
    gridDim.x = grid; gridDim.y = 1; blockDim.x = block; blockDim.y = 1;
    for (unsigned b = 0; b < grid; b++) { blockIdx.x = b; blockIdx.y = 0; threadIdx.x = 0; threadIdx.y = 0; f(); }
}

// One piece: n records of `text` (bounds relative to the piece's first byte; q: null unless format 1; vstart / vend [n][vstride] or null, the last
// column holds the bounds after the last modifier) -> its part of S in out[0 .. *out_n) (-2: out_cap is too small), counts[3] = written, too
// short, mismatched records.  tile / chunk as MIRGE_FQ_TILE_BYTES / MIRGE_FQ_CHUNK_BYTES; grid: workgroups of either kernel (few: the strides run).
extern "C" int sim_fq_piece(const uint8_t* text, const int64_t* lstart, const int64_t* lend, const int64_t* qstart, const int64_t* qend,
                            const int64_t* vstart, const int64_t* vend, int32_t vstride, int64_t n, int32_t format, int32_t min_len, int64_t tile,
                            int64_t chunk, int32_t grid, uint8_t* out, int64_t out_cap, int64_t* out_n, unsigned long long* counts) {
    *out_n = 0;
    counts[0] = counts[1] = counts[2] = 0;
    if (n <= 0) return 0;
    if (tile < 16 || tile > MIRGE_FQ_MAX_TILE || (tile & 15)) return -1;
    chunk = std::max(chunk, tile) / tile * tile;
    FqJob j;
    std::memset(&j, 0, sizeof(j));
    j.text = text; j.lstart = lstart; j.lend = lend; j.qstart = qstart; j.qend = qend;
    if (vstart) { j.vstart = vstart; j.vend = vend; j.vstride = (uint32_t)vstride; j.voff = (uint32_t)vstride - 1; }
    j.n = (uint32_t)n; j.format = format; j.min_len = min_len;
    std::vector<FqRec> recs((size_t)n);
    std::vector<unsigned long long> bytes((size_t)n + 1, 0ull), off((size_t)n + 1, 0ull);
    launch((unsigned)std::max(1, grid), MIRGE_BLOCK, [&] { k_fq_measure(j, recs.data(), bytes.data(), counts); });
    for (int64_t r = 0; r < n; r++) off[(size_t)r + 1] = off[(size_t)r] + bytes[(size_t)r];
    const unsigned long long total = off[(size_t)n];
    if (counts[2]) return 0;  // (the host refuses the piece here)
    if ((int64_t)total > out_cap) return -2;
    for (unsigned long long at = 0; at < total; at += (unsigned long long)chunk) {
        const uint32_t nn = (uint32_t)std::min<unsigned long long>((unsigned long long)chunk, total - at);
        uint8_t* buf = static_cast<uint8_t*>(std::aligned_alloc(16, ((size_t)nn + 15) & ~size_t(15)));  // exactly the chunk: a byte past it is a finding
        if (!buf) return -3;
        launch((unsigned)std::max(1, grid), MIRGE_BLOCK, [&] { k_fq_write(text, recs.data(), off.data(), (uint32_t)n, format, at, nn, (uint32_t)tile, buf); });
        std::memcpy(out + at, buf, nn);
        std::free(buf);
    }
    *out_n = (int64_t)total;
    return 0;
}

#ifdef FQ_SIM_MAIN
int main() {
    uint64_t state = 99, sum = 0;
    auto rnd = [&](uint64_t m) { state = state * 6364136223846793005ull + 1442695040888963407ull; return (state >> 33) % m; };
    for (int set = 0; set < 36; set++) {
        const int format = 1 + set % 3, n = (int)rnd(700), stride = 1 + (int)rnd(3), min_len = set % 2 ? 16 : 0;
        const bool trim = set % 4 != 0, cr_ok = set % 5 == 0;
        std::string text, want;
        std::vector<int64_t> ls, le, qs, qe, vs, ve;
        const size_t lens[] = {0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 300, 5000};
        for (int r = 0; r < n; r++) {
            const size_t L = rnd(8) ? 15 + rnd(40) : lens[rnd(12)], H = rnd(6) ? 2 + rnd(20) : lens[1 + rnd(10)];
            const bool cr = cr_ok && rnd(3) == 0;
            std::string head, seq, qual;
            if (format != 3) { head = format == 1 ? "@" : ">"; for (size_t p = 1; p < H; p++) head += (char)('a' + rnd(26)); }
            for (size_t p = 0; p < L; p++) { seq += "ACGTNacgu."[rnd(10)]; qual += (char)(33 + rnd(60)); }
            if (format != 3) text += head + (cr ? "\r\n" : "\n");
            ls.push_back((int64_t)text.size());
            text += seq + (cr ? "\r" : "");
            le.push_back((int64_t)text.size());
            text += "\n";
            if (format == 1) {
                text += cr ? "+x\r\n" : "+\n";
                qs.push_back((int64_t)text.size());
                text += qual + (cr ? "\r" : "");
                qe.push_back((int64_t)text.size());
                text += "\n";
            }
            const size_t a = trim ? rnd(L + 1) : 0, b = trim ? a + rnd(L - a + 1) : L;
            for (int s = 0; s < stride; s++) { vs.push_back(ls.back() + (int64_t)(s == stride - 1 ? a : 0)); ve.push_back(ls.back() + (int64_t)(s == stride - 1 ? b : L)); }
            if ((int)(b - a) >= min_len) {
                if (format != 3) want += head + "\n";
                want += seq.substr(a, b - a) + "\n";
                if (format == 1) want += "+\n" + qual.substr(a, b - a) + "\n";
            }
        }
        text += "\n\n\n\n\n\n\n\n";
        const int64_t tiles[] = {64, 256, MIRGE_FQ_MAX_TILE}, chunks[] = {4096, 32 << 20};
        std::vector<uint8_t> out(want.size() + 16);
        int64_t out_n = 0;
        unsigned long long counts[3];
        if (sim_fq_piece((const uint8_t*)text.data(), ls.data(), le.data(), format == 1 ? qs.data() : nullptr, format == 1 ? qe.data() : nullptr, trim ? vs.data() : nullptr,
                         trim ? ve.data() : nullptr, stride, n, format, min_len, tiles[set % 3], chunks[set % 2], 1 + set % 3, out.data(), (int64_t)want.size(), &out_n, counts))
            return 1;
        if (out_n != (int64_t)want.size() || std::memcmp(out.data(), want.data(), want.size()) != 0 || counts[0] + counts[1] != (unsigned long long)n || counts[2]) {
            std::printf("fq_sim: set %d differs\n", set);
            return 2;
        }
        for (size_t x = 0; x < want.size(); x++) sum += out[x];
    }
    std::printf("fq_sim: 36 sets equal their plain construction, checksum %llu\n", (unsigned long long)sum);
    return 0;
}
#endif
