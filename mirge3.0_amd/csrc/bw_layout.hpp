// bw_layout.hpp -- the host bookkeeping of a bigWig file (mirge3_amd/bigwig.py holds the specification): header, zoom headers, total
// summary, chromosome B+ tree and the R-trees, from the per-block sizes and bounds that the device hands back.  Plain C++ without HIP:
// native_bw.hpp and tests/hostsim/bw_sim.cpp both build their files with it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#define MIRGE_BW_MAGIC 0x888FFC26u
#define MIRGE_BW_TREE_MAGIC 0x78CA8C91u
#define MIRGE_BW_INDEX_MAGIC 0x2468ACE0u
#define MIRGE_BW_RTREE_BLOCK 256u

struct BwPlaced { uint32_t chrom, start, end; uint64_t off, size; };  // a block in the file
struct BwTotals { uint64_t bases = 0; double vmin = 0, vmax = 0, sum = 0, sq = 0; };
struct BwZoomHead { uint32_t reduction; uint64_t data_at, index_at; };

struct BwBytes {
    std::vector<uint8_t> b;
    void raw(const void* p, size_t n) { const uint8_t* q = static_cast<const uint8_t*>(p); b.insert(b.end(), q, q + n); }
    void u8(uint8_t v) { b.push_back(v); }
    void u16(uint16_t v) { for (int k = 0; k < 2; k++) b.push_back((uint8_t)(v >> (8 * k))); }
    void u32(uint32_t v) { for (int k = 0; k < 4; k++) b.push_back((uint8_t)(v >> (8 * k))); }
    void u64(uint64_t v) { for (int k = 0; k < 8; k++) b.push_back((uint8_t)(v >> (8 * k))); }
    void f64(double v) { uint64_t w; std::memcpy(&w, &v, 8); u64(w); }
    void pad_to(size_t n) { b.resize(n, 0); }
};

// levels of a bulk-loaded tree over n items with B per node: counts[0] = leaves .. counts.back() = 1 (the root)
inline std::vector<uint64_t> bw_levels(uint64_t n, uint64_t B) {
    std::vector<uint64_t> counts{std::max<uint64_t>(1, (n + B - 1) / B)};
    while (counts.back() > 1) counts.push_back((counts.back() + B - 1) / B);
    return counts;
}

// keys: the chromosome names sorted by bytes (chromId = index), sizes[chromId]; the tree lies at file offset `at`
inline void bw_chrom_tree(const std::vector<std::string>& keys, const std::vector<uint32_t>& sizes, uint64_t at, BwBytes& o) {
    const uint64_t n = keys.size(), B = std::min<uint64_t>(256, n);
    size_t ks = 0;
    for (const auto& k : keys) ks = std::max(ks, k.size());
    o.u32(MIRGE_BW_TREE_MAGIC); o.u32((uint32_t)B); o.u32((uint32_t)ks); o.u32(8); o.u64(n); o.u64(0);
    const std::vector<uint64_t> counts = bw_levels(n, B);
    const uint64_t node = 4 + B * (ks + 8);
    std::vector<uint64_t> first(counts.size());
    uint64_t pos = at + 32;
    for (size_t lv = counts.size(); lv-- > 0;) { first[lv] = pos; pos += counts[lv] * node; }
    for (size_t lv = counts.size(); lv-- > 0;) {
        uint64_t span = B;
        for (size_t k = 0; k < lv; k++) span *= B;
        const uint64_t sub = span / B;
        for (uint64_t k = 0; k < counts[lv]; k++) {
            const uint64_t lo = k * span, hi = std::min(n, (k + 1) * span);
            const size_t node_at = o.b.size();
            o.u8(lv == 0 ? 1 : 0); o.u8(0); o.u16((uint16_t)((hi - lo + sub - 1) / sub));
            for (uint64_t i = lo; i < hi; i += sub) {
                const size_t key_at = o.b.size();
                o.raw(keys[i].data(), keys[i].size());
                o.pad_to(key_at + ks);
                if (lv == 0) { o.u32((uint32_t)i); o.u32(sizes[i]); }
                else o.u64(first[lv - 1] + (i / sub) * node);
            }
            o.pad_to(node_at + node);
        }
    }
}

// the R-tree over `blocks` at file offset `at`; data_end = where the indexed data ends
inline void bw_rtree(const std::vector<BwPlaced>& blocks, uint64_t at, uint64_t data_end, BwBytes& o) {
    const uint64_t n = blocks.size(), B = MIRGE_BW_RTREE_BLOCK;
    auto top_of = [&](uint64_t lo, uint64_t hi, uint32_t& tc, uint32_t& te) {
        tc = te = 0;
        for (uint64_t i = lo; i < hi; i++)
            if (blocks[i].chrom > tc || (blocks[i].chrom == tc && blocks[i].end > te)) { tc = blocks[i].chrom; te = blocks[i].end; }
    };
    uint32_t tc = 0, te = 0;
    top_of(0, n, tc, te);
    o.u32(MIRGE_BW_INDEX_MAGIC); o.u32((uint32_t)B); o.u64(n);
    o.u32(n ? blocks[0].chrom : 0); o.u32(n ? blocks[0].start : 0); o.u32(tc); o.u32(te);
    o.u64(data_end); o.u32(1); o.u32(0);
    const std::vector<uint64_t> counts = bw_levels(n, B);
    auto node_size = [&](size_t lv) { return (uint64_t)4 + B * (lv == 0 ? 32 : 24); };
    std::vector<uint64_t> first(counts.size());
    uint64_t pos = at + 48;
    for (size_t lv = counts.size(); lv-- > 0;) { first[lv] = pos; pos += counts[lv] * node_size(lv); }
    for (size_t lv = counts.size(); lv-- > 0;) {
        uint64_t span = B;
        for (size_t k = 0; k < lv; k++) span *= B;
        const uint64_t sub = span / B;
        for (uint64_t k = 0; k < counts[lv]; k++) {
            const uint64_t lo = std::min(n, k * span), hi = std::min(n, (k + 1) * span);
            const size_t node_at = o.b.size();
            o.u8(lv == 0 ? 1 : 0); o.u8(0); o.u16((uint16_t)((hi - lo + sub - 1) / sub));
            for (uint64_t i = lo; i < hi; i += sub) {
                if (lv == 0) {
                    const BwPlaced& p = blocks[i];
                    o.u32(p.chrom); o.u32(p.start); o.u32(p.chrom); o.u32(p.end); o.u64(p.off); o.u64(p.size);
                } else {
                    uint32_t c = 0, e = 0;
                    top_of(i, std::min(n, i + sub), c, e);
                    o.u32(blocks[i].chrom); o.u32(blocks[i].start); o.u32(c); o.u32(e); o.u64(first[lv - 1] + (i / sub) * node_size(lv - 1));
                }
            }
            o.pad_to(node_at + (size_t)node_size(lv));
        }
    }
}

// bytes [0, tree end) of the file: header, zoom headers, total summary, chromosome tree.  The data start behind them.
inline void bw_front(const std::vector<std::string>& keys, const std::vector<uint32_t>& sizes, const std::vector<BwZoomHead>& zoom, uint64_t index_at,
                     const BwTotals& t, uint32_t uncompress_buf, BwBytes& o) {
    const uint64_t Z = zoom.size(), summary_at = 64 + 24 * Z, tree_at = summary_at + 40;
    BwBytes tree;
    bw_chrom_tree(keys, sizes, tree_at, tree);
    o.u32(MIRGE_BW_MAGIC); o.u16(4); o.u16((uint16_t)Z); o.u64(tree_at); o.u64(tree_at + tree.b.size()); o.u64(index_at);
    o.u16(0); o.u16(0); o.u64(0); o.u64(summary_at); o.u32(uncompress_buf); o.u64(0);
    for (const auto& z : zoom) { o.u32(z.reduction); o.u32(0); o.u64(z.data_at); o.u64(z.index_at); }
    o.u64(t.bases); o.f64(t.vmin); o.f64(t.vmax); o.f64(t.sum); o.f64(t.sq);
    o.raw(tree.b.data(), tree.b.size());
}
inline uint64_t bw_front_bytes(const std::vector<std::string>& keys, size_t n_zoom) {
    const uint64_t n = keys.size(), B = std::min<uint64_t>(256, n);
    size_t ks = 0;
    for (const auto& k : keys) ks = std::max(ks, k.size());
    uint64_t nodes = 0;
    for (uint64_t c : bw_levels(n, B)) nodes += c;
    return 64 + 24 * n_zoom + 40 + 32 + nodes * (4 + B * (ks + 8));
}
