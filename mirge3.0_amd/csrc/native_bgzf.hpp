// native_bgzf.hpp -- part of mirge_native.hip (one translation unit): `--bgzf-out`, the text of `--sam-out` and `--coverage` written as
// BGZF where it is produced (kernels_bgzf.hpp; the format: mirge3_amd/bgzf.py).  BgzfSink sits between an exporter's text chunk and
// StagePipe (native_stage.hpp).  A stream S is cut into blocks of `block` bytes and a chunk holds a whole number of them, so the file
// is a function of S and the block size alone.  Per chunk: the exporter's `fill` puts the chunk's bytes into one of two device
// buffers; k_bgzf_text makes every block a member in its slot; one exclusive scan of the sizes and k_bam_compact close the gaps; the
// offsets, then the packed bytes, go to the chunk's half of the page-locked staging (as mirge_bam_write_device's take does) and into the
// file at the running offset, and the members' offsets are noted for the `.gzi`.  MIRGE_BGZF_DEFLATE=host: the chunk's text goes to the
// half as it does without the switch, and zlib level 6 makes the members on MIRGE_GZ_THREADS host threads (bam_host_member): the A/B
// route and the tests' second implementation.  Every file is written as `<path>.tmp` and renamed by the caller's commit_all when all
// files of the call are whole.  The blocks are the calling export's (its PoolScope).
// MIRGE_BGZF_BLOCK_BYTES (64 .. 65280, default 65280) and MIRGE_BGZF_DEFLATE (device | host) are read per call.
#pragma once

static int bam_host_member(const uint8_t* src, uint32_t n, std::vector<uint8_t>& out);  // native_bam.hpp

static const uint8_t kBgzfEofBlock[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#define MIRGE_BGZF_STATS 8  // int64 per file: file bytes, members stored, fixed, dynamic, members, stream bytes, 0, 0

// the block size of a call: block_bytes > 0 as given, else MIRGE_BGZF_BLOCK_BYTES, else 65280
static int bgzf_block_bytes(const std::string& who, int64_t block_bytes, uint32_t& block) {
    const long long v = block_bytes > 0 ? (long long)block_bytes : (long long)env_bytes("MIRGE_BGZF_BLOCK_BYTES", MIRGE_BAM_MAX_BLOCK);
    if (v < 64 || v > MIRGE_BAM_MAX_BLOCK) return fail(-1, who + ": a BGZF block holds 64 .. 65280 bytes (MIRGE_BGZF_BLOCK_BYTES)");
    block = (uint32_t)v;
    return 0;
}
static int bgzf_route(const std::string& who, bool& on_host) {
    const char* dv = std::getenv("MIRGE_BGZF_DEFLATE");
    on_host = dv && std::strcmp(dv, "host") == 0;
    if (dv && *dv && !on_host && std::strcmp(dv, "device") != 0) return fail(-1, who + ": MIRGE_BGZF_DEFLATE is 'device' or 'host'");
    return 0;
}

// one stream: its length, its two files, what has been written
struct BgzfStream {
    OutFile gz, gzi;
    unsigned long long bytes = 0, file_at = 0, members = 0;
    long long forms[3] = {0, 0, 0};
    std::vector<uint64_t> index;  // (compressed offset, uncompressed offset) of every member behind the first
    explicit BgzfStream(const std::string& who) : gz(who, true), gzi(who, true) {}
    int open(const char* path, const char* gzi_path) { CHECK(gz.open(path)); return gzi.open(gzi_path); }
    void stats(int64_t* out) const {
        out[0] = (int64_t)file_at; out[1] = forms[0]; out[2] = forms[1]; out[3] = forms[2]; out[4] = (int64_t)members; out[5] = (int64_t)bytes;
        out[6] = out[7] = 0;
    }
};

struct BgzfSink {
    PoolScope& scope;
    std::string who;
    uint32_t block = MIRGE_BAM_MAX_BLOCK;
    bool on_host = false;
    int T = 16;
    BgzfSink(PoolScope& s, std::string w) : scope(s), who(std::move(w)) {}
    int configure(int64_t block_bytes) {
        CHECK(bgzf_block_bytes(who, block_bytes, block));
        CHECK(bgzf_route(who, on_host));
        T = (int)std::max<size_t>(1, std::min<size_t>(env_bytes("MIRGE_GZ_THREADS", 16), 256));
        return 0;
    }
    // The streams, one behind the other, in chunks of chunk_bytes rounded down to whole blocks (one block at least).
    // fill(s, at, n, dst, &text): queue the production of bytes [at, at + n) of stream s somewhere in dst[0 .. n + 32) (16-aligned) and
    // say where in `text`.  Behind run() every stream's .gz ends with the EOF block and its .gzi is written; nothing is committed.
    // run = chunks (the members of bytes [0, bytes) of every stream) + close (the EOF blocks and the indexes).  A stream that arrives in parts
    // (`--trimmed-out`: native_fq.hpp) calls chunks once per part, with `bytes` = the part's length, a multiple of the block size except for the
    // last part, and `base` = the stream offset of the part's first byte: `at` counts within the part, the index holds stream offsets.
    template <class Fill>
    int run(BgzfStream* const* streams, int n_streams, size_t chunk_bytes, Fill fill) {
        CHECK(chunks(streams, n_streams, chunk_bytes, 0ull, fill));
        return close(streams, n_streams);
    }
    template <class Fill>
    int chunks(BgzfStream* const* streams, int n_streams, size_t chunk_bytes, unsigned long long base, Fill fill) {
        mirge_ctx* const c = scope.c;
        struct Chunk { int s; unsigned long long at; uint32_t n; };
        unsigned long long longest = 0;
        for (int s = 0; s < n_streams; s++) longest = std::max(longest, streams[s]->bytes);
        const size_t cb = (size_t)std::max<unsigned long long>(1, std::min<unsigned long long>(std::min<size_t>(chunk_bytes, (size_t)1 << 30) / block, (longest + block - 1) / block));
        const size_t cbytes = cb * block;
        std::vector<Chunk> plan;
        for (int s = 0; s < n_streams; s++)
            for (unsigned long long at = 0; at < streams[s]->bytes; at += cbytes)
                plan.push_back(Chunk{s, at, (uint32_t)std::min<unsigned long long>(cbytes, streams[s]->bytes - at)});
        const uint32_t slot_stride = (block + 31u + 15u) & ~15u;
        const size_t half = cb * slot_stride, meta = ((cb + 1) * 4 + 15) & ~size_t(15);
        uint8_t *d_text[2] = {nullptr, nullptr}, *d_comp[2] = {nullptr, nullptr}, *d_slots = nullptr;
        uint32_t *d_sizes = nullptr, *d_boff[2] = {nullptr, nullptr};
        void* tmp = nullptr;
        size_t tb = 0;
        std::vector<std::vector<uint8_t>> members;
        std::vector<uint8_t> joined;
        if (!plan.empty()) {
            StagePipe pipe(c, who, "a chunk failed on the device");
            CHECK(pipe.ensure(on_host ? cbytes : half + meta));
            for (int h = 0; h < (plan.size() < 2 ? 1 : 2); h++) {
                CHECK(scope.get(&d_text[h], cbytes + 48));
                if (!on_host) { CHECK(scope.get(&d_comp[h], half + 16)); CHECK(scope.get(&d_boff[h], cb + 1)); }
            }
            if (!on_host) {
                CHECK(scope.get(&d_slots, half + 16)); CHECK(scope.get(&d_sizes, cb + 1));
                HIPOK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, d_sizes, d_boff[0], (int)(cb + 1), c->stream));
                CHECK(scope.get((uint8_t**)&tmp, std::max<size_t>(tb, 16)));
            }
            auto queue = [&](unsigned long long ci) -> int {
                const Chunk& k = plan[(size_t)ci];
                const int h = (int)(ci & 1);
                const size_t nb = ((size_t)k.n + block - 1) / block;
                const uint8_t* text = nullptr;
                CHECK(fill(k.s, k.at, k.n, d_text[h], &text));
                if (text < d_text[h] || text > d_text[h] + 32) return fail(-6, who + ": a chunk's text lies outside its buffer");
                if (on_host) { HIPOK(hipMemcpyAsync(pipe.half(ci), text, k.n, hipMemcpyDeviceToHost, c->stream)); return 0; }
                {
                    LaunchScope ls(c, "k_bgzf_text", (double)k.n);
                    hipLaunchKernelGGL(k_bgzf_text, dim3((unsigned)nb), dim3(MIRGE_BLOCK), 0, c->stream, text, (unsigned long long)k.n, 0ull, (uint32_t)nb, block,
                                       slot_stride, d_slots, d_sizes);
                }
                HIPOK(hipMemsetAsync(d_sizes + nb, 0, 4, c->stream));
                HIPOK(hipcub::DeviceScan::ExclusiveSum(tmp, tb, d_sizes, d_boff[h], (int)(nb + 1), c->stream));
                {
                    LaunchScope ls(c, "k_bam_compact", (double)nb);
                    hipLaunchKernelGGL(k_bam_compact, dim3((unsigned)std::min<size_t>(nb, (size_t)c->n_cu * 8)), dim3(MIRGE_BLOCK), 0, c->stream, (const uint8_t*)d_slots,
                                       slot_stride, (const uint32_t*)d_sizes, (const uint32_t*)d_boff[h], (uint32_t)nb, d_comp[h]);
                }
                HIPOK(hipMemcpyAsync(pipe.half(ci) + half, d_boff[h], (nb + 1) * 4, hipMemcpyDeviceToHost, c->stream));
                return 0;
            };
            auto take = [&](unsigned long long ci) -> int {  // chunk ci's event has passed: fetch it, write it behind what its file holds
                const Chunk& k = plan[(size_t)ci];
                BgzfStream& st = *streams[k.s];
                const int h = (int)(ci & 1);
                const size_t nb = ((size_t)k.n + block - 1) / block;
                uint8_t* stage = pipe.half(ci);
                const uint8_t* src = stage;
                size_t total = 0;
                std::vector<uint32_t> at(nb + 1, 0u);
                if (!on_host) {
                    const uint32_t* boff = reinterpret_cast<const uint32_t*>(stage + half);  // exclusive scan of the members' sizes
                    for (size_t b = 0; b <= nb; b++) at[b] = boff[b];
                    total = at[nb];
                    for (size_t b = 0; b < nb; b++)
                        if (at[b + 1] < at[b] + 26u || at[b + 1] - at[b] > slot_stride) return fail(-6, who + ": a member of a chunk does not fit its slot");
                    if (hipMemcpyAsync(stage, d_comp[h], total, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
                        return fail(-2, who + ": the copy of a chunk failed");
                } else {
                    members.resize(nb);
                    std::atomic<int> bad{0};
                    mirge_gz::parallel_for((int)nb, T, [&](int b) {
                        const size_t b0 = (size_t)b * block;
                        if (bam_host_member(stage + b0, (uint32_t)std::min<size_t>(block, k.n - b0), members[(size_t)b])) bad = 1;
                    });
                    if (bad) return fail(-6, who + ": zlib could not deflate a block");
                    joined.clear();
                    for (size_t b = 0; b < nb; b++) { at[b] = (uint32_t)joined.size(); joined.insert(joined.end(), members[b].begin(), members[b].end()); }
                    at[nb] = (uint32_t)joined.size();
                    total = joined.size(); src = joined.data();
                }
                for (size_t b = 0; b < nb; b++) {
                    if (st.members) { st.index.push_back(st.file_at + at[b]); st.index.push_back(base + k.at + (unsigned long long)b * block); }
                    st.members++;
                    const uint32_t btype = (src[at[b] + 18] >> 1) & 3u;
                    if (btype < 3u) st.forms[btype]++;
                }
                if (int r = st.gz.put(src, total, st.file_at)) return r;
                st.file_at += total;
                return 0;
            };
            CHECK(pipe.run(plan.size(), queue, take));
        }
        return 0;
    }
    int close(BgzfStream* const* streams, int n_streams) {
        for (int s = 0; s < n_streams; s++) {
            BgzfStream& st = *streams[s];
            CHECK(st.gz.put(kBgzfEofBlock, sizeof(kBgzfEofBlock), st.file_at));
            st.file_at += sizeof(kBgzfEofBlock);
            std::vector<uint8_t> idx;
            auto p64 = [&](uint64_t v) { for (int x = 0; x < 8; x++) idx.push_back((uint8_t)(v >> (8 * x))); };
            p64(st.index.size() / 2);
            for (uint64_t v : st.index) p64(v);
            CHECK(st.gzi.put(idx.data(), idx.size(), 0));
        }
        return 0;
    }
};

// n bytes from the host as one .gz file with its .gzi, by the kernels of `--bgzf-out` (tests, other callers).  block_bytes <= 0:
// MIRGE_BGZF_BLOCK_BYTES.  stats_out[MIRGE_BGZF_STATS]: BgzfStream::stats.
extern "C" int mirge_bgzf_write(mirge_ctx* c, const uint8_t* bytes, int64_t n, int64_t block_bytes, const char* path, const char* gzi_path, int64_t* stats_out) {
    const std::string who = "mirge_bgzf_write";
    if (!c || n < 0 || (n && !bytes) || !path || !gzi_path) return fail(-1, who + ": bad argument");
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    BgzfStream st(who);
    BgzfStream* const streams[1] = {&st};
    PoolScope scope(c);
    BgzfSink sink(scope, who);
    CHECK(sink.configure(block_bytes));
    st.bytes = (unsigned long long)n;
    CHECK(st.open(path, gzi_path));
    auto fill = [&](int, unsigned long long at, uint32_t nn, uint8_t* dst, const uint8_t** text) -> int {
        HIPOK(hipMemcpyAsync(dst, bytes + at, nn, hipMemcpyHostToDevice, c->stream));
        *text = dst;
        return 0;
    };
    CHECK(sink.run(streams, 1, env_bytes("MIRGE_BGZF_CHUNK_BYTES", (size_t)32 << 20), fill));
    CHECK(commit_all({&st.gz, &st.gzi}));
    if (stats_out) st.stats(stats_out);
    return 0;
}
