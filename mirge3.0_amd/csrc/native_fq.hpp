// native_fq.hpp -- part of mirge_native.hip (one translation unit): `--trimmed-out` (kernels_fq.hpp; the specification: mirge3_amd/trimmed_out.py).
// mirge_fqout is the writer of ONE sample: its file(s), the stream offset and -- for BGZF -- the partial last block, alive across the pieces of a
// streamed sample.  mirge_reads_parse_trim_out is mirge_reads_parse_trim_qc plus, on the SAME ParseJob,
//   fq_measure  between parse_lines and parse_pack (k_seq_class writes the sliced bounds back over the parser's arrays): k_fq_measure, one 64-bit
//               scan -> rec_off[n + 1]; a quality line of the wrong length fails the call here, before the piece writes anything;
//   fq_emit     behind a parse_pack that succeeded: the piece's part of S in chunks of MIRGE_FQ_CHUNK_BYTES (default 32 MiB) by k_fq_write with
//               tiles of MIRGE_FQ_TILE_BYTES (a multiple of 16, at most MIRGE_FQ_MAX_TILE), through the page-locked halves (StagePipe) into the
//               file at the running offset.  S never exists whole.
// BGZF (gzi_path given): chunk bounds are multiples of the block size B in STREAM coordinates.  What a piece leaves behind its last whole block stays
// in a B-byte device carry and is the front of the next piece's first chunk; finish makes what is left the last, short member, writes the EOF block
// and the .gzi and commits.  The members are BgzfSink's (k_bgzf_text + k_bam_compact, or zlib with MIRGE_BGZF_DEFLATE=host): the file is a function
// of S and B alone.  Every file is written as `<path>.tmp`; a writer destroyed without finish, or one whose piece failed, leaves nothing.
#pragma once

struct mirge_fqout {
    mirge_ctx* ctx = nullptr;
    std::string who = "mirge_reads_parse_trim_out";
    bool gz = false, broken = false, finished = false;
    int32_t format = 0;  // of the first piece; every later piece has the same
    uint32_t block = MIRGE_BAM_MAX_BLOCK;
    bool on_host = false;
    int T = 16;
    OutFile plain;
    BgzfStream st;
    uint8_t* d_carry = nullptr;  // [block + 16]: S[done, done + carry_n)
    uint32_t carry_n = 0;
    unsigned long long done = 0;  // bytes of S in the file (plain) or in its members (BGZF)
    unsigned long long records = 0, written = 0, too_short = 0, stream = 0;
    mirge_fqout() : plain("mirge_reads_parse_trim_out", true), st("mirge_reads_parse_trim_out") {}
    void abandon() { plain.discard(); st.gz.discard(); st.gzi.discard(); broken = true; }
};

// a piece between fq_measure and fq_emit
struct FqPiece {
    PoolScope scope;
    FqRec* recs = nullptr;
    unsigned long long *bytes = nullptr, *off = nullptr, *counts = nullptr, total = 0, written = 0, too_short = 0;
    uint32_t n = 0;
    explicit FqPiece(mirge_ctx* c) : scope(c) {}
};

extern "C" void mirge_fqout_destroy(mirge_fqout* f) {
    if (!f) return;
    if (f->ctx && f->d_carry) { (void)hipStreamSynchronize(f->ctx->stream); f->ctx->release(f->d_carry); }
    delete f;  // (files not committed go with their OutFile)
}

extern "C" int mirge_fqout_create(mirge_ctx* c, const char* path, const char* gzi_path, int64_t block_bytes, mirge_fqout** out) {
    const std::string who = "mirge_fqout_create";
    if (!c || !path || !*path || !out) return fail(-1, who + ": bad argument");
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    auto f = std::make_unique<mirge_fqout>();
    f->ctx = c;
    f->gz = gzi_path != nullptr;
    if (f->gz) {  // (a wrong MIRGE_BGZF_* value: before anything is opened)
        CHECK(bgzf_block_bytes(who, block_bytes, f->block));
        CHECK(bgzf_route(who, f->on_host));
        f->T = (int)std::max<size_t>(1, std::min<size_t>(env_bytes("MIRGE_GZ_THREADS", 16), 256));
        CHECK(dalloc(c, &f->d_carry, (size_t)f->block + 16));
        const int rc = f->st.open(path, gzi_path);
        if (rc) { mirge_fqout_destroy(f.release()); return rc; }
    } else {
        CHECK(f->plain.open(path));
    }
    *out = f.release();
    return 0;
}

static int fq_sizes(const std::string& who, size_t& tile, size_t& chunk) {
    tile = env_bytes("MIRGE_FQ_TILE_BYTES", MIRGE_FQ_MAX_TILE);
    if (tile < 16 || tile > MIRGE_FQ_MAX_TILE || (tile & 15)) return fail(-1, who + ": MIRGE_FQ_TILE_BYTES is a multiple of 16, 16 .. " + std::to_string(MIRGE_FQ_MAX_TILE));
    chunk = env_bytes("MIRGE_FQ_CHUNK_BYTES", (size_t)32 << 20);
    chunk = std::min<size_t>((size_t)1 << 30, std::max(chunk, tile)) / tile * tile;
    return 0;
}

// J after parse_lines -> P: every record's place and bytes, rec_off, the counts
static void fq_piece_free(FqPiece* P) { delete P; }
static int fq_measure(ParseJob& J, const TrimOpts* topt, int32_t min_len, mirge_fqout* f, FqPiece** piece) {
    mirge_ctx* c = J.c;
    *piece = nullptr;
    const std::string& who = f->who;
    if (f->broken || f->finished) return fail(-1, who + ": the writer has failed or is finished");
    if (!J.n_raw) return 0;
    if (!f->format) f->format = J.format;
    if (f->format != J.format) return fail(-1, who + ": the pieces of a sample have one format");
    if (J.n_raw >= 0x7FFFFFF0u) return fail(-5, who + ": 2^31 records or more in one piece (hipCUB's scan takes an int count)");
    const bool trimming = topt && topt->n_mods > 0;
    if (J.format == 1 && (!J.qstart || !J.qend)) return fail(-1, who + ": internal: the quality lines were not marked");
    const size_t n = J.n_raw;
    std::unique_ptr<FqPiece, void (*)(FqPiece*)> owner(new FqPiece(c), fq_piece_free);
    FqPiece& P = *owner;
    CHECK(P.scope.get(&P.recs, n));
    CHECK(P.scope.get(&P.bytes, n + 1));
    CHECK(P.scope.get(&P.off, n + 1));
    CHECK(P.scope.get(&P.counts, 4));
    HIPOK(hipMemsetAsync(P.bytes + n, 0, 8, c->stream));
    HIPOK(hipMemsetAsync(P.counts, 0, 32, c->stream));
    FqJob j;
    std::memset(&j, 0, sizeof(j));
    j.text = J.dtext;
    j.lstart = trimming ? J.lstart : J.dstart; j.lend = trimming ? J.lend : J.dend;
    j.qstart = J.format == 1 ? J.qstart : nullptr; j.qend = J.format == 1 ? J.qend : nullptr;
    if (trimming) {  // the read after the LAST modifier
        j.vstart = J.dstart; j.vend = J.dend;
        j.vstride = (uint32_t)(J.n_seq / J.n_raw); j.voff = j.vstride - 1;
    }
    j.n = J.n_raw; j.format = J.format; j.min_len = min_len > 0 ? min_len : 0;
    {
        LaunchScope ls(c, "k_fq_measure", (double)n);
        hipLaunchKernelGGL(k_fq_measure, dim3(grid_for(c, n)), dim3(MIRGE_BLOCK), 0, c->stream, j, P.recs, P.bytes, P.counts);
    }
    size_t tb = 0;
    void* tmp = nullptr;
    HIPOK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, P.bytes, P.off, (int)(n + 1), c->stream));
    CHECK(P.scope.get((uint8_t**)&tmp, std::max<size_t>(tb, 16)));
    HIPOK(hipcub::DeviceScan::ExclusiveSum(tmp, tb, P.bytes, P.off, (int)(n + 1), c->stream));
    unsigned long long h[4] = {0, 0, 0, 0};
    HIPOK(hipMemcpyAsync(h, P.counts, 24, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(&h[3], P.off + n, 8, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    HIPOK(hipGetLastError());
    if (h[2]) return fail(-9, "--trimmed-out: mirge_reads_parse: a record's quality line is not as long as its sequence line");
    P.n = J.n_raw; P.written = h[0]; P.too_short = h[1]; P.total = h[3];
    *piece = owner.release();
    return 0;
}

static void fq_launch_write(mirge_ctx* c, const ParseJob& J, const FqPiece& P, unsigned long long at, uint32_t nn, size_t tile, uint8_t* dst) {
    const size_t tiles = ((size_t)nn + tile - 1) / tile;
    LaunchScope ls(c, "k_fq_write", (double)nn);
    hipLaunchKernelGGL(k_fq_write, dim3((unsigned)std::min<size_t>(tiles, (size_t)c->n_cu * 32)), dim3(MIRGE_BLOCK), 0, c->stream, (const uint8_t*)J.dtext,
                       (const FqRec*)P.recs, (const unsigned long long*)P.off, P.n, (int32_t)J.format, at, nn, (uint32_t)tile, dst);
}

// the piece's part of S into the writer's file(s); J's text is still on the device
static int fq_emit(ParseJob& J, mirge_fqout* f, FqPiece* piece) {
    mirge_ctx* c = J.c;
    const std::string& who = f->who;
    if (!piece || !piece->n) return 0;
    FqPiece& P = *piece;
    size_t tile, chunk;
    CHECK(fq_sizes(who, tile, chunk));
    const unsigned long long total = P.total;
    if (!f->gz) {
        if (total) {
            const size_t buf = (size_t)std::min<unsigned long long>(chunk, total);
            uint8_t* d_text[2] = {nullptr, nullptr};
            StagePipe pipe(c, who);
            CHECK(pipe.ensure(buf));
            CHECK(P.scope.get(&d_text[0], buf + 16));
            if (total > buf) CHECK(P.scope.get(&d_text[1], buf + 16));
            auto queue = [&](unsigned long long ci) -> int {
                const unsigned long long at0 = ci * chunk;
                const uint32_t nn = (uint32_t)std::min<unsigned long long>(chunk, total - at0);
                fq_launch_write(c, J, P, at0, nn, tile, d_text[ci & 1]);
                HIPOK(hipMemcpyAsync(pipe.half(ci), d_text[ci & 1], nn, hipMemcpyDeviceToHost, c->stream));
                return 0;
            };
            auto take = [&](unsigned long long ci) -> int {
                const unsigned long long at0 = ci * chunk;
                return f->plain.put(pipe.half(ci), (size_t)std::min<unsigned long long>(chunk, total - at0), f->done + at0);
            };
            CHECK(pipe.run((total + chunk - 1) / chunk, queue, take));
        }
        f->done += total;
    } else if (total) {
        // combined coordinates: x < carry_n is the carry's byte x, else the piece's byte x - carry_n; x stands at stream offset done + x
        const uint32_t B = f->block, carry_n = f->carry_n;
        const unsigned long long avail = (unsigned long long)carry_n + total, full = avail / B * B;
        if (full) {
            BgzfSink sink(P.scope, who);
            sink.block = B; sink.on_host = f->on_host; sink.T = f->T;
            BgzfStream* const gzs[1] = {&f->st};
            f->st.bytes = full;
            auto fill = [&](int, unsigned long long at, uint32_t nn, uint8_t* dst, const uint8_t** text) -> int {
                const uint32_t hpart = at < carry_n ? (uint32_t)std::min<unsigned long long>(nn, carry_n - at) : 0u, pad = (16u - (hpart & 15u)) & 15u, bn = nn - hpart;
                if (hpart) HIPOK(hipMemcpyAsync(dst + pad, f->d_carry + at, hpart, hipMemcpyDeviceToDevice, c->stream));
                if (bn) fq_launch_write(c, J, P, at + hpart - carry_n, bn, tile, dst + pad + hpart);  // (16-byte stores start at a multiple of 16)
                *text = dst + pad;
                return 0;
            };
            CHECK(sink.chunks(gzs, 1, chunk, f->done, fill));
        }
        // what lies behind the last whole block: the new carry (nothing was cut: the old carry stays in front of it)
        const unsigned long long tail_start = full ? full - carry_n : 0ull;
        const uint32_t tail_n = (uint32_t)(total - tail_start), keep = full ? 0u : carry_n;
        if (tail_n) {
            uint8_t* d_tail = nullptr;
            CHECK(P.scope.get(&d_tail, (size_t)tail_n + 16));
            fq_launch_write(c, J, P, tail_start, tail_n, tile, d_tail);
            HIPOK(hipMemcpyAsync(f->d_carry + keep, d_tail, tail_n, hipMemcpyDeviceToDevice, c->stream));
        }
        f->done += full;
        f->carry_n = keep + tail_n;
    }
    HIPOK(hipStreamSynchronize(c->stream));
    HIPOK(hipGetLastError());
    f->records += P.n; f->written += P.written; f->too_short += P.too_short; f->stream += total;
    return 0;
}

extern "C" int mirge_reads_parse_trim_out(mirge_ctx* c, const char* text, int64_t nbytes, int32_t format, int32_t min_len, const mirge_trim* trim,
                                          mirge_qc* qc, mirge_fqout* fq, mirge_reads** out, int64_t* n_records) {
    if (qc && qc->ctx != c) return fail(-1, "mirge_reads_parse_trim_out: the accumulator belongs to another context");
    if (fq && fq->ctx != c) return fail(-1, "mirge_reads_parse_trim_out: the writer belongs to another context");
    const int rc = reads_parse_impl(c, text, nbytes, format, min_len, trim, nullptr, out, n_records, nullptr, qc, fq);
    if (rc && fq) fq->abandon();  // (a failed piece: no trimmed file of this sample)
    return rc;
}

extern "C" int mirge_fqout_finish(mirge_ctx* c, mirge_fqout* f, int64_t* stats_out) {
    const std::string who = "mirge_fqout_finish";
    if (!c || !f || f->ctx != c) return fail(-1, who + ": bad argument");
    if (f->broken || f->finished) return fail(-1, who + ": the writer has failed or is finished");
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    int rc = 0;
    if (f->gz) {
        BgzfStream* const gzs[1] = {&f->st};
        {
            PoolScope scope(c);
            BgzfSink sink(scope, who);
            sink.block = f->block; sink.on_host = f->on_host; sink.T = f->T;
            if (f->carry_n) {  // the last, short member
                const uint32_t carry_n = f->carry_n;
                f->st.bytes = carry_n;
                auto fill = [&](int, unsigned long long at, uint32_t nn, uint8_t* dst, const uint8_t** text) -> int {
                    HIPOK(hipMemcpyAsync(dst, f->d_carry + at, nn, hipMemcpyDeviceToDevice, c->stream));
                    *text = dst;
                    return 0;
                };
                rc = sink.chunks(gzs, 1, (size_t)f->block, f->done, fill);
                if (rc == 0) { f->done += carry_n; f->carry_n = 0; }
            }
            if (rc == 0) rc = sink.close(gzs, 1);
        }
        f->st.bytes = f->stream;
        if (rc == 0 && f->done != f->stream) rc = fail(-6, who + ": the members do not add up to the stream");
        if (rc == 0) rc = commit_all({&f->st.gz, &f->st.gzi});
    } else {
        rc = f->plain.commit();
    }
    if (rc) { f->abandon(); return rc; }
    f->finished = true;
    if (stats_out) {
        stats_out[0] = (int64_t)f->records; stats_out[1] = (int64_t)f->written; stats_out[2] = (int64_t)f->stream;
        stats_out[3] = f->gz ? (int64_t)f->st.file_at : (int64_t)f->stream;
        stats_out[4] = f->gz ? (int64_t)f->st.members : 0;
        for (int k = 0; k < 3; k++) stats_out[5 + k] = f->gz ? f->st.forms[k] : 0;
    }
    return 0;
}
