// native_qc.hpp -- part of mirge_native.hip (one translation unit): --read-qc (kernels_qc.hpp).  mirge_qc is the accumulator of one sample: the
// 64-bit tables of both views in device memory, alive across the pieces of a streamed sample.  mirge_reads_parse_trim_qc is mirge_reads_parse_trim
// plus qc_accumulate on the SAME ParseJob, between parse_lines and parse_pack (k_seq_class writes the sliced bounds back over dstart / dend): per
// view k_qc_read<true> alone (MIRGE_QC_FORM=read, the default), or with MIRGE_QC_FORM=pos k_qc_pos (base, qual) + k_qc_read<false> (the per-read figures).
// mirge_qc_class_profile: k_qc_class over the groups of the dictionary, behind the cascade.
#pragma once

#ifndef MIRGE_QC_DEFAULT_POS
#define MIRGE_QC_DEFAULT_POS 0  // the lane-per-read form unless MIRGE_QC_FORM says otherwise: the faster one where both were measured (profiles/read_qc.md)
#endif

struct mirge_qc {
    mirge_ctx* ctx = nullptr;
    unsigned long long* tab = nullptr;  // [2][MIRGE_QC_VIEW_WORDS]
    int32_t has_qual = 0;               // a FASTQ piece went in
    int64_t pieces = 0;
};

extern "C" void mirge_qc_destroy(mirge_qc* q) {
    if (!q) return;
    if (q->ctx && q->tab) { (void)hipStreamSynchronize(q->ctx->stream); q->ctx->release(q->tab); }
    delete q;
}

extern "C" int mirge_qc_create(mirge_ctx* c, mirge_qc** out) {
    if (!c || !out) return fail(-1, "mirge_qc_create: bad argument");
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    auto q = std::make_unique<mirge_qc>();
    q->ctx = c;
    int rc = dalloc(c, &q->tab, (size_t)2 * MIRGE_QC_VIEW_WORDS);
    if (rc) return rc;
    hipError_t e = hipMemsetAsync(q->tab, 0, (size_t)2 * MIRGE_QC_VIEW_WORDS * 8, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { mirge_qc_destroy(q.release()); return fail(-2, std::string("mirge_qc_create: ") + hipGetErrorString(e)); }
    *out = q.release();
    return 0;
}

extern "C" int mirge_qc_fetch(mirge_ctx* c, const mirge_qc* q, int64_t* tables, int32_t* has_qual) {
    if (!c || !q || q->ctx != c || !tables) return fail(-1, "mirge_qc_fetch: bad argument");
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    HIPOK(hipMemcpyAsync(tables, q->tab, (size_t)2 * MIRGE_QC_VIEW_WORDS * 8, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    if (has_qual) *has_qual = q->has_qual;
    return 0;
}

// -> 1 the lane-per-position form, 0 the lane-per-read form, < 0 an error (MIRGE_QC_FORM=pos | read, read per call: A/B and tests)
static int qc_form_pos() {
    const char* const form = std::getenv("MIRGE_QC_FORM");
    if (!form || !*form) return MIRGE_QC_DEFAULT_POS;
    if (!std::strcmp(form, "pos")) return 1;
    if (!std::strcmp(form, "read")) return 0;
    return fail(-1, "mirge_reads_parse_trim_qc: MIRGE_QC_FORM is pos or read");
}

// J after parse_lines: its text, lines and trimmed bounds -> the tables of q (both views)
static int qc_accumulate(ParseJob& J, const TrimOpts* topt, int32_t min_len, mirge_qc* q) {
    mirge_ctx* c = J.c;
    if (!J.n_raw) return 0;
    const int pos = qc_form_pos();
    if (pos < 0) return pos;
    const bool trimming = topt && topt->n_mods > 0;
    const bool fastq = J.format == 1 && J.qstart && J.qend;
    static std::once_flag lds_once;
    static hipError_t lds_err = hipSuccess;
    std::call_once(lds_once, [] {
        lds_err = hipFuncSetAttribute(reinterpret_cast<const void*>(k_qc_pos), hipFuncAttributeMaxDynamicSharedMemorySize, MIRGE_QC_POS_LDS_WORDS * 4);
        if (lds_err == hipSuccess)
            lds_err = hipFuncSetAttribute(reinterpret_cast<const void*>(k_qc_read<true>), hipFuncAttributeMaxDynamicSharedMemorySize, MIRGE_QC_POS_LDS_WORDS * 4);
    });
    HIPOK(lds_err);
    QcJob j;
    std::memset(&j, 0, sizeof(j));
    j.text = J.dtext;
    j.lstart = trimming ? J.lstart : J.dstart; j.lend = trimming ? J.lend : J.dend;
    j.qstart = fastq ? J.qstart : nullptr; j.qend = fastq ? J.qend : nullptr;
    j.n = J.n_raw;
    j.min_len = min_len > 0 ? min_len : 0;
    j.base = topt && topt->base ? topt->base : 33;
    if (fastq) q->has_qual = 1;
    q->pieces++;
    const unsigned lds = (unsigned)((fastq ? MIRGE_QC_POS_LDS_WORDS : MIRGE_QC_P * MIRGE_QC_NL) * 4);
    const unsigned per_block = MIRGE_QC_POS_THREADS / 64 * MIRGE_QC_POS_BATCH;  // records a workgroup of k_qc_pos takes per step
    const unsigned pos_grid = (unsigned)std::max<size_t>(1, std::min<size_t>((size_t)c->n_cu, ((size_t)J.n_raw + per_block - 1) / per_block));
    const unsigned read_grid = (unsigned)std::max<size_t>(1, std::min<size_t>((size_t)c->n_cu, ((size_t)J.n_raw + MIRGE_BLOCK - 1) / MIRGE_BLOCK));
    for (int view = 0; view < 2; view++) {
        j.view = view;
        if (view == 1 && trimming) {  // the read after the LAST modifier
            j.vstart = J.dstart; j.vend = J.dend;
            j.vstride = (uint32_t)(J.n_seq / J.n_raw); j.voff = j.vstride - 1;
        }
        unsigned long long* const tab = q->tab + (size_t)view * MIRGE_QC_VIEW_WORDS;
        if (pos) {
            { LaunchScope ls(c, "k_qc_pos", (double)J.n_raw);
              hipLaunchKernelGGL(k_qc_pos, dim3(pos_grid), dim3(MIRGE_QC_POS_THREADS), lds, c->stream, j, tab); }
            LaunchScope ls(c, "k_qc_read", (double)J.n_raw);
            hipLaunchKernelGGL(k_qc_read<false>, dim3(read_grid), dim3(MIRGE_BLOCK), 0, c->stream, j, tab);
        } else {
            LaunchScope ls(c, "k_qc_read_tables", (double)J.n_raw);
            hipLaunchKernelGGL(k_qc_read<true>, dim3(read_grid), dim3(MIRGE_BLOCK), lds, c->stream, j, tab);
        }
    }
    HIPOK(hipGetLastError());
    return 0;
}

extern "C" int mirge_reads_parse_trim_qc(mirge_ctx* c, const char* text, int64_t nbytes, int32_t format, int32_t min_len, const mirge_trim* trim,
                                         mirge_qc* qc, mirge_reads** out, int64_t* n_records) {
    if (qc && qc->ctx != c) return fail(-1, "mirge_reads_parse_trim_qc: the accumulator belongs to another context");
    return reads_parse_impl(c, text, nbytes, format, min_len, trim, nullptr, out, n_records, nullptr, qc);
}

extern "C" int mirge_qc_class_profile(mirge_ctx* c, const mirge_reads* U, const mirge_result* res, int32_t n_pass, int64_t* out) {
    const std::string who = "mirge_qc_class_profile";
    if (!c || !U || !res || !out || U->ctx != c || n_pass < 0 || n_pass > MIRGE_MAX_PASSES) return fail(-1, who + ": bad argument");
    if (U->n_samples < 1) return fail(-1, who + ": the read set has no count matrix (collapse it or mirge_reads_set_counts)");
    if (res->n != U->n || res->n_pass != n_pass) return fail(-1, who + ": result and read set differ in size, or n_pass is not the result's");
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    static_assert(MIRGE_QC_NGROUPS == MIRGE_NGROUPS, "read groups");
    const int32_t S = U->n_samples;
    const size_t cells = (size_t)S * (size_t)(n_pass + 1) * (MIRGE_QC_P + 1) * MIRGE_QC_NL * 2;
    QcClassGroups gs;
    std::memset(&gs, 0, sizeof(gs));
    uint64_t total = 0;
    for (int gi = 0; gi < MIRGE_NGROUPS; gi++) {
        const ReadGroup& g = U->g[gi];
        if (!g.n) continue;
        if (res->g[gi].n != g.n || !res->g[gi].pass || !g.counts) return fail(-1, who + ": the result is not this read set's");
        const int k = gs.n_groups++;
        gs.pass[k] = res->g[gi].pass; gs.seq[k] = g.seq; gs.nmask[k] = g.nmask; gs.len[k] = g.len; gs.counts[k] = g.counts;
        gs.len16[k] = is_long_group(gi) ? 1 : 0;
        gs.start[k] = (uint32_t)total;
        total += g.n;
    }
    if (total >= 0xFFFFFFF0ull) return fail(-5, who + ": more than 2^32 reads");
    gs.start[gs.n_groups] = (uint32_t)total;
    PoolScope scope(c);
    unsigned long long* d;
    CHECK(scope.get(&d, cells));
    HIPOK(hipMemsetAsync(d, 0, cells * 8, c->stream));
    if (total) {
        const size_t tile = (size_t)(n_pass + 1) * MIRGE_QC_CLASS_TILE * MIRGE_QC_NL * 2 * 8;
        const int use_lds = tile <= 64 * 1024 ? 1 : 0;
        LaunchScope ls(c, "k_qc_class", (double)total * S);
        hipLaunchKernelGGL(k_qc_class, dim3((unsigned)grid_for(c, (size_t)total), (unsigned)S), dim3(MIRGE_BLOCK), use_lds ? tile : 0, c->stream, gs, S, n_pass,
                           use_lds, d);
    }
    HIPOK(hipMemcpyAsync(out, d, cells * 8, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    HIPOK(hipGetLastError());
    return 0;
}
