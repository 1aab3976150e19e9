// native_genome.hpp -- part of mirge_native.hip (one translation unit): the genome of the A-to-I report's filter on the device
// (mirge_genome_create / _create_packed / _destroy) and the two bowtie runs it replaces (mirge_genome_align_counts;
// mirge2_tRF_a2i.py:1056-1096,1297-1316).  Kernels: kernels_genome.hpp.
#pragma once

struct mirge_genome {
    int device = 0;
    uint64_t* text = nullptr;     // packed stream (bowtie's .4.ebwt order), padded
    uint64_t* s_start = nullptr;  // [n_str + 1]
    uint64_t n_bases = 0;
    uint32_t n_str = 0;
};

extern "C" void mirge_genome_destroy(mirge_genome* g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    if (g->text) (void)hipFree(g->text);
    if (g->s_start) (void)hipFree(g->s_start);
    delete g;
}

// the stream (bytes, bowtie's bit order) and its stretch starts -> a device genome; packed may hold more bytes than the bases need
static int genome_upload(mirge_ctx* c, const uint8_t* packed, uint64_t n_packed, uint64_t n_bases, const std::vector<uint64_t>& starts,
                         mirge_genome** out) {
    if (starts.size() > 0xFFFFFFFFull) return fail(-1, "mirge_genome: more than 2^32 stretches");
    if (n_packed * 4 < n_bases) return fail(-1, "mirge_genome: the packed stream is shorter than its records announce");
    HIPOK(hipSetDevice(c->device));
    std::unique_ptr<mirge_genome, void (*)(mirge_genome*)> g(new mirge_genome, mirge_genome_destroy);
    g->device = c->device;
    g->n_bases = n_bases;
    g->n_str = (uint32_t)starts.size();
    const uint64_t words = (n_bases + 31) / 32 + 4;  // the scan reads up to three words past a window's first
    HIPOK(hipMalloc(&g->text, words * 8));
    HIPOK(hipMemset(g->text, 0, words * 8));
    const uint64_t nb = std::min<uint64_t>(n_packed, (n_bases + 3) / 4);
    if (nb) HIPOK(hipMemcpy(g->text, packed, nb, hipMemcpyHostToDevice));
    std::vector<uint64_t> s(starts);
    s.push_back(n_bases);
    HIPOK(hipMalloc(&g->s_start, s.size() * 8));
    HIPOK(hipMemcpy(g->s_start, s.data(), s.size() * 8, hipMemcpyHostToDevice));
    *out = g.release();
    return 0;
}

// ASCII references (the <org>_genome.fa beside the index): every character but A/C/G/T (either case) is ambiguous, as bowtie-build
// makes it; a stretch ends at one and at every reference's end
extern "C" int mirge_genome_create(mirge_ctx* c, const char* ascii, const int64_t* offsets, int64_t n_refs, mirge_genome** out) {
    if (!c || !offsets || n_refs < 0 || !out || (offsets[n_refs] > 0 && !ascii)) return fail(-1, "mirge_genome_create: bad argument");
    static int8_t code[256];
    static std::once_flag once;
    std::call_once(once, [] {
        std::memset(code, -1, sizeof(code));
        code['A'] = code['a'] = 0; code['C'] = code['c'] = 1; code['G'] = code['g'] = 2; code['T'] = code['t'] = 3;
    });
    std::vector<uint8_t> packed((size_t)(offsets[n_refs] + 3) / 4 + 1, 0);
    std::vector<uint64_t> starts;
    uint64_t pos = 0;
    for (int64_t r = 0; r < n_refs; r++) {
        if (offsets[r + 1] < offsets[r]) return fail(-1, "mirge_genome_create: offsets decrease");
        bool open = false;
        for (int64_t i = offsets[r]; i < offsets[r + 1]; i++) {
            const int8_t v = code[(uint8_t)ascii[i]];
            if (v < 0) { open = false; continue; }
            if (!open) { starts.push_back(pos); open = true; }
            packed[pos >> 2] |= (uint8_t)(v << (2 * (pos & 3)));
            pos++;
        }
    }
    return genome_upload(c, packed.data(), packed.size(), pos, starts, out);
}

// bowtie's own reference files: packed = .4.ebwt as it is, rec_off / rec_len / rec_first = the .3.ebwt records (off ambiguous
// characters, then a stretch of len bases; first: a new reference starts).  Positions are 64-bit (.ebwtl).
extern "C" int mirge_genome_create_packed(mirge_ctx* c, const uint8_t* packed, int64_t n_packed, const uint64_t* rec_off,
                                          const uint64_t* rec_len, const uint8_t* rec_first, int64_t n_rec, mirge_genome** out) {
    if (!c || n_packed < 0 || n_rec < 0 || !out || (n_packed > 0 && !packed) || (n_rec > 0 && (!rec_off || !rec_len || !rec_first)))
        return fail(-1, "mirge_genome_create_packed: bad argument");
    std::vector<uint64_t> starts;
    uint64_t pos = 0;
    bool open = false;  // a record with no N in front of it continues the stretch before it (same reference)
    for (int64_t r = 0; r < n_rec; r++) {
        if (rec_first[r] || rec_off[r]) open = false;
        if (!rec_len[r]) continue;
        if (!open) { starts.push_back(pos); open = true; }
        pos += rec_len[r];
    }
    return genome_upload(c, packed, (uint64_t)n_packed, pos, starts, out);
}

extern "C" int mirge_genome_align_counts(mirge_ctx* c, const mirge_genome* g, const char* queries, const int64_t* offsets, int64_t n,
                                         int32_t n_mm, int32_t seedlen, int32_t maxtotal, int32_t trim5, int32_t trim3, uint32_t* out) {
    if (!c || !g || !offsets || n < 0 || (n > 0 && !out) || n_mm < 0 || n_mm > 2 || seedlen < 1 || maxtotal < 0 || maxtotal > 2 ||
        trim5 < 0 || trim3 < 0)
        return fail(-1, "mirge_genome_align_counts: bad argument (0 <= n_mm <= 2, 0 <= maxtotal <= 2, seedlen >= 1)");
    if (n > (int64_t)(0xFFFFFFFFu / 6)) return fail(-1, "mirge_genome_align_counts: too many queries for one call");
    if (n == 0) return 0;
    if (offsets[n] > 0 && !queries) return fail(-1, "mirge_genome_align_counts: no query text");
    for (int64_t i = 0; i < n; i++) {
        if (offsets[i + 1] < offsets[i]) return fail(-1, "mirge_genome_align_counts: offsets decrease");
        if (offsets[i + 1] - offsets[i] - trim5 - trim3 > MIRGE_GENOME_MAXLEN)
            return fail(-1, "mirge_genome_align_counts: a query is longer than " + std::to_string(MIRGE_GENOME_MAXLEN) + " nt after trimming");
    }
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    const int P = n_mm + 1;
    const uint32_t nqs = (uint32_t)(2 * n), nk = nqs * (uint32_t)P;
    // Key length.  A genome position probes every table, and a random k-mer is one of the n_keys keys of the longest table with
    // probability n_keys / 4^k: k is the least with 4^k >= 32 n_keys (about 0.03 candidate verifications per position and table
    // for pieces at least k long), at least 8, at most 13.  Its bitmap is 4^k bits: 2 MiB at k = 12 (10^5 queries, -n 1) sits in
    // every XCD's 4 MiB L2, 8 MiB at 13 in the Infinity Cache.  Shorter pieces (-n 1 halves of short reads) take tables of their
    // own length, where the rate is their count over 4^length: the candidates there are the alignments such a short piece has.
    int kmax = 8;
    while (kmax < MIRGE_GENOME_MAXK && (1ull << (2 * kmax)) < 32ull * nk) kmax++;
    uint64_t bm_off[MIRGE_GENOME_MAXK + 1] = {0};
    uint64_t bm_words = 0;
    for (int k = 1; k <= kmax; k++) { bm_off[k] = bm_words; bm_words += std::max<uint64_t>(1, (1ull << (2 * k)) / 32); }
    char* d_ascii = nullptr; int64_t* d_off = nullptr; GenomeQS* d_qs = nullptr;
    uint64_t *d_keys = nullptr, *d_skeys = nullptr, *d_bmoff = nullptr; uint32_t *d_vals = nullptr, *d_svals = nullptr, *d_bitmap = nullptr, *d_tab = nullptr;
    unsigned long long* d_counts = nullptr; void* d_tmp = nullptr;
    size_t tmp_bytes = 0;
    HIPOK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr,
                                              (uint32_t*)nullptr, (int)nk, 0, 64, c->stream));
    int rc = 0;
    auto run = [&]() -> int {
        CHECK(dalloc(c, &d_ascii, (size_t)std::max<int64_t>(offsets[n], 1)));
        CHECK(dalloc(c, &d_off, (size_t)n + 1));
        CHECK(dalloc(c, &d_qs, nqs));
        CHECK(dalloc(c, &d_keys, nk)); CHECK(dalloc(c, &d_skeys, nk));
        CHECK(dalloc(c, &d_vals, nk)); CHECK(dalloc(c, &d_svals, nk));
        CHECK(dalloc(c, &d_bmoff, MIRGE_GENOME_MAXK + 1));
        CHECK(dalloc(c, &d_bitmap, bm_words));
        CHECK(dalloc(c, &d_tab, 2 * (MIRGE_GENOME_MAXK + 1)));
        CHECK(dalloc(c, &d_counts, (size_t)n * 3));
        CHECK(c->alloc(&d_tmp, tmp_bytes));
        if (offsets[n]) HIPOK(hipMemcpyAsync(d_ascii, queries, (size_t)offsets[n], hipMemcpyHostToDevice, c->stream));
        HIPOK(hipMemcpyAsync(d_off, offsets, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));
        HIPOK(hipMemcpyAsync(d_bmoff, bm_off, sizeof(bm_off), hipMemcpyHostToDevice, c->stream));
        HIPOK(hipMemsetAsync(d_bitmap, 0, bm_words * 4, c->stream));
        HIPOK(hipMemsetAsync(d_tab, 0, 2 * (MIRGE_GENOME_MAXK + 1) * 4, c->stream));
        HIPOK(hipMemsetAsync(d_counts, 0, (size_t)n * 3 * 8, c->stream));
        {
            LaunchScope ls(c, "k_genome_queries", (double)n);
            const GenomeQueryArgs qa{d_ascii, d_off, (uint32_t)n, n_mm, seedlen, trim5, trim3, kmax};
            hipLaunchKernelGGL(k_genome_queries, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, qa, d_qs, d_keys, d_vals);
        }
        HIPOK(hipcub::DeviceRadixSort::SortPairs(d_tmp, tmp_bytes, d_keys, d_skeys, d_vals, d_svals, (int)nk, 0, 64, c->stream));
        {
            LaunchScope ls(c, "k_genome_index", (double)nk);
            hipLaunchKernelGGL(k_genome_index, dim3((nk + 255) / 256), dim3(256), 0, c->stream, d_skeys, nk, d_bmoff, d_bitmap, d_tab,
                               d_tab + MIRGE_GENOME_MAXK + 1);
        }
        uint32_t tab[2 * (MIRGE_GENOME_MAXK + 1)];
        HIPOK(hipMemcpyAsync(tab, d_tab, sizeof(tab), hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipStreamSynchronize(c->stream));
        GenomeScanArgs sa{};
        sa.text = g->text; sa.n_bases = g->n_bases; sa.s_start = g->s_start; sa.n_str = g->n_str;
        sa.bitmap = d_bitmap; sa.skeys = d_skeys; sa.svals = d_svals; sa.qs = d_qs; sa.counts = d_counts;
        sa.n_mm = n_mm; sa.maxtotal = maxtotal; sa.ntab = 0;
        for (int k = 1; k <= kmax; k++) {
            const uint32_t b = tab[k], e = tab[MIRGE_GENOME_MAXK + 1 + k];
            if (e <= b) continue;
            sa.tab_k[sa.ntab] = k; sa.tab_bm[sa.ntab] = bm_off[k]; sa.tab_b[sa.ntab] = b; sa.tab_e[sa.ntab] = e;
            sa.ntab++;
        }
        if (sa.ntab && g->n_bases) {
            const uint64_t strips = (g->n_bases + MIRGE_GENOME_STRIP - 1) / MIRGE_GENOME_STRIP;
            LaunchScope ls(c, "k_genome_scan", (double)g->n_bases);
            hipLaunchKernelGGL(k_genome_scan, dim3((unsigned)grid_for(c, strips)), dim3(256), 0, c->stream, sa);
        }
        std::vector<unsigned long long> h((size_t)n * 3);
        HIPOK(hipMemcpyAsync(h.data(), d_counts, h.size() * 8, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipStreamSynchronize(c->stream));
        HIPOK(hipGetLastError());
        for (size_t i = 0; i < h.size(); i++) out[i] = h[i] > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)h[i];
        return 0;
    };
    rc = run();
    if (rc) (void)hipStreamSynchronize(c->stream);
    c->drain();
    for (void* p : {(void*)d_ascii, (void*)d_off, (void*)d_qs, (void*)d_keys, (void*)d_skeys, (void*)d_vals, (void*)d_svals, (void*)d_bmoff,
                    (void*)d_bitmap, (void*)d_tab, (void*)d_counts, d_tmp})
        c->release(p);
    return rc;
}
