// native_genome.hpp -- part of mirge_native.hip (one translation unit): the genome of the A-to-I report's filter on the device
// (mirge_genome_create / _create_packed / _destroy), the two bowtie runs it replaces (mirge_genome_align_counts;
// mirge2_tRF_a2i.py:1056-1096,1297-1316), the same alignments with their positions (mirge_genome_align_loci, and
// mirge_genome_align_loci_strata: the best stratum only, bowtie's --best --strata) and the clustering
// of such records (mirge_loci_cluster; novel_mir.py:81-150).  Kernels: kernels_genome.hpp.
#pragma once

struct mirge_genome {
    int device = 0;
    uint64_t* text = nullptr;     // packed stream (bowtie's .4.ebwt order), padded
    uint64_t* s_start = nullptr;  // [n_str + 1]
    uint32_t* str_ref = nullptr;  // [n_str] the reference a stretch lies in
    uint64_t* str_off = nullptr;  // [n_str] where it starts inside that reference, ambiguous characters counted
    uint64_t n_bases = 0;
    uint32_t n_str = 0;
    uint32_t n_refs = 0;
};

extern "C" void mirge_genome_destroy(mirge_genome* g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    if (g->text) (void)hipFree(g->text);
    if (g->s_start) (void)hipFree(g->s_start);
    if (g->str_ref) (void)hipFree(g->str_ref);
    if (g->str_off) (void)hipFree(g->str_off);
    delete g;
}

// the stream (bytes, bowtie's bit order) and its stretch starts -> a device genome; packed may hold more bytes than the bases need
static int genome_upload(mirge_ctx* c, const uint8_t* packed, uint64_t n_packed, uint64_t n_bases, const std::vector<uint64_t>& starts,
                         const std::vector<uint32_t>& sref, const std::vector<uint64_t>& soff, uint32_t n_refs, mirge_genome** out) {
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
    g->n_refs = n_refs;
    HIPOK(hipMalloc(&g->str_ref, std::max<size_t>(1, sref.size()) * 4));
    HIPOK(hipMalloc(&g->str_off, std::max<size_t>(1, soff.size()) * 8));
    if (!sref.empty()) {
        HIPOK(hipMemcpy(g->str_ref, sref.data(), sref.size() * 4, hipMemcpyHostToDevice));
        HIPOK(hipMemcpy(g->str_off, soff.data(), soff.size() * 8, hipMemcpyHostToDevice));
    }
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
    std::vector<uint64_t> starts, soff;
    std::vector<uint32_t> sref;
    uint64_t pos = 0;
    for (int64_t r = 0; r < n_refs; r++) {
        if (offsets[r + 1] < offsets[r]) return fail(-1, "mirge_genome_create: offsets decrease");
        bool open = false;
        for (int64_t i = offsets[r]; i < offsets[r + 1]; i++) {
            const int8_t v = code[(uint8_t)ascii[i]];
            if (v < 0) { open = false; continue; }
            if (!open) { starts.push_back(pos); sref.push_back((uint32_t)r); soff.push_back((uint64_t)(i - offsets[r])); open = true; }
            packed[pos >> 2] |= (uint8_t)(v << (2 * (pos & 3)));
            pos++;
        }
    }
    return genome_upload(c, packed.data(), packed.size(), pos, starts, sref, soff, (uint32_t)n_refs, out);
}

// bowtie's own reference files: packed = .4.ebwt as it is, rec_off / rec_len / rec_first = the .3.ebwt records (off ambiguous
// characters, then a stretch of len bases; first: a new reference starts).  Positions are 64-bit (.ebwtl).
extern "C" int mirge_genome_create_packed(mirge_ctx* c, const uint8_t* packed, int64_t n_packed, const uint64_t* rec_off,
                                          const uint64_t* rec_len, const uint8_t* rec_first, int64_t n_rec, mirge_genome** out) {
    if (!c || n_packed < 0 || n_rec < 0 || !out || (n_packed > 0 && !packed) || (n_rec > 0 && (!rec_off || !rec_len || !rec_first)))
        return fail(-1, "mirge_genome_create_packed: bad argument");
    std::vector<uint64_t> starts, soff;
    std::vector<uint32_t> sref;
    uint64_t pos = 0, inref = 0;  // inref: where the next record starts inside its reference
    int64_t ref = -1;             // references are numbered by their `first` records, as bowtie numbers them
    bool open = false;  // a record with no N in front of it continues the stretch before it (same reference)
    for (int64_t r = 0; r < n_rec; r++) {
        if (rec_first[r]) { ref++; inref = 0; }
        if (rec_first[r] || rec_off[r]) open = false;
        inref += rec_off[r];
        if (!rec_len[r]) continue;
        if (ref < 0) return fail(-1, "mirge_genome_create_packed: the first record does not start a reference");
        if (!open) { starts.push_back(pos); sref.push_back((uint32_t)ref); soff.push_back(inref); open = true; }
        pos += rec_len[r];
        inref += rec_len[r];
    }
    return genome_upload(c, packed, (uint64_t)n_packed, pos, starts, sref, soff, (uint32_t)(ref + 1), out);
}

// ---- the query tables of one scan (both exports below): queries on the device, their pieces sorted into the key tables, the
// presence bitmaps, the scan's arguments.  genome_tables_build fills it from a PoolScope: the call's, or one batch's.
struct GenomeTables {
    char* d_ascii = nullptr; int64_t* d_off = nullptr; GenomeQS* d_qs = nullptr;
    uint64_t *d_keys = nullptr, *d_skeys = nullptr, *d_bmoff = nullptr;
    uint32_t *d_vals = nullptr, *d_svals = nullptr, *d_bitmap = nullptr, *d_tab = nullptr;
    unsigned long long* d_counts = nullptr; void* d_tmp = nullptr;
    GenomeScanArgs sa{};
    int64_t n = 0;
    // what genome_tables_build's copies read and fill: a GenomeTables stands in front of the scope its blocks come from
    std::vector<int64_t> off;
    uint64_t bm_off[MIRGE_GENOME_MAXK + 1] = {0};
    uint32_t tab[2 * (MIRGE_GENOME_MAXK + 1)] = {0};
};

static int genome_check_args(const char* who, mirge_ctx* c, const mirge_genome* g, const char* queries, const int64_t* offsets, int64_t n,
                             int32_t n_mm, int32_t seedlen, int32_t maxtotal, int32_t trim5, int32_t trim3) {
    const std::string w(who);
    if (!c || !g || !offsets || n < 0 || n_mm < 0 || n_mm > 2 || maxtotal < 0 || maxtotal > 2 || trim5 < 0 || trim3 < 0)
        return fail(-1, w + ": bad argument (0 <= n_mm <= 2, 0 <= maxtotal <= 2)");
    // bowtie's own floor for -l.  Below n_mm + 1 a piece of the seed would be empty -- exact in every window, so that it would own
    // every alignment and, having no table, report none
    if (seedlen < MIRGE_GENOME_MINSEED)
        return fail(-1, w + ": seedlen " + std::to_string(seedlen) + " is below the floor of " + std::to_string(MIRGE_GENOME_MINSEED) +
                            " (bowtie -l)");
    if (n > (int64_t)(0xFFFFFFFFu / 8)) return fail(-1, w + ": too many queries for one call");
    if (n == 0) return 0;
    if (offsets[n] > 0 && !queries) return fail(-1, w + ": no query text");
    for (int64_t i = 0; i < n; i++) {
        if (offsets[i + 1] < offsets[i]) return fail(-1, w + ": offsets decrease");
        if (offsets[i + 1] - offsets[i] - trim5 - trim3 > MIRGE_GENOME_MAXLEN)
            return fail(-1, w + ": a query is longer than " + std::to_string(MIRGE_GENOME_MAXLEN) + " nt after trimming");
    }
    return 0;
}

// queries [q0, q0 + n) of the caller's arrays -> tables and scan arguments; counts zeroed.  The stream is synchronised on return.
static int genome_tables_build(PoolScope& scope, const mirge_genome* g, const char* queries, const int64_t* offsets, int64_t q0, int64_t n,
                               int32_t n_mm, int32_t seedlen, int32_t maxtotal, int32_t trim5, int32_t trim3, int32_t norc, GenomeTables& t) {
    mirge_ctx* const c = scope.c;
    const int P = n_mm + 1;
    const uint32_t nqs = (uint32_t)(2 * n), nk = nqs * (uint32_t)P;
    // Key length.  A genome position probes every table, and a random k-mer is one of the n_keys keys of the longest table with
    // probability n_keys / 4^k: k is the least with 4^k >= 32 n_keys (about 0.03 candidate verifications per position and table
    // for pieces at least k long), at least 8, at most 13.  Its bitmap is 4^k bits: 2 MiB at k = 12 (10^5 queries, -n 1) sits in
    // every XCD's 4 MiB L2, 8 MiB at 13 in the Infinity Cache.  Shorter pieces (-n 1 halves of short reads) take tables of their
    // own length, where the rate is their count over 4^length: the candidates there are the alignments such a short piece has.
    int kmax = 8;
    while (kmax < MIRGE_GENOME_MAXK && (1ull << (2 * kmax)) < 32ull * nk) kmax++;
    uint64_t* const bm_off = t.bm_off;
    std::vector<int64_t>& off = t.off;
    uint32_t* const tab = t.tab;
    uint64_t bm_words = 0;
    bm_off[0] = 0;
    for (int k = 1; k <= kmax; k++) { bm_off[k] = bm_words; bm_words += std::max<uint64_t>(1, (1ull << (2 * k)) / 32); }
    size_t tmp_bytes = 0;
    HIPOK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr,
                                              (uint32_t*)nullptr, (int)nk, 0, 64, c->stream));
    t.n = n;
    const int64_t b0 = offsets[q0], nb = offsets[q0 + n] - b0;
    off.resize((size_t)n + 1);
    for (int64_t i = 0; i <= n; i++) off[(size_t)i] = offsets[q0 + i] - b0;
    CHECK(scope.get(&t.d_ascii, (size_t)std::max<int64_t>(nb, 1)));
    CHECK(scope.get(&t.d_off, (size_t)n + 1));
    CHECK(scope.get(&t.d_qs, nqs));
    CHECK(scope.get(&t.d_keys, nk)); CHECK(scope.get(&t.d_skeys, nk));
    CHECK(scope.get(&t.d_vals, nk)); CHECK(scope.get(&t.d_svals, nk));
    CHECK(scope.get(&t.d_bmoff, MIRGE_GENOME_MAXK + 1));
    CHECK(scope.get(&t.d_bitmap, bm_words));
    CHECK(scope.get(&t.d_tab, 2 * (MIRGE_GENOME_MAXK + 1)));
    CHECK(scope.get(&t.d_counts, (size_t)n * 3));
    CHECK(scope.get((uint8_t**)&t.d_tmp, tmp_bytes));
    if (nb) HIPOK(hipMemcpyAsync(t.d_ascii, queries + b0, (size_t)nb, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(t.d_off, off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(t.d_bmoff, bm_off, sizeof(t.bm_off), hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemsetAsync(t.d_bitmap, 0, bm_words * 4, c->stream));
    HIPOK(hipMemsetAsync(t.d_tab, 0, 2 * (MIRGE_GENOME_MAXK + 1) * 4, c->stream));
    HIPOK(hipMemsetAsync(t.d_counts, 0, (size_t)n * 3 * 8, c->stream));
    {
        LaunchScope ls(c, "k_genome_queries", (double)n);
        const GenomeQueryArgs qa{t.d_ascii, t.d_off, (uint32_t)n, n_mm, seedlen, trim5, trim3, kmax, norc};
        hipLaunchKernelGGL(k_genome_queries, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, qa, t.d_qs, t.d_keys, t.d_vals);
    }
    HIPOK(hipcub::DeviceRadixSort::SortPairs(t.d_tmp, tmp_bytes, t.d_keys, t.d_skeys, t.d_vals, t.d_svals, (int)nk, 0, 64, c->stream));
    {
        LaunchScope ls(c, "k_genome_index", (double)nk);
        hipLaunchKernelGGL(k_genome_index, dim3((nk + 255) / 256), dim3(256), 0, c->stream, t.d_skeys, nk, t.d_bmoff, t.d_bitmap, t.d_tab,
                           t.d_tab + MIRGE_GENOME_MAXK + 1);
    }
    HIPOK(hipMemcpyAsync(tab, t.d_tab, sizeof(t.tab), hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    GenomeScanArgs& sa = t.sa;
    sa = GenomeScanArgs{};
    sa.text = g->text; sa.n_bases = g->n_bases; sa.s_start = g->s_start; sa.n_str = g->n_str;
    sa.bitmap = t.d_bitmap; sa.skeys = t.d_skeys; sa.svals = t.d_svals; sa.qs = t.d_qs; sa.counts = t.d_counts;
    sa.n_mm = n_mm; sa.maxtotal = maxtotal; sa.ntab = 0;
    for (int k = 1; k <= kmax; k++) {
        const uint32_t b = tab[k], e = tab[MIRGE_GENOME_MAXK + 1 + k];
        if (e <= b) continue;
        sa.tab_k[sa.ntab] = k; sa.tab_bm[sa.ntab] = bm_off[k]; sa.tab_b[sa.ntab] = b; sa.tab_e[sa.ntab] = e;
        sa.ntab++;
    }
    return 0;
}

// the count pass over the genome and its [n][3] result on the host (stream synchronised)
static int genome_count_pass(mirge_ctx* c, const mirge_genome* g, GenomeTables& t, std::vector<unsigned long long>& h) {
    if (t.sa.ntab && g->n_bases) {
        const uint64_t strips = (g->n_bases + MIRGE_GENOME_STRIP - 1) / MIRGE_GENOME_STRIP;
        LaunchScope ls(c, "k_genome_scan", (double)g->n_bases);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_genome_scan<false>), dim3((unsigned)grid_for(c, strips)), dim3(256), 0, c->stream, t.sa);
    }
    h.resize((size_t)t.n * 3);
    HIPOK(hipMemcpyAsync(h.data(), t.d_counts, h.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    HIPOK(hipGetLastError());
    return 0;
}

extern "C" int mirge_genome_align_counts(mirge_ctx* c, const mirge_genome* g, const char* queries, const int64_t* offsets, int64_t n,
                                         int32_t n_mm, int32_t seedlen, int32_t maxtotal, int32_t trim5, int32_t trim3, uint32_t* out) {
    if (n > 0 && !out) return fail(-1, "mirge_genome_align_counts: bad argument (no output)");
    CHECK(genome_check_args("mirge_genome_align_counts", c, g, queries, offsets, n, n_mm, seedlen, maxtotal, trim5, trim3));
    if (n == 0) return 0;
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    GenomeTables t;
    std::vector<unsigned long long> h;
    PoolScope scope(c);
    CHECK(genome_tables_build(scope, g, queries, offsets, 0, n, n_mm, seedlen, maxtotal, trim5, trim3, 0, t));
    CHECK(genome_count_pass(c, g, t, h));
    for (size_t i = 0; i < h.size(); i++) out[i] = h[i] > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)h[i];
    return 0;
}

// ---- alignments with positions (mirge_genome_align_loci[_strata]): the count pass, then the same scan as a fill pass, then two
// stable sorts.  strata: the count pass counts by SEED mismatches; a query's best stratum is the first of its three counts that is
// not zero, and only that stratum is sized, capped by max_loci and filled
struct mirge_loci {  // on the host: the records in (reference, offset, query, strand) order
    std::vector<uint32_t> query, ref;
    std::vector<uint64_t> off;
    std::vector<uint8_t> strand, mm;
};

#define MIRGE_LOCI_BATCH (1 << 20)        // queries per scan: 2^21 keys under -n 0 keep the k = 13 table at the 1/32 fill it was sized for
#define MIRGE_LOCI_MAX_RECORDS 0x7FFFFFFFll  // hipCUB sorts take an int count

extern "C" void mirge_loci_destroy(mirge_loci* l) { delete l; }
extern "C" int64_t mirge_loci_count(const mirge_loci* l) { return l ? (int64_t)l->query.size() : 0; }

extern "C" int mirge_loci_fetch(const mirge_loci* l, uint32_t* query, uint32_t* ref, uint64_t* off, uint8_t* strand, uint8_t* mm) {
    if (!l) return fail(-1, "mirge_loci_fetch: bad argument");
    const size_t n = l->query.size();
    if (n && (!query || !ref || !off || !strand || !mm)) return fail(-1, "mirge_loci_fetch: bad argument");
    if (n) {
        std::memcpy(query, l->query.data(), n * 4); std::memcpy(ref, l->ref.data(), n * 4); std::memcpy(off, l->off.data(), n * 8);
        std::memcpy(strand, l->strand.data(), n); std::memcpy(mm, l->mm.data(), n);
    }
    return 0;
}

extern "C" int mirge_genome_align_loci_strata(mirge_ctx* c, const mirge_genome* g, const char* queries, const int64_t* offsets, int64_t n,
                                              int32_t n_mm, int32_t seedlen, int32_t maxtotal, int32_t trim5, int32_t trim3,
                                              int64_t max_loci, int32_t norc, int32_t strata, uint64_t* totals, mirge_loci** out) {
    if (!out || max_loci < 0 || (n > 0 && !totals)) return fail(-1, "mirge_genome_align_loci: bad argument");
    CHECK(genome_check_args("mirge_genome_align_loci", c, g, queries, offsets, n, n_mm, seedlen, maxtotal, trim5, trim3));
    if (n > (int64_t)(0xFFFFFFFFu >> 3)) return fail(-1, "mirge_genome_align_loci: too many queries for one call");
    std::unique_ptr<mirge_loci> res(new mirge_loci);
    if (n == 0) { *out = res.release(); return 0; }
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    int64_t batch = MIRGE_LOCI_BATCH;
    if (const char* e = std::getenv("MIRGE_LOCI_BATCH")) { const long long v = std::atoll(e); if (v > 0 && v < batch) batch = v; }
    const int64_t n_batches = (n + batch - 1) / batch;
    GenomeTables t;
    uint64_t *d_range, *d_pos, *d_pos2, *d_roff;
    uint32_t *d_cursor, *d_meta, *d_meta2, *d_flag, *d_rq, *d_rref;
    uint8_t *d_rs, *d_rmm, *d_best = nullptr; void* d_tmp;
    std::vector<uint64_t> range((size_t)n + 1, 0);
    std::vector<unsigned long long> h;
    std::vector<uint8_t> best(strata ? (size_t)n : 0, 0);
    std::vector<uint32_t> cur;
    uint32_t flag = 0;
    PoolScope scope(c);
    // ---- pass 1: every query's total; what it reports (all of them, or none when -m caps it) -> its range of the records
    for (int64_t b = 0; b < n_batches; b++) {
        const int64_t q0 = b * batch, nq = std::min(batch, n - q0);
        std::optional<PoolScope> one;  // of several batches, each has its tables to itself; one batch's serve the fill pass as they are
        if (n_batches > 1) one.emplace(c);
        CHECK(genome_tables_build(one ? *one : scope, g, queries, offsets, q0, nq, n_mm, seedlen, maxtotal, trim5, trim3, norc ? 1 : 0, t));
        t.sa.strata = strata ? 1 : 0;
        CHECK(genome_count_pass(c, g, t, h));
        for (int64_t i = 0; i < nq; i++) {
            const unsigned long long* hc = &h[(size_t)i * 3];
            const uint64_t tot = hc[0] + hc[1] + hc[2];
            totals[q0 + i] = tot;
            uint64_t rep = tot;  // what the query reports: everything, or its best stratum
            if (strata) {
                const int b = hc[0] ? 0 : (hc[1] ? 1 : 2);
                best[(size_t)(q0 + i)] = (uint8_t)b;
                rep = hc[b];
            }
            range[(size_t)(q0 + i) + 1] = (max_loci && rep > (uint64_t)max_loci) ? 0 : rep;
        }
    }
    for (int64_t i = 0; i < n; i++) range[(size_t)i + 1] += range[(size_t)i];
    const uint64_t n_rec = range[(size_t)n];
    if (n_rec > (uint64_t)MIRGE_LOCI_MAX_RECORDS)
        return fail(-1, "mirge_genome_align_loci: " + std::to_string(n_rec) + " alignments to report; cap repeats with max_loci");
    if (n_rec == 0) { *out = res.release(); return 0; }
    CHECK(scope.get(&d_range, (size_t)n + 1)); CHECK(scope.get(&d_cursor, (size_t)n)); CHECK(scope.get(&d_flag, 1));
    CHECK(scope.get(&d_pos, n_rec)); CHECK(scope.get(&d_pos2, n_rec)); CHECK(scope.get(&d_meta, n_rec)); CHECK(scope.get(&d_meta2, n_rec));
    HIPOK(hipMemcpyAsync(d_range, range.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemsetAsync(d_cursor, 0, (size_t)n * 4, c->stream));
    HIPOK(hipMemsetAsync(d_flag, 0, 4, c->stream));
    if (strata) {
        CHECK(scope.get(&d_best, (size_t)n));
        HIPOK(hipMemcpyAsync(d_best, best.data(), (size_t)n, hipMemcpyHostToDevice, c->stream));
    }
    // ---- pass 2: the same scan writes the records
    for (int64_t b = 0; b < n_batches; b++) {
        const int64_t q0 = b * batch, nq = std::min(batch, n - q0);
        if (range[(size_t)(q0 + nq)] == range[(size_t)q0]) continue;  // nothing to report from this batch
        std::optional<PoolScope> one;  // (several batches: this one's tables, built again)
        if (n_batches > 1) {
            one.emplace(c);
            CHECK(genome_tables_build(*one, g, queries, offsets, q0, nq, n_mm, seedlen, maxtotal, trim5, trim3, norc ? 1 : 0, t));
        }
        t.sa.range = d_range + q0; t.sa.cursor = d_cursor + q0; t.sa.rec_pos = d_pos; t.sa.rec_meta = d_meta; t.sa.overflow = d_flag;
        t.sa.query_base = (uint32_t)q0;
        t.sa.strata = strata ? 1 : 0; t.sa.best = strata ? d_best + q0 : nullptr;
        if (t.sa.ntab && g->n_bases) {
            const uint64_t strips = (g->n_bases + MIRGE_GENOME_STRIP - 1) / MIRGE_GENOME_STRIP;
            LaunchScope ls(c, "k_genome_scan_fill", (double)g->n_bases);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_genome_scan<true>), dim3((unsigned)grid_for(c, strips)), dim3(256), 0, c->stream, t.sa);
        }
        HIPOK(hipStreamSynchronize(c->stream));
    }
    cur.resize((size_t)n);
    HIPOK(hipMemcpyAsync(cur.data(), d_cursor, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    HIPOK(hipGetLastError());
    for (int64_t i = 0; i < n && !flag; i++) flag = cur[(size_t)i] != range[(size_t)i + 1] - range[(size_t)i];
    if (flag) return fail(-1, "mirge_genome_align_loci: the fill pass and the count pass disagree");
    // ---- order: stable by (query, strand), then stable by stream position, which rises with (reference, offset)
    int qbits = 1, pbits = 1;
    while (qbits < 29 && (1ll << qbits) < n) qbits++;
    while (pbits < 64 && (1ull << pbits) <= g->n_bases) pbits++;
    size_t tb1 = 0, tb2 = 0;
    HIPOK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb1, d_meta, d_meta2, d_pos, d_pos2, (int)n_rec, 2, 3 + qbits, c->stream));
    HIPOK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb2, d_pos2, d_pos, d_meta2, d_meta, (int)n_rec, 0, pbits, c->stream));
    CHECK(scope.get((uint8_t**)&d_tmp, std::max(tb1, tb2)));
    HIPOK(hipcub::DeviceRadixSort::SortPairs(d_tmp, tb1, d_meta, d_meta2, d_pos, d_pos2, (int)n_rec, 2, 3 + qbits, c->stream));
    HIPOK(hipcub::DeviceRadixSort::SortPairs(d_tmp, tb2, d_pos2, d_pos, d_meta2, d_meta, (int)n_rec, 0, pbits, c->stream));
    CHECK(scope.get(&d_rq, n_rec)); CHECK(scope.get(&d_rref, n_rec)); CHECK(scope.get(&d_roff, n_rec));
    CHECK(scope.get(&d_rs, n_rec)); CHECK(scope.get(&d_rmm, n_rec));
    {
        LaunchScope ls(c, "k_genome_loci_finish", (double)n_rec);
        hipLaunchKernelGGL(k_genome_loci_finish, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, c->stream, (uint32_t)n_rec, d_pos,
                           d_meta, g->s_start, g->n_str, g->str_ref, g->str_off, d_rq, d_rref, d_roff, d_rs, d_rmm);
    }
    res->query.resize(n_rec); res->ref.resize(n_rec); res->off.resize(n_rec); res->strand.resize(n_rec); res->mm.resize(n_rec);
    HIPOK(hipMemcpyAsync(res->query.data(), d_rq, n_rec * 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(res->ref.data(), d_rref, n_rec * 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(res->off.data(), d_roff, n_rec * 8, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(res->strand.data(), d_rs, n_rec, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(res->mm.data(), d_rmm, n_rec, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    HIPOK(hipGetLastError());
    *out = res.release();
    return 0;
}

extern "C" int mirge_genome_align_loci(mirge_ctx* c, const mirge_genome* g, const char* queries, const int64_t* offsets, int64_t n,
                                       int32_t n_mm, int32_t seedlen, int32_t maxtotal, int32_t trim5, int32_t trim3, int64_t max_loci,
                                       int32_t norc, uint64_t* totals, mirge_loci** out) {
    return mirge_genome_align_loci_strata(c, g, queries, offsets, n, n_mm, seedlen, maxtotal, trim5, trim3, max_loci, norc, 0, totals, out);
}

// ---- clusters of coordinate-sorted records (mirge_loci_cluster)
extern "C" int mirge_loci_cluster(mirge_ctx* c, int64_t n, const uint32_t* ref, const uint64_t* off, const uint8_t* strand,
                                  const uint32_t* query, int64_t n_queries, const int32_t* qlen, const int64_t* qcount, int64_t n_refs,
                                  const uint8_t* ref_skip, int32_t threshold, int32_t minus_first_only, int32_t* cluster,
                                  int64_t* n_clusters, uint32_t* c_ref, uint8_t* c_strand, uint64_t* c_start, uint64_t* c_end,
                                  int64_t* c_reads, uint32_t* c_members) {
    if (!c || n < 0 || n > MIRGE_LOCI_MAX_RECORDS || !n_clusters || n_queries < 0 || n_refs < 0)
        return fail(-1, "mirge_loci_cluster: bad argument");
    *n_clusters = 0;
    if (n == 0) return 0;
    if (!ref || !off || !strand || !query || !qlen || !qcount || !ref_skip || !cluster || !c_ref || !c_strand || !c_start || !c_end ||
        !c_reads || !c_members)
        return fail(-1, "mirge_loci_cluster: bad argument");
    for (int64_t i = 0; i < n; i++) {
        if (ref[i] >= (uint64_t)n_refs || query[i] >= (uint64_t)n_queries || strand[i] > 1)
            return fail(-1, "mirge_loci_cluster: a record names a reference, query or strand that does not exist");
        if (i && (ref[i] < ref[i - 1] || (ref[i] == ref[i - 1] && off[i] < off[i - 1])))
            return fail(-1, "mirge_loci_cluster: the records are not sorted by (reference, offset)");
    }
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    const uint32_t N = (uint32_t)n;
    uint32_t *d_ref, *d_query, *d_vals, *d_perm, *d_flag, *d_fsum, *d_kept, *d_ksum, *t_ref, *t_members, nc = 0;
    uint64_t *d_off, *d_keys, *d_skeys, *t_start;
    unsigned long long *t_end, *t_reads;
    uint8_t *d_strand, *d_skip, *d_dropped, *t_strand;
    int32_t *d_qlen, *d_cluster; int64_t* d_qcount;
    ClusterItem *d_items, *d_scanned; void* d_tmp;
    PoolScope scope(c);
    CHECK(scope.get(&d_ref, N)); CHECK(scope.get(&d_query, N)); CHECK(scope.get(&d_off, N)); CHECK(scope.get(&d_strand, N));
    CHECK(scope.get(&d_qlen, (size_t)n_queries)); CHECK(scope.get(&d_qcount, (size_t)n_queries)); CHECK(scope.get(&d_skip, (size_t)n_refs));
    CHECK(scope.get(&d_keys, N)); CHECK(scope.get(&d_skeys, N)); CHECK(scope.get(&d_vals, N)); CHECK(scope.get(&d_perm, N));
    CHECK(scope.get(&d_items, N)); CHECK(scope.get(&d_scanned, N));
    CHECK(scope.get(&d_flag, N)); CHECK(scope.get(&d_fsum, N)); CHECK(scope.get(&d_kept, N)); CHECK(scope.get(&d_ksum, N));
    CHECK(scope.get(&d_dropped, N)); CHECK(scope.get(&d_cluster, N));
    CHECK(scope.get(&t_ref, N)); CHECK(scope.get(&t_members, N)); CHECK(scope.get(&t_start, N)); CHECK(scope.get(&t_end, N));
    CHECK(scope.get(&t_reads, N)); CHECK(scope.get(&t_strand, N));
    HIPOK(hipMemcpyAsync(d_ref, ref, (size_t)N * 4, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(d_query, query, (size_t)N * 4, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(d_off, off, (size_t)N * 8, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(d_strand, strand, (size_t)N, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(d_qlen, qlen, (size_t)n_queries * 4, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(d_qcount, qcount, (size_t)n_queries * 8, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(d_skip, ref_skip, (size_t)n_refs, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemsetAsync(t_end, 0, (size_t)N * 8, c->stream));
    HIPOK(hipMemsetAsync(t_reads, 0, (size_t)N * 8, c->stream));
    HIPOK(hipMemsetAsync(t_members, 0, (size_t)N * 4, c->stream));
    size_t tb = 0, tb_sort = 0, tb_scan = 0, tb_sum = 0;
    HIPOK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb_sort, d_keys, d_skeys, d_vals, d_perm, (int)N, 0, 33, c->stream));
    HIPOK(hipcub::DeviceScan::InclusiveScan(nullptr, tb_scan, d_items, d_scanned, ClusterScanOp(), (int)N, c->stream));
    HIPOK(hipcub::DeviceScan::InclusiveSum(nullptr, tb_sum, d_flag, d_fsum, (int)N, c->stream));
    tb = std::max(tb_sort, std::max(tb_scan, tb_sum));
    CHECK(scope.get((uint8_t**)&d_tmp, tb));
    const dim3 grid((N + 255) / 256), block(256);
    { LaunchScope ls(c, "k_cluster_keys", (double)N);
      hipLaunchKernelGGL(k_cluster_keys, grid, block, 0, c->stream, N, d_ref, d_strand, d_keys, d_vals); }
    HIPOK(hipcub::DeviceRadixSort::SortPairs(d_tmp, tb_sort, d_keys, d_skeys, d_vals, d_perm, (int)N, 0, 33, c->stream));
    { LaunchScope ls(c, "k_cluster_items", (double)N);
      hipLaunchKernelGGL(k_cluster_items, grid, block, 0, c->stream, N, d_skeys, d_perm, d_off, d_query, d_qlen, d_items); }
    HIPOK(hipcub::DeviceScan::InclusiveScan(d_tmp, tb_scan, d_items, d_scanned, ClusterScanOp(), (int)N, c->stream));
    { LaunchScope ls(c, "k_cluster_flags", (double)N);
      hipLaunchKernelGGL(k_cluster_flags, grid, block, 0, c->stream, N, d_scanned, d_perm, d_off, threshold, d_flag); }
    HIPOK(hipcub::DeviceScan::InclusiveSum(d_tmp, tb_sum, d_flag, d_fsum, (int)N, c->stream));
    { LaunchScope ls(c, "k_cluster_kept", (double)N);
      hipLaunchKernelGGL(k_cluster_kept, grid, block, 0, c->stream, N, d_scanned, d_flag, d_fsum, d_skip, minus_first_only, d_kept, d_dropped); }
    HIPOK(hipcub::DeviceScan::InclusiveSum(d_tmp, tb_sum, d_kept, d_ksum, (int)N, c->stream));
    { LaunchScope ls(c, "k_cluster_assign", (double)N);
      const ClusterTable tab{t_ref, t_strand, t_start, t_end, t_reads, t_members};
      hipLaunchKernelGGL(k_cluster_assign, grid, block, 0, c->stream, N, d_scanned, d_perm, d_kept, d_ksum, d_dropped, d_off, d_query, d_qlen,
                         d_qcount, d_cluster, tab); }
    HIPOK(hipMemcpyAsync(&nc, d_ksum + (N - 1), 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(cluster, d_cluster, (size_t)N * 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    if (nc) {
        HIPOK(hipMemcpyAsync(c_ref, t_ref, (size_t)nc * 4, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipMemcpyAsync(c_strand, t_strand, (size_t)nc, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipMemcpyAsync(c_start, t_start, (size_t)nc * 8, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipMemcpyAsync(c_end, t_end, (size_t)nc * 8, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipMemcpyAsync(c_reads, t_reads, (size_t)nc * 8, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipMemcpyAsync(c_members, t_members, (size_t)nc * 4, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipStreamSynchronize(c->stream));
    }
    HIPOK(hipGetLastError());
    *n_clusters = nc;
    return 0;
}

// ---- windows of the genome as text (mirge_genome_fetch): templateSeq of calculateFeature and the precursor windows of
// get_precursors.  The caller computes the bounds (it knows the references' lengths); the kernel only copies.
extern "C" int mirge_genome_fetch(mirge_ctx* c, const mirge_genome* g, int64_t n, const uint32_t* ref, const int64_t* start,
                                  const int64_t* len, const uint8_t* minus, const uint8_t* rna, const int64_t* out_off, char* out) {
    if (!c || !g || n < 0 || n > 0x7FFFFFFFll) return fail(-1, "mirge_genome_fetch: bad argument");
    if (n == 0) return 0;
    if (!ref || !start || !len || !minus || !rna || !out_off || out_off[0] != 0 || (out_off[n] > 0 && !out))
        return fail(-1, "mirge_genome_fetch: bad argument");
    std::vector<GenomeWindow> win((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        if (ref[i] >= g->n_refs || start[i] < 0 || len[i] < 0 || len[i] > 0x7FFFFFFFll || out_off[i + 1] - out_off[i] != len[i])
            return fail(-1, "mirge_genome_fetch: a window names a reference that does not exist, starts before base 0 or its "
                            "output stretch is not its length");
        GenomeWindow w{};
        w.start = (uint64_t)start[i]; w.out_off = (uint64_t)out_off[i]; w.ref = ref[i]; w.len = (uint32_t)len[i];
        w.minus = minus[i] ? 1 : 0; w.rna = rna[i] ? 1 : 0;
        win[(size_t)i] = w;
    }
    if (out_off[n] == 0) return 0;
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    GenomeWindow* d_win; char* d_out;
    PoolScope scope(c);
    CHECK(scope.get(&d_win, (size_t)n)); CHECK(scope.get(&d_out, (size_t)out_off[n]));
    HIPOK(hipMemcpyAsync(d_win, win.data(), (size_t)n * sizeof(GenomeWindow), hipMemcpyHostToDevice, c->stream));
    { LaunchScope ls(c, "k_genome_fetch", (double)out_off[n]);
      hipLaunchKernelGGL(k_genome_fetch, dim3((uint32_t)n), dim3(64), 0, c->stream, (uint32_t)n, d_win, g->text, g->s_start, g->n_str,
                         g->str_ref, g->str_off, d_out); }
    HIPOK(hipMemcpyAsync(out, d_out, (size_t)out_off[n], hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    HIPOK(hipGetLastError());
    return 0;
}
