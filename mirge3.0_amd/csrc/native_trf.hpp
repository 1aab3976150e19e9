// native_trf.hpp -- part of mirge_native.hip (one translation unit): the two device calls behind the tRNA fragment report
// (kernels_trf.hpp).  mirge_trf_hits: the rows' probe tables made sure of, a counting pass, one exclusive scan, the writing pass into
// every row's own stretch, one radix sort of (row, global position) keys, the records finished and copied to the host.
// mirge_trf_assign: the predefined tRFs uploaded as one CSR, one kernel over the rows.  Every call's blocks: one PoolScope.
// mirge_trf_cluster (--trf-clusters): the points packed to their templates' columns, then density, nearest denser point and border
// over a tile list of (group, MIRGE_BLOCK points), with the O(n) steps of the reference's loop on the host between the launches.
#pragma once

struct mirge_trf_hits {  // on the host: the records in (row, reference, offset) order
    std::vector<uint32_t> row, ref;
    std::vector<int32_t> off;
    std::vector<uint8_t> mm, cls, type;
};

extern "C" void mirge_trf_hits_destroy(mirge_trf_hits* h) { delete h; }
extern "C" int64_t mirge_trf_hits_count(const mirge_trf_hits* h) { return h ? (int64_t)h->row.size() : 0; }
extern "C" int mirge_trf_hits_fetch(const mirge_trf_hits* h, uint32_t* row, uint32_t* ref, int32_t* off, uint8_t* mm, uint8_t* cls, uint8_t* type) {
    if (!h) return fail(-1, "mirge_trf_hits_fetch: bad argument");
    const size_t n = h->row.size();
    if (n && (!row || !ref || !off || !mm || !cls || !type)) return fail(-1, "mirge_trf_hits_fetch: bad argument");
    if (n) {
        std::memcpy(row, h->row.data(), n * 4); std::memcpy(ref, h->ref.data(), n * 4); std::memcpy(off, h->off.data(), n * 4);
        std::memcpy(mm, h->mm.data(), n); std::memcpy(cls, h->cls.data(), n); std::memcpy(type, h->type.data(), n);
    }
    return 0;
}

// the read groups and the cascade's answer (res == nullptr: none) as the tRF kernels read them
static int trf_groups(const std::string& who, const mirge_reads* U, const mirge_result* res, TrfTables& t) {
    if (res && res->n != U->n) return fail(-1, who + ": result and read set differ");
    static_assert(MIRGE_TRF_MAXG == MIRGE_NGROUPS, "read groups");
    for (int gi = 0; gi < MIRGE_NGROUPS; gi++) {
        const ReadGroup& g = U->g[gi];
        if (g.n && g.orig) return fail(-1, who + ": the read set is not a collapse result");
        if (res && g.n != res->g[gi].n && !res->dmeta) return fail(-1, who + ": result and read set differ");
        t.g[gi] = TrfGroup{g.seq, g.nmask, g.len, res ? res->g[gi].pass : nullptr, res ? res->g[gi].mm : nullptr, g.counts, g.base, g.n,
                           is_long_group(gi) ? 0 : g.W, 0};
    }
    return 0;
}

extern "C" int mirge_trf_hits_run(mirge_ctx* c, const mirge_reads* U, const mirge_result* res, int32_t mature_pass, const mirge_lib* mature_lib,
                                  const mirge_policy* mature_pol, int32_t primary_pass, const mirge_lib* primary_lib,
                                  const mirge_policy* primary_pol, const int64_t* rows, int64_t n_rows, const int32_t* anticodon,
                                  mirge_trf_hits** out) {
    const std::string who = "mirge_trf_hits_run";
    if (!c || !U || !res || !out || !mature_lib || !mature_pol || !primary_lib || !primary_pol || n_rows < 0 || (n_rows && !rows) ||
        (mature_lib->n_refs && !anticodon) || mature_pass < 0 || primary_pass < 0 || mature_pass == primary_pass ||
        mature_pass >= res->n_pass || primary_pass >= res->n_pass)
        return fail(-1, who + ": bad argument");
    if (n_rows >= 0x7FFFFFF0ll) return fail(-5, who + ": too many rows for one call");
    // offsets are reported as the window's start in the reference and the stratum is a TOTAL mismatch count: end-to-end policies
    // without a 5' trim (the two tRNA passes, manifoldAlign.py:85)
    for (const mirge_policy* p : {mature_pol, primary_pol})
        if (p->mode != 1 || p->trim5 || p->trim3 || p->mm < 0 || p->mm > 2 || p->maxtotal != p->mm) return fail(-1, who + ": not a -v policy without trims");
    std::unique_ptr<mirge_trf_hits> hits(new mirge_trf_hits);
    if (n_rows == 0) { *out = hits.release(); return 0; }
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    TrfTables t;
    std::memset(&t, 0, sizeof(t));
    CHECK(trf_groups(who, U, res, t));
    std::vector<uint32_t> r32((size_t)n_rows);
    for (int64_t k = 0; k < n_rows; k++) {
        if (rows[k] < 0 || rows[k] >= U->n) return fail(-1, who + ": row index out of range");
        r32[(size_t)k] = (uint32_t)rows[k];
    }
    // every probe table the rows can ask for (the cascade may have answered these passes from whole-read tables or a merged library)
    int32_t hist[MIRGE_MAX_READ_LEN + 1];
    reads_lengths_present(U, hist);
    CHECK(prepare_tables(const_cast<mirge_lib*>(mature_lib), *mature_pol, hist, false));
    CHECK(prepare_tables(const_cast<mirge_lib*>(primary_lib), *primary_pol, hist, false));
    t.cls[0].lib = mature_lib->view(); t.cls[1].lib = primary_lib->view();
    std::memcpy(&t.cls[0].pol, mature_pol, sizeof(MirgePolicy)); std::memcpy(&t.cls[1].pol, primary_pol, sizeof(MirgePolicy));
    t.cls[0].pass = mature_pass; t.cls[1].pass = primary_pass;

    const size_t n = (size_t)n_rows;
    uint32_t *d_rows, *d_flags, *d_row, *d_ref, flag = 0;
    int32_t *d_ac, *d_off;
    unsigned long long *d_cnt, *d_start, *d_keys = nullptr, *d_keys2, n_rec = 0;
    uint8_t *d_mm, *d_cls, *d_type;
    void* d_tmp;
    auto hits_pass = [&](bool write) {
        for (int W : {1, 2, 4, 8}) {
            bool present = false;
            for (int gi = 0; gi < MIRGE_NGROUPS; gi++) present = present || (t.g[gi].n && t.g[gi].W == W);
            if (!present) continue;
            LaunchScope ls(c, write ? "k_trf_hits_write" : "k_trf_hits_count", (double)n);
            const dim3 grid(grid_for(c, n)), block(MIRGE_BLOCK);
#define MIRGE_TRF_LAUNCH(WW)                                                                                                              \
    if (write) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_trf_hits<WW, true>), grid, block, 0, c->stream, t, (const uint32_t*)d_rows, (uint32_t)n, \
                                  d_cnt, (const unsigned long long*)d_start, d_keys, d_flags);                                            \
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_trf_hits<WW, false>), grid, block, 0, c->stream, t, (const uint32_t*)d_rows, (uint32_t)n,    \
                            d_cnt, (const unsigned long long*)d_start, d_keys, d_flags)
            switch (W) {
                case 1: MIRGE_TRF_LAUNCH(1); break;
                case 2: MIRGE_TRF_LAUNCH(2); break;
                case 4: MIRGE_TRF_LAUNCH(4); break;
                default: MIRGE_TRF_LAUNCH(8); break;
            }
#undef MIRGE_TRF_LAUNCH
        }
    };
    PoolScope scope(c);  // (behind r32, hits, n_rec and flag, which the copies read or fill: they outlive its wait)
    const size_t n_ac = std::max<size_t>((size_t)mature_lib->n_refs, 1);
    CHECK(scope.get(&d_rows, n)); CHECK(scope.get(&d_flags, 16)); CHECK(scope.get(&d_ac, n_ac));
    CHECK(scope.get(&d_cnt, n + 1)); CHECK(scope.get(&d_start, n + 1));
    HIPOK(hipMemcpyAsync(d_rows, r32.data(), n * 4, hipMemcpyHostToDevice, c->stream));
    if (mature_lib->n_refs) HIPOK(hipMemcpyAsync(d_ac, anticodon, (size_t)mature_lib->n_refs * 4, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemsetAsync(d_flags, 0, 64, c->stream));
    HIPOK(hipMemsetAsync(d_cnt, 0, (n + 1) * 8, c->stream));
    t.anticodon = d_ac;
    hits_pass(false);
    size_t tb = 0;
    HIPOK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, d_cnt, d_start, (int)(n + 1), c->stream));
    CHECK(scope.get((uint8_t**)&d_tmp, std::max<size_t>(tb, 16)));
    HIPOK(hipcub::DeviceScan::ExclusiveSum(d_tmp, tb, d_cnt, d_start, (int)(n + 1), c->stream));
    HIPOK(hipMemcpyAsync(&n_rec, d_start + n, 8, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(&flag, d_flags, 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    HIPOK(hipGetLastError());
    if (flag & 1u) return fail(-1, who + ": a row is neither a mature-tRNA nor a primary-tRNA read");
    if (flag & 4u) return fail(-1, who + ": a probe table is missing");
    if (n_rec >= 0x7FFFFFF0ull) return fail(-5, who + ": " + std::to_string(n_rec) + " alignments to report in one call");
    if (n_rec == 0) { *out = hits.release(); return 0; }
    CHECK(scope.get(&d_keys, (size_t)n_rec)); CHECK(scope.get(&d_keys2, (size_t)n_rec));
    hits_pass(true);
    // ---- (row, global position) ascending = (row, reference, offset)
    int rbits = 1;
    while (rbits < 31 && (1ull << rbits) < (unsigned long long)n) rbits++;
    size_t tb2 = 0;
    HIPOK(hipcub::DeviceRadixSort::SortKeys(nullptr, tb2, d_keys, d_keys2, (int)n_rec, 0, 32 + rbits, c->stream));
    if (tb2 > std::max<size_t>(tb, 16)) { scope.give(d_tmp); CHECK(scope.get((uint8_t**)&d_tmp, tb2)); }
    HIPOK(hipcub::DeviceRadixSort::SortKeys(d_tmp, tb2, d_keys, d_keys2, (int)n_rec, 0, 32 + rbits, c->stream));
    CHECK(scope.get(&d_row, (size_t)n_rec)); CHECK(scope.get(&d_ref, (size_t)n_rec)); CHECK(scope.get(&d_off, (size_t)n_rec));
    CHECK(scope.get(&d_mm, (size_t)n_rec)); CHECK(scope.get(&d_cls, (size_t)n_rec)); CHECK(scope.get(&d_type, (size_t)n_rec));
    {
        LaunchScope ls(c, "k_trf_finish", (double)n_rec);
        hipLaunchKernelGGL(k_trf_finish, dim3(grid_for(c, (size_t)n_rec)), dim3(MIRGE_BLOCK), 0, c->stream, t, (const uint32_t*)d_rows,
                           (const unsigned long long*)d_keys2, (uint32_t)n_rec, d_row, d_ref, d_off, d_mm, d_cls, d_type);
    }
    hits->row.resize(n_rec); hits->ref.resize(n_rec); hits->off.resize(n_rec); hits->mm.resize(n_rec); hits->cls.resize(n_rec); hits->type.resize(n_rec);
    HIPOK(hipMemcpyAsync(hits->row.data(), d_row, n_rec * 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(hits->ref.data(), d_ref, n_rec * 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(hits->off.data(), d_off, n_rec * 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(hits->mm.data(), d_mm, n_rec, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(hits->cls.data(), d_cls, n_rec, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(hits->type.data(), d_type, n_rec, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(&flag, d_flags, 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    HIPOK(hipGetLastError());
    if (flag) return fail(-1, who + ": the writing pass and the counting pass disagree");
    *out = hits.release();
    return 0;
}

extern "C" int mirge_trf_assign(mirge_ctx* c, const mirge_reads* U, const mirge_result* res, int64_t n_rows, const int64_t* read,
                                const int32_t* tref, const int32_t* start, int64_t n_tref, const int64_t* ref_ptr, int64_t n_trf,
                                const int64_t* str_off, const char* str, const int32_t* c_start, const int32_t* c_end, const int32_t* rank,
                                int32_t* dist, int32_t* trf) {
    const std::string who = "mirge_trf_assign";
    if (!c || !U || !res || n_rows < 0 || n_tref < 0 || n_trf < 0 || (n_rows && (!read || !tref || !start || !dist || !trf)) ||
        (n_tref && !ref_ptr) || (n_trf && (!str_off || !c_start || !c_end || !rank)) || n_rows >= 0x7FFFFFF0ll || n_tref >= 0x7FFFFFF0ll ||
        n_trf >= 0x7FFFFFF0ll)
        return fail(-1, who + ": bad argument");
    if (n_rows == 0) return 0;
    const int64_t n_str = n_trf ? str_off[n_trf] : 0;
    if (n_str < 0 || n_str >= 0x7FFFFFF0ll || (n_str && !str) || (n_trf && str_off[0] != 0)) return fail(-1, who + ": the tRF strings are malformed");
    for (int64_t k = 0; k < n_trf; k++)
        if (str_off[k + 1] < str_off[k]) return fail(-1, who + ": the tRF strings are malformed");
    for (int64_t r = 0; r < n_tref; r++)
        if (ref_ptr[r] < 0 || ref_ptr[r + 1] < ref_ptr[r] || ref_ptr[r + 1] > n_trf) return fail(-1, who + ": the tRF table is malformed");
    std::vector<uint32_t> r32((size_t)n_rows), p32((size_t)n_tref + 1, 0u), o32((size_t)n_trf + 1, 0u);
    for (int64_t k = 0; k < n_rows; k++) {
        if (read[k] < 0 || read[k] >= U->n || tref[k] >= n_tref || start[k] < 1) return fail(-1, who + ": a row is out of range");
        r32[(size_t)k] = (uint32_t)read[k];
    }
    for (int64_t r = 0; r <= n_tref && n_tref; r++) p32[(size_t)r] = (uint32_t)ref_ptr[r];
    for (int64_t k = 0; k <= n_trf && n_trf; k++) o32[(size_t)k] = (uint32_t)str_off[k];
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    TrfTables t;
    std::memset(&t, 0, sizeof(t));
    CHECK(trf_groups(who, U, res, t));
    const size_t n = (size_t)n_rows, nt = (size_t)n_trf;
    uint32_t *d_read, *d_ptr, *d_soff;
    int32_t *d_tref, *d_start, *d_cs, *d_ce, *d_rank, *d_dist, *d_trf;
    uint8_t* d_str;
    PoolScope scope(c);  // (the host vectors above outlive its wait)
    CHECK(scope.get(&d_read, n)); CHECK(scope.get(&d_tref, n)); CHECK(scope.get(&d_start, n)); CHECK(scope.get(&d_dist, n)); CHECK(scope.get(&d_trf, n));
    CHECK(scope.get(&d_ptr, (size_t)n_tref + 1)); CHECK(scope.get(&d_soff, nt + 1)); CHECK(scope.get(&d_str, (size_t)n_str + 16));
    CHECK(scope.get(&d_cs, nt + 1)); CHECK(scope.get(&d_ce, nt + 1)); CHECK(scope.get(&d_rank, nt + 1));
    HIPOK(hipMemcpyAsync(d_read, r32.data(), n * 4, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(d_tref, tref, n * 4, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(d_start, start, n * 4, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(d_ptr, p32.data(), ((size_t)n_tref + 1) * 4, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(d_soff, o32.data(), (nt + 1) * 4, hipMemcpyHostToDevice, c->stream));
    if (n_str) HIPOK(hipMemcpyAsync(d_str, str, (size_t)n_str, hipMemcpyHostToDevice, c->stream));
    if (nt) {
        HIPOK(hipMemcpyAsync(d_cs, c_start, nt * 4, hipMemcpyHostToDevice, c->stream));
        HIPOK(hipMemcpyAsync(d_ce, c_end, nt * 4, hipMemcpyHostToDevice, c->stream));
        HIPOK(hipMemcpyAsync(d_rank, rank, nt * 4, hipMemcpyHostToDevice, c->stream));
    }
    TrfInfor f{d_ptr, d_soff, d_str, d_cs, d_ce, d_rank, (uint32_t)n_tref, (uint32_t)n_trf};
    {
        LaunchScope ls(c, "k_trf_assign", (double)n);
        hipLaunchKernelGGL(k_trf_assign, dim3(grid_for(c, n)), dim3(MIRGE_BLOCK), 0, c->stream, t, f, (const uint32_t*)d_read, (const int32_t*)d_tref,
                           (const int32_t*)d_start, (uint32_t)n, d_dist, d_trf);
    }
    HIPOK(hipMemcpyAsync(dist, d_dist, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(trf, d_trf, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    HIPOK(hipGetLastError());
    return 0;
}

extern "C" int mirge_trf_row_counts(mirge_ctx* c, const mirge_reads* U, const int64_t* rows, int64_t n_rows, uint32_t* out) {
    const std::string who = "mirge_trf_row_counts";
    if (!c || !U || n_rows < 0 || (n_rows && (!rows || !out)) || U->n_samples < 1) return fail(-1, who + ": bad argument");
    if ((unsigned long long)n_rows * (unsigned long long)U->n_samples >= 0x7FFFFFF0ull) return fail(-5, who + ": too many rows for one call");
    if (n_rows == 0) return 0;
    std::vector<uint32_t> r32((size_t)n_rows);
    for (int64_t k = 0; k < n_rows; k++) {
        if (rows[k] < 0 || rows[k] >= U->n) return fail(-1, who + ": row index out of range");
        r32[(size_t)k] = (uint32_t)rows[k];
    }
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    TrfTables t;
    std::memset(&t, 0, sizeof(t));
    CHECK(trf_groups(who, U, nullptr, t));
    const size_t n = (size_t)n_rows, total = n * (size_t)U->n_samples;
    uint32_t *d_rows, *d_out;
    PoolScope scope(c);
    CHECK(scope.get(&d_rows, n)); CHECK(scope.get(&d_out, total));
    HIPOK(hipMemcpyAsync(d_rows, r32.data(), n * 4, hipMemcpyHostToDevice, c->stream));
    {
        LaunchScope ls(c, "k_trf_row_counts", (double)total);
        hipLaunchKernelGGL(k_trf_row_counts, dim3(grid_for(c, total)), dim3(MIRGE_BLOCK), 0, c->stream, t, (const uint32_t*)d_rows, (uint32_t)n,
                           (int32_t)U->n_samples, d_out);
    }
    HIPOK(hipMemcpyAsync(out, d_out, total * 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    HIPOK(hipGetLastError());
    return 0;
}

// ---- density-peak clustering (kernels_trf.hpp: k_trf_cluster_pack, k_trf_density, k_trf_nearest, k_trf_border)
// Per point (CSR grp_ptr over the groups), 1-based within the group as the reference's indices are: rho, delta, nneigh (0: none), order (the
// 0-based position in sort_rho_idx), cl (-1: none), halo (0: halo or no cluster); per group nclust, and centre[grp_ptr[g] + k] = the
// centre of cluster k + 1 (0 behind the group's last cluster).
extern "C" int mirge_trf_cluster(mirge_ctx* c, const mirge_reads* U, int64_t n_grp, const int64_t* grp_ptr, const int64_t* read,
                                 const int32_t* off, const double* rp100k, const int32_t* tlen, int64_t n_gauss, const double* gauss,
                                 float* rho, float* delta, int32_t* nneigh, int32_t* order, int32_t* cl, int32_t* halo, int32_t* nclust,
                                 int32_t* centre) {
    const std::string who = "mirge_trf_cluster";
    if (!c || !U || n_grp < 0 || n_grp >= 0x7FFFFFF0ll || !grp_ptr || (n_grp && (!tlen || !nclust)) || n_gauss < 1 || !gauss)
        return fail(-1, who + ": bad argument");
    if (grp_ptr[0] != 0) return fail(-1, who + ": the group table is malformed");
    int max_tlen = 0;
    for (int64_t g = 0; g < n_grp; g++) {
        if (grp_ptr[g + 1] < grp_ptr[g]) return fail(-1, who + ": the group table is malformed");
        if (tlen[g] < 1) return fail(-1, who + ": a template has no columns");
        if (tlen[g] > MIRGE_TRF_CL_MAXCOL)
            return fail(-1, who + ": a template of " + std::to_string(tlen[g]) + " columns is longer than " + std::to_string(MIRGE_TRF_CL_MAXCOL));
        max_tlen = std::max(max_tlen, (int)tlen[g]);
    }
    const int64_t n_pts = grp_ptr[n_grp];
    if (n_pts >= 0x7FFFFFF0ll) return fail(-5, who + ": too many points for one call");
    if (n_pts && (!read || !off || !rp100k || !rho || !delta || !nneigh || !order || !cl || !halo || !centre)) return fail(-1, who + ": bad argument");
    if (n_gauss < 2 * (int64_t)max_tlen + 1) return fail(-1, who + ": the Gaussian table ends before distance 2 * the longest template");
    for (int64_t g = 0; g < n_grp; g++) nclust[g] = 0;
    if (n_pts == 0) return 0;
    const size_t n = (size_t)n_pts, ng = (size_t)n_grp;
    std::vector<uint32_t> r32(n), p32(ng + 1), tile_grp, tile_first;
    std::vector<int32_t> pt_tlen(n);
    for (int64_t k = 0; k < n_pts; k++) {
        if (read[k] < 0 || read[k] >= U->n) return fail(-1, who + ": a point's read is out of range");
        if (!(rp100k[k] >= 0.0) || !std::isfinite(rp100k[k])) return fail(-1, who + ": a point's RP100K is not a finite number >= 0");
        r32[(size_t)k] = (uint32_t)read[k];
    }
    uint32_t n_tile[2] = {0, 0};  // NW = 4, then NW = 8
    for (int pass = 0; pass < 2; pass++)
        for (size_t g = 0; g < ng; g++) {
            p32[g + 1] = (uint32_t)grp_ptr[g + 1];
            if ((tlen[g] > 128) != (pass == 1)) continue;
            for (int64_t k = grp_ptr[g]; k < grp_ptr[g + 1]; k++) pt_tlen[(size_t)k] = tlen[g];
            for (int64_t f = grp_ptr[g]; f < grp_ptr[g + 1]; f += MIRGE_BLOCK) { tile_grp.push_back((uint32_t)g); tile_first.push_back((uint32_t)f); n_tile[pass]++; }
        }
    p32[0] = 0;
    const size_t nt = tile_grp.size(), ngauss = (size_t)std::min<int64_t>(n_gauss, MIRGE_TRF_CL_MAXG);
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    TrfTables t;
    std::memset(&t, 0, sizeof(t));
    CHECK(trf_groups(who, U, nullptr, t));
    uint32_t *d_read, *d_flags, *d_ptr, *d_tg, *d_tf, flag = 0;
    int32_t *d_off, *d_tlen, *d_start, *d_end, *d_nn, *d_ord, *d_cl, *d_cen, *d_ncl, *d_dcen;
    uint64_t* d_words;
    double *d_rp, *d_gauss;
    float *d_rho, *d_delta, *d_bmax;
    std::vector<int32_t> cen(n, -1), dcen(n);
    std::vector<float> bmax(n);
    TrfClusterView v;
    auto tiles = [&](const char* name, auto launch4, auto launch8) {
        for (int pass = 0; pass < 2; pass++) {
            if (!n_tile[pass]) continue;
            LaunchScope ls(c, name, (double)n_tile[pass] * MIRGE_BLOCK);
            if (pass == 0) launch4(dim3(n_tile[0]), 0u); else launch8(dim3(n_tile[1]), n_tile[0]);
        }
    };
    PoolScope scope(c);  // (the host vectors and `flag` above outlive its wait)
    CHECK(scope.get(&d_read, n)); CHECK(scope.get(&d_off, n)); CHECK(scope.get(&d_tlen, n)); CHECK(scope.get(&d_start, n)); CHECK(scope.get(&d_end, n));
    CHECK(scope.get(&d_words, n * 2 * MIRGE_TRF_CL_MAXW)); CHECK(scope.get(&d_rp, n)); CHECK(scope.get(&d_gauss, ngauss)); CHECK(scope.get(&d_flags, 16));
    CHECK(scope.get(&d_ptr, ng + 1)); CHECK(scope.get(&d_tg, nt)); CHECK(scope.get(&d_tf, nt)); CHECK(scope.get(&d_rho, n)); CHECK(scope.get(&d_delta, n));
    CHECK(scope.get(&d_nn, n)); CHECK(scope.get(&d_ord, n)); CHECK(scope.get(&d_cl, n)); CHECK(scope.get(&d_cen, n)); CHECK(scope.get(&d_ncl, ng));
    CHECK(scope.get(&d_bmax, n)); CHECK(scope.get(&d_dcen, n));
    HIPOK(hipMemcpyAsync(d_read, r32.data(), n * 4, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(d_off, off, n * 4, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(d_tlen, pt_tlen.data(), n * 4, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(d_rp, rp100k, n * 8, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(d_gauss, gauss, ngauss * 8, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(d_ptr, p32.data(), (ng + 1) * 4, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(d_tg, tile_grp.data(), nt * 4, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(d_tf, tile_first.data(), nt * 4, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemsetAsync(d_flags, 0, 64, c->stream));
    {
        LaunchScope ls(c, "k_trf_cluster_pack", (double)n);
        hipLaunchKernelGGL(k_trf_cluster_pack, dim3(grid_for(c, n)), dim3(MIRGE_BLOCK), 0, c->stream, t, (const uint32_t*)d_read, (const int32_t*)d_off,
                           (const int32_t*)d_tlen, (uint32_t)n, d_words, d_start, d_end, d_flags);
    }
    HIPOK(hipMemcpyAsync(&flag, d_flags, 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    HIPOK(hipGetLastError());
    if (flag & 1u) return fail(-1, who + ": a point's read is of the long class");
    if (flag & 2u) return fail(-1, who + ": a point does not fit its template");
    v = TrfClusterView{d_words, d_start, d_end, d_rp, d_ptr, d_tg, d_tf, d_gauss, (int32_t)ngauss, 0};
    tiles("k_trf_density",
          [&](dim3 g, uint32_t t0) { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_trf_density<4>), g, dim3(MIRGE_BLOCK), 0, c->stream, v, t0, d_rho); },
          [&](dim3 g, uint32_t t0) { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_trf_density<8>), g, dim3(MIRGE_BLOCK), 0, c->stream, v, t0, d_rho); });
    tiles("k_trf_nearest",
          [&](dim3 g, uint32_t t0) { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_trf_nearest<4>), g, dim3(MIRGE_BLOCK), 0, c->stream, v, t0, (const float*)d_rho, d_delta, d_nn, d_ord); },
          [&](dim3 g, uint32_t t0) { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_trf_nearest<8>), g, dim3(MIRGE_BLOCK), 0, c->stream, v, t0, (const float*)d_rho, d_delta, d_nn, d_ord); });
    HIPOK(hipMemcpyAsync(rho, d_rho, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(delta, d_delta, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(nneigh, d_nn, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(order, d_ord, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    HIPOK(hipGetLastError());
    if (trf_cluster_assign(n_grp, grp_ptr, rho, delta, nneigh, order, cl, centre, nclust, cen.data()))
        return fail(-1, who + ": the density order is no permutation");
    HIPOK(hipMemcpyAsync(d_cl, cl, n * 4, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(d_cen, cen.data(), n * 4, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(d_ncl, nclust, ng * 4, hipMemcpyHostToDevice, c->stream));
    tiles("k_trf_border",
          [&](dim3 g, uint32_t t0) { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_trf_border<4>), g, dim3(MIRGE_BLOCK), 0, c->stream, v, t0, (const float*)d_rho, (const int32_t*)d_cl, (const int32_t*)d_cen, (const int32_t*)d_ncl, d_bmax, d_dcen); },
          [&](dim3 g, uint32_t t0) { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_trf_border<8>), g, dim3(MIRGE_BLOCK), 0, c->stream, v, t0, (const float*)d_rho, (const int32_t*)d_cl, (const int32_t*)d_cen, (const int32_t*)d_ncl, d_bmax, d_dcen); });
    HIPOK(hipMemcpyAsync(bmax.data(), d_bmax, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(dcen.data(), d_dcen, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    HIPOK(hipGetLastError());
    trf_cluster_halo(n_grp, grp_ptr, rho, cl, nclust, bmax.data(), dcen.data(), halo);
    return 0;
}
