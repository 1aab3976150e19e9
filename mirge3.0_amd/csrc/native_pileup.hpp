// native_pileup.hpp -- part of mirge_native.hip (one translation unit): the (cluster, read) rows of a sample's
// <sample>_modified_selected_sorted.tsv as a gapless pile-up per cluster (mirge_cluster_diagonals, mirge_cluster_pileup), what
// the reference makes with two pairwise2.align.localms calls per row and string stacking (readCluster.py:41-142).
// Kernels: kernels_pileup.hpp.
#pragma once

static int pileup_check_flat(const std::string& w, const char* text, const int64_t* off, int64_t n, int64_t maxlen, const char* what) {
    if (!off || (off[n] > 0 && !text) || off[0] != 0) return fail(-1, w + ": bad " + what + " arrays");
    for (int64_t i = 0; i < n; i++) {
        if (off[i + 1] < off[i]) return fail(-1, w + ": " + what + " offsets decrease");
        if (off[i + 1] - off[i] > maxlen) return fail(-1, w + ": a " + what + " is longer than " + std::to_string(maxlen) + " nt");
    }
    return 0;
}

extern "C" int mirge_cluster_diagonals(mirge_ctx* c, const char* reads, const int64_t* r_off, int64_t n_rows, const char* clusters,
                                       const int64_t* c_off, int64_t n_clusters, const uint32_t* row_cluster, int32_t* diag,
                                       int32_t* score, int32_t* identity, uint8_t* flag) {
    const std::string w("mirge_cluster_diagonals");
    if (!c || n_rows < 0 || n_clusters < 0 || n_rows > 0x7FFFFFFFll) return fail(-1, w + ": bad argument");
    if (n_rows == 0) return 0;
    if (!row_cluster || !diag || !score || !identity || !flag) return fail(-1, w + ": bad argument");
    CHECK(pileup_check_flat(w, reads, r_off, n_rows, MIRGE_PILEUP_MAXREAD, "read"));
    CHECK(pileup_check_flat(w, clusters, c_off, n_clusters, MIRGE_PILEUP_MAXCLUSTER, "cluster"));
    for (int64_t i = 0; i < n_rows; i++)
        if (row_cluster[i] >= (uint64_t)n_clusters) return fail(-1, w + ": a row names a cluster that does not exist");
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    const uint32_t N = (uint32_t)n_rows;
    char *d_reads, *d_clu; int64_t *d_roff, *d_coff; uint32_t* d_rc;
    int32_t *d_diag, *d_score, *d_id; uint8_t* d_flag;
    PoolScope scope(c);
    CHECK(scope.get(&d_reads, (size_t)r_off[n_rows])); CHECK(scope.get(&d_clu, (size_t)c_off[n_clusters]));
    CHECK(scope.get(&d_roff, (size_t)n_rows + 1)); CHECK(scope.get(&d_coff, (size_t)n_clusters + 1)); CHECK(scope.get(&d_rc, N));
    CHECK(scope.get(&d_diag, N)); CHECK(scope.get(&d_score, N)); CHECK(scope.get(&d_id, N)); CHECK(scope.get(&d_flag, N));
    if (r_off[n_rows]) HIPOK(hipMemcpyAsync(d_reads, reads, (size_t)r_off[n_rows], hipMemcpyHostToDevice, c->stream));
    if (c_off[n_clusters]) HIPOK(hipMemcpyAsync(d_clu, clusters, (size_t)c_off[n_clusters], hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(d_roff, r_off, ((size_t)n_rows + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(d_coff, c_off, ((size_t)n_clusters + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(d_rc, row_cluster, (size_t)N * 4, hipMemcpyHostToDevice, c->stream));
    { LaunchScope ls(c, "k_cluster_diagonals", (double)N);
      hipLaunchKernelGGL(k_cluster_diagonals, dim3((N + MIRGE_PILEUP_BLOCK - 1) / MIRGE_PILEUP_BLOCK), dim3(MIRGE_PILEUP_BLOCK), 0, c->stream,
                         N, d_reads, d_roff, d_clu, d_coff, d_rc, d_diag, d_score, d_id, d_flag); }
    HIPOK(hipMemcpyAsync(diag, d_diag, (size_t)N * 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(score, d_score, (size_t)N * 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(identity, d_id, (size_t)N * 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(flag, d_flag, (size_t)N, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    HIPOK(hipGetLastError());
    return 0;
}

// rows [row_start[k], row_start[k + 1]) are cluster k's.  col_off[n_clusters + 1] (out): where each cluster's columns start in
// tally[][5]; tally holds cap_cols columns -- sum(C) + 2 * (MAXREAD - 1) * n_clusters always suffices.
extern "C" int mirge_cluster_pileup(mirge_ctx* c, const char* reads, const int64_t* r_off, int64_t n_rows, const int64_t* c_len,
                                    const int64_t* row_start, int64_t n_clusters, const int32_t* diag, const int64_t* count,
                                    int32_t* head, int32_t* tail, int64_t* col_off, int64_t* tally, int64_t cap_cols) {
    const std::string w("mirge_cluster_pileup");
    if (!c || n_rows < 0 || n_clusters < 0 || n_rows > 0x7FFFFFFFll || n_clusters > 0x7FFFFFFFll || !col_off || cap_cols < 0)
        return fail(-1, w + ": bad argument");
    col_off[0] = 0;
    if (n_clusters == 0) return 0;
    if (!c_len || !row_start || !head || !tail || !tally || (n_rows && (!diag || !count))) return fail(-1, w + ": bad argument");
    std::vector<int64_t> r0(1, 0);
    CHECK(pileup_check_flat(w, reads, n_rows ? r_off : r0.data(), n_rows, MIRGE_PILEUP_MAXREAD, "read"));
    if (row_start[0] != 0 || row_start[n_clusters] != n_rows) return fail(-1, w + ": the row ranges do not cover the rows");
    std::vector<int64_t> c_off((size_t)n_clusters + 1, 0);
    std::vector<PileupItem> items;
    for (int64_t k = 0; k < n_clusters; k++) {
        if (row_start[k + 1] < row_start[k]) return fail(-1, w + ": the row ranges decrease");
        if (c_len[k] < 0 || c_len[k] > MIRGE_PILEUP_MAXCLUSTER)
            return fail(-1, w + ": a cluster is longer than " + std::to_string(MIRGE_PILEUP_MAXCLUSTER) + " nt");
        c_off[k + 1] = c_off[k] + c_len[k];
        for (int64_t r = row_start[k]; r < row_start[k + 1]; r++) {  // a diagonal on which read and cluster overlap
            const int64_t L = r_off[r + 1] - r_off[r];
            if (L < 1 || c_len[k] < 1 || diag[r] < -(L - 1) || diag[r] > c_len[k] - 1)
                return fail(-1, w + ": a row's diagonal leaves its read and cluster without a common column");
        }
        const bool whole = row_start[k + 1] - row_start[k] <= MIRGE_PILEUP_CHUNK;
        for (int64_t r = row_start[k]; r < row_start[k + 1]; r += MIRGE_PILEUP_CHUNK)
            items.push_back(PileupItem{(uint32_t)k, (uint32_t)r, (uint32_t)std::min<int64_t>(r + MIRGE_PILEUP_CHUNK, row_start[k + 1]), whole ? 1u : 0u});
        if (row_start[k + 1] == row_start[k]) items.push_back(PileupItem{(uint32_t)k, (uint32_t)row_start[k], (uint32_t)row_start[k], 1u});
    }
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    const uint32_t NI = (uint32_t)items.size();
    char* d_reads; int64_t *d_roff, *d_coff, *d_count, *d_col;
    int32_t *d_diag, *d_head, *d_tail; PileupItem* d_items; unsigned long long* d_tally;
    PoolScope scope(c);  // (r0, c_off and items, which the copies read, outlive it)
    const size_t nb = n_rows ? (size_t)r_off[n_rows] : 0;
    CHECK(scope.get(&d_reads, nb)); CHECK(scope.get(&d_roff, (size_t)n_rows + 1)); CHECK(scope.get(&d_coff, (size_t)n_clusters + 1));
    CHECK(scope.get(&d_count, (size_t)n_rows)); CHECK(scope.get(&d_col, (size_t)n_clusters + 1)); CHECK(scope.get(&d_diag, (size_t)n_rows));
    CHECK(scope.get(&d_head, (size_t)n_clusters)); CHECK(scope.get(&d_tail, (size_t)n_clusters)); CHECK(scope.get(&d_items, (size_t)NI));
    if (nb) HIPOK(hipMemcpyAsync(d_reads, reads, nb, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(d_roff, n_rows ? r_off : r0.data(), ((size_t)n_rows + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemcpyAsync(d_coff, c_off.data(), ((size_t)n_clusters + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (n_rows) {
        HIPOK(hipMemcpyAsync(d_count, count, (size_t)n_rows * 8, hipMemcpyHostToDevice, c->stream));
        HIPOK(hipMemcpyAsync(d_diag, diag, (size_t)n_rows * 4, hipMemcpyHostToDevice, c->stream));
    }
    HIPOK(hipMemcpyAsync(d_items, items.data(), (size_t)NI * sizeof(PileupItem), hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemsetAsync(d_head, 0, (size_t)n_clusters * 4, c->stream));
    HIPOK(hipMemsetAsync(d_tail, 0, (size_t)n_clusters * 4, c->stream));
    { LaunchScope ls(c, "k_pileup_extent", (double)n_rows);
      hipLaunchKernelGGL(k_pileup_extent, dim3(NI), dim3(64), 0, c->stream, NI, d_items, d_roff, d_coff, d_diag, d_head, d_tail); }
    HIPOK(hipMemcpyAsync(head, d_head, (size_t)n_clusters * 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipMemcpyAsync(tail, d_tail, (size_t)n_clusters * 4, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    for (int64_t k = 0; k < n_clusters; k++) {  // the paddings place every cluster's columns
        if (head[k] < 0 || head[k] >= MIRGE_PILEUP_MAXREAD || tail[k] < 0 || tail[k] >= MIRGE_PILEUP_MAXREAD)
            return fail(-3, w + ": a padding out of range came back from the device");
        col_off[k + 1] = col_off[k] + head[k] + c_len[k] + tail[k];
    }
    const int64_t cols = col_off[n_clusters];
    if (cols > cap_cols) return fail(-1, w + ": the tally array is too small for the columns");
    if (cols == 0) return 0;
    CHECK(scope.get(&d_tally, (size_t)cols * 5));
    HIPOK(hipMemcpyAsync(d_col, col_off, ((size_t)n_clusters + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPOK(hipMemsetAsync(d_tally, 0, (size_t)cols * 40, c->stream));
    { LaunchScope ls(c, "k_pileup_tally", (double)n_rows);
      hipLaunchKernelGGL(k_pileup_tally, dim3(NI), dim3(64), 0, c->stream, NI, d_items, d_reads, d_roff, d_coff, d_diag, d_count, d_head,
                         d_tail, d_col, d_tally); }
    HIPOK(hipMemcpyAsync(tally, d_tally, (size_t)cols * 40, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    HIPOK(hipGetLastError());
    return 0;
}
