// native_umi.hpp -- part of mirge_native.hip (one translation unit): --umi-cluster directional (kernels_umi.hpp): the launch sequence of the
// founder flags, behind mirge_umi_cluster and behind mirge_reads_parse_umi with dedup == 2 (native_reads.hpp).
#pragma once

// what the last call on this thread saw: tagged reads, eligible ones, count-1 reads with a count-1 neighbour, propagation rounds, table slots
static thread_local int64_t g_umi_stats[5] = {0, 0, 0, 0, 0};

static int umi_check_layout(const std::string& who, int32_t front, int32_t back) {
    if (front < 0 || back < 0 || front + back < 1 || front + back > MIRGE_UMI_MAXTAG)
        return fail(-1, who + ": the UMI is the first f and the last b letters with 1 <= f + b <= " + std::to_string(MIRGE_UMI_MAXTAG));
    return 0;
}

// d_founder (device, [T->n], handle order): 1 = the read founds a molecule.  T: a collapse result with one count column.
static int umi_cluster_device(mirge_ctx* c, const mirge_reads* T, int32_t front, int32_t back, uint8_t* d_founder, int64_t* n_founders) {
    const std::string who = "mirge_umi_cluster";
    CHECK(umi_check_layout(who, front, back));
    for (int64_t& s : g_umi_stats) s = 0;
    *n_founders = 0;
    if (T->n == 0) return 0;
    if (T->n_samples != 1) return fail(-1, who + ": the tagged reads must be a collapse result with one count column");
    if (T->n >= 0x7FFFFFF0ll) return fail(-5, who + ": too many tagged reads for one call");
    UmiView v;
    std::memset(&v, 0, sizeof(v));
    static_assert(MIRGE_UMI_NG == MIRGE_NWIDTHS, "the groups without an N come first");
    for (int gi = 0; gi < MIRGE_NGROUPS; gi++) {
        const ReadGroup& g = T->g[gi];
        if (g.n && (g.orig || !g.counts || !g.first)) return fail(-1, who + ": the tagged reads are not a collapse result");
        if (gi < MIRGE_UMI_NG && g.n) v.g[gi] = UmiGroup{g.seq, g.len, g.counts, g.first, g.base, g.n, is_long_group(gi) ? 1 : 0, 0};
    }
    v.front = front; v.back = back; v.n_nodes = (uint32_t)T->n;
    v.hash_keep = ~0ull;
    if (const char* e = std::getenv("MIRGE_TEST_UMI_HASH_BITS")) {  // (tests: collisions on purpose)
        const int bits = std::atoi(e);
        if (bits >= 0 && bits < 64) v.hash_keep = (1ull << bits) - 1;
    }
    uint64_t slots = 256;
    while (slots < 2 * (uint64_t)v.n_nodes) slots <<= 1;
    v.tab_mask = slots - 1;
    const size_t n = v.n_nodes;
    uint64_t *tab, *label;
    uint32_t *state, *words;  // words[0] = a round changed a label; [1..3] = founders, eligible, linked
    int64_t rounds = 0;
    uint32_t tally[4] = {0, 0, 0, 0}, changed = 0;
    PoolScope scope(c);
    CHECK(scope.get(&tab, (size_t)slots)); CHECK(scope.get(&label, n)); CHECK(scope.get(&state, n)); CHECK(scope.get(&words, (size_t)4));
    HIPOK(hipMemsetAsync(tab, 0xFF, (size_t)slots * 8, c->stream));
    HIPOK(hipMemsetAsync(label, 0xFF, n * 8, c->stream));
    HIPOK(hipMemsetAsync(state, 0, n * 4, c->stream));
    HIPOK(hipMemsetAsync(words, 0, 16, c->stream));
    const dim3 grid(grid_for(c, n)), block(MIRGE_BLOCK);
    { LaunchScope ls(c, "k_umi_insert", (double)n); hipLaunchKernelGGL(k_umi_insert, grid, block, 0, c->stream, v, tab, state); }
    { LaunchScope ls(c, "k_umi_edges", (double)n); hipLaunchKernelGGL(k_umi_edges, grid, block, 0, c->stream, v, (const uint64_t*)tab, state, label); }
    for (;;) {
        { LaunchScope ls(c, "k_umi_round", (double)n); hipLaunchKernelGGL(k_umi_round, grid, block, 0, c->stream, v, (const uint64_t*)tab, (const uint32_t*)state, label, words); }
        HIPOK(hipMemcpyAsync(&changed, words, 4, hipMemcpyDeviceToHost, c->stream));
        HIPOK(hipStreamSynchronize(c->stream));
        HIPOK(hipGetLastError());
        rounds++;
        if (!changed) break;
        // (labels only fall, and a round that changes something lowers one: more rounds than nodes cannot be)
        if (rounds > (int64_t)n + 1) return fail(-3, who + ": the label propagation did not settle");
        HIPOK(hipMemsetAsync(words, 0, 4, c->stream));
    }
    { LaunchScope ls(c, "k_umi_comp_big", (double)n); hipLaunchKernelGGL(k_umi_comp_big, grid, block, 0, c->stream, v, state, (const uint64_t*)label); }
    { LaunchScope ls(c, "k_umi_founders", (double)n); hipLaunchKernelGGL(k_umi_founders, grid, block, 0, c->stream, v, (const uint32_t*)state, (const uint64_t*)label, d_founder, words); }
    HIPOK(hipMemcpyAsync(tally, words, 16, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    HIPOK(hipGetLastError());
    *n_founders = tally[1];
    g_umi_stats[0] = T->n; g_umi_stats[1] = tally[2]; g_umi_stats[2] = tally[3]; g_umi_stats[3] = rounds; g_umi_stats[4] = (int64_t)slots;
    return 0;
}

extern "C" int mirge_umi_cluster(mirge_ctx* c, const mirge_reads* tagged, int32_t front, int32_t back, uint8_t* founder_out, int64_t* n_founders) {
    const std::string who = "mirge_umi_cluster";
    if (!c || !tagged || tagged->ctx != c || !n_founders || (tagged->n && !founder_out)) return fail(-1, who + ": bad argument");
    CHECK(umi_check_layout(who, front, back));
    HIPOK(hipSetDevice(c->device)); CHECK(join_pending_now(c));
    *n_founders = 0;
    if (tagged->n == 0) { for (int64_t& s : g_umi_stats) s = 0; return 0; }
    PoolScope scope(c);
    uint8_t* d;
    CHECK(scope.get(&d, (size_t)tagged->n));
    CHECK(umi_cluster_device(c, tagged, front, back, d, n_founders));
    HIPOK(hipMemcpyAsync(founder_out, d, (size_t)tagged->n, hipMemcpyDeviceToHost, c->stream));
    HIPOK(hipStreamSynchronize(c->stream));
    return 0;
}

// the last mirge_umi_cluster / clustering parse of this thread: out[0..4] = tagged reads, eligible reads, count-1 reads with a count-1
// neighbour, rounds of the label propagation, slots of the lookup table
extern "C" int mirge_umi_cluster_stats(int64_t* out) {
    if (!out) return fail(-1, "mirge_umi_cluster_stats: bad argument");
    for (int k = 0; k < 5; k++) out[k] = g_umi_stats[k];
    return 0;
}
