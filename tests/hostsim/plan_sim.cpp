// plan_sim.cpp -- the probe plan tables and the libraries' longest valid run on the CPU: csrc/mirge_core.hpp and
// csrc/mirge_libbuild.hpp themselves, and the text of a merged library (csrc/native_host.hpp), for tests/test_plan_reflen_host.py.
// No HIP.
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mirge_native.h"
#include "mirge_core.hpp"
#include "mirge_isotype.hpp"
#include "mirge_libbuild.hpp"
#include "native_host.hpp"

// out[0] = longest run of valid bases (MirgeHostLib::max_run), out[1] = kmax, out[2] = total (bases and separators);
// run_of_inv: the same run computed from the packed invalid bitmap alone, as mirge_lib_create_packed does
extern "C" int plansim_lib(const char* seq, const int64_t* off, int64_t n_refs, int64_t* out, int64_t* run_of_inv) {
    MirgeHostLib h;
    std::string err;
    if (mirge_hostlib_build(h, seq, off, n_refs, err)) return -1;
    out[0] = (int64_t)h.max_run; out[1] = h.kmax; out[2] = (int64_t)h.total;
    *run_of_inv = (int64_t)mirge_longest_valid_run(h.inv.data(), h.total);
    return 0;
}

// Two member libraries and the library mirge_cascade_run merges them into (merged_library_text, then mirge_hostlib_build as
// mirge_lib_create does): out = {max_run of a, of b, of the merged library, the merged library's total}
extern "C" int plansim_merged(const char* seq_a, const int64_t* off_a, int64_t n_a, const char* seq_b, const int64_t* off_b, int64_t n_b,
                              int64_t* out) {
    MirgeHostLib a, b, m;
    std::string err, seq;
    std::vector<int64_t> off;
    if (mirge_hostlib_build(a, seq_a, off_a, n_a, err) || mirge_hostlib_build(b, seq_b, off_b, n_b, err)) return -1;
    const MirgeHostLib* members[2] = {&a, &b};
    merged_library_text(members, 2, seq, off);
    if (mirge_hostlib_build(m, seq.data(), off.data(), (int64_t)off.size() - 1, err)) return -1;
    out[0] = a.max_run; out[1] = b.max_run; out[2] = m.max_run; out[3] = (int64_t)m.total;
    return 0;
}

// valid windows of length L in the library, by brute force over its invalid bitmap: windows[L] for L = 0 .. n_len - 1
extern "C" int plansim_windows(const char* seq, const int64_t* off, int64_t n_refs, int64_t* windows, int32_t n_len) {
    MirgeHostLib h;
    std::string err;
    if (mirge_hostlib_build(h, seq, off, n_refs, err)) return -1;
    for (int L = 0; L < n_len; L++) {
        int64_t n = 0;
        for (uint64_t g = 0; L >= 1 && g + (uint64_t)L <= h.total; g++) {
            bool ok = true;
            for (int k = 0; k < L && ok; k++) ok = !((h.inv[(g + k) >> 6] >> ((g + k) & 63)) & 1ull);
            n += ok;
        }
        windows[L] = n;
    }
    return 0;
}

// the plan table of (policy, K, npos): np[L] and probe q of length L as out_pr[(L * MIRGE_MAX_PROBES + q) * 4 + {a1, k1, gap, k2}].
// max_window < 0: mirge_plan_table_fill called WITHOUT the bound (its default); returns MIRGE_MAX_PROBES
extern "C" int plansim_plan(const MirgePolicy* pol, int32_t K, int64_t npos, int32_t max_window, uint8_t* out_np, int32_t* out_pr) {
    const MirgePolicy p = *pol;
    std::vector<MirgePlanTable> t(1);
    std::memset(&t[0], 0, sizeof(MirgePlanTable));
    if (max_window < 0) mirge_plan_table_fill(p, K, (uint64_t)npos, t[0]);
    else mirge_plan_table_fill(p, K, (uint64_t)npos, t[0], max_window);
    for (int L = 0; L <= MIRGE_MAX_READ_LEN; L++) {
        out_np[L] = t[0].np[L];
        for (int q = 0; q < MIRGE_MAX_PROBES; q++) {
            const MirgeProbe& pr = t[0].pr[L][q];
            int32_t* o = out_pr + ((size_t)L * MIRGE_MAX_PROBES + q) * 4;
            o[0] = pr.a1; o[1] = pr.k1; o[2] = pr.gap; o[3] = pr.k2;
        }
    }
    return MIRGE_MAX_PROBES;
}
