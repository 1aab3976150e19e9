"""The probe plans know the longest window a library can hold (csrc/mirge_core.hpp, mirge_plan_table_fill's ``max_window``;
csrc/mirge_libbuild.hpp, MirgeHostLib::max_run): a read trimmed to more than the library's longest run of valid bases gets no
probe, every shorter one exactly the probes it had.  On the CPU: the two headers themselves, compiled into
tests/hostsim/plan_sim.cpp.  The yardsticks are numpy on the library's text (the longest run) and a brute-force count of the
valid windows of every length."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mirge3_amd  # noqa: F401
from mirge3_amd import synth
from mirge3_amd.cascade import PASSES, policies
from mirge3_amd.seqio import FlatSeqs

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostsim", "plan_sim.cpp")
SO = os.path.join(HERE, "hostsim", "_build", "libplansim.so")
CSRC = os.path.join(HERE, "..", "mirge3.0_amd", "csrc")
MAX_LEN = 255  # MIRGE_MAX_READ_LEN


def _sim():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("mirge_core.hpp", "mirge_libbuild.hpp", "native_host.hpp")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-pthread", "-I", CSRC, "-o", SO, SRC])
    return C.CDLL(SO)


def _lib_args(seqs):
    fs = FlatSeqs.from_list(seqs)
    d, o = np.ascontiguousarray(fs.data), np.ascontiguousarray(fs.offsets, dtype=np.int64)
    return d, o, (C.c_void_p(d.ctypes.data), C.c_void_p(o.ctypes.data), C.c_int64(len(seqs)))


def lib_facts(seqs):
    """(max_run, kmax, total) as mirge_hostlib_build computes them; the run from the packed bitmap alone must agree"""
    d, o, args = _lib_args(seqs)
    out = np.zeros(3, dtype=np.int64)
    inv_run = C.c_int64(-1)
    assert _sim().plansim_lib(*args, C.c_void_p(out.ctypes.data), C.byref(inv_run)) == 0
    assert inv_run.value == out[0]
    return int(out[0]), int(out[1]), int(out[2])


def merged_facts(seqs_a, seqs_b):
    """(max_run of a, of b, of the library merged from both as a run of same-policy passes is, its total)"""
    da, oa, a = _lib_args(seqs_a)
    db, ob, b = _lib_args(seqs_b)
    out = np.zeros(4, dtype=np.int64)
    assert _sim().plansim_merged(*a, *b, C.c_void_p(out.ctypes.data)) == 0
    return tuple(int(x) for x in out)


def windows_by_length(seqs, n_len):
    d, o, args = _lib_args(seqs)
    w = np.zeros(n_len, dtype=np.int64)
    assert _sim().plansim_windows(*args, C.c_void_p(w.ctypes.data), C.c_int32(n_len)) == 0
    return w


def plan(pol, K, npos, max_window):
    """(np[256], probes [256, MAX_PROBES, 4]); ``max_window`` None = the call without the bound"""
    sim = _sim()
    np_out = np.zeros(MAX_LEN + 1, dtype=np.uint8)
    pr = np.full((MAX_LEN + 1) * 16 * 4, -99, dtype=np.int32)
    n = sim.plansim_plan(C.byref(pol), C.c_int32(K), C.c_int64(npos), C.c_int32(-1 if max_window is None else max_window),
                         C.c_void_p(np_out.ctypes.data), C.c_void_p(pr.ctypes.data))
    assert 1 <= n <= 16
    return np_out, pr[:(MAX_LEN + 1) * n * 4].reshape(MAX_LEN + 1, n, 4)


def longest_run_numpy(seqs):
    """the longest stretch of A/C/G/T/U inside one reference"""
    return max([len(m) for s in seqs for m in re.findall(r"[ACGTUacgtu]+", s)] + [0])


def _rand(rng, L):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=L))


def _libraries():
    """name -> sequences: the tiny synthetic set's libraries, a miRNA library whose longest reference holds an N, a library of
    one reference, one without a valid base, and the two members of a merged library whose bounds differ (the second holds an N
    inside its longest reference) with the text they merge into"""
    rng = np.random.default_rng(77)
    sl = synth.make_libraries(seed=41, scale="tiny")
    out = {k: v.seqs.to_list() for k, v in sl.libs.items() if k in ("mirna", "hairpin", "mature_trna", "snorna")}
    short = [_rand(rng, int(L)) for L in rng.integers(18, 23, size=30)]
    long_n = _rand(rng, 12) + "N" + _rand(rng, 15)  # 28 nt, but no window beyond 22 (the short ones) is free of the N
    out["internal_n"] = short[:10] + [long_n] + short[10:]
    out["single"] = [_rand(rng, 24)]
    out["all_n"] = ["NNNNNNNNNNNN", "NNNN"]
    # a merged run of passes is ONE library over the members' references in order (merged_library_text)
    out["merged_member_a"] = short
    out["merged_member_b"] = [_rand(rng, int(L)) for L in rng.integers(40, 62, size=12)] + [_rand(rng, 30) + "N" + _rand(rng, 44)]
    out["merged"] = out["merged_member_a"] + out["merged_member_b"]  # (what the merged text is: checked against plansim_merged below)
    return out


LIBS = _libraries()


def test_longest_run_is_the_longest_stretch_of_valid_bases():
    runs = {name: lib_facts(seqs)[0] for name, seqs in LIBS.items()}
    for name, seqs in LIBS.items():
        assert runs[name] == longest_run_numpy(seqs), name
    assert runs["internal_n"] == 22 and max(len(s) for s in LIBS["internal_n"]) == 28  # shorter than its longest reference
    assert runs["all_n"] == 0 and runs["single"] == 24
    # the merged library, through merged_library_text: the maximum over its members' own computed bounds, which differ
    ra, rb, rm, total = merged_facts(LIBS["merged_member_a"], LIBS["merged_member_b"])
    assert (ra, rb) == (runs["merged_member_a"], runs["merged_member_b"]) and ra != rb
    assert rm == max(ra, rb) == runs["merged"] and total == lib_facts(LIBS["merged"])[2]
    assert rb == longest_run_numpy(LIBS["merged_member_b"]) < max(len(s) for s in LIBS["merged_member_b"])
    # a run of whole 64-base words (the word-at-a-time path) and one that ends on a word's last base
    rng = np.random.default_rng(3)
    for L in (63, 64, 65, 128, 200, 300):
        seqs = [_rand(rng, 5), _rand(rng, L), _rand(rng, 7) + "N" + _rand(rng, 9)]
        assert lib_facts(seqs)[0] == L
        assert lib_facts([_rand(rng, 58)] + seqs)[0] == max(L, 58)  # the long reference starts off a word boundary


@pytest.mark.parametrize("pass_index", range(len(PASSES)))
@pytest.mark.parametrize("libname", sorted(LIBS))
def test_plan_is_empty_above_the_bound_and_unchanged_below(libname, pass_index):
    pol = policies(len(PASSES))[pass_index]
    seqs = LIBS[libname]
    M, kmax, total = lib_facts(seqs)
    np_old, pr_old = plan(pol, kmax, total, None)
    np_def, pr_def = plan(pol, kmax, total, MAX_LEN)
    assert np.array_equal(np_old, np_def) and np.array_equal(pr_old, pr_def)  # the default bounds nothing
    np_new, pr_new = plan(pol, kmax, total, min(M, MAX_LEN))
    top = min(M, MAX_LEN)
    assert np.array_equal(np_new[:top + 1], np_old[:top + 1]) and np.array_equal(pr_new[:top + 1], pr_old[:top + 1])
    assert not np_new[top + 1:].any()
    assert (pr_new[top + 1:] == 0).all()  # empty probes: a1 = k1 = gap = k2 = 0
    # today's plan probes every length beyond the policy's mismatch count: the bound is what removes them
    assert (np_old[max(top, pol.mm) + 1:] > 0).all()
    # zero windows exist exactly where the plan says so
    n_len = min(M + 6, MAX_LEN + 1)
    w = windows_by_length(seqs, n_len)
    for L in range(1, n_len):
        assert (w[L] == 0) == (L > M), (L, M, int(w[L]))
        if L > pol.mm:
            assert (np_new[L] == 0) == (w[L] == 0), (L, int(np_new[L]), int(w[L]))
