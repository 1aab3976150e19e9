"""The kernels of ``--read-qc`` on the CPU: ``csrc/kernels_qc.hpp`` itself compiled for the host (tests/hostsim/qc_sim.cpp: the launches in the
order of csrc/native_qc.hpp, a workgroup's threads one after the other between its barriers) against the restatement (tests/qc_restate.py),
exactly: every entry of both views on the named cases (tests/qc_cases.py) and on 300 random small texts, in either form of the text
histogram, fed in one piece and in three; the class profile against a NumPy restatement on random dictionaries with S = 1 and 3.  The
trimmed bounds handed to the kernels are the restatement's (on the device they are k_trim's: tests/test_read_qc_gpu.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import qc_cases
import qc_restate
import mirge3_amd  # noqa: F401
from mirge3_amd import readqc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostsim", "qc_sim.cpp")
SO = os.path.join(HERE, "hostsim", "_build", "libqcsim.so")
CSRC = os.path.join(HERE, "..", "mirge3.0_amd", "csrc")


@pytest.fixture(scope="module")
def sim():
    deps = [SRC, os.path.join(CSRC, "kernels_qc.hpp")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])
    return C.CDLL(SO)


def run_sim(sim, case, form_pos, pieces=1, pos_grid=2):
    """the case's text through the simulated launches -> the entries of both views"""
    buf, recs = qc_restate.views(case["text"], case["fmt"], case["min_len"], case["opts"])
    n = len(recs)
    text = np.frombuffer(buf, np.uint8)
    raw = qc_restate.records(case["text"], case["fmt"])  # the line bounds as k_nl_mark leaves them: a '\r' still inside
    arr = lambda xs: np.asarray(list(xs) or [0], dtype=np.int64)
    ls, le = arr(r[0] for r in raw), arr(r[1] for r in raw)
    fastq = case["fmt"] == 1
    qs, qe = (arr(r[2] for r in raw), arr(r[3] for r in raw)) if fastq else (None, None)
    stages = qc_restate.n_stages(case["opts"], fastq)
    stride = stages if case["per_modifier"] and stages > 1 else 1
    vs = ve = None
    if stages:  # [n][stride]: the last column is the read after the last modifier, the others hold what must not be looked at
        vs, ve = np.full((max(n, 1), stride), 3, np.int64), np.full((max(n, 1), stride), 1 << 40, np.int64)
        for i, r in enumerate(recs):
            vs[i, -1], ve[i, -1] = r["trimmed"]
    tab = np.zeros((2, readqc.VIEW_WORDS), np.uint64)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    cuts = [n * k // pieces for k in range(pieces + 1)]
    for r0, r1 in zip(cuts, cuts[1:]):
        rc = sim.sim_qc_accumulate(p(text), p(ls), p(le), p(qs), p(qe), p(vs), p(ve), C.c_int32(stride), C.c_int64(r0), C.c_int64(r1),
                                   C.c_int32(case["min_len"]), C.c_int32((case["opts"] or {}).get("base", 33)), C.c_int32(form_pos), C.c_int32(pos_grid), p(tab))
        assert rc == 0
    return readqc.sample_entries(tab.astype(np.int64), fastq)


def test_the_layout_constants_are_the_kernels():
    src = open(os.path.join(CSRC, "kernels_qc.hpp")).read()
    assert "#define MIRGE_QC_P 256" in src and "#define MIRGE_QC_NQ 94" in src and "#define MIRGE_QC_LENGTH 8 " in src
    from mirge3_amd import _ffi
    assert readqc.VIEW_WORDS == _ffi.QC_VIEW_WORDS == 8 + 65536 + 257 * 5 + 257 * 94 + 94 + 101 + 257 * 5


@pytest.mark.parametrize("form_pos", [1, 0], ids=["pos", "read"])
@pytest.mark.parametrize("name", sorted(qc_cases.all_cases()))
def test_cases_equal_the_restatement(sim, name, form_pos):
    case = qc_cases.all_cases()[name]
    want = qc_cases.expected(name)
    assert run_sim(sim, case, form_pos) == want
    assert run_sim(sim, case, form_pos, pieces=3, pos_grid=1) == want


def test_the_cases_hold_what_they_are_named_for():
    e = qc_cases.expected
    assert e("empty_text")[("reads", "raw", None, None, None)] == 0
    assert e("empty_sequence_lines")[("empty_reads", "raw", None, None, None)] == 2
    ov = e("lengths_around_the_wave_and_the_overflow_row")
    assert ov[("length", "raw", 300, None, None)] == 2 and sum(v for k, v in ov.items() if k[:3] == ("base", "raw", 256)) == 1 + 2 * 44
    assert sum(ov.get(("first", "raw", 256, l, None), 0) for l in "ACGTN") == 4
    assert ("length", "trimmed", 1, None, None) not in ov and ov[("length", "raw", 1, None, None)] == 2
    assert e("crlf")[("bases", "raw", None, None, None)] == 13 + 17
    lc = e("lower_case_u_iupac_and_dot")
    assert lc[("base", "raw", 4, "T", None)] == 1 and lc[("base", "raw", 18, "N", None)] == 1 and lc[("reads_with_N", "raw", None, None, None)] == 4
    q = e("qualities_at_both_ends")
    assert q[("qual", "raw", 0, 0, None)] == 2 and q[("qual", "raw", 1, 93, None)] == 3 and q[("qual_clamped", "raw", None, None, None)] == 2
    assert e("phred64_with_bytes_below_the_base")[("qual_clamped", "raw", None, None, None)] == 2 + 3
    mm = e("quality_line_of_the_wrong_length")
    assert mm[("qual_length_mismatch", "raw", None, None, None)] == 2 and mm[("qual_length_mismatch", "trimmed", None, None, None)] == 2
    assert sum(v for k, v in mm.items() if k[0] == "qual" and k[1] == "raw") == 8 + 4
    assert e("a_thousand_records")[("reads", "raw", None, None, None)] == 1000
    z = e("trimmed_to_length_zero")
    assert z[("empty_reads", "trimmed", None, None, None)] == 3 and z[("empty_reads", "raw", None, None, None)] == 0
    u = e("reads_under_the_minimum_length")
    assert u[("reads", "raw", None, None, None)] == 5 and u[("reads", "trimmed", None, None, None)] == 2
    f = e("fasta")
    assert ("qual_clamped", "raw", None, None, None) not in f and not any(k[0] in ("qual", "meanq") for k in f)


def test_random_texts_equal_the_restatement(sim):
    seen = {"trimmed_differs": 0, "crlf": 0, "fasta": 0}
    for seed in range(300):
        case = qc_cases.random_text(seed)
        want = qc_cases.restated(case)
        assert run_sim(sim, case, seed % 2, pieces=1 + seed % 3, pos_grid=1 + seed % 2) == want, seed
        seen["trimmed_differs"] += want[("bases", "raw", None, None, None)] != want[("bases", "trimmed", None, None, None)]
        seen["crlf"] += b"\r" in case["text"]
        seen["fasta"] += case["fmt"] == 2
    assert min(seen.values()) > 20, seen


@pytest.mark.parametrize("S", [1, 3])
def test_class_profile_equals_numpy(sim, S):
    rng = np.random.default_rng(S)
    n_pass = 9
    for trial in range(6):
        na, nb = int(rng.integers(0, 900)), int(rng.integers(0, 40))
        g = {}
        for key, n, lo, hi in (("a", na, 0, 256), ("b", nb, 256, 4000)):
            g[key] = dict(ps=rng.integers(-1, n_pass, max(n, 1)).astype(np.int8), seq=rng.integers(0, 1 << 62, max(n, 1)).astype(np.uint64),
                          nm=(rng.integers(0, 8, max(n, 1)) == 0).astype(np.uint64), ln=rng.integers(lo, hi, max(n, 1)),
                          cnt=(rng.integers(0, 3, (max(n, 1), S)) * rng.integers(1, 5000, (max(n, 1), S))).astype(np.uint32))
        with_mask = trial % 2 == 1
        la, lb = g["a"]["ln"].astype(np.uint8), g["b"]["ln"].astype(np.uint16)
        out = np.zeros((S, n_pass + 1, 257, 5, 2), np.uint64)
        p = lambda a: C.c_void_p(a.ctypes.data)
        rc = sim.sim_qc_class(C.c_int64(na), p(g["a"]["ps"]), p(g["a"]["seq"]), p(g["a"]["nm"]) if with_mask else None, p(la), p(g["a"]["cnt"]),
                              C.c_int64(nb), p(g["b"]["ps"]), p(g["b"]["seq"]), p(g["b"]["nm"]), p(lb), p(g["b"]["cnt"]),
                              C.c_int32(S), C.c_int32(n_pass), C.c_int32(trial % 3 != 2), C.c_int32(1 + trial % 3), p(out))
        assert rc == 0
        parts = []
        for key, n, masked in (("a", na, with_mask), ("b", nb, True)):
            x = g[key]
            first = np.where((x["ln"] == 0) | (masked & (x["nm"] == 1)), 4, (x["seq"] & np.uint64(3)).astype(np.int64))
            parts.append((x["ps"][:n].astype(np.int64), x["ln"][:n], first[:n], x["cnt"][:n]))
        want = qc_restate.class_profile(*[np.concatenate([q[k] for q in parts]) for k in range(4)], n_pass)
        assert np.array_equal(out.astype(np.int64), want), trial
        assert want[..., 0].sum() == sum(int(q[3].sum()) for q in parts)
