"""The kernels of ``--trimmed-out`` on the CPU: ``csrc/kernels_fq.hpp`` itself compiled for the host (tests/hostsim/fq_sim.cpp: the launches in
the order of csrc/native_fq.hpp, a workgroup's threads one after the other between its barriers) against the restatement
(tests/fq_restate.py), exact bytes: the named cases (tests/fq_cases.py) and 300 random small texts, tiles of 64, 256 and the default, chunks
of 4096 and the default, one piece and three.  The bounds handed to the kernels are the restatement's (on the device they are k_trim's:
tests/test_trimmed_out_gpu.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fq_cases
import fq_restate
import qc_restate

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostsim", "fq_sim.cpp")
SO = os.path.join(HERE, "hostsim", "_build", "libfqsim.so")
CSRC = os.path.join(HERE, "..", "mirge3.0_amd", "csrc")
DEFAULT_TILE, DEFAULT_CHUNK = 16384, 32 << 20


@pytest.fixture(scope="module")
def sim():
    deps = [SRC, os.path.join(CSRC, "kernels_fq.hpp")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])
    return C.CDLL(SO)


def run_sim(sim, case, tile=DEFAULT_TILE, chunk=DEFAULT_CHUNK, pieces=1, grid=2):
    """the case's text through the simulated launches, cut into ``pieces`` at record bounds -> (S, records written, too short, mismatched)"""
    fmt = case["fmt"]
    buf, recs = qc_restate.views(case["text"], fmt, case["min_len"], case["opts"])
    raw = qc_restate.records(case["text"], fmt)  # the line bounds as k_nl_mark leaves them: a '\r' still inside
    heads = fq_restate.header_bounds(case["text"], fmt)
    n = len(recs)
    stages = qc_restate.n_stages(case["opts"], fmt == 1)
    stride = stages if case["per_modifier"] and stages > 1 else 1
    out, totals = b"", [0, 0, 0]
    cuts = [n * k // pieces for k in range(pieces + 1)]
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    for r0, r1 in zip(cuts, cuts[1:]):
        if r1 <= r0:
            continue
        base = heads[r0][0]  # a piece starts with its first record's header
        text = np.frombuffer(buf[base:], np.uint8)
        arr = lambda xs: np.asarray(list(xs), dtype=np.int64) - base
        ls, le = arr(r[0] for r in raw[r0:r1]), arr(r[1] for r in raw[r0:r1])
        qs, qe = (arr(r[2] for r in raw[r0:r1]), arr(r[3] for r in raw[r0:r1])) if fmt == 1 else (None, None)
        vs = ve = None
        if stages:  # [n][stride]: the last column is the read after the last modifier, the others hold what must not be looked at
            vs, ve = np.full((r1 - r0, stride), 3, np.int64), np.full((r1 - r0, stride), 1 << 40, np.int64)
            for i, r in enumerate(recs[r0:r1]):
                vs[i, -1], ve[i, -1] = r["trimmed"][0] - base, r["trimmed"][1] - base
        cap = 2 * len(buf) + 16
        dst = np.full(cap, 0xEE, np.uint8)
        out_n = C.c_int64()
        counts = np.zeros(3, np.uint64)
        rc = sim.sim_fq_piece(p(text), p(ls), p(le), p(qs), p(qe), p(vs), p(ve), C.c_int32(stride), C.c_int64(r1 - r0), C.c_int32(fmt), C.c_int32(case["min_len"]),
                              C.c_int64(tile), C.c_int64(chunk), C.c_int32(grid), p(dst), C.c_int64(cap), C.byref(out_n), p(counts))
        assert rc == 0
        out += dst[:out_n.value].tobytes()
        totals = [a + int(b) for a, b in zip(totals, counts)]
    return out, totals


@pytest.mark.parametrize("name", sorted(fq_cases.all_cases()))
def test_cases_equal_the_restatement(sim, name):
    case = fq_cases.all_cases()[name]
    want = fq_cases.expected(name)
    st = fq_restate.stats(case["text"], case["fmt"], case["min_len"], case["opts"])
    for tile in (64, 256, DEFAULT_TILE):
        for chunk in (4096, DEFAULT_CHUNK):
            for pieces, grid in ((1, 2), (3, 1)):
                got, (written, short, mismatch) = run_sim(sim, case, tile, chunk, pieces, grid)
                assert got == want, (tile, chunk, pieces)
                assert (written, written + short, mismatch) == (st["written"], st["records"], 0)
    assert st["stream_bytes"] == len(want)


def test_the_cases_hold_what_they_are_named_for():
    e, cases = fq_cases.expected, fq_cases.all_cases()
    assert e("empty_text") == b"" and e("every_record_dropped") == b""
    assert e("one_record") == b"@r0\nTGAGGTAGTAGGTTGTATAGTT\n+\nIIIIIIIIIIIIIIIIIIIIII\n"
    heads = [len(line) for line in e("header_lengths").split(b"\n")[0::4][:-1]]
    assert heads == [1, 15, 16, 17, 255, 300, 1, 16]
    assert b"\r" not in e("crlf") and b"\r" not in e("crlf_with_names") and b"\r" in cases["crlf_with_names"]["text"]
    assert e("crlf_with_names") == e("third_line_with_a_name") and b"+a" not in e("third_line_with_a_name") and b"@a 1:N:0\n" in e("third_line_with_a_name")
    long = e("a_long_read_behind_a_long_header").split(b"\n")
    assert len(long[4]) == 300 and len(long[5]) == 4980 == len(long[7])
    assert e("six_hundred_one_byte_records") == b"\n" * 600
    tiny = e("tiny_records_and_empty_reads")
    assert tiny.count(b"\n") == 600 and b"\n\n" in tiny and len(tiny) < 4 * 600
    assert b"acgtuUNnRYSWKMBDHV.ACGT" in e("lower_case_u_iupac_and_dot")
    cut = fq_cases.all_cases()["a_cut_and_a_quality_trim"]
    recs = qc_restate.views(cut["text"], 1, 16, cut["opts"])[1]
    assert all(r["trimmed"][0] == r["line"][0] + 3 for r in recs) and any(r["trimmed"][1] < r["line"][1] - 2 for r in recs)
    assert e("fasta_with_empty_sequences") == b">r0\nACGTACGT\n>r1\n\n>r2\nacgun\n>r3\n\n>r4\nGGGGCCCC\n>r5\n\n"
    assert e("empty_sequence_lines").count(b"\n\n+\n\n") == 2
    assert e("reads_under_the_minimum_length").count(b"@") == 2
    with pytest.raises(fq_restate.QualityLengthMismatch):
        fq_cases.restated(fq_cases.error_case())


def test_the_error_case_is_flagged_and_writes_nothing(sim):
    got, (written, short, mismatch) = run_sim(sim, fq_cases.error_case())
    assert mismatch == 2 and got == b""


def test_random_texts_equal_the_restatement(sim):
    seen = {"trimmed": 0, "crlf": 0, "fasta": 0, "dropped": 0}
    for seed in range(300):
        case = fq_cases.random_text(seed)
        want = fq_cases.restated(case)
        got, (written, short, mismatch) = run_sim(sim, case, (64, 256, DEFAULT_TILE)[seed % 3], (4096, DEFAULT_CHUNK)[seed % 2], 1 + 2 * (seed % 2), 1 + seed % 2)
        assert got == want and mismatch == 0, seed
        assert written == fq_restate.stats(case["text"], case["fmt"], case["min_len"], case["opts"])["written"]
        seen["trimmed"] += bool(case["opts"]) and len(want) > 0
        seen["crlf"] += b"\r" in case["text"]
        seen["fasta"] += case["fmt"] == 2
        seen["dropped"] += short > 0 and written > 0
    assert min(seen.values()) > 20, seen
