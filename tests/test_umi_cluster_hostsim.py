"""The kernels of ``--umi-cluster directional`` on the CPU: ``csrc/kernels_umi.hpp`` itself compiled for the host
(tests/hostsim/umi_sim.cpp: the launches of csrc/native_umi.hpp, a launch's threads one after the other) against the restatement
(tests/umi_restate.py: UMI-tools' sequential search with ties both ways, and the closed form with founder flags).  The cases are those of the
GPU test (tests/umi_cases.py); flags are compared exactly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import umi_cases
import umi_restate

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostsim", "umi_sim.cpp")
SO = os.path.join(HERE, "hostsim", "_build", "libumisim.so")
CSRC = os.path.join(HERE, "..", "mirge3.0_amd", "csrc")


@pytest.fixture(scope="module")
def sim():
    deps = [SRC, os.path.join(CSRC, "kernels_umi.hpp")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])
    return C.CDLL(SO)


def run_sim(sim, reads, counts, f, b, hash_bits=-1, first=None):
    n = len(reads)
    data = np.frombuffer("".join(reads).encode(), np.uint8) if n else np.zeros(1, np.uint8)
    off = np.zeros(n + 1, np.int64)
    np.cumsum([len(r) for r in reads], out=off[1:])
    cnt = np.asarray(counts, dtype=np.uint32).reshape(-1)
    fst = np.arange(n, dtype=np.uint32) if first is None else np.asarray(first, dtype=np.uint32)
    out = np.full(max(n, 1), 7, np.uint8)
    stats = np.zeros(4, np.int64)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = sim.sim_umi_cluster(p(data), p(off), C.c_int64(n), p(cnt if n else np.zeros(1, np.uint32)), p(fst if n else np.zeros(1, np.uint32)),
                             C.c_int32(f), C.c_int32(b), C.c_int32(hash_bits), p(out), p(stats))
    return rc, out[:n], dict(zip(("founders", "eligible", "linked", "rounds"), stats.tolist()))


@pytest.mark.parametrize("name", sorted(umi_cases.all_cases()))
def test_flags_equal_the_restatement(sim, name):
    _, reads, counts, f, b = umi_cases.all_cases()[name]
    want = umi_cases.expected(name)
    rc, got, stats = run_sim(sim, reads, counts, f, b)
    assert rc == 0
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (name, bad[:5], [reads[i] for i in bad[:5]])
    assert stats["founders"] == int(want.sum())
    assert stats["eligible"] == sum(umi_restate.eligible(r, f, b) for r in reads)


def test_cases_hold_what_they_are_for():
    cases = umi_cases.all_cases()
    _, reads, counts, f, b = cases["threshold"]
    w = umi_cases.expected("threshold").reshape(-1, 2)
    # (v, a) pairs in the order c(v) = 1 | 2, 2 | 3, 3 | 1000, 1000 | 2^31, 2^31 with c(a) = 2 c(v) - 1, then 2 c(v) - 2
    assert w.tolist() == [[1, 0]] + [[0, 1], [1, 1]] * 4 and max(counts) == 2 ** 32 - 1
    _, reads, counts, f, b = cases["non_edges"]
    w = dict(zip(reads, umi_cases.expected("non_edges").tolist()))
    by_len = {L: [w[r] for r in reads if len(r) == L] for L in (255, 256, 257, 300, 8, 7)}
    assert by_len[255] == [1, 0, 0] and by_len[256] == [1, 0, 0] and by_len[257] == [1, 1, 1] and by_len[300] == [1, 1, 1]
    assert by_len[8] == [1, 0, 0] and by_len[7] == [1, 1]
    assert all(w[r] for r in reads if 29 <= len(r) <= 31)  # the non-edges: every read stands alone
    # the path: 600 nodes in a line, whatever the order of the reads; one founder alone, none but the count-2 read with it
    for name in ("chain_alone", "chain_shuffled"):
        _, reads, counts, f, b = cases[name]
        far, reached, deg = umi_cases.path_length(reads, f, b)
        assert reached == 600 and deg == 2 and (far == 599 if name == "chain_alone" else far >= 300)
        assert umi_cases.expected(name).tolist() == [1] + [0] * 599
    assert umi_cases.expected("chain_big_end").tolist() == [0] * 600 + [1]
    _, reads, counts, f, b = cases["heavy"]
    assert len(reads) > 8000 and 0 < umi_cases.expected("heavy").sum() < len(reads)
    assert umi_cases.expected("nothing_eligible").all()


def test_the_path_takes_rounds_and_collisions_change_nothing(sim):
    _, reads, counts, f, b = umi_cases.all_cases()["chain_alone"]
    rc, got, stats = run_sim(sim, reads, counts, f, b)
    assert rc == 0 and stats["linked"] == 600 and stats["rounds"] >= 2
    _, reads, counts, f, b = umi_cases.all_cases()["collisions"]
    want = umi_cases.expected("collisions")
    for bits in (6, 0):
        rc, got, _ = run_sim(sim, reads, counts, f, b, hash_bits=bits)
        assert rc == 0 and np.array_equal(got, want), bits


def test_a_layout_beyond_32_letters_is_refused(sim):
    assert run_sim(sim, ["ACGT" * 20], [1], 20, 20)[0] == -1
    assert run_sim(sim, ["ACGT" * 20], [1], 0, 0)[0] == -1
