"""The kernels of ``--coverage`` on the CPU: ``csrc/kernels_cov.hpp`` itself compiled for the host (tests/hostsim/cov_sim.cpp: the launches
of csrc/native_cov.hpp, hipCUB's sort and scans as std::sort and loops) against the per-base brute force of tests/cov_cases.py, on the
cases of the GPU test.  Runs and text are compared exactly; the formatter runs at the default tile and at 64 bytes, where tile and chunk
boundaries fall inside numbers and names."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cov_cases

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostsim", "cov_sim.cpp")
SO = os.path.join(HERE, "hostsim", "_build", "libcovsim.so")
CSRC = os.path.join(HERE, "..", "mirge3.0_amd", "csrc")


@pytest.fixture(scope="module")
def sim():
    deps = [SRC, os.path.join(CSRC, "kernels_cov.hpp")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", "-o", SO, SRC])
    return C.CDLL(SO)


def run_sim(sim, iv, names, stranded, tile=8160, chunk=32 << 20, with_text=True, n_rank=None):
    n = int(iv["rank"].size)
    cap = 2 * n + 1
    out = dict(strand=np.full(cap, 9, np.uint8), chrom=np.zeros(cap, np.int32), start=np.zeros(cap, np.int64), end=np.zeros(cap, np.int64),
               depth=np.zeros(cap, np.int64))
    data = np.frombuffer("".join(names).encode(), np.uint8) if names else np.zeros(1, np.uint8)
    off = np.zeros(len(names) + 1, np.int64)
    np.cumsum([len(x) for x in names], out=off[1:])
    text_cap = 120 * cap
    text = np.zeros(text_cap, np.uint8)
    stats = np.zeros(5, np.int64)
    p = lambda a: C.c_void_p(a.ctypes.data)
    q = lambda a: p(a) if n else C.c_void_p(0)
    rc = sim.sim_coverage(C.c_int64(n), q(iv["rank"]), q(iv["start"]), q(iv["len"]), q(iv["weight"]), q(iv["minus"]),
                          C.c_int32(len(names) if n_rank is None else n_rank), C.c_int32(1 if stranded else 0), p(out["strand"]), p(out["chrom"]),
                          p(out["start"]), p(out["end"]), p(out["depth"]), p(data) if with_text else C.c_void_p(0), p(off), C.c_uint32(tile),
                          C.c_uint32(chunk), p(text), C.c_int64(text_cap), p(stats))
    st = dict(zip(("runs", "plus", "weight", "bytes", "plus_bytes"), stats.tolist()))
    return rc, {k: v[:st["runs"]] for k, v in out.items()}, bytes(text[:st["bytes"]]), st


@pytest.mark.parametrize("stranded", [False, True], ids=["unstranded", "stranded"])
@pytest.mark.parametrize("name", sorted(cov_cases.all_cases()))
def test_runs_and_text_equal_the_brute_force(sim, name, stranded):
    iv, names = cov_cases.all_cases()[name]
    want = cov_cases.expected(name, stranded)
    for tile, chunk in ((8160, 32 << 20), (64, 4096)):
        rc, got, text, st = run_sim(sim, iv, names, stranded, tile, chunk)
        assert rc == 0
        for k in ("strand", "chrom", "start", "end", "depth"):
            assert np.array_equal(got[k], want[k]), (name, k, tile)
        assert st["weight"] == int(iv["weight"].astype(np.uint64).sum()) and st["plus"] == int((want["strand"] == 0).sum())
        assert text == cov_cases.text(want, names), (name, tile)
        assert st["plus_bytes"] == len(cov_cases.text(want, names, 0))


def test_cases_hold_what_they_are_for():
    e = cov_cases.expected
    assert e("empty", False)["start"].size == 0 and e("one", True)["depth"].tolist() == [3]
    assert (e("abut_equal", False)["start"].tolist(), e("abut_equal", False)["end"].tolist()) == ([0], [20])
    assert e("abut_equal", True)["strand"].tolist() == [0, 1] and e("abut_unequal", False)["depth"].tolist() == [3, 4]
    assert list(zip(*(e("cancel_chain", True)[k].tolist() for k in ("strand", "start", "end", "depth")))) == [(0, 0, 25, 5), (0, 25, 35, 3), (1, 35, 40, 3)]
    assert list(zip(*(e("cancel_chain", False)[k].tolist() for k in ("start", "end", "depth")))) == [(0, 25, 5), (25, 40, 3)]
    assert e("many_equal", False)["depth"].tolist() == [10000]
    b = e("chrom_boundary", False)
    assert b["chrom"].tolist() == [2, 3, 3, 5, 7, 8] and b["end"][0] == b["start"][1] == 50 and b["end"][4] == b["start"][5] == 61
    s = e("strands", False)
    assert list(zip(s["chrom"].tolist(), s["start"].tolist(), s["end"].tolist(), s["depth"].tolist())) == [(0, 0, 20, 2), (0, 30, 50, 3), (1, 5, 25, 8)]
    assert e("strands", True)["strand"].tolist() == [0, 0, 0, 0, 1, 1, 1]
    assert e("large_weights", False)["depth"].max() == 3 * (2 ** 32 - 1) + 1 > 2 ** 33
    x = e("extreme_positions", False)
    assert x["start"].min() == 0 and x["end"].max() == 2 ** 31 - 1
    t = cov_cases.text(e("text", True), cov_cases.all_cases()["text"][1])
    assert b"c\t8\t9\t9\nc\t9\t10\t10\n" in t and b"\t99999\t100000\t100000\n" in t and b"\t99998\t99999\t99999\n" in t
    assert len(cov_cases.all_cases()["count_65537"][0]["rank"]) == 65537


def test_an_interval_outside_the_contract_is_refused(sim):
    names = ["a", "b"]
    ok = (0, 5, 7, 3, 0)
    for bad in ((2, 5, 7, 3, 0), (-1, 5, 7, 3, 0), (0, -1, 7, 3, 0), (0, 5, 0, 3, 0), (0, 5, 7, 0, 0), (0, 2 ** 31 - 7, 7, 1, 0)):
        rc, _, _, _ = run_sim(sim, cov_cases.make([ok, bad, ok]), names, False)
        assert rc == -1, bad
    assert run_sim(sim, cov_cases.make([ok, (1, 2 ** 31 - 8, 7, 1, 1)]), names, True)[0] == 0
