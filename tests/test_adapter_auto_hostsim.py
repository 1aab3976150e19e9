"""The kernels of ``-a auto`` on the CPU: ``csrc/kernels_adapter.hpp`` itself compiled for the host (tests/hostsim/ad_sim.cpp: the launches in
the order of csrc/native_adapter.hpp, a launch's threads one after the other, the workgroup reductions and the four lanes of a walk step
as loops) against the restatement (tests/ad_restate.py), exactly: every field of ``mirge_adapter`` and, as probes, C and M of every
12-mer of the case, of absent ones and of a code past the table, with the table filled by either form.  The cases are those of the GPU test (tests/ad_cases.py) and 300
random small sets in which the rules for equal C decide."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ad_cases
import ad_restate
import mirge3_amd  # noqa: F401
from mirge3_amd import _ffi

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostsim", "ad_sim.cpp")
SO = os.path.join(HERE, "hostsim", "_build", "libadsim.so")
CSRC = os.path.join(HERE, "..", "mirge3.0_amd", "csrc")


@pytest.fixture(scope="module")
def sim():
    deps = [SRC, os.path.join(CSRC, "kernels_adapter.hpp"), os.path.join(CSRC, "kernels_ec.hpp")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])
    return C.CDLL(SO)


def run_sim(sim, reads, counts, codes, seed_grid, by_sort):
    n = len(reads)
    text = "".join(reads).encode()
    data = np.frombuffer(text, np.uint8) if text else np.zeros(1, np.uint8)
    off = np.zeros(n + 1, np.int64)
    np.cumsum([len(r) for r in reads], out=off[1:])
    cnt = np.asarray(counts or [0], dtype=np.uint32)
    probe = np.asarray(codes, dtype=np.uint32)
    psum, pmask = np.zeros(len(codes), np.uint64), np.zeros(len(codes), np.uint64)
    out = _ffi.MirgeAdapter()
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = sim.sim_adapter_infer(p(data), p(off), C.c_int64(n), p(cnt), C.c_int32(seed_grid), C.c_int32(by_sort), C.byref(out), p(probe), C.c_int64(len(codes)), p(psum), p(pmask))
    assert rc == 0
    return out.as_dict(), psum.tolist(), pmask.tolist()


def check(sim, reads, counts, want, codes, seed_grid, by_sort):
    got, psum, pmask = run_sim(sim, reads, counts, codes, seed_grid, by_sort)
    assert got == ad_restate.fields(want)
    wsum, wmask = ad_cases.probe_answers(want, codes)
    assert psum == wsum and pmask == wmask


@pytest.mark.parametrize("by_sort", [1, 0], ids=["sort", "atomic"])
@pytest.mark.parametrize("name", sorted(ad_cases.all_cases()))
def test_cases_equal_the_restatement(sim, name, by_sort):
    ad_cases.holds(name)
    c = ad_cases.all_cases()[name]
    check(sim, c["reads"], c["counts"], ad_cases.expected(name), ad_cases.probes(name), 1024, by_sort)  # (64 slots a thread)


def test_random_sets_equal_the_restatement(sim):
    ties = {"seed": 0, "left": 0, "right": 0}
    found = 0
    for seed in range(300):
        c = ad_cases.random_set(seed)
        want = ad_restate.infer(c["reads"], c["counts"])
        check(sim, c["reads"], c["counts"], want, ad_restate.probes_of(c["reads"], extra=[seed, 4 ** 12 - 1 - seed, 4 ** 12]), 8192, seed % 2)  # (8 slots a thread; the two forms in turn)
        for k in ties:
            ties[k] += want["ties"][k]
        found += want["len"] > 0
    assert found > 250 and min(ties.values()) > 0, ties  # equal C decided a seed, a left step and a right step somewhere
