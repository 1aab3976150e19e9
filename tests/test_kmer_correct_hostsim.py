"""The kernels of ``--kmer-correct`` on the CPU: ``csrc/kernels_ec.hpp`` itself compiled for the host (tests/hostsim/ec_sim.cpp: the
launches of a round in the order of csrc/native_ec.hpp, a launch's threads one after the other, the wave kernel's lanes as a loop)
against the restatement (tests/ec_restate.py), exactly: final reads, the rounds in which a read changed, the tallies of every round.
The cases are those of the GPU test (tests/ec_cases.py) and random small sets; everything again with the hash cut to 4 bits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ec_cases
import ec_restate

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostsim", "ec_sim.cpp")
SO = os.path.join(HERE, "hostsim", "_build", "libecsim.so")
CSRC = os.path.join(HERE, "..", "mirge3.0_amd", "csrc")


@pytest.fixture(scope="module")
def sim():
    deps = [SRC, os.path.join(CSRC, "kernels_ec.hpp")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])
    return C.CDLL(SO)


def run_sim(sim, case, hash_bits=-1):
    reads, n = case["reads"], len(case["reads"])
    text = "".join(reads).encode()
    data = np.frombuffer(text, np.uint8) if text else np.zeros(1, np.uint8)
    off = np.zeros(n + 1, np.int64)
    np.cumsum([len(r) for r in reads], out=off[1:])
    cnt = np.asarray(case["counts"] or [0], dtype=np.uint32)
    fst = np.arange(max(n, 1), dtype=np.uint32)
    fin = np.zeros(max(len(text), 1), np.uint8)
    mask = np.zeros(max(n, 1), np.uint32)
    rounds = case["ke"] - case["ks"] + 1
    stats = np.zeros(7 * rounds, np.int64)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = sim.sim_kmer_correct(p(data), p(off), C.c_int64(n), p(cnt), p(fst), C.c_int32(case["ks"]), C.c_int32(case["ke"]), C.c_int32(case["H"]),
                              C.c_int32(hash_bits), p(fin), p(mask), p(stats))
    final = [fin[off[i]:off[i + 1]].tobytes().decode() for i in range(n)]
    which = [[case["ks"] + b for b in range(rounds) if (int(mask[i]) >> b) & 1] for i in range(n)]
    tallies = [dict(zip(ec_restate.TALLIES, stats[7 * r:7 * r + 7].tolist())) for r in range(rounds)]
    return rc, final, which, tallies


def check(sim, case, want, hash_bits):
    rc, final, which, tallies = run_sim(sim, case, hash_bits)
    assert rc == 0
    assert final == want["final"]
    assert which == want["rounds"]
    assert tallies == want["tallies"]


@pytest.mark.parametrize("hash_bits", [-1, 4])
@pytest.mark.parametrize("name", sorted(ec_cases.all_cases()))
def test_cases_equal_the_restatement(sim, name, hash_bits):
    check(sim, ec_cases.all_cases()[name], ec_cases.expected(name), hash_bits)


@pytest.mark.parametrize("hash_bits", [-1, 4])
def test_random_sets_equal_the_restatement(sim, hash_bits):
    corrected = 0
    for seed in range(400):
        letters = "AC" if seed % 3 == 0 else "ACGT"
        case = ec_cases.random_set(seed, letters=letters)
        want = ec_restate.correct(case["reads"], case["counts"], case["ks"], case["ke"], case["H"])
        check(sim, case, want, hash_bits)
        corrected += sum(t["corrected"] + t["ambiguous"] for t in want["tallies"])
    assert corrected > 100


def test_a_bad_range_is_refused(sim):
    case = dict(ec_cases.all_cases()["tie"])
    for ks, ke in ((7, 9), (10, 32), (11, 10)):
        assert run_sim(sim, dict(case, ks=ks, ke=ke))[0] == -1
