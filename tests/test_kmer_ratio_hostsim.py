"""The kernels of ``--kmer-ratio`` on the CPU: ``csrc/kernels_ec.hpp`` itself compiled for the host (tests/hostsim/ec_ratio_sim.cpp: a
round's launches in the order of csrc/native_ec.hpp, k_ec_dominate and k_ec_fold between the spectrum and the classification) against
the restatement of sentences 2a and 2b (tests/ec_ratio_restate.py), exactly: final reads, the rounds in which a read changed, the
tallies, and per round the k-mers above H and the dominated among them.  The named cases of tests/ec_ratio_cases.py, its 300 small
random sets, and the cases of tests/ec_cases.py without a ratio; everything again with the hash cut to 4 bits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ec_cases
import ec_ratio_cases
import ec_restate

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostsim", "ec_ratio_sim.cpp")
SO = os.path.join(HERE, "hostsim", "_build", "libecratiosim.so")
CSRC = os.path.join(HERE, "..", "mirge3.0_amd", "csrc")


@pytest.fixture(scope="module")
def sim():
    deps = [SRC, os.path.join(CSRC, "kernels_ec.hpp")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])
    return C.CDLL(SO)


def run_sim(sim, case, hash_bits=-1, ratio=None):
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
    ad = np.zeros(2 * rounds, np.int64)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = sim.sim_kmer_correct_ratio(p(data), p(off), C.c_int64(n), p(cnt), p(fst), C.c_int32(case["ks"]), C.c_int32(case["ke"]), C.c_int32(case["H"]),
                                    C.c_int32(case["R"] if ratio is None else ratio), C.c_int32(hash_bits), p(fin), p(mask), p(stats), p(ad))
    return rc, {"final": [fin[off[i]:off[i + 1]].tobytes().decode() for i in range(n)],
                "rounds": [[case["ks"] + b for b in range(rounds) if (int(mask[i]) >> b) & 1] for i in range(n)],
                "tallies": [dict(zip(ec_restate.TALLIES, stats[7 * r:7 * r + 7].tolist())) for r in range(rounds)],
                "above": ad[0::2].tolist(), "dominated": ad[1::2].tolist()}


def check(sim, case, want, hash_bits, ratio=None):
    rc, got = run_sim(sim, case, hash_bits, ratio)
    assert rc == 0
    for key in ("final", "rounds", "tallies", "above", "dominated"):
        assert got[key] == want[key], key


@pytest.mark.parametrize("hash_bits", [-1, 4])
@pytest.mark.parametrize("name", sorted(ec_ratio_cases.all_cases()))
def test_cases_equal_the_restatement(sim, name, hash_bits):
    check(sim, ec_ratio_cases.all_cases()[name], ec_ratio_cases.expected(name), hash_bits)


@pytest.mark.parametrize("hash_bits", [-1, 4])
def test_random_sets_equal_the_restatement(sim, hash_bits):
    for case, want in ec_ratio_cases.random_sets():
        check(sim, case, want, hash_bits)


@pytest.mark.parametrize("name", sorted(ec_cases.all_cases()))
def test_without_a_ratio_nothing_changes(sim, name):
    case = ec_cases.all_cases()[name]
    zeros = [0] * (case["ke"] - case["ks"] + 1)
    check(sim, case, dict(ec_cases.expected(name), above=zeros, dominated=zeros), -1, ratio=0)


def test_a_bad_ratio_is_refused(sim):
    case = ec_ratio_cases.all_cases()["edge_80"]
    for ratio in (1, -1, -8):
        assert run_sim(sim, case, ratio=ratio)[0] == -1
