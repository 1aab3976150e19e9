"""The kernels of ``--unmapped-nearest`` on the CPU: ``csrc/kernels_nearest.hpp`` itself compiled for the host (tests/hostsim/near_sim.cpp: the launches
in the order of csrc/native_nearest.hpp, a workgroup's threads one after the other between its barriers) against the restatement
(tests/near_restate.py), exactly: D, hairpin, s and e of every query of the named cases (tests/near_cases.py) and of the random set, in the
instance the length selects and with every query in the 64-bit instance, with chunks of 64 bases and of the default 4096; the dictionary
route (flag, selection, masks from the packed words, the cap) on a made-up dictionary with annotated rows mixed in."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import near_cases
import near_restate
import mirge3_amd  # noqa: F401
from mirge3_amd import nearest
from mirge3_amd.seqio import FlatSeqs

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostsim", "near_sim.cpp")
SO = os.path.join(HERE, "hostsim", "_build", "libnearsim.so")
CSRC = os.path.join(HERE, "..", "mirge3.0_amd", "csrc")
FIELDS = ("dist", "hairpin", "start", "end")


@pytest.fixture(scope="module")
def sim():
    deps = [SRC, os.path.join(CSRC, "kernels_nearest.hpp")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC])
    lib = C.CDLL(SO)
    lib.sim_nearest_unmapped.restype = C.c_int64
    return lib


def _flat(seqs):
    f = FlatSeqs.from_list(list(seqs))
    data = np.ascontiguousarray(f.data if f.data.size else np.zeros(1, np.uint8))
    return data, np.ascontiguousarray(f.offsets, dtype=np.int64), len(f)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def sim_scan(sim, queries, hairpins, chunk_bases, force64, tile_grid=2):
    q, q_off, n = _flat(queries)
    t, t_off, n_t = _flat(hairpins)
    out = {k: np.full(max(n, 1), -7, np.int32) for k in FIELDS}
    rc = sim.sim_nearest_scan(_p(q), _p(q_off), C.c_int64(n), _p(t), _p(t_off), C.c_int64(n_t), chunk_bases, force64, tile_grid, *(_p(out[k]) for k in FIELDS))
    assert rc == 0
    return {k: a[:n].astype(np.int64) for k, a in out.items()}


def check(sim, queries, hairpins, want=None):
    want = want or near_restate.nearest_all(queries, hairpins)
    for chunk_bases in (64, 4096):
        for force64 in (0, 1):
            got = sim_scan(sim, queries, hairpins, chunk_bases, force64)
            for k in FIELDS:
                assert np.array_equal(got[k], want[k]), (k, chunk_bases, force64, np.flatnonzero(got[k] != want[k])[:5])
    return want


@pytest.mark.parametrize("case", near_cases.CASES, ids=lambda c: c["name"])
def test_named_cases_equal_the_restatement(sim, case):
    check(sim, case["queries"], case["hairpins"])


def test_random_set_equals_the_restatement(sim):
    for hairpins, queries in near_cases.random_sets():
        check(sim, queries, hairpins)


def test_more_than_one_tile_and_a_striding_tile_grid(sim):
    """600 queries of both instances over one library: three tiles per instance, walked by one and by two rows of workgroups"""
    rng = random.Random(11)
    hairpins = [near_cases.rnd_seq(rng, rng.randint(30, 110)) for _ in range(9)]
    queries = []
    for i in range(600):
        h = rng.choice(hairpins)
        n = rng.randint(12, min(64, len(h)))
        at = rng.randrange(len(h) - n + 1)
        queries.append(near_cases.edit(rng, h[at:at + n], rng.randint(0, 4)))
    want = near_restate.nearest_all(queries, hairpins)
    for tile_grid in (1, 2):
        got = sim_scan(sim, queries, hairpins, 64, 0, tile_grid)
        for k in FIELDS:
            assert np.array_equal(got[k], want[k]), (k, tile_grid)


def pack(seqs):
    """reads of at most 64 nt -> (words [W][n], nmask [W][n], lengths) with W = 2"""
    n = len(seqs)
    w, nm = np.zeros((2, max(n, 1)), np.uint64), np.zeros((2, max(n, 1)), np.uint64)
    for i, s in enumerate(seqs):
        for p, ch in enumerate(s):
            if ch in "ACGT":
                w[p >> 5, i] |= np.uint64("ACGT".index(ch) << (2 * (p & 31)))
            else:
                nm[p >> 5, i] |= np.uint64(1 << (2 * (p & 31)))
    return w, nm, np.array([len(s) for s in seqs] + [0], dtype=np.uint8)


@pytest.mark.parametrize("K", [1, 3, 8])
def test_dictionary_route_keeps_the_capped_rows_of_the_unannotated(sim, K):
    rng = random.Random(5 + K)
    hairpins = [near_cases.rnd_seq(rng, rng.randint(40, 100)) for _ in range(7)] + [""]
    reads = []
    for i in range(700):
        h = rng.choice(hairpins[:7])
        n = rng.randint(8, min(64, len(h)))
        at = rng.randrange(len(h) - n + 1)
        reads.append(near_cases.edit(rng, h[at:at + n], rng.choice([0, 0, 1, 2, 3, 4, 9]))[:64] if i % 6 else near_cases.rnd_seq(rng, rng.randint(1, 64), "ACGTN"))
    a = [r for r in reads if len(r) <= 31]
    b = [r for r in reads if len(r) > 31]
    rows = a + b  # handle order: group A, then group B
    ps = np.array([(-1 if i % 4 else i % 3) for i in range(len(rows))], dtype=np.int8)
    wa, na, la = pack(a)
    wb, nb, lb = pack(b)
    wa, na = np.ascontiguousarray(wa[:1]), np.ascontiguousarray(na[:1])
    pa, pb = (np.ascontiguousarray(np.append(x, 0), dtype=np.int8) for x in (ps[:len(a)], ps[len(a):]))
    t, t_off, n_t = _flat(hairpins)
    for chunk_bases in (64, 4096):
        out = dict(row=np.zeros(len(rows) + 1, np.uint32), **{k: np.zeros(len(rows) + 1, np.int32) for k in FIELDS})
        stats = np.zeros(5, np.int64)
        kept = sim.sim_nearest_unmapped(C.c_int64(len(a)), _p(wa), _p(na), _p(la), _p(pa), C.c_int64(len(b)), _p(wb), _p(nb), _p(lb), _p(pb), _p(t), _p(t_off),
                                        C.c_int64(n_t), K, chunk_bases, _p(out["row"]), *(_p(out[k]) for k in FIELDS), _p(stats))
        want_rows, want = [], []
        unm = [i for i in range(len(rows)) if ps[i] < 0]
        for i in unm:
            r = near_restate.nearest(rows[i], hairpins)
            if near_restate.reported(rows[i], r[0], K):
                want_rows.append(i)
                want.append(r)
        assert kept == len(want_rows) > 20
        assert out["row"][:kept].tolist() == want_rows
        assert [tuple(int(out[k][j]) for k in FIELDS) for j in range(kept)] == want
        lens = [len(rows[i]) for i in unm]
        assert stats.tolist() == [len(unm), sum(n < 12 for n in lens), sum(n > 64 for n in lens), sum(12 <= n <= 64 for n in lens), kept]
        assert all(d <= nearest.cap(K, len(rows[i])) for i, (d, _, _, _) in zip(want_rows, want))


def test_stand_alone_program_builds_and_runs(tmp_path):
    """-DNEAR_SIM_MAIN: the program a sanitizer build runs (here without a sanitizer: that it is a program, and that it ends well)"""
    exe = tmp_path / "near_sim"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DNEAR_SIM_MAIN", "-o", str(exe), SRC])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("near_sim: 40 sets, checksum "), r.stdout + r.stderr
