"""The clustering kernels of ``--trf-clusters`` on the CPU: ``csrc/kernels_trf.hpp`` itself compiled for the host
(tests/hostsim/trf_cluster_sim.cpp: a workgroup's threads behind a barrier, the tile list and the host steps of csrc/native_trf.hpp)
against the reference's clustering restated in NumPy (tests/test_trf_clusters.py: ``restate``).  Every returned array is compared
exactly, ``rho`` as float32 bits: the Gaussian values are the host's and the sum is ordered, so there is no tolerance to choose.
``synth_groups`` is shared with the GPU test (tests/test_trf_clusters_gpu.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_trf_hostsim import _flat
from test_trf_clusters import restate

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostsim", "trf_cluster_sim.cpp")
SO = os.path.join(HERE, "hostsim", "_build", "libtrfclustersim.so")
CSRC = os.path.join(HERE, "..", "mirge3.0_amd", "csrc")
KEYS = ("rho", "delta", "nneigh", "order", "cl", "halo", "centre", "nclust")
# (columns of the template, points): 130 columns = five 32-column words, boundaries at 32, 64 and 96; a group of one between two large
# ones; 65 = past a wave, 300 = past a workgroup (256) and an LDS tile (128); 90 columns takes the four-word kernels, 256 is the cap
SHAPES = [(130, 300), (130, 1), (130, 65), (130, 2), (130, 3), (90, 70), (256, 40), (130, 129)]


def gauss(n):
    import math
    return np.asarray([math.exp(-(float(d) / 3.0) ** 2) for d in range(n)], dtype=np.float64)


def synth_groups(seed=17, shapes=SHAPES):
    """-> (reads, groups): groups = [dict(tlen, read = indices into reads, off, rp, dashed)].  Reads of 16 .. min(130, tlen) nt (to 200 on
    the 256-column template), most of them fragments that start and end around a few places of the template (contained in, partly
    over and beside one another) with a substitution or an N here and there, the rest anywhere; RP100K log-uniform over 0.001 .. 5000"""
    rng = np.random.default_rng(seed)
    reads, index, groups = [], {}, []
    for tlen, n in shapes:
        t = "".join("ACGT"[x] for x in rng.integers(0, 4, tlen))
        max_len = 200 if tlen > 130 else min(130, tlen)
        spots = [(0, 31), (0, 33), (30, 64), (33, 97), (60, tlen), (0, tlen), (tlen - 40, tlen)]
        g = dict(tlen=tlen, read=[], off=[], rp=[], dashed=[])
        seen = set()
        while len(g["read"]) < n:
            if rng.integers(0, 4):
                s0, e0 = spots[int(rng.integers(0, len(spots)))]
                s, e = s0 + int(rng.integers(-3, 4)), e0 + int(rng.integers(-3, 4))
            else:
                s = int(rng.integers(0, tlen - 16))
                e = s + int(rng.integers(16, max_len + 1))
            s, e = max(s, 0), min(e, tlen)
            if e - s < 16 or e - s > max_len:
                continue
            rd = list(t[s:e])
            for _ in range(int(rng.integers(0, 3))):
                p = int(rng.integers(0, len(rd)))
                rd[p] = "ACGTN"[int(rng.integers(0, 5))]
            rd = "".join(rd)
            if (rd, s) in seen:
                continue
            seen.add((rd, s))
            if rd not in index:
                index[rd] = len(reads)
                reads.append(rd)
            g["read"].append(index[rd]); g["off"].append(s)
            g["rp"].append(max(0.001, round(float(10 ** rng.uniform(-3, 3.7)), 3)))
            g["dashed"].append("-" * s + rd + "-" * (tlen - e))
        groups.append(g)
    return reads, groups


def flat_groups(groups):
    ptr = np.zeros(len(groups) + 1, np.int64)
    np.cumsum([len(g["read"]) for g in groups], out=ptr[1:])
    cat = lambda k, dt: np.asarray([x for g in groups for x in g[k]], dtype=dt)
    return ptr, cat("read", np.int64), cat("off", np.int32), cat("rp", np.float64), np.asarray([g["tlen"] for g in groups], np.int32)


@pytest.fixture(scope="module")
def want():
    """the restatement of every group, computed once and shared"""
    reads, groups = synth_groups()
    parts = [restate(g["dashed"], g["rp"]) for g in groups]
    return reads, groups, {k: np.concatenate([p[k] for p in parts]) for k in KEYS}


def check_case(want):
    reads, groups, w = want
    assert any("N" in r for r in reads) and {len(r) > 64 for r in reads} == {True, False} and max(len(r) for r in reads) > 130
    assert (w["rho"] < 5).any() and (w["rho"] >= 5).any() and (w["nclust"] >= 2).any() and (w["nclust"][[1, 3, 4]] <= 1).all()
    assert ((w["halo"] == 0) & (w["cl"] > 0)).any() and (w["halo"] > 0).any()
    for g in groups[:1]:  # partial overlap, no overlap and containment among the first group's pairs
        iv = [(o, o + len(reads[r])) for r, o in zip(g["read"], g["off"])]
        assert any(a[1] <= b[0] for a in iv for b in iv) and any(a[0] < b[0] < a[1] < b[1] for a in iv for b in iv)
        assert any(a[0] <= b[0] and b[1] <= a[1] and a != b for a in iv for b in iv)


def assert_equal(got, w):
    for k in KEYS:
        a, b = np.asarray(got[k]), w[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, (k, bad[:5], a[bad[:5]], b[bad[:5]])


@pytest.fixture(scope="module")
def sim():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("kernels_trf.hpp", "mirge_core.hpp")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-pthread", "-o", SO, SRC])
    return C.CDLL(SO)


def run_sim(sim, reads, groups, n_gauss=None):
    rd, roff = _flat(reads)
    ptr, read, off, rp, tlen = flat_groups(groups)
    g = gauss(n_gauss if n_gauss is not None else 2 * int(tlen.max()) + 1)
    n = int(ptr[-1])
    out = dict(rho=np.zeros(n, np.float32), delta=np.zeros(n, np.float32), nclust=np.zeros(len(groups), np.int32))
    for k in ("nneigh", "order", "cl", "halo", "centre"):
        out[k] = np.full(n, -7, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = sim.sim_trf_cluster(p(rd), p(roff), C.c_int64(len(reads)), C.c_int64(len(groups)), p(ptr), p(read), p(off), p(rp), p(tlen),
                             C.c_int64(g.shape[0]), p(g), *(p(out[k]) for k in ("rho", "delta", "nneigh", "order", "cl", "halo", "nclust", "centre")))
    return rc, out


def test_case_holds_what_it_is_for(want):
    check_case(want)


def test_arrays_equal_the_restatement(sim, want):
    reads, groups, w = want
    rc, got = run_sim(sim, reads, groups)
    assert rc == 0
    assert_equal(got, w)


def test_a_point_beyond_its_template_is_refused(sim):
    reads = ["ACGTACGTACGTACGTACGT"]
    rc, _ = run_sim(sim, reads, [dict(tlen=30, read=[0], off=[11], rp=[1.0])], n_gauss=61)
    assert rc == -102
