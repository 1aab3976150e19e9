"""Probe plans that know the longest window a library can hold (native_cascade.hpp, plan_max_window; mirge_core.hpp,
mirge_plan_table_fill): a read trimmed to more than the library's longest run of valid bases gets no probe, and a wave without a
probe leaves align_hybrid at once.  Nothing a read is annotated with may change.

Per read against ``oracle.cascade`` on the same reads, through every route that reads the plan -- k_cascade_bulk (the bulk
group), k_cascade_fused (a 2-word group beyond MIRGE_SPEC_MAX reads), k_cascade_spec (the groups of reads with an N), and, in a
fresh process with the hooks of tests/test_gpu_parity.py::test_staged_cascade_for_every_group, one k_pass launch per pass -- and
with MIRGE_PLAN_REFLEN=0 against =1: identical annotation, walks and survivor counts."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from helpers import oracle_libs_from
import mirge3_amd  # noqa: F401
from mirge3_amd import _ffi, synth
from mirge3_amd.cascade import Cascade, ISO_PASS
from mirge3_amd.seqio import FlatSeqs, Library

pytestmark = pytest.mark.gpu

STAGED = os.environ.get("MIRGE_BULK_FUSED") == "0"  # the fresh process of test_staged_route_in_a_fresh_process


def _rand(rng, L):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=L))


def _random_reads(rng, n, lo, hi):
    lens = rng.integers(lo, hi + 1, size=n)
    return ["".join(map(chr, row[:L])) for row, L in zip(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n, hi))], lens)]


def _mutate(rng, s, q):
    return s[:q] + "ACGT"[("ACGT".index(s[q]) + int(rng.integers(1, 4))) % 4] + s[q + 1:]


def _world():
    """Tiny libraries (miRNAs of 18-25 nt, M = 25) and the distinct reads of the sample, by kind"""
    rng = np.random.default_rng(909)
    sl = synth.make_libraries(seed=44, scale="tiny")
    mir = sl.libs["mirna"]
    seqs = mir.seqs.to_list() + [_rand(rng, 25) for _ in range(4)] + [_rand(rng, 24) for _ in range(2)]
    libs = dict(sl.libs)
    libs["mirna"] = Library(list(mir.names) + [f"crafted-{i}" for i in range(6)], FlatSeqs.from_list(seqs))
    M = max(len(s) for s in seqs)
    assert M == 25 and min(len(s) for s in seqs) >= 18
    longest = [s for s in seqs if len(s) == M]
    flank = lambda body: _rand(rng, 1) + body + _rand(rng, 2)  # the isomiR pass trims one base in front and two behind
    edge = []
    for s in longest:
        edge += [flank(s) for _ in range(3)]                        # trimmed length M: IS a longest reference
        edge += [flank(_mutate(rng, s, 7)), flank(_mutate(rng, _mutate(rng, s, 3), 19))]  # ... with one and two substitutions
        edge += [flank(s[:M - 1]), flank(s[1:]), flank(_mutate(rng, s[1:], 11))]          # trimmed length M - 1
        edge += [flank(s + _rand(rng, 1)), flank(_rand(rng, 1) + s), flank(s + _rand(rng, 3))]  # M + 1, M + 1, M + 3: no window
        edge += [s, s[:20], s[2:]]                                  # untrimmed: the exact pass
    # reads of 16-50 nt out of every library, some with a substitution: one-word and two-word groups
    cut = []
    for key in ("mirna", "hairpin", "mature_trna", "pre_trna", "snorna", "rrna", "ncrna_others", "mrna"):
        lib = libs[key].seqs.to_list()
        for k in range(260):
            s = lib[int(rng.integers(0, len(lib)))]
            L = int(rng.integers(16, 51))
            a = int(rng.integers(0, max(1, len(s) - L + 1)))
            r = s[a:a + L]
            if len(r) < 16 or "N" in r:
                continue
            if k % 3 == 0:
                r = _mutate(rng, r, int(rng.integers(0, len(r))))
            if key == "pre_trna" and k % 2:
                r = r[:45] + "TTTT"
            cut.append(r)
    cut += [s for s in synth.make_reads(sl, 4000, seed=6).to_list() if "N" not in s and 16 <= len(s) <= 50]
    with_n = [s[:q] + "N" + s[q + 1:] for s in edge + cut[::3] for q in (int(rng.integers(0, len(s))),)]
    filler = _random_reads(rng, 70000, 18, 31) + _random_reads(rng, 34000, 32, 50)
    reads = list(dict.fromkeys(edge + cut + with_n + filler))
    return dict(sl=sl, libs=libs, M=M, longest=longest, edge=edge, reads=reads)


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world():
    w = _world()
    fs = FlatSeqs.from_list(w["reads"])
    o = oracle.cascade(fs.data, fs.offsets, oracle_libs_from(w["libs"]), n_pass=9, indexed=True)
    w["want"] = {s: tuple(int(a[i]) for a in o) for i, s in enumerate(w["reads"])}
    w["flat"] = fs
    return w


def _run(ctx, world, reflen):
    """The sample through a cascade over NEW libraries (plans are kept per library) with MIRGE_PLAN_REFLEN set as asked ->
    {read: annotation}, launches by kernel, walks, survivor units of the bulk launch"""
    old = os.environ.get("MIRGE_PLAN_REFLEN")
    os.environ["MIRGE_PLAN_REFLEN"] = "1" if reflen else "0"
    try:
        casc = Cascade(ctx, world["libs"])
        raw = _ffi.DeviceReads.pack(ctx, world["flat"])
        ctx.profile(True)
        ctx.profile_reset()
        uq, res = casc.collapse_and_run(raw)
        f = res.fetch()
        recs = {name: (l, u) for name, l, _, u in ctx.profile_records() if l}
        ctx.profile(False)
        walks = _ffi.cascade_walks(ctx)
        useq = uq.unpack().to_list()
        groups = uq.group_counts()
        got = dict(zip(useq, zip(*(a.tolist() for a in f))))
        res.close(); uq.close(); raw.close(); casc.close()
    finally:
        ctx.profile(False)
        if old is None:
            os.environ.pop("MIRGE_PLAN_REFLEN")
        else:
            os.environ["MIRGE_PLAN_REFLEN"] = old
    return dict(got=got, recs=recs, walks=walks, groups=groups)


@pytest.fixture(scope="module")
def runs(ctx, world):
    return {reflen: _run(ctx, world, reflen) for reflen in (True, False)}


def _launched(recs, prefix):
    return sum(l for name, (l, _) in recs.items() if name.startswith(prefix))


def test_annotation_is_the_oracles(world, runs):
    r = runs[True]
    want = world["want"]
    assert len(r["got"]) == len(want)
    bad = [(s, g, want[s]) for s, g in r["got"].items() if g != want[s]]
    assert not bad, (len(bad), bad[:5])
    # the routes: a bulk group of >= 65 536 one-word reads, a 2-word group beyond 32 768, two groups with an N far below
    g = np.sort(r["groups"][r["groups"] > 0])
    assert len(g) == 4 and g[-1] >= 65536 and 32768 < g[-2] < g[-1] and g[1] < 32768, r["groups"]
    if STAGED:
        assert _launched(r["recs"], "k_pass[") >= 4 * 5 and not _launched(r["recs"], "k_cascade_"), r["recs"]
    else:
        for k in ("k_cascade_bulk", "k_cascade_fused", "k_cascade_spec"):
            assert _launched(r["recs"], k) >= 1, (k, sorted(r["recs"]))
        assert _launched(r["recs"], "k_cascade_spec") == 2 and not _launched(r["recs"], "k_pass["), sorted(r["recs"])
    # trimmed length M is still found, M + 1 never: by the isomiR pass, at offset 0 of a longest reference
    M, longest = world["M"], set(world["longest"])
    hits_M = [s for s in world["edge"] if len(s) == M + 3 and s[1:-2] in longest]
    assert len(hits_M) >= 12
    by_iso = [s for s in hits_M if want[s][0] == ISO_PASS and want[s][2] == 0 and want[s][3] == 0]
    assert len(by_iso) >= len(hits_M) // 2, (len(by_iso), len(hits_M))
    assert any(want[s][0] == ISO_PASS and want[s][3] == 2 for s in world["edge"] if len(s) == M + 3)
    assert any(want[s][0] == ISO_PASS for s in world["edge"] if len(s) == M + 2)
    assert not any(v[0] == ISO_PASS for s, v in want.items() if len(s) > M + 3)
    # reads with an N and reads of the 2-word group are annotated too
    assert sum(1 for s, v in want.items() if "N" in s and v[0] >= 0) >= 50
    assert sum(1 for s, v in want.items() if len(s) >= 32 and v[0] >= 0) >= 200


def test_switch_changes_no_annotation_walk_or_survivor_count(runs):
    on, off = runs[True], runs[False]
    assert on["got"] == off["got"]
    assert on["walks"] == off["walks"] and on["walks"][2] >= 5
    assert np.array_equal(on["groups"], off["groups"])
    assert {k: v[0] for k, v in on["recs"].items()} == {k: v[0] for k, v in off["recs"].items()}  # the same launches
    # reads handed to every pass (the survivors of the pass before), summed by the profiler per cascade launch
    casc = [k for k in on["recs"] if k.startswith("k_cascade_bulk") or k.startswith("k_pass[")]
    assert casc
    for k in casc:
        assert on["recs"][k][1] == off["recs"][k][1], (k, on["recs"][k], off["recs"][k])
    assert sum(on["recs"][k][1] for k in casc) > len(on["got"])  # more than one pass saw reads


if not STAGED:  # (the fresh process runs the two tests above and nothing else)
    def test_staged_route_in_a_fresh_process():
        """One k_pass launch per pass for every group (MIRGE_FUSED_MAX=0, MIRGE_BULK_FUSED=0: read once per process)"""
        root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k", "oracles or switch_changes"],
                           env=dict(os.environ, MIRGE_FUSED_MAX="0", MIRGE_BULK_FUSED="0"), capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0 and "2 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
