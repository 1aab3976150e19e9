"""k_part_dedup as a persistent, software-pipelined kernel: a workgroup walks buckets w, w + grid, ... with the next bucket's
records and the bucket after's share words in flight, holds the read-outs of MIRGE_DEDUP_K buckets in registers and reserves their
output range with one add.  The shapes are the smallest at which that can go wrong -- one radix level (the plain chain inside the
same loop), two levels with 128 and 256 buckets (four shares per bucket: the pipeline) -- each with the grid capped at one
workgroup (every pipeline stage and a tail that is no multiple of K), at three, at B - 1 (workgroups of one and of two buckets)
and uncapped, with the one output cursor and with the eight sharded ones, on uniform and Zipf duplicates and on 40 templates only
(most buckets empty, empty buckets between full ones in a workgroup's sequence, groups whose total is 0).  The hooks are read once
per process, so every case is a fresh process; the expectation is numpy's dictionary, sequence -> (count, first index), built as
in test_partitioned_collapse_sizes_and_skew."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

WORKER = """
import sys, numpy as np
sys.path.insert(0, %r)
import mirge3_amd
from mirge3_amd import _ffi
from mirge3_amd.seqio import FlatSeqs

def sample(n, kind, distinct):
    rng = np.random.default_rng(n %% 1000 + len(kind))
    n_tmpl = n if distinct else max(n // 3, 1000)
    lens = rng.integers(16, 32, size=n_tmpl)
    off = np.zeros(n_tmpl + 1, np.int64); np.cumsum(lens, out=off[1:])
    tmpl = FlatSeqs(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=int(off[-1]))], off)
    if kind == "uniform":
        idx = rng.integers(0, n_tmpl, size=n)
    elif kind == "zipf":
        idx = np.minimum(rng.zipf(1.2, size=n) - 1, n_tmpl - 1)
    else:  # forty templates: at most 40 of the 64..256 buckets hold anything
        idx = rng.integers(0, 40, size=n)
    return tmpl, idx

def check(ctx, n, kind, distinct=False):
    tmpl, idx = sample(n, kind, distinct)
    raw = _ffi.DeviceReads.pack(ctx, tmpl.take(idx))
    u = raw.collapse()
    cnt, first = u.counts()
    got_seqs = u.unpack().to_list()
    tl = tmpl.to_list()
    canon = {}
    key_of = np.empty(len(tl), np.int64)
    for t, sq in enumerate(tl):  # templates may coincide by chance: the expectation goes through the sequences
        key_of[t] = canon.setdefault(sq, t)
    uk, ufirst, ucnt = np.unique(key_of[idx], return_index=True, return_counts=True)
    want = {tl[k]: (int(c), int(f)) for k, f, c in zip(uk, ufirst, ucnt)}
    got = {sq: (int(c), int(f)) for sq, c, f in zip(got_seqs, cnt[:, 0], first)}
    assert len(got_seqs) == len(want) and got == want, (n, kind, len(got_seqs), len(want))
    u.close(); raw.close()

ctx = _ffi.Context(0)
ctx.profile(True); ctx.profile_reset()
distinct = sys.argv[3] == "distinct"
for n in map(int, sys.argv[1].split(",")):
    for kind in sys.argv[2].split(","):
        check(ctx, n, kind, distinct)
ctx.sync()
names = sorted(set(nm for nm, l, ms, un in ctx.profile_records() if l))
print("OK", " ".join(names))
""" % ROOT


def run_worker(shapes, kinds, env, distinct=False):
    clean = {k: v for k, v in os.environ.items()
             if k not in ("MIRGE_DEDUP_GRID", "MIRGE_DEDUP_SHARDED", "MIRGE_TEST_SMALL_PART", "MIRGE_PART_NB1")}
    r = subprocess.run([sys.executable, "-c", WORKER, ",".join(map(str, shapes)), ",".join(kinds), "distinct" if distinct else "dup"],
                       env=dict(clean, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
    return r.stdout.split("OK", 1)[1].split()


# n -> B, the final buckets (collapse_phase_a: the first power of two from 64 with B * 2048 >= n)
SHAPES = {65536: 64, 131073: 128, 300001: 256}
KINDS = ("uniform", "zipf", "forty")


@pytest.mark.parametrize("sharded", ["0", "1"])
@pytest.mark.parametrize("grid", ["1", "3", None])
def test_pipelined_dedup_under_a_capped_grid(grid, sharded):
    """One workgroup walks every bucket (all pipeline stages, the K-grouping and its tail), three workgroups, and the grid as the
    launcher sizes it: one level with R = G = 32 regions (n = 65 536), two levels with B = 128 and 256 and four shares."""
    env = {"MIRGE_DEDUP_SHARDED": sharded}
    if grid:
        env["MIRGE_DEDUP_GRID"] = grid
    names = run_worker(list(SHAPES), KINDS, env)
    assert "k_part_dedup.w1" in names and "k_part_split.w1" in names
    assert ("k_part_compact.w1" in names) == (sharded == "1")
    assert not any(nm.startswith("k_collapse_insert_key") for nm in names)  # no call fell back to the global-atomic table


@pytest.mark.parametrize("sharded", ["0", "1"])
@pytest.mark.parametrize("n", list(SHAPES))
def test_pipelined_dedup_with_one_bucket_short_of_a_full_grid(n, sharded):
    """Grid B - 1: workgroup 0 has two buckets, every other one a single bucket."""
    names = run_worker([n], KINDS, {"MIRGE_DEDUP_SHARDED": sharded, "MIRGE_DEDUP_GRID": str(SHAPES[n] - 1)})
    assert "k_part_dedup.w1" in names and not any(nm.startswith("k_collapse_insert_key") for nm in names)


@pytest.mark.parametrize("grid", ["3", None])
def test_pipelined_dedup_beyond_the_prefetch_depth(grid):
    """Buckets with more records than are asked for one bucket ahead (depth x threads = 1 024): 200 000 and 250 000 reads, every
    template its own sequence, in 128 buckets of ~1 560 and ~1 950 records -- the 2048-slot and the 4096-slot instance."""
    names = run_worker([200000, 250000], ["uniform"], {"MIRGE_DEDUP_GRID": grid} if grid else {}, distinct=True)
    assert "k_part_dedup.w1" in names and not any(nm.startswith("k_collapse_insert_key") for nm in names)


def test_plain_chain_over_two_level_shares_under_a_capped_grid():
    """MIRGE_PART_NB1=16 at 131 072 reads: 64 buckets in two levels with sixteen shares each -- more than four, so the plain
    chain, with share offsets, 2 048 records per bucket in the 4096-slot table, three workgroups."""
    names = run_worker([131072], ["uniform", "forty"], {"MIRGE_PART_NB1": "16", "MIRGE_DEDUP_GRID": "3"})
    assert "k_part_dedup.w1" in names and "k_part_split.w1" in names


def test_overflowing_tables_still_fall_back_under_a_capped_grid():
    """MIRGE_TEST_SMALL_PART=1 keeps 64 buckets at 2 500 000 reads: every table overflows, the flag must fire from a workgroup
    that goes on to its next bucket, and the call must be redone with the global-atomic table."""
    names = run_worker([2500000], ["uniform"], {"MIRGE_TEST_SMALL_PART": "1", "MIRGE_DEDUP_GRID": "3"})
    assert "k_part_dedup.w1" in names and any(nm.startswith("k_collapse_insert_key") for nm in names)
