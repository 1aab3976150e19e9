#!/usr/bin/env python3
"""Time the A-to-I report's genome filter on the device (``mirge_genome_align_counts``) at genome scale.

Builds a synthetic genome straight in bowtie's packed form -- ``.4.ebwt`` (2 bits per base) and ``.3.ebwt`` records with N
stretches between the stretches of bases, over several references -- with planted repeat families, writes it to a directory,
reads it once to warm the page cache, then per query count (miRNA-like reads drawn from the genome, 0..2 changes, 1 % copies
of one read) times:

  load    ebwt.read_records (the two files from the page cache, no base decoded)
  upload  _ffi.DeviceGenome (stretch table on the host, the stream to HBM)
  scan    the two runs of the filter: -n 1 (unique_best) and -n 0 (aligned), each one call = index build + scan + read-back
  kernels k_genome_queries / k_genome_index / k_genome_scan device times (the context's event profiler)

  python tools/genome_filter_time.py --bases 3100000000 --queries 1000,10000,100000 --out profiles/genome_filter_3g.md
"""
import argparse
import os
import struct
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import mirge3_amd  # noqa: E402,F401
from mirge3_amd import _ffi, ebwt  # noqa: E402
from mirge3_amd.a2i import GpuGenome  # noqa: E402


def synth_packed(n_bases, n_refs, seed):
    """-> packed bytes, records (off, len, first): random bases, N stretches of 1..50 000 between stretches, repeat families"""
    rng = np.random.default_rng(seed)
    packed = rng.integers(0, 256, (n_bases + 3) // 4, dtype=np.uint8)
    # repeat families: 300-byte (1 200-nt) and 75-byte (300-nt) units copied at byte boundaries, one byte changed per copy
    for unit, copies in ((300, 40000), (75, 400000)):
        fam = rng.integers(0, 256, unit, dtype=np.uint8)
        at = rng.integers(0, packed.shape[0] - unit, copies)
        idx = (at[:, None] + np.arange(unit)).ravel()
        packed[idx] = np.tile(fam, copies)
        packed[at + rng.integers(0, unit, copies)] = rng.integers(0, 256, copies, dtype=np.uint8)
    # records: every reference cut into stretches by N runs
    per_ref = 40
    cuts = np.unique(rng.integers(1, n_bases, n_refs * per_ref - 1))
    n_rec = cuts.shape[0] + 1
    ln = np.diff(np.concatenate([[0], cuts, [n_bases]])).astype(np.int64)
    off = rng.integers(1, 50000, n_rec).astype(np.int64)
    first = np.zeros(n_rec, dtype=bool)
    first[::per_ref] = True
    off[first] = 0
    return packed, off, ln, first


def write_index(d, packed, off, ln, first):
    base = os.path.join(d, "synth_genome")
    with open(base + ".3.ebwt", "wb") as fh:
        fh.write(struct.pack("<iI", 1, off.shape[0]))
        rec = np.zeros(off.shape[0], dtype=[("o", "<u4"), ("l", "<u4"), ("f", "u1")])
        rec["o"], rec["l"], rec["f"] = off, ln, first
        fh.write(rec.tobytes())
    packed.tofile(base + ".4.ebwt")
    open(base + ".1.ebwt", "wb").close()  # (names are not read on this path: the file only marks the index as present)
    return base


def draw_queries(packed, n, rng):
    total = packed.shape[0] * 4
    L = rng.integers(18, 26, n)
    pos = rng.integers(0, total - 30, n)
    i = pos[:, None] + np.arange(25)
    codes = (packed[i >> 2] >> (2 * (i & 3))) & 3
    rep = rng.random(n) < 0.01  # duplicates of one read
    codes[rep] = codes[0]
    for k in range(n):
        for _ in range(int(rng.integers(0, 3))):
            p = int(rng.integers(0, L[k]))
            codes[k, p] = (codes[k, p] + 1) % 4
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
    return [letters[k, :L[k]].tobytes().decode() for k in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=3_100_000_000)
    ap.add_argument("--refs", type=int, default=25)
    ap.add_argument("--queries", default="1000,10000,100000")
    ap.add_argument("--dir", default=None, help="where the index files go (default: a temporary directory)")
    ap.add_argument("--out", default=None, help="write the table (markdown) here as well")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    t = time.perf_counter()
    packed, off, ln, first = synth_packed(a.bases, a.refs, a.seed)
    t_synth = time.perf_counter() - t
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        base = write_index(d, packed, off, ln, first)
        rng = np.random.default_rng(a.seed + 1)
        qsets = {int(n): draw_queries(packed, int(n), rng) for n in a.queries.split(",")}
        del packed
        ebwt.read_records(base)  # page cache warm
        ctx = _ffi.Context(0)
        say(f"synthetic genome: {a.bases} bases, {off.shape[0]} stretches over {a.refs} references, "
            f"{int(off.sum())} N (made in {t_synth:.1f} s)")
        say("")
        say("| queries | load s | upload s | -n 1 call s | -n 0 call s | filter end to end s | k_genome_scan ms (-n 1 / -n 0) | index kernels ms | hits -n 1 |")
        say("|---|---|---|---|---|---|---|---|---|")
        for n, qs in qsets.items():
            t = time.perf_counter()
            pk, o, l_, f = ebwt.read_records(base)
            t_load = time.perf_counter() - t
            t = time.perf_counter()
            g = _ffi.DeviceGenome(ctx, packed=pk, records=(o, l_, f))
            ctx.sync()
            t_up = time.perf_counter() - t
            del pk
            gg = GpuGenome(ctx, g)
            gg.unique_best(qs[:64])  # code objects loaded, pool warm
            ctx.profile(True)
            ctx.profile_reset()
            t = time.perf_counter()
            _, c1, _ = gg.counts(qs, 1)
            t1 = time.perf_counter() - t
            r1 = {nm: ms for nm, _, ms, _ in ctx.profile_records()}
            ctx.profile_reset()
            t = time.perf_counter()
            gg.counts(qs, 0)
            t0 = time.perf_counter() - t
            r0 = {nm: ms for nm, _, ms, _ in ctx.profile_records()}
            ctx.profile(False)
            idx_ms = sum(r1.get(k, 0) + r0.get(k, 0) for k in ("k_genome_queries", "k_genome_index"))
            say(f"| {n} | {t_load:.3f} | {t_up:.3f} | {t1:.3f} | {t0:.3f} | {t_load + t_up + t1 + t0:.3f} | "
                f"{r1.get('k_genome_scan', 0):.1f} / {r0.get('k_genome_scan', 0):.1f} | {idx_ms:.2f} | {int(c1.astype(np.int64).sum())} |")
            g.close()
        ctx.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
