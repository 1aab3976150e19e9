#!/usr/bin/env python3
"""Time ``mirge_genome_align_loci`` beside ``mirge_genome_align_counts`` at genome scale: the synthetic genome of
tools/genome_filter_time.py, per query count the two calls interleaved (counts, loci, counts, loci, ...), medians and spread, and the
loci call's kernels from the context's event profiler in one more call (count pass, fill pass, the rest = sorts, index, copies).

  python tools/genome_loci_time.py --bases 3100000000 --queries 100000,1000000 --repeats 5 --out profiles/genome_loci_run.md
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import genome_filter_time as gft  # noqa: E402
import mirge3_amd  # noqa: E402,F401
from mirge3_amd import _ffi, ebwt  # noqa: E402
from mirge3_amd.seqio import FlatSeqs  # noqa: E402


def draw_queries(packed, n, rng):
    """genome_filter_time.draw_queries without its per-query loop (10^6 queries)"""
    L = rng.integers(18, 26, n)
    pos = rng.integers(0, packed.shape[0] * 4 - 30, n)
    i = pos[:, None] + np.arange(25)
    codes = (packed[i >> 2] >> (2 * (i & 3))) & 3
    codes[rng.random(n) < 0.01] = codes[0]
    for _ in range(2):
        hit = rng.random(n) < 0.5
        p = rng.integers(0, L)
        codes[hit, p[hit]] = (codes[hit, p[hit]] + 1) % 4
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
    return [letters[k, :L[k]].tobytes().decode() for k in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=3_100_000_000)
    ap.add_argument("--refs", type=int, default=25)
    ap.add_argument("--queries", default="100000,1000000")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n-mm", dest="n_mm", type=int, default=0)
    ap.add_argument("--seedlen", type=int, default=25)
    ap.add_argument("--max-loci", dest="max_loci", type=int, default=3)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    packed, off, ln, first = gft.synth_packed(a.bases, a.refs, a.seed)
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        base = gft.write_index(d, packed, off, ln, first)
        rng = np.random.default_rng(a.seed + 1)
        qsets = {int(n): FlatSeqs.from_list(draw_queries(packed, int(n), rng)) for n in a.queries.split(",")}
        del packed
        ctx = _ffi.Context(0)
        pk, o, l_, f = ebwt.read_records(base)
        g = _ffi.DeviceGenome(ctx, packed=pk, records=(o, l_, f))
        del pk
        say(f"synthetic genome: {a.bases} bases, {off.shape[0]} stretches over {a.refs} references; -n {a.n_mm} -l {a.seedlen} "
            f"-m {a.max_loci}, both strands; {a.repeats} interleaved repeats")
        say("")
        say("| queries | counts call s (median, min..max) | loci call s (median, min..max) | loci / counts | records | capped queries | "
            "count pass ms | fill pass ms | index kernels ms | rest of the loci call ms |")
        say("|---|---|---|---|---|---|---|---|---|---|")
        for n, qs in qsets.items():
            g.align_loci(qs, a.n_mm, a.seedlen, 2, 0, 0, a.max_loci)  # code objects loaded, pool warm at this size
            g.align_counts(qs, a.n_mm, a.seedlen, 2, 0, 0)
            tc, tl = [], []
            for _ in range(a.repeats):
                t = time.perf_counter()
                g.align_counts(qs, a.n_mm, a.seedlen, 2, 0, 0)
                tc.append(time.perf_counter() - t)
                t = time.perf_counter()
                loci = g.align_loci(qs, a.n_mm, a.seedlen, 2, 0, 0, a.max_loci)
                tl.append(time.perf_counter() - t)
            ctx.profile(True)
            ctx.profile_reset()
            t = time.perf_counter()
            g.align_loci(qs, a.n_mm, a.seedlen, 2, 0, 0, a.max_loci)
            t_prof = time.perf_counter() - t
            r = {nm: ms for nm, _, ms, _ in ctx.profile_records()}
            ctx.profile(False)
            idx = r.get("k_genome_queries", 0) + r.get("k_genome_index", 0)
            rest = t_prof * 1000 - r.get("k_genome_scan", 0) - r.get("k_genome_scan_fill", 0) - idx
            mc, ml = float(np.median(tc)), float(np.median(tl))
            say(f"| {n} | {mc:.3f} ({min(tc):.3f}..{max(tc):.3f}) | {ml:.3f} ({min(tl):.3f}..{max(tl):.3f}) | {ml / mc:.2f} | "
                f"{loci['query'].shape[0]} | {int((loci['totals'] > a.max_loci).sum()) if a.max_loci else 0} | {r.get('k_genome_scan', 0):.1f} | "
                f"{r.get('k_genome_scan_fill', 0):.1f} | {idx:.2f} | {rest:.1f} |")
        g.close()
        ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
