#!/usr/bin/env python3
"""Time the device half of ``--unmapped-align`` and the text around it on synthetic clusters: random references of 20 to 30 nt
(one per cluster) and reads of 16 to 25 nt cut from them (60 % exact, 25 % with one or two changes, 15 % random).  Per size:
the cluster genome's build, run 1 (-n 0 -l 25 --norc -m 3), run 2 (-n 1 -l 15 -5 1 -3 3 --norc) on the reads run 1 left, with
and without ``strata`` -- the two interleaved (plain, strata, plain, strata, ...), medians and spread -- and the host text
(the two SAMs, combine, decorate, select, sort).  The plain call is the code ``mirge_genome_align_loci`` ran before ``strata``
existed, so strata / plain is the one ratio with a yardstick.

  python tools/unmapped_align_time.py --sizes 10000x100000,100000x1000000 --repeats 5 --out profiles/unmapped_align_run.md
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import mirge3_amd  # noqa: E402,F401
from mirge3_amd import _ffi, a2i, unmapped_align as ua  # noqa: E402
from mirge3_amd.seqio import FlatSeqs  # noqa: E402

LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


def synth(n_refs, n_reads, rng):
    rl = rng.integers(20, 31, n_refs)
    codes = rng.integers(0, 4, (n_refs, 30)).astype(np.uint8)
    refs = [LETTERS[codes[k, :rl[k]]].tobytes().decode() for k in range(n_refs)]
    pick = rng.integers(0, n_refs, n_reads)
    L = np.minimum(rng.integers(16, 26, n_reads), rl[pick])
    start = (rng.random(n_reads) * (rl[pick] - L + 1)).astype(np.int64)
    rc = codes[pick[:, None], np.minimum(start[:, None] + np.arange(25), 29)]
    kind = rng.random(n_reads)
    for lo in (0.60, 0.72):  # one change above 0.60, a second above 0.72
        hit = (kind >= lo) & (kind < 0.85)
        p = (rng.random(n_reads) * L).astype(np.int64)
        rc[hit, p[hit]] = (rc[hit, p[hit]] + 1) % 4
    rnd = kind >= 0.85
    rc[rnd] = rng.integers(0, 4, (int(rnd.sum()), 25))
    letters = LETTERS[rc]
    return refs, [letters[k, :L[k]].tobytes().decode() for k in range(n_reads)]


def spread(t):
    return f"{float(np.median(t)):.3f} ({min(t):.3f}..{max(t):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000x100000,100000x1000000", help="clusters x reads, comma separated")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--text-repeats", dest="text_repeats", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = _ffi.Context(0)
    say(f"synthetic clusters of 20..30 nt, reads of 16..25 nt; {a.repeats} interleaved repeats; seconds as median (min..max)")
    say("")
    say("| clusters | reads | genome build | run 1 | run 1 records / over -m | reads to run 2 | run 2 plain | run 2 strata | strata / plain | "
        "run 2 records plain / strata | count pass ms plain / strata | fill pass ms plain / strata | host text |")
    say("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for size in a.sizes.split(","):
        n_refs, n_reads = (int(x) for x in size.split("x"))
        refs, reads = synth(n_refs, n_reads, np.random.default_rng(a.seed))
        names = [f"mir{k + 1}_{2 + k % 7}" for k in range(n_reads)]
        c_names = [f"S:miRCluster_{k + 1}_{len(r)}:chr1:{1 + 100 * k}_{100 * k + len(r)}+" for k, r in enumerate(refs)]
        flat_refs, flat = FlatSeqs.from_list(refs), FlatSeqs.from_list(reads)
        tb = []
        for _ in range(a.repeats):
            t = time.perf_counter()
            dev = _ffi.DeviceGenome(ctx, seqs=flat_refs)
            tb.append(time.perf_counter() - t)
            dev.close()
        dev = _ffi.DeviceGenome(ctx, seqs=flat_refs)
        g = a2i.GpuGenome(ctx, dev)
        run1 = lambda: g.loci(flat, n_mm=0, seedlen=25, maxtotal=2, max_loci=3, norc=True)
        l1 = run1()
        t1 = []
        for _ in range(a.repeats):
            t = time.perf_counter()
            l1 = run1()
            t1.append(time.perf_counter() - t)
        l1["capped"] = l1["totals"] > 3
        hit = np.zeros(n_reads, dtype=bool)
        hit[l1["query"]] = True
        i_names, i_seqs = [names[k] for k in np.nonzero(~hit)[0]], [reads[k] for k in np.nonzero(~hit)[0]]
        flat2 = FlatSeqs.from_list(i_seqs)
        run2 = lambda strata: g.loci(flat2, maxtotal=2, norc=True, strata=strata, **ua.RUN2)
        run2(False), run2(True)
        tp, ts = [], []
        for _ in range(a.repeats):
            t = time.perf_counter()
            lp = run2(False)
            tp.append(time.perf_counter() - t)
            t = time.perf_counter()
            l2 = run2(True)
            ts.append(time.perf_counter() - t)
        prof = {}
        for strata in (False, True):
            ctx.profile(True)
            ctx.profile_reset()
            run2(strata)
            prof[strata] = {nm: ms for nm, _, ms, _ in ctx.profile_records()}
            ctx.profile(False)
        dev.close()
        l2["capped"] = np.zeros(len(i_names), dtype=bool)
        tt = []
        c_lens = [len(r) for r in refs]
        for _ in range(a.text_repeats):
            with tempfile.TemporaryDirectory() as d:
                t = time.perf_counter()
                with open(os.path.join(d, "tmp1.sam"), "w") as fh:
                    fh.write(ua.cluster_sam_text(names, reads, l1, c_names, c_lens))
                with open(os.path.join(d, "tmp2.sam"), "w") as fh:
                    fh.write(ua.cluster_sam_text(i_names, i_seqs, l2, c_names, c_lens, "", 1, 3))
                ua.combine_sam(os.path.join(d, "tmp1.sam"), os.path.join(d, "tmp2.sam"), os.path.join(d, "c.sam"))
                ua.decorate_sam(os.path.join(d, "c.sam"), dict(zip(names, reads)), os.path.join(d, "m.sam"), dict(zip(c_names, refs)))
                ua.parse_refine_sam(os.path.join(d, "m.sam"), os.path.join(d, "a.tsv"), os.path.join(d, "b.tsv"))
                ua.sort_tsv(os.path.join(d, "a.tsv"), os.path.join(d, "as.tsv"))
                ua.sort_tsv(os.path.join(d, "b.tsv"), os.path.join(d, "bs.tsv"))
                tt.append(time.perf_counter() - t)
        say(f"| {n_refs} | {n_reads} | {spread(tb)} | {spread(t1)} | {l1['query'].shape[0]} / {int(l1['capped'].sum())} | {len(i_names)} | "
            f"{spread(tp)} | {spread(ts)} | {float(np.median(ts)) / float(np.median(tp)):.3f} | {lp['query'].shape[0]} / {l2['query'].shape[0]} | "
            f"{prof[False].get('k_genome_scan', 0):.1f} / {prof[True].get('k_genome_scan', 0):.1f} | "
            f"{prof[False].get('k_genome_scan_fill', 0):.1f} / {prof[True].get('k_genome_scan_fill', 0):.1f} | {spread(tt)} |")
        if a.out:  # after every size: a later size that runs out of time leaves the earlier rows
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
