#!/usr/bin/env python3
"""Time the device half of ``--unmapped-features`` and the text around it on synthetic clusters with a heavy tail of row counts:
clusters of 20 to 30 nt on a random genome, most with 3 to 8 rows, a few with 10^4 to 10^5 (reads = windows of the cluster and its
flanks of 16 to 25 nt, one in five with a changed base).  Per size the three device calls -- ``mirge_cluster_diagonals``,
``mirge_cluster_pileup``, ``mirge_genome_fetch`` -- interleaved (diagonals, pile-up, fetch, diagonals, ...), medians and spread,
and the host text (``write_features`` from the table to the three files, its device calls included and reported apart).  There
is no earlier code to compare with: these are the step's first numbers.

  python tools/unmapped_features_time.py --sizes 2000x2x20000,10000x4x100000 --repeats 5 --out profiles/unmapped_features_time.txt
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import mirge3_amd  # noqa: E402,F401
from mirge3_amd import _ffi, unmapped_features as uf  # noqa: E402
from mirge3_amd.seqio import FlatSeqs  # noqa: E402

_RC = str.maketrans("ACGT", "TGCA")


def synth(n_small, n_heavy, heavy_rows, rng):
    """-> chromosome names, sequences, table lines of a <sample>_modified_selected_sorted.tsv"""
    n = n_small + n_heavy
    per_chr = 2000
    n_chr = (n + per_chr - 1) // per_chr
    names = [f"chr{k + 1}" for k in range(n_chr)]
    refs = ["".join("ACGT"[int(c)] for c in rng.integers(0, 4, 200 * per_chr + 400)) for _ in names]
    heavy = set(rng.choice(n, n_heavy, replace=False).tolist())
    lines, k_read = [], 0
    for k in range(n):
        chrom = k // per_chr
        start = 200 + 200 * (k % per_chr) + 1
        clen = int(rng.integers(20, 31))
        strand = "+-"[k % 2]
        ext = refs[chrom][start - 1 - 8:start - 1 + clen + 8]
        ext = ext.translate(_RC)[::-1] if strand == "-" else ext
        cseq = ext[8:8 + clen]
        name = f"S:miRCluster_{k + 1}_{clen}:{names[chrom]}:{start}_{start + clen - 1}{strand}"
        rows = heavy_rows if k in heavy else int(rng.integers(3, 9))
        a = rng.integers(4, 12, rows)
        ln = np.minimum(rng.integers(16, 26, rows), 8 + clen + 4 - a)
        hit = rng.random(rows) < 0.2
        for r in range(rows):
            s = ext[int(a[r]):int(a[r]) + int(ln[r])]
            if hit[r]:
                p = int(rng.integers(0, len(s)))
                s = s[:p] + "ACGT"[("ACGT".index(s[p]) + 1) % 4] + s[p + 1:]
            k_read += 1
            c = int(rng.integers(2, 200))
            lines.append(f"mir{k_read}_{c}\t{c}\t{s}\t{cseq}\t0\t{name}\t1\t255\t{len(s)}M\t*\t0\t0\t{s}\t{'I' * len(s)}\tNM:i:0\n")
    return names, refs, lines


def spread(t):
    return f"{float(np.median(t)) * 1e3:.2f} ms ({min(t) * 1e3:.2f}..{max(t) * 1e3:.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000x2x20000,10000x4x100000", help="small clusters x heavy clusters x rows of a heavy one")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    out = []

    def say(s):
        print(s, flush=True)
        out.append(s)
    ctx = _ffi.Context(0)
    say(f"# tools/unmapped_features_time.py --sizes {a.sizes} --repeats {a.repeats} --seed {a.seed}")
    for size in a.sizes.split(","):
        n_small, n_heavy, heavy_rows = (int(x) for x in size.split("x"))
        rng = np.random.default_rng(a.seed)
        names, refs, lines = synth(n_small, n_heavy, heavy_rows, rng)
        g = _ffi.DeviceGenome(ctx, seqs=FlatSeqs.from_list(refs))
        g.ref_names, g.ref_lens = names, [len(r) for r in refs]
        with tempfile.TemporaryDirectory() as d:
            with open(os.path.join(d, "S_modified_selected_sorted.tsv"), "w") as fh:
                fh.write("".join(lines))
            chroms, content = uf.read_clusters(os.path.join(d, "S_modified_selected_sorted.tsv"))
            clusters = [(e[3], e[5], e[6]) for c in chroms for e in content[c]]
            n_rows = [len(c[1]) for c in clusters]
            row_start = np.concatenate(([0], np.cumsum(n_rows))).astype(np.int64)
            reads = FlatSeqs.from_list([s for c in clusters for s in c[1]])
            cseqs = FlatSeqs.from_list([c[0] for c in clusters])
            count = np.array([x for c in clusters for x in c[2]], dtype=np.int64)
            rowc = np.repeat(np.arange(len(clusters)), n_rows)
            wins = np.arange(2 * len(clusters))
            w_ref = (wins // 2 // 2000).astype(np.uint32) % len(refs)
            w_start = 100 + 200 * ((wins // 2) % 2000)
            t_d, t_p, t_f = [], [], []
            for rep in range(a.repeats + 1):  # the first round warms the pool and is dropped
                t = time.perf_counter(); dg = _ffi.cluster_diagonals(ctx, reads, cseqs, rowc); t_d.append(time.perf_counter() - t)
                t = time.perf_counter(); _ffi.cluster_pileup(ctx, reads, [len(c[0]) for c in clusters], row_start, dg["diag"], count)
                t_p.append(time.perf_counter() - t)
                t = time.perf_counter(); g.fetch(w_ref, w_start, np.full(wins.shape[0], 114), wins % 2, np.ones(wins.shape[0])); t_f.append(time.perf_counter() - t)
            say(f"{len(clusters)} clusters ({n_heavy} of {heavy_rows} rows), {len(reads)} rows, {int(dg['flag'].astype(bool).sum())} flagged")
            say(f"  mirge_cluster_diagonals (host call, copies included)  {spread(t_d[1:])}")
            say(f"  mirge_cluster_pileup                                  {spread(t_p[1:])}")
            say(f"  mirge_genome_fetch, {wins.shape[0]} windows of 114 nt          {spread(t_f[1:])}")
            t = time.perf_counter()
            res = uf.features_sample(ctx, "S", d, g)
            total = time.perf_counter() - t
            say(f"  features_sample end to end {total:.3f} s: diagonals {res['diagonals_s']:.3f}, pile-up {res['pileup_s']:.3f}, genome windows "
                f"{res['fetch_s']:.3f}, host text {res['text_s']:.3f} (+ reading and grouping the table, building the row strings); "
                f"{res['rows']} feature rows, {res['precursors']} precursors, {res['fallback']} rows on the host route")
        g.close()
    ctx.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
