#!/usr/bin/env python3
"""Time ``--coverage``'s device call (``mirge_coverage_write_device``, both modes) beside ``--sam-out``'s (``mirge_sam_write_device``) and
``--sorted-bam``'s on its default route (``mirge_bam_write_device``) on the two synthetic samples of ``tools/sam_out_time.py``: ``--reads``
raw reads with Zipf counts over a few hundred thousand unique reads, and all-distinct.  The four calls are interleaved, round by round;
per call the median of ``--rounds`` rounds with min .. max on the host's wall clock (every call ends in a device synchronise and a closed
file; one warm-up round pays for staging buffers and lift tables).  Once, for information: a NumPy sort-based restatement of the runs on
the same intervals (its line count must equal the device's), the number of intervals, lines and bytes.

  python tools/coverage_time.py --reads 3000000 --rounds 5 --out profiles/coverage_time.md
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
import mirge3_amd  # noqa: E402,F401
from mirge3_amd import _ffi, bam_export, coverage, sam_export  # noqa: E402
from mirge3_amd.cascade import PASSES, Cascade  # noqa: E402
from mirge3_amd.seqio import FlatSeqs  # noqa: E402
from sam_out_time import libraries  # noqa: E402

ORG = "synthorg"


def unique_reads(rng, libs, n):
    """sam_out_time.unique_reads, drawn in batches: n distinct reads of 18 to 30 nt cut from the mRNA / ncRNA / rRNA / snoRNA
    references and whole miRNAs"""
    out = set(libs["mirna"].seqs.to_list())
    pools = [libs[k].seqs.to_list() for k in ("mrna", "ncrna_others", "rrna", "snorna")]
    while len(out) < n:
        m = max(1024, int(1.2 * (n - len(out))))
        which, u, L, v = rng.integers(0, len(pools), size=m), rng.random(size=m), rng.integers(18, 31, size=m), rng.random(size=m)
        for k in range(m):
            pool = pools[which[k]]
            q = pool[int(u[k] * len(pool))]
            o = int(v[k] * (len(q) - L[k] + 1))
            out.add(q[o:o + L[k]])
    return sorted(out)[:n]


def numpy_intervals(casc, uniq, res):
    """the sample's intervals from the fetched result and the lift tables, vectorised (what k_cov_intervals computes on the device)"""
    classes, arr, keep = sam_export.pass_tables(casc, ORG)
    names, flat, off = coverage.rank_tables(casc, ORG, None)
    ps, ref, roff, _ = res.fetch()
    counts, _ = uniq.counts()
    lens = np.diff(uniq.unpack().offsets)
    cols = [[], [], [], [], []]
    for p, a in zip(classes.tolist(), keep):
        sel = np.flatnonzero((ps == p) & (counts[:, 0] > 0))
        sel = sel[a["chrom_of_ref"][ref[sel]] >= 0]
        if sel.size == 0:
            continue
        r = ref[sel].astype(np.int64)
        n = lens[sel] - int(PASSES[p][3].get("trim5", 0)) - int(PASSES[p][3].get("trim3", 0))
        pos = roff[sel].astype(np.int64) + 1
        minus = a["minus"][r] != 0
        start, found, n_seg = pos.copy(), np.zeros(sel.size, bool), a["seg_ptr"][r + 1] - a["seg_ptr"][r]
        for k in range(int(n_seg.max())):
            live = (k < n_seg) & ~found
            idx = np.where(live, a["seg_ptr"][r] + k, 0)
            s = a["seg_s"][idx].astype(np.int64)
            hit = live & (s <= pos) & (pos <= a["seg_e"][idx])
            lifted = np.where(minus, a["cds_hi"][idx] - (pos - s) - n + 1, a["cds_lo"][idx] + (pos - s))
            start[hit] = lifted[hit]
            found |= hit
        for c, v in zip(cols, (flat[off[p] + a["chrom_of_ref"][r]], start - 1, n, counts[sel, 0], minus)):
            c.append(v)
    return coverage.as_intervals(*[np.concatenate(c) for c in cols]), names


def numpy_runs(iv, stranded):
    """events, one sort by key, a prefix sum, the three selections: the device's pipeline in NumPy; -> number of runs"""
    strand = (iv["minus"].astype(np.int64) if stranded else 0) << 55
    hi = strand | iv["rank"].astype(np.int64) << 31
    key = np.concatenate([hi | iv["start"], hi | (iv["start"] + iv["len"])])
    delta = np.concatenate([iv["weight"].astype(np.int64), -iv["weight"].astype(np.int64)])
    o = np.argsort(key, kind="stable")
    key, S = key[o], np.cumsum(delta[o])
    last = np.concatenate([key[1:] != key[:-1], [True]])
    key, S = key[last], S[last]
    change = S != np.concatenate([[0], S[:-1]])
    key, S = key[change], S[change]
    assert S[-1] == 0 and S.min() >= 0
    return int((S != 0).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=3_000_000)
    ap.add_argument("--zipf-unique", type=int, default=300_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.Generator(np.random.PCG64(5))
    libs = libraries(rng)
    bam_header = ("@HD\tVN:1.0\n" + "".join(f"@SQ\tSN:chr{k}\tLN:{1 << 28}\n" for k in range(1, 23))).encode()
    ctx = _ffi.Context(0)
    casc = Cascade(ctx, libs)
    calls = ("coverage_unstranded", "coverage_stranded", "sam_out", "sorted_bam")
    lines = [f"`tools/coverage_time.py --reads {a.reads} --zipf-unique {a.zipf_unique} --rounds {a.rounds}`: host wall clock per call, "
             "median (min .. max) of the rounds, the four calls interleaved; files written to a temporary directory.", ""]
    shown = 0
    for shape in ("zipf", "distinct"):
        n_u = a.zipf_unique if shape == "zipf" else a.reads
        reads = unique_reads(rng, libs, n_u)
        if shape == "zipf":
            w = 1.0 / np.arange(1, n_u + 1) ** 1.1
            cnt = np.maximum(1, np.floor(w / w.sum() * a.reads)).astype(np.uint32)
            rng.shuffle(cnt)
        else:
            cnt = np.ones(n_u, dtype=np.uint32)
        raw = _ffi.DeviceReads.pack(ctx, FlatSeqs.from_list(reads))
        uniq = raw.collapse(None, 1, weights=cnt)
        raw.close()
        res = casc.run(uniq)
        order = uniq.first_appearance_order()
        ctx.sync()
        tmp = tempfile.mkdtemp(prefix="coverage_time_")
        f = {k: os.path.join(tmp, k) for k in ("S1.bedgraph", "S1.plus.bedgraph", "S1.minus.bedgraph", "S1.sam", "S1_sorted.bam", "S1_sorted.bai")}
        ts = {c: [] for c in calls}
        info = {}
        for rnd in range(a.rounds + 1):
            for call in calls:
                t0 = time.perf_counter()
                if call == "coverage_unstranded":
                    info[call] = coverage.write_sample(casc, uniq, res, order, 0, [f["S1.bedgraph"]], False, ORG)
                elif call == "coverage_stranded":
                    info[call] = coverage.write_sample(casc, uniq, res, order, 0, [f["S1.plus.bedgraph"], f["S1.minus.bedgraph"]], True, ORG)
                elif call == "sam_out":
                    info[call] = sam_export.write_sample(casc, uniq, res, order, 0, f["S1.sam"], sam_export.DEFAULT_HEADER, ORG)
                else:
                    info[call] = bam_export.write_sample(casc, uniq, res, order, 0, f["S1_sorted.bam"], f["S1_sorted.bai"], bam_header, ORG)
                if rnd:
                    ts[call].append(time.perf_counter() - t0)
        iv, _names = numpy_intervals(casc, uniq, res)
        t0 = time.perf_counter()
        np_runs = [numpy_runs(iv, False), numpy_runs(iv, True)]
        t_np = (time.perf_counter() - t0) / 2
        cu, cs = info["coverage_unstranded"], info["coverage_stranded"]
        assert np_runs == [cu["lines"], cs["lines"]] and iv["rank"].size == cu["intervals"], (np_runs, cu, cs, iv["rank"].size)
        lines += [f"**{shape}**: {len(uniq)} unique reads, {cu['intervals']} intervals of summed weight {cu['weight']}; unstranded {cu['lines']} lines / "
                  f"{cu['bytes']} bytes, stranded {cs['lines']} lines / {cs['bytes']} bytes; `<sample>.sam` {info['sam_out'][0]} lines / {info['sam_out'][1]} "
                  f"bytes; `_sorted.bam` {info['sorted_bam'][2]} bytes.  NumPy sort-based restatement of the runs alone (no text, one mode): "
                  f"{t_np * 1e3:.1f} ms.", "", "| call | median ms | min .. max ms |", "|---|---|---|"]
        for call in calls:
            v = ts[call]
            lines.append(f"| {call} | {statistics.median(v) * 1e3:.1f} | {min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f} |")
        lines.append("")
        for p in f.values():
            if os.path.exists(p):
                os.remove(p)
        os.rmdir(tmp)
        res.close(); uniq.close()
        print("\n".join(lines[shown:]), flush=True)
        shown = len(lines)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
