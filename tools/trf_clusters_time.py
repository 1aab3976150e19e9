#!/usr/bin/env python3
"""Time ``--trf-clusters`` on the synthetic sample of tools/trf_report_time.py, extended by fragments (exact and with one substitution)
of two tRNAs so that one group holds about ``--small`` and one about ``--large`` points.  Median (min .. max) of ``--rounds`` rounds,
taken in turn within each round: the device call (``mirge_trf_cluster``, everything from the upload of the points to the arrays on the
host) and the host text (``trf.write_clusters`` without that call).  The NumPy restatement of the reference's clustering
(tests/test_trf_clusters.py: ``restate``) is timed on the ``--small`` group alone: it is the only other implementation there is, and
the reference's pure-Python loops would not finish on the large group.

  python tools/trf_clusters_time.py --rounds 5 --out profiles/trf_clusters.md
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "tests")))
import mirge3_amd  # noqa: E402,F401
from mirge3_amd import _ffi, synth, trf  # noqa: E402
from mirge3_amd.cascade import Cascade  # noqa: E402
from mirge3_amd.seqio import FlatSeqs  # noqa: E402
import trf_report_time as base  # noqa: E402


def fragments(rng, seq, n):
    """n distinct reads of 16 nt or more from ``seq``: every window first, then windows with one substitution"""
    out = {}
    for L in range(len(seq), 15, -1):
        for s in range(len(seq) - L + 1):
            if len(out) < n:
                out[seq[s:s + L]] = 1
    while len(out) < n:
        L = int(rng.integers(16, len(seq) + 1))
        s = int(rng.integers(0, len(seq) - L + 1))
        p = int(rng.integers(0, L))
        w = seq[s:s + L]
        out[w[:p] + "ACGT"[("ACGT".index(w[p]) + int(rng.integers(1, 4))) % 4] + w[p + 1:]] = 1
    return list(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--pool", type=int, default=100_000)
    ap.add_argument("--trnas", type=int, default=600)
    ap.add_argument("--small", type=int, default=2000)
    ap.add_argument("--large", type=int, default=20000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.Generator(np.random.PCG64(17))
    sl = synth.make_libraries(seed=5, scale="small")
    sl.libs["mature_trna"], sl.libs["pre_trna"] = base.trna_libraries(rng, a.trnas)
    mix = dict(synth.DEFAULT_MIX, mature_trna=0.04, pre_trna=0.01, random=0.12)
    sample = synth.make_reads(sl, a.reads, seed=3, mix=mix, pool=a.pool).to_list()
    mseq = sl.libs["mature_trna"].seqs.to_list()
    for ref, n in ((6, a.small), (12, a.large)):  # (the first tRNA of two isodecoder families)
        for rd in fragments(rng, mseq[ref], n):
            sample += [rd] * int(min(200, rng.zipf(1.6)))
    reads = FlatSeqs.from_list(sample)
    tmp = tempfile.mkdtemp(prefix="trf_clusters_time_")
    org = "synthorg"
    base.write_annotation(rng, tmp, org, sl.libs["mature_trna"], sl.libs["pre_trna"])
    ann = trf.load_annotation(tmp, org, print)
    ctx = _ffi.Context(0)
    casc = Cascade(ctx, sl.libs)
    mlib, plib = sl.libs["mature_trna"], sl.libs["pre_trna"]
    anticodon = np.full(len(mlib.names), base.AC, dtype=np.int32)
    tabs = trf.InforTables(ann.infor)
    fig = {k: [] for k in ("trf_cluster_s", "trf_cluster_text_s")}
    info, groups_seen = {}, []
    for rnd_i in range(a.rounds + 1):  # (the first round pays for first allocations and is not counted)
        raw = _ffi.DeviceReads.pack(ctx, reads)
        uniq, res = casc.collapse_and_run(raw)
        raw.close()
        order = uniq.first_appearance_order()
        ps = res.fetch()[0]
        rows = np.concatenate([order[ps[order] == trf.MATURE_PASS], order[ps[order] == trf.PRIMARY_PASS]])
        counts = uniq.counts()[0]
        sums = [int(counts[ps == p].sum()) for p in (trf.MATURE_PASS, trf.PRIMARY_PASS)]
        rec = _ffi.trf_hits(ctx, uniq, res, trf.MATURE_PASS, casc.dev_libs[trf.MATURE_PASS], casc.policies[trf.MATURE_PASS], trf.PRIMARY_PASS,
                            casc.dev_libs[trf.PRIMARY_PASS], casc.policies[trf.PRIMARY_PASS], rows, anticodon)
        rd = uniq.unpack().take(rows).to_list()

        def assign(arows):
            return _ffi.trf_assign(ctx, uniq, res, [rows[k] for k, _, _ in arows], [tabs.index.get(nm, -1) for _, nm, _ in arows],
                                   [st for _, _, st in arows], tabs.ref_ptr, tabs.strings, tabs.c_start, tabs.c_end, tabs.rank)

        def cluster(groups):
            groups_seen[:] = groups
            ptr = np.zeros(len(groups) + 1, dtype=np.int64)
            np.cumsum([len(g["rows"]) for g in groups], out=ptr[1:])
            return _ffi.trf_cluster(ctx, uniq, ptr, [rows[k] for g in groups for k in g["rows"]], [o for g in groups for o in g["off"]],
                                    [x for g in groups for x in g["rp"]], [g["tlen"] for g in groups])

        tm = {}
        hits = trf.hits_by_row(rd, rec, mlib.names, plib.names)
        out = trf.write_reports(tmp, ["S1"], rd, counts[rows], hits, [sums[0]], [sums[1]], ann, dict(zip(plib.names, plib.seqs.to_list())),
                                trf.library_order(mlib.names, plib.names), assign, lambda msg: None, cluster, tm)
        sizes = sorted((len(g["rows"]) for g in groups_seen), reverse=True)
        info = dict(raw_reads=len(reads), unique_reads=len(uniq), trna_rows=int(rows.size), groups=out["clusters"]["groups"],
                    points=out["clusters"]["points"], largest_groups=sizes[:3], written_clusters=sum(out["clusters"]["clusters"].values()))
        res.close(); uniq.close()
        if rnd_i:
            for k in fig:
                fig[k].append(tm[k])
    from test_trf_clusters import restate
    g = min(groups_seen, key=lambda g: abs(len(g["rows"]) - a.small))
    t = time.perf_counter()
    restate(g["dashed"], g["rp"])
    t_np = time.perf_counter() - t
    lines = ["# --trf-clusters on one MI355X (tools/trf_clusters_time.py)", "",
             f"`--reads {a.reads} --pool {a.pool} --trnas {a.trnas} --small {a.small} --large {a.large} --rounds {a.rounds}`: " +
             ", ".join(f"{k} = {v}" for k, v in info.items()), "", "| figure | median s | min .. max |", "|---|---|---|"]
    for k, v in fig.items():
        lines.append(f"| {k} | {statistics.median(v):.4f} | {min(v):.4f} .. {max(v):.4f} |")
    lines.append(f"| numpy_restatement_s (the group of {len(g['rows'])} points alone, once) | {t_np:.4f} | |")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
