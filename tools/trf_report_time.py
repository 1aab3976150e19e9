#!/usr/bin/env python3
"""Time ``--trf-report`` on one synthetic sample: ``--reads`` raw reads (Zipf counts over ``--pool`` templates, about 5 % of them
tRNA-derived) against synth.py's ``small`` library set whose tRNA libraries are replaced by ``--trnas`` references in isodecoder
families of six (identical bodies, 1-3 differing bases).  Median (min .. max) of ``--rounds`` rounds for three figures: the hits
call (``mirge_trf_hits_run``), the assignment call (``mirge_trf_assign``) and the host text of ``mirge3_amd/trf.py`` (everything else
``write_reports`` does).  For scale, the same sample's collapse + cascade call and its per-read CSVs (mapped.csv / unmapped.csv on
the device) are timed beside them.

  python tools/trf_report_time.py --reads 10000000 --rounds 5 --out profiles/trf_report.md
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import mirge3_amd  # noqa: E402,F401
from mirge3_amd import PASS_COLUMNS, _ffi, synth, trf  # noqa: E402
from mirge3_amd.cascade import Cascade  # noqa: E402
from mirge3_amd.fastpath import names_by_pass  # noqa: E402
from mirge3_amd.seqio import FlatSeqs, Library  # noqa: E402

AC = 33


def rnd(rng, n):
    return "".join("ACGT"[int(c)] for c in rng.integers(0, 4, size=n))


def trna_libraries(rng, n):
    mature = []
    for i in range(n):
        if i % 6 == 0:
            head = rnd(rng, int(rng.integers(70, 91)) - 3) + "CCA"
            mature.append(head)
            continue
        s = list(head)
        for p in rng.integers(0, len(s) - 3, size=int(rng.integers(1, 4))):
            s[p] = "ACGT"[("ACGT".index(s[p]) + int(rng.integers(1, 4))) % 4]
        mature.append("".join(s))
    names = [f"tRNA-{i + 1}-mature" for i in range(n)]
    pre = [rnd(rng, int(rng.integers(5, 16))) + m[:-3] + "".join("ACG"[int(x)] for x in rng.integers(0, 3, size=int(rng.integers(8, 20))))
           for m in mature]  # (trailers without T, as synth.py's: its primary reads are the trailer's end plus a T run)
    return Library(names, FlatSeqs.from_list(mature)), Library([f"pre_tRNA-{i + 1}" for i in range(n)], FlatSeqs.from_list(pre))


def write_annotation(rng, libdir, org, mature, primary):
    d = os.path.join(libdir, org, "annotation.Libs")
    os.makedirs(d)
    seqs = mature.seqs.to_list()
    with open(os.path.join(d, org + trf.FILES[0]), "w") as fh:
        fh.write("".join(f">{nm}\n{s}\n{'.' * AC}XXX{'.' * (len(s) - AC - 3)}\n" for nm, s in zip(mature.names, seqs)))
    with open(os.path.join(d, org + trf.FILES[1]), "w") as fh:
        fh.write("".join(f"{nm},AA{i // 6 % 20},NNN\n" for lib in (mature, primary) for i, nm in enumerate(lib.names)))
    with open(os.path.join(d, org + trf.FILES[2]), "w") as fh:
        fh.write("unique tRNA,duplicated tRNAs\n")
    clusters = []
    with open(os.path.join(d, org + trf.FILES[3]), "w") as fh:
        fh.write("tRF cluster,type,anticodon,position,sequence,tRNA sequence\n")
        for nm, s in zip(mature.names, seqs):
            for k in range(int(rng.integers(2, 13))):
                L = int(rng.integers(15, 40))
                o = int(rng.integers(0, len(s) - L + 1))
                clusters.append(f"{nm}_Cluster{k + 1}")
                fh.write(f"{clusters[-1]},tRF,NNN,{o + 1}-{o + L},{s[o:o + L]},{s}\n")
    with open(os.path.join(d, org + trf.FILES[4]), "w") as fh:
        fh.write("".join(f"m-{c},{c}\n" for c in clusters))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--pool", type=int, default=400_000)
    ap.add_argument("--trnas", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.Generator(np.random.PCG64(17))
    sl = synth.make_libraries(seed=5, scale="small")
    sl.libs["mature_trna"], sl.libs["pre_trna"] = trna_libraries(rng, a.trnas)
    mix = dict(synth.DEFAULT_MIX, mature_trna=0.04, pre_trna=0.01, random=0.12)
    reads = synth.make_reads(sl, a.reads, seed=3, mix=mix, pool=a.pool)
    tmp = tempfile.mkdtemp(prefix="trf_report_time_")
    org = "synthorg"
    write_annotation(rng, tmp, org, sl.libs["mature_trna"], sl.libs["pre_trna"])
    ann = trf.load_annotation(tmp, org, print)
    ctx = _ffi.Context(0)
    casc = Cascade(ctx, sl.libs)
    mlib, plib = sl.libs["mature_trna"], sl.libs["pre_trna"]
    anticodon = np.full(len(mlib.names), AC, dtype=np.int32)
    tabs = trf.InforTables(ann.infor)
    header = ",".join(["Sequence", "annotFlag"] + PASS_COLUMNS[:9] + ["S1"]) + "\n"
    fig = {k: [] for k in ("collapse_cascade_s", "per_read_csv_s", "trf_hits_s", "trf_assign_s", "trf_host_text_s")}
    info = {}
    for rnd_i in range(a.rounds + 1):  # (the first round pays for the probe tables and is not counted)
        raw = _ffi.DeviceReads.pack(ctx, reads)
        ctx.sync()
        t = time.perf_counter()
        uniq, res = casc.collapse_and_run(raw)
        ctx.sync()
        t_cc = time.perf_counter() - t
        raw.close()
        order = uniq.first_appearance_order()
        t = time.perf_counter()
        _ffi.annotation_csv_device(ctx, uniq, res, os.path.join(tmp, "mapped.csv"), os.path.join(tmp, "unmapped.csv"), header, order,
                                   list(range(casc.n_pass)), 9, names_by_pass(casc))
        t_csv = time.perf_counter() - t
        ps = res.fetch()[0]
        rows = np.concatenate([order[ps[order] == trf.MATURE_PASS], order[ps[order] == trf.PRIMARY_PASS]])
        counts = uniq.counts()[0]
        sums = [int(counts[ps == p].sum()) for p in (trf.MATURE_PASS, trf.PRIMARY_PASS)]
        t = time.perf_counter()
        rec = _ffi.trf_hits(ctx, uniq, res, trf.MATURE_PASS, casc.dev_libs[trf.MATURE_PASS], casc.policies[trf.MATURE_PASS], trf.PRIMARY_PASS,
                            casc.dev_libs[trf.PRIMARY_PASS], casc.policies[trf.PRIMARY_PASS], rows, anticodon)
        t_hits = time.perf_counter() - t
        rd = uniq.unpack().take(rows).to_list()
        t_assign = [0.0]

        def assign(arows):
            t1 = time.perf_counter()
            out = _ffi.trf_assign(ctx, uniq, res, [rows[k] for k, _, _ in arows], [tabs.index.get(nm, -1) for _, nm, _ in arows],
                                  [st for _, _, st in arows], tabs.ref_ptr, tabs.strings, tabs.c_start, tabs.c_end, tabs.rank)
            t_assign[0] = time.perf_counter() - t1
            return out

        t = time.perf_counter()
        hits = trf.hits_by_row(rd, rec, mlib.names, plib.names)
        out = trf.write_reports(tmp, ["S1"], rd, counts[rows], hits, [sums[0]], [sums[1]], ann, dict(zip(plib.names, plib.seqs.to_list())),
                                trf.library_order(mlib.names, plib.names), assign, lambda msg: None)
        t_text = time.perf_counter() - t - t_assign[0]
        info = dict(raw_reads=len(reads), unique_reads=len(uniq), trna_rows=int(rows.size), trna_raw_reads=sum(sums),
                    hit_records=int(rec["row"].shape[0]), report_rows=out["printed"])
        res.close(); uniq.close()
        if rnd_i:
            for k, v in zip(fig, (t_cc, t_csv, t_hits, t_assign[0], t_text)):
                fig[k].append(v)
    lines = ["# --trf-report on one MI355X (tools/trf_report_time.py)", "",
             f"`--reads {a.reads} --pool {a.pool} --trnas {a.trnas} --rounds {a.rounds}`: " + ", ".join(f"{k} = {v}" for k, v in info.items()), "",
             "| figure | median s | min .. max |", "|---|---|---|"]
    for k, v in fig.items():
        lines.append(f"| {k} | {statistics.median(v):.4f} | {min(v):.4f} .. {max(v):.4f} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
