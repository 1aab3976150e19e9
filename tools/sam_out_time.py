#!/usr/bin/env python3
"""Time ``--sam-out``'s device call (``mirge_sam_write_device``) on one synthetic sample of ``--reads`` raw reads, twice: with Zipf
counts over a few hundred thousand unique reads (a miRNA sample: a handful of rows stand for most lines) and all-distinct (every
row one line).  Per shape: the call into a real file and into /dev/null (the difference is the share that is the file write),
text bytes, GB/s, best and spread of ``--repeats`` runs; and ``format_sam_host`` on the first 10^5 lines for scale.

  python tools/sam_out_time.py --reads 10000000 --repeats 3 --out profiles/sam_out_time.txt
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import mirge3_amd  # noqa: E402,F401
from mirge3_amd import _ffi, sam_export  # noqa: E402
from mirge3_amd.cascade import Cascade  # noqa: E402
from mirge3_amd.seqio import FlatSeqs, Library  # noqa: E402


def rnd(rng, n):
    return "".join("ACGT"[int(c)] for c in rng.integers(0, 4, size=n))


def libraries(rng):
    def lib(prefix, n, length):
        seqs = [rnd(rng, length) for _ in range(n)]
        names = [f"{prefix}{i}" for i in range(n)]
        heads = [f"{nm} chr{1 + i % 22} segs:1-{length // 2},{length // 2 + 1}-{length} cds:{'+-'[i % 2]}:{10_000 + 5000 * i}-"
                 f"{10_000 + 5000 * i + length // 2 - 1},{20_000_000 + 5000 * i}-{20_000_000 + 5000 * i + length - length // 2 - 1}"
                 for i, nm in enumerate(names)]
        return Library(names, FlatSeqs.from_list(seqs), heads)
    return {"mirna": lib("miR-", 2000, 22), "hairpin": lib("mir-", 1500, 90), "mature_trna": lib("tRNA-", 400, 74),
            "pre_trna": lib("pre-tRNA-", 400, 92), "snorna": lib("SNO", 1000, 130), "rrna": lib("RR", 50, 1800),
            "ncrna_others": lib("NC", 3000, 300), "mrna": lib("ENST", 6000, 900)}


def unique_reads(rng, libs, n):
    """n distinct reads of 18 to 30 nt cut from the mRNA / ncRNA / rRNA / snoRNA references and whole miRNAs"""
    out = set(libs["mirna"].seqs.to_list())
    pools = [libs[k].seqs.to_list() for k in ("mrna", "ncrna_others", "rrna", "snorna")]
    while len(out) < n:
        pool = pools[int(rng.integers(0, len(pools)))]
        q = pool[int(rng.integers(0, len(pool)))]
        L = int(rng.integers(18, 31))
        o = int(rng.integers(0, len(q) - L + 1))
        out.add(q[o:o + L])
    return sorted(out)[:n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--zipf-unique", type=int, default=300_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.Generator(np.random.PCG64(5))
    libs = libraries(rng)
    ctx = _ffi.Context(0)
    casc = Cascade(ctx, libs)
    report = []
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
        tmp = tempfile.mkdtemp(prefix="sam_out_time_")
        path = os.path.join(tmp, "S1.sam")
        line = {"shape": shape, "unique_reads": len(uniq)}
        for target, key in ((path, "file"), ("/dev/null", "dev_null")):
            ts = []
            for _ in range(a.repeats + 1):  # the first run pays for the staging buffers and the lift tables
                t0 = time.perf_counter()
                n_lines, n_bytes = sam_export.write_sample(casc, uniq, res, order, 0, target, sam_export.DEFAULT_HEADER, "synthorg")
                ts.append(time.perf_counter() - t0)
            line.update({"lines": n_lines, "text_bytes": n_bytes, key + "_first_s": round(ts[0], 4), key + "_best_s": round(min(ts[1:]), 4),
                         key + "_worst_s": round(max(ts[1:]), 4), key + "_GB_per_s": round(n_bytes / min(ts[1:]) / 1e9, 3)})
        line["file_write_share"] = round(1.0 - line["dev_null_best_s"] / line["file_best_s"], 3)
        # the plain Python restatement on a slice of about 10^5 lines
        useq = uniq.unpack().to_list()
        counts, _ = uniq.counts()
        ann = res.fetch()
        k, acc = 0, 0
        while k < len(order) and acc < 100_000:
            acc += int(counts[order[k], 0]); k += 1
        t0 = time.perf_counter()
        body = sam_export.format_sam_host(useq, *ann, counts, order[:k], 0, sam_export.host_passes(casc), "synthorg")
        line["format_sam_host_lines"] = body.count(b"\n")
        line["format_sam_host_s"] = round(time.perf_counter() - t0, 4)
        os.remove(path); os.rmdir(tmp)
        res.close(); uniq.close()
        report.append(line)
        print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            for line in report:
                fh.write(repr(line) + "\n")


if __name__ == "__main__":
    main()
