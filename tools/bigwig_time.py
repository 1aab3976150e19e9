#!/usr/bin/env python3
"""Time ``--coverage-bigwig``'s device call (``mirge_bigwig_write_device``, unstranded) on its default route and with
``MIRGE_BW_DEFLATE=none`` beside ``--coverage``'s bedGraph call and ``--sam-out``'s call, on the two synthetic samples of
``tools/coverage_time.py``: ``--reads`` raw reads with Zipf counts over a few hundred thousand unique reads, and all-distinct.  The four
calls are interleaved, round by round; per call the median of ``--rounds`` rounds with min .. max on the host's wall clock (one warm-up
round).  File sizes: the bedGraph, the bigWig of both routes, and what ``bigwig.write_host`` with zlib level 6 would write -- taken by
deflating the raw file's blocks with Python's zlib (the raw file is ``write_host``'s byte for byte, and only the blocks differ).

  python tools/bigwig_time.py --reads 3000000 --rounds 5 --out profiles/bigwig_time.md
"""
import argparse
import os
import statistics
import struct
import sys
import tempfile
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
import mirge3_amd  # noqa: E402,F401
from mirge3_amd import _ffi, bigwig, coverage, sam_export  # noqa: E402
from mirge3_amd.cascade import Cascade  # noqa: E402
from mirge3_amd.seqio import FlatSeqs  # noqa: E402
from coverage_time import ORG, unique_reads  # noqa: E402
from sam_out_time import libraries  # noqa: E402


def blocks_of(buf, index_at):
    """(offset, size) of every block under the R-tree at ``index_at``"""
    out = []

    def walk(off):
        leaf, _, cnt = struct.unpack_from("<BBH", buf, off)
        for i in range(cnt):
            if leaf:
                out.append(struct.unpack_from("<QQ", buf, off + 4 + 32 * i + 16))
            else:
                walk(struct.unpack_from("<Q", buf, off + 4 + 24 * i + 16)[0])

    walk(index_at + 48)
    return out


def zlib6_size(path):
    """the size of the raw file at ``path`` with every block as a zlib level 6 stream"""
    buf = open(path, "rb").read()
    zooms, = struct.unpack_from("<H", buf, 6)
    indexes = [struct.unpack_from("<Q", buf, 24)[0]] + [struct.unpack_from("<Q", buf, 64 + 24 * k + 16)[0] for k in range(zooms)]
    size = len(buf)
    for at in indexes:
        for off, n in blocks_of(buf, at):
            size += len(zlib.compress(buf[off:off + n], 6)) - n
    return size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=3_000_000)
    ap.add_argument("--zipf-unique", type=int, default=300_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.Generator(np.random.PCG64(5))
    libs = libraries(rng)
    header = ("@HD\tVN:1.0\n" + "".join(f"@SQ\tSN:chr{k}\tLN:{1 << 28}\n" for k in range(1, 23))).encode()
    sq = bigwig.parse_sizes(header)
    sq_names = [n for n, _ in sq]
    ctx = _ffi.Context(0)
    casc = Cascade(ctx, libs)
    calls = ("bigwig_device", "bigwig_none", "coverage_bedgraph", "sam_out")
    lines = [f"`tools/bigwig_time.py --reads {a.reads} --zipf-unique {a.zipf_unique} --rounds {a.rounds}`: host wall clock per call, "
             "median (min .. max) of the rounds, the four calls interleaved; unstranded; files written to a temporary directory.", ""]
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
        tmp = tempfile.mkdtemp(prefix="bigwig_time_")
        f = {k: os.path.join(tmp, k) for k in ("S1.bw", "S1.none.bw", "S1.bedgraph", "S1.sam")}
        ts = {c: [] for c in calls}
        info = {}
        for rnd in range(a.rounds + 1):
            for call in calls:
                os.environ["MIRGE_BW_DEFLATE"] = "none" if call == "bigwig_none" else "device"
                t0 = time.perf_counter()
                if call == "bigwig_device":
                    info[call] = bigwig.write_sample(casc, uniq, res, order, 0, [f["S1.bw"]], False, ORG, sq)[0]
                elif call == "bigwig_none":
                    info[call] = bigwig.write_sample(casc, uniq, res, order, 0, [f["S1.none.bw"]], False, ORG, sq)[0]
                elif call == "coverage_bedgraph":
                    info[call] = coverage.write_sample(casc, uniq, res, order, 0, [f["S1.bedgraph"]], False, ORG, sq_names)
                else:
                    info[call] = sam_export.write_sample(casc, uniq, res, order, 0, f["S1.sam"], sam_export.DEFAULT_HEADER, ORG)
                if rnd:
                    ts[call].append(time.perf_counter() - t0)
        bd, bn, cb = info["bigwig_device"], info["bigwig_none"], info["coverage_bedgraph"]
        assert bd["items"] == bn["items"] == cb["lines"] and bd["zoom_records"] == bn["zoom_records"], (bd, bn, cb)
        med = {c: statistics.median(ts[c]) for c in calls}
        lines += [f"**{shape}**: {len(uniq)} unique reads, {cb['intervals']} intervals, {bd['items']} runs in {bd['sections']} sections, {bd['levels']} zoom "
                  f"levels (records: {', '.join(map(str, bd['zoom_records'])) or 'none'}).  Bytes: bedGraph {cb['bytes']}, bigWig {bd['bytes']} (device "
                  f"deflate), {bn['bytes']} (`MIRGE_BW_DEFLATE=none`), {zlib6_size(f['S1.none.bw'])} (`write_host`'s blocks at zlib level 6).  "
                  f"The bigWig call stays below `--sam-out`'s call: {'yes' if med['bigwig_device'] < med['sam_out'] else 'NO'}.", "",
                  "| call | median ms | min .. max ms |", "|---|---|---|"]
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
