#!/usr/bin/env python3
"""Time ``--sorted-bam``'s device call (``mirge_bam_write_device``) on the two synthetic samples of ``tools/sam_out_time.py`` -- Zipf
counts over a few hundred thousand unique reads, and all-distinct -- of ``--reads`` raw reads.  Per shape five calls are interleaved
round by round (after one unrecorded warm-up round, which pays for the staging buffers and the lift tables): the device deflate, the
``MIRGE_BAM_DEFLATE=dynamic`` route (the same parse, per block also a Huffman code of its own), the ``MIRGE_BAM_DEFLATE=tight`` route
(the dynamic route's forms on a closer parse), the ``MIRGE_BAM_DEFLATE=host`` route
(zlib level 6 on ``--threads`` host threads: the same blocks, so its file size is zlib's on them) and ``--sam-out``'s call on the same
build, the closest existing work.  Reported: median, min and max seconds of ``--repeats`` rounds, stream bytes, file bytes of the four
routes, the dynamic and the tight file's members by deflate block type (and how many dynamic headers use run symbols), and the share of
the device file's excess over zlib's that the dynamic and the tight route remove.

  python tools/sorted_bam_time.py --reads 10000000 --repeats 7 --out profiles/sorted_bam_time.txt
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import mirge3_amd  # noqa: E402,F401
from mirge3_amd import _ffi, bam_export, sam_export  # noqa: E402
from mirge3_amd.cascade import Cascade  # noqa: E402
from mirge3_amd.seqio import FlatSeqs  # noqa: E402
from sam_out_time import libraries, unique_reads  # noqa: E402


def members_by_btype(path):
    """[stored, fixed, dynamic, dynamic with run symbols in the header] members of a BGZF file (the EOF block, a fixed one, not counted).
    A dynamic block's header: BFINAL, BTYPE, HLIT, HDIST, HCLEN in 17 bits, then the lengths of the codes of 16, 17 and 18, 3 bits each
    (RFC 1951, 3.2.7): all three zero = no run symbol is used"""
    with open(path, "rb") as fh:
        data = fh.read()
    out, at = [0, 0, 0, 0], 0
    while at < len(data) - 28:
        btype = (data[at + 18] >> 1) & 3
        out[btype] += 1
        if btype == 2 and (int.from_bytes(data[at + 18:at + 22], "little") >> 17) & 0x1FF:
            out[3] += 1
        at += (data[at + 16] | (data[at + 17] << 8)) + 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--zipf-unique", type=int, default=300_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--routes", default="device,dynamic,tight,host,sam_out",
                    help="the calls to time, e.g. 'device' alone for an A/B of two builds of the library (MIRGE_NATIVE_SO)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    routes = [r for r in ("device", "dynamic", "tight", "host", "sam_out") if r in a.routes.split(",")]
    rng = np.random.Generator(np.random.PCG64(5))
    libs = libraries(rng)
    header = ("@HD\tVN:1.0\n" + "".join(f"@SQ\tSN:chr{k}\tLN:{1 << 28}\n" for k in range(1, 23))).encode()
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
        tmp = tempfile.mkdtemp(prefix="sorted_bam_time_")
        bam, bai, sam = (os.path.join(tmp, f) for f in ("S1_sorted.bam", "S1_sorted.bai", "S1.sam"))
        ts = {r: [] for r in routes}
        line = {"shape": shape, "unique_reads": len(uniq), "threads": a.threads}
        for rnd in range(a.repeats + 1):
            for route in routes:
                os.environ.pop("MIRGE_BAM_DEFLATE", None)
                if route in ("dynamic", "tight", "host"):
                    os.environ["MIRGE_BAM_DEFLATE"] = route
                t0 = time.perf_counter()
                if route == "sam_out":
                    _, n_text = sam_export.write_sample(casc, uniq, res, order, 0, sam, sam_export.DEFAULT_HEADER, "synthorg")
                    line["sam_text_bytes"] = n_text
                else:
                    n_rec, n_stream, n_file = bam_export.write_sample(casc, uniq, res, order, 0, bam, bai, header, "synthorg", threads=a.threads)
                    line.update({"records": n_rec, "stream_bytes": n_stream, route + "_file_bytes": n_file, "bai_bytes": os.path.getsize(bai)})
                if rnd:
                    ts[route].append(time.perf_counter() - t0)
                elif route in ("dynamic", "tight"):
                    line[route + "_members_stored_fixed_dynamic_withruns"] = members_by_btype(bam)
        os.environ.pop("MIRGE_BAM_DEFLATE", None)
        for route, v in ts.items():
            line.update({route + "_median_s": round(statistics.median(v), 4), route + "_min_s": round(min(v), 4), route + "_max_s": round(max(v), 4)})
        if "device" in routes and "host" in routes:
            line["device_over_zlib6_size"] = round(line["device_file_bytes"] / line["host_file_bytes"], 3)
        if "device" in routes and "host" in routes and "dynamic" in routes:
            line["dynamic_over_zlib6_size"] = round(line["dynamic_file_bytes"] / line["host_file_bytes"], 3)
            line["dynamic_closes_of_the_gap"] = round((line["device_file_bytes"] - line["dynamic_file_bytes"]) / max(1, line["device_file_bytes"] - line["host_file_bytes"]), 3)
        if "device" in routes and "host" in routes and "tight" in routes:
            line["tight_over_zlib6_size"] = round(line["tight_file_bytes"] / line["host_file_bytes"], 3)
            line["tight_closes_of_the_gap"] = round((line["device_file_bytes"] - line["tight_file_bytes"]) / max(1, line["device_file_bytes"] - line["host_file_bytes"]), 3)
        for f in (bam, bai, sam):
            if os.path.exists(f):
                os.remove(f)
        os.rmdir(tmp)
        res.close(); uniq.close()
        report.append(line)
        print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            for line in report:
                fh.write(repr(line) + "\n")


if __name__ == "__main__":
    main()
