#!/usr/bin/env python3
"""Time ``--bgzf-out`` beside the plain text calls on the two synthetic samples of ``tools/sam_out_time.py`` / ``tools/coverage_time.py``:
``--reads`` raw reads with Zipf counts over a few hundred thousand unique reads, and all-distinct.  Per exporter (``--sam-out``,
``--coverage`` unstranded and stranded) three calls are interleaved, round by round: the plain call, the device route
(``MIRGE_BGZF_DEFLATE=device``) and the host route (``=host``: the same blocks through zlib level 6).  Per call the median of ``--rounds``
rounds with min .. max on the host's wall clock (every call ends in a device synchronise and closed, renamed files; one warm-up round
pays for staging buffers and lift tables).  Beside the times: the plain file's bytes, both routes' file bytes and the members per form.
Every ``.gz`` of the last round is inflated and compared with the plain file.

  python tools/bgzf_out_time.py --reads 3000000 --rounds 5 --out profiles/bgzf_out_time.md
"""
import argparse
import gzip
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.dirname(__file__)))
import mirge3_amd  # noqa: E402,F401
from mirge3_amd import _ffi, coverage, sam_export  # noqa: E402
from mirge3_amd.cascade import Cascade  # noqa: E402
from mirge3_amd.seqio import FlatSeqs  # noqa: E402
from coverage_time import ORG, unique_reads  # noqa: E402
from sam_out_time import libraries  # noqa: E402

EXPORTERS = ("sam_out", "coverage_unstranded", "coverage_stranded")
ROUTES = ("plain", "device", "host")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=3_000_000)
    ap.add_argument("--zipf-unique", type=int, default=300_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="zipf,distinct")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.Generator(np.random.PCG64(5))
    libs = libraries(rng)
    ctx = _ffi.Context(0)
    casc = Cascade(ctx, libs)
    lines = [f"`tools/bgzf_out_time.py --reads {a.reads} --zipf-unique {a.zipf_unique} --rounds {a.rounds}`: host wall clock per call, "
             "median (min .. max) of the rounds; per exporter the plain call, the device route and the host route interleaved; files written "
             f"to a temporary directory; host route on {os.environ.get('MIRGE_GZ_THREADS') or 16} threads (MIRGE_GZ_THREADS, default 16).", ""]
    shown = 0
    for shape in a.shapes.split(","):
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
        tmp = tempfile.mkdtemp(prefix="bgzf_out_time_")
        ts = {(e, r): [] for e in EXPORTERS for r in ROUTES}
        info, paths = {}, {}
        for rnd in range(a.rounds + 1):
            for e in EXPORTERS:
                for r in ROUTES:
                    gz = r != "plain"
                    if gz:
                        os.environ["MIRGE_BGZF_DEFLATE"] = r
                    d = os.path.join(tmp, r)
                    os.makedirs(d, exist_ok=True)
                    t0 = time.perf_counter()
                    if e == "sam_out":
                        p = [os.path.join(d, "S1.sam.gz" if gz else "S1.sam")]
                        out = sam_export.write_sample(casc, uniq, res, order, 0, p[0], sam_export.DEFAULT_HEADER, ORG, bgzf_out=gz)
                        st = dict(text=out[1] + len(sam_export.DEFAULT_HEADER), bgzf=[out[2]] if gz else None)
                    else:
                        stranded = e == "coverage_stranded"
                        p = coverage.sample_paths(d, "S1", stranded, gz)
                        out = coverage.write_sample(casc, uniq, res, order, 0, p, stranded, ORG, bgzf_out=gz)
                        st = dict(text=out["bytes"], bgzf=out.get("bgzf"))
                    if rnd:
                        ts[e, r].append(time.perf_counter() - t0)
                    info[e, r], paths[e, r] = st, [str(x) for x in p]
        os.environ.pop("MIRGE_BGZF_DEFLATE", None)
        lines += [f"**{shape}**: {len(uniq)} unique reads", "",
                  "| exporter | route | median ms | min .. max ms | file bytes | of the text | members stored / fixed / dynamic |", "|---|---|---|---|---|---|---|"]
        for e in EXPORTERS:
            text = info[e, "plain"]["text"]
            for r in ROUTES:
                v, st = ts[e, r], info[e, r]
                if r == "plain":
                    size, forms = text, ""
                else:
                    size = sum(f["file_bytes"] for f in st["bgzf"])
                    forms = " / ".join(str(sum(f[k] for f in st["bgzf"])) for k in ("stored", "fixed", "dynamic")) if r == "device" else "(zlib's)"
                    for pg, pp in zip(paths[e, r], paths[e, "plain"]):  # the last round's files
                        with open(pg, "rb") as fg, open(pp, "rb") as fp:
                            assert gzip.decompress(fg.read()) == fp.read(), (e, r, pg)
                lines.append(f"| {e} | {r} | {statistics.median(v) * 1e3:.1f} | {min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f} | {size} | "
                             f"{size / max(text, 1):.3f} | {forms} |")
            dev, host = (sum(f["file_bytes"] for f in info[e, r]["bgzf"]) for r in ("device", "host"))
            lines.append(f"| {e} | device / host file bytes | | | {dev / max(host, 1):.2f} x | | |")
        lines.append("")
        shutil.rmtree(tmp)
        res.close(); uniq.close()
        print("\n".join(lines[shown:]), flush=True)
        shown = len(lines)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
