#!/usr/bin/env python3
"""File sizes of ``--sorted-bam``'s device routes on the CPU, exact: ``csrc/kernels_bam.hpp`` compiled for the host
(tests/hostsim/bam_sim.cpp) writes the device's bytes.  Two synthetic streams of about ``--records`` records each, drawn as
``tools/sorted_bam_time.py`` draws its samples (Zipf counts over a tenth as many unique reads; all-distinct), annotated by the oracle's
cascade.  Printed per stream: the file under ``deflate`` 1 (device), 2 (dynamic) and 3 (tight), under zlib level 6 on the same blocks
(what ``MIRGE_BAM_DEFLATE=host`` writes), the tight file's members by form, and what each ingredient of the tight parse buys: the
harness is rebuilt with the build knobs of ``kernels_bam.hpp`` (``-DMIRGE_BAM_TIGHT_...``), one ingredient more per row.

  python tools/bam_parse_sizes.py --records 9000
"""
import argparse
import os
import subprocess
import sys
import zlib

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [os.path.join(ROOT, "tools"), ROOT, os.path.join(ROOT, "tests")]
import mirge3_amd  # noqa: E402,F401
import oracle  # noqa: E402
from mirge3_amd.cascade import PASSES  # noqa: E402
from mirge3_amd.seqio import FlatSeqs  # noqa: E402
from sam_out_time import libraries, unique_reads  # noqa: E402
import test_sorted_bam_hostsim as hostsim  # noqa: E402

BLOCK = 65280
ROWS = [("matches may cross segment ends", dict(RECORD=0, REPEAT=0, REGIONS=0, LAZY=0)),
        ("+ record-aligned candidates", dict(RECORD=1, REPEAT=0, REGIONS=0, LAZY=0)),
        ("+ repeat distance", dict(RECORD=1, REPEAT=1, REGIONS=0, LAZY=0)),
        ("+ region tables, look-back 0", dict(RECORD=1, REPEAT=1, REGIONS=1, LAZY=0, LOOKBACK=0)),
        ("+ region tables, look-back 1", dict(RECORD=1, REPEAT=1, REGIONS=1, LAZY=0, LOOKBACK=1)),
        ("+ region tables, look-back 2", dict(RECORD=1, REPEAT=1, REGIONS=1, LAZY=0, LOOKBACK=2)),
        ("+ lazy step below 32, look-back 0", dict(RECORD=1, REPEAT=1, REGIONS=1, LAZY=1, LOOKBACK=0)),
        ("+ lazy step below 32, look-back 1", dict(RECORD=1, REPEAT=1, REGIONS=1, LAZY=1, LOOKBACK=1)),
        ("+ lazy step below 32, look-back 2 (the route as built)", dict(RECORD=1, REPEAT=1, REGIONS=1, LAZY=1, LOOKBACK=2)),
        ("the route with a lazy step below 258", dict(LAZY_BELOW=258))]


def harness(knobs):
    """the host harness built with these knobs (tools/tmp/, rebuilt when a source is newer) becomes the one hostsim.run loads"""
    tag = "_".join(f"{k}{v}" for k, v in sorted(knobs.items())) or "default"
    so = os.path.join(ROOT, "tools", "tmp", f"libbamsim_{tag}.so")
    csrc = os.path.join(ROOT, "mirge3.0_amd", "csrc")
    deps = [hostsim.SRC, os.path.join(csrc, "kernels_sam.hpp"), os.path.join(csrc, "kernels_bam.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        flags = [f"-DMIRGE_BAM_TIGHT_{k}={v}" for k, v in knobs.items()]
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-pthread"] + flags + ["-o", so, hostsim.SRC])
    hostsim.SO = so


def members_by_btype(members):
    out, at = [0, 0, 0], 0
    while at < len(members):
        out[(members[at + 18] >> 1) & 3] += 1
        at += (members[at + 16] | (members[at + 17] << 8)) + 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=9000, help="records per stream (about 110 bytes each)")
    a = ap.parse_args()
    rng = np.random.Generator(np.random.PCG64(5))
    libs = libraries(rng)
    header = ("@HD\tVN:1.0\n" + "".join(f"@SQ\tSN:chr{k}\tLN:{1 << 28}\n" for k in range(1, 23))).encode()
    olibs = [(libs[PASSES[p][1]].seqs.data, libs[PASSES[p][1]].seqs.offsets) for p in range(9)]
    for shape in ("zipf", "distinct"):
        n_u = max(1, a.records // 10) if shape == "zipf" else a.records
        reads = unique_reads(rng, libs, n_u)
        if shape == "zipf":
            w = 1.0 / np.arange(1, n_u + 1) ** 1.1
            cnt = np.maximum(1, np.floor(w / w.sum() * a.records)).astype(np.uint32)
            rng.shuffle(cnt)
        else:
            cnt = np.ones(n_u, dtype=np.uint32)
        fr = FlatSeqs.from_list(reads)
        ann = oracle.cascade(fr.data, fr.offsets, olibs, n_pass=9, indexed=True)
        args = (libs, reads, *ann, cnt.reshape(-1, 1), np.arange(n_u), 0, header, BLOCK)
        harness({})
        stream, n_rec = hostsim.run(*args, 0)
        z6 = 28
        for at in range(0, len(stream), BLOCK):
            z = zlib.compressobj(6, zlib.DEFLATED, -15)
            z6 += 26 + len(z.compress(stream[at:at + BLOCK]) + z.flush())
        print(f"## {shape}: {n_u} unique reads, {n_rec} records, stream {len(stream)} B in {-(-len(stream) // BLOCK)} blocks; zlib level 6 on the blocks: {z6} B")
        print("| parse | file | against zlib 6 | members stored / fixed / dynamic |\n|---|---|---|---|")
        for name, deflate in (("`device` (deflate 1)", 1), ("`dynamic` (deflate 2)", 2), ("`tight` (deflate 3)", 3)):
            members, _ = hostsim.run(*args, deflate)
            print(f"| {name} | {len(members) + 28} B | {(len(members) + 28) / z6:.3f} x | {' / '.join(map(str, members_by_btype(members)))} |")
        for name, knobs in ROWS:
            harness(knobs)
            members, _ = hostsim.run(*args, 3)
            print(f"| tight: {name} | {len(members) + 28} B | {(len(members) + 28) / z6:.3f} x | {' / '.join(map(str, members_by_btype(members)))} |")
        print(flush=True)


if __name__ == "__main__":
    main()
