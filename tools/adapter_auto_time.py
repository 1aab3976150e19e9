#!/usr/bin/env python3
"""Time ``-a auto`` on a synthetic sample: ``--reads`` FASTQ records (10 M) at ``--cycles`` (50) cycles, inserts of 18 .. 30 nt drawn
Zipf-like from ``--templates`` sequences, each followed by the Illumina small-RNA adapter and what follows it on a flow cell, every
letter substituted with probability ``--error`` (0.5 %).  The file is written to ``--dir`` (plain FASTQ, about 1.1 GB) and removed.

``--rounds`` rounds (one more in front that pays for first allocations), in every round one after the other: ``head_text`` (the first
MIRGE_ADAPTER_HEAD_READS records from the file), the head's parse + collapse (``mirge_reads_parse`` without trimming, ``mirge_collapse``),
``mirge_adapter_infer`` on that dictionary with the table filled by either form (MIRGE_ADAPTER_COUNT), and the sample's own parse + trim call (``mirge_reads_parse_trim`` of the whole text with the
adapter given).  Median (min .. max), host wall clock around each call.  Then, outside the timing, one more pass with the launches
bracketed by events: the device time of every kernel of the head's parse + collapse, of the ``k_ad_*`` kernels and of the sample's
parse + trim.

  python tools/adapter_auto_time.py --rounds 5 --out profiles/adapter_auto.md
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
import mirge3_amd  # noqa: E402,F401
from mirge3_amd import _ffi, adapter_auto  # noqa: E402
from mirge3_amd.collapse import ILLUMINA_3P  # noqa: E402

LETTERS = np.frombuffer(b"ACGT", np.uint8)
FORMS = ("sort", "atomic")  # how the table is filled: store-and-sum, or an atomic add and or per window
BEHIND = b"TCACATCACGATCTCGTATGCCGTCTTCTGCTTG" + b"A" * 64  # index, flow-cell oligo, poly-A


def write_sample(path, rng, n_reads, n_templates, error, cycles, chunk=1_000_000):
    """the FASTQ file, a million records at a time; -> the number of bytes"""
    lens = rng.integers(18, 31, size=n_templates)
    tpl = LETTERS[rng.integers(0, 4, size=(n_templates, max(30, cycles)))]  # (only a template's first letters are used)
    after = np.frombuffer(ILLUMINA_3P.encode() + BEHIND, np.uint8)
    pos = np.arange(cycles, dtype=np.int16)[None, :]
    total = 0
    with open(path, "wb") as fh:
        for lo in range(0, n_reads, chunk):
            n = min(chunk, n_reads - lo)
            which = np.minimum((rng.pareto(1.1, size=n) * 10).astype(np.int64), n_templates - 1)
            rel = pos - lens[which].astype(np.int16)[:, None]  # < 0: inside the insert
            reads = np.where(rel < 0, tpl[which][:, :cycles], after[np.clip(rel, 0, after.size - 1)])
            wrong = rng.random(reads.shape, dtype=np.float32) < error
            step = rng.integers(1, 4, size=reads.shape, dtype=np.uint8)
            reads = np.where(wrong, LETTERS[(np.searchsorted(LETTERS, reads) + step) % 4], reads).astype(np.uint8)
            rec = np.empty((n, 3 + cycles + 3 + cycles + 1), np.uint8)
            rec[:, 0:3] = np.frombuffer(b"@r\n", np.uint8)
            rec[:, 3:3 + cycles] = reads
            rec[:, 3 + cycles:6 + cycles] = np.frombuffer(b"\n+\n", np.uint8)
            rec[:, 6 + cycles:6 + 2 * cycles] = ord("I")
            rec[:, -1] = 10
            fh.write(rec.tobytes())
            total += rec.size
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--templates", type=int, default=20_000)
    ap.add_argument("--error", type=float, default=0.005)
    ap.add_argument("--cycles", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dir", default=None, help="where the FASTQ file is written (default: a temporary directory)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = _ffi.Context(0)
    rng = np.random.Generator(np.random.PCG64(2027))
    head_n = adapter_auto.head_reads()
    trim = _ffi.MirgeTrim.make(adapter=ILLUMINA_3P, quality_back=10)
    fig = {k: [] for k in ("head_text_s", "head_parse_collapse_s") + tuple(f"adapter_infer_{f}_s" for f in FORMS) + ("sample_parse_trim_s",)}
    kernels, found = {}, {}
    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        path = os.path.join(tmp, "sample.fastq")
        size = write_sample(path, rng, a.reads, a.templates, a.error, a.cycles)
        text = np.fromfile(path, dtype=np.uint8)
        for rnd in range(a.rounds + 2):
            profiled = rnd == a.rounds + 1  # (outside the timing)
            tm = {}
            t = time.perf_counter()
            head = adapter_auto.head_text(path, head_n)
            tm["head_text_s"] = time.perf_counter() - t
            if profiled:
                ctx.profile(True); ctx.profile_reset()
            t = time.perf_counter()
            raw, n_rec = _ffi.DeviceReads.parse(ctx, head, 1, 0, None)
            d0 = raw.collapse()
            ctx.sync()
            tm["head_parse_collapse_s"] = time.perf_counter() - t
            if profiled:
                kernels["head parse + collapse"] = ctx.profile_records()
                ctx.profile_reset()
            for form in FORMS:  # (MIRGE_ADAPTER_COUNT is read per call: both forms in every round)
                os.environ["MIRGE_ADAPTER_COUNT"] = form
                t = time.perf_counter()
                res = d0.adapter_infer()
                tm[f"adapter_infer_{form}_s"] = time.perf_counter() - t
                if profiled:
                    kernels[f"mirge_adapter_infer, MIRGE_ADAPTER_COUNT={form}"] = ctx.profile_records()
                    ctx.profile_reset()
                found[form] = res
            del os.environ["MIRGE_ADAPTER_COUNT"]
            assert found["sort"] == found["atomic"]
            info = dict(res, records=n_rec, distinct=len(d0))
            d0.close(); raw.close()
            t = time.perf_counter()
            whole, n_all = _ffi.DeviceReads.parse(ctx, text, 1, 16, trim)
            ctx.sync()
            tm["sample_parse_trim_s"] = time.perf_counter() - t
            if profiled:
                kernels["sample parse + trim"] = ctx.profile_records()
                ctx.profile(False)
            kept = len(whole)
            whole.close()
            if 0 < rnd <= a.rounds:
                for k in fig:
                    fig[k].append(tm[k])
    lines = ["# -a auto on one MI355X (tools/adapter_auto_time.py)", "",
             f"`--reads {a.reads} --templates {a.templates} --error {a.error} --cycles {a.cycles} --rounds {a.rounds}`, "
             f"MIRGE_ADAPTER_HEAD_READS = {head_n}, FASTQ text {size / 1e6:.0f} MB, head {len(head) / 1e6:.1f} MB", "",
             f"planted `{ILLUMINA_3P}`, inferred `{info['seq']}` (" + ", ".join(f"{k} = {v}" for k, v in info.items() if k != "seq") + ")", "",
             f"the sample's parse + trim call: {n_all} records, {kept} reads kept (counted per modifier of the chain)", "",
             "| figure | median s | min .. max |", "|---|---|---|"]
    for k, v in fig.items():
        lines.append(f"| {k} | {statistics.median(v):.4f} | {min(v):.4f} .. {max(v):.4f} |")
    lines += ["", "device time of the kernels of one more pass (event-bracketed launches, outside the timing), ms (launches):", ""]
    for what, recs in kernels.items():
        lines += [f"{what}:", "", "| kernel | ms | launches |", "|---|---|---|"]
        lines += [f"| {name} | {ms:.3f} | {launches} |" for name, launches, ms, _ in recs]
        lines += [f"| all | {sum(r[2] for r in recs):.3f} | {sum(r[1] for r in recs)} |", ""]
    text_out = "\n".join(lines)
    print(text_out)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text_out)


if __name__ == "__main__":
    main()
