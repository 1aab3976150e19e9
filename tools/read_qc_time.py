#!/usr/bin/env python3
"""Time ``--read-qc`` on two synthetic FASTQ samples held in host memory: ``--reads`` records (10 M) of 51 nt -- an insert of 18 .. 30 nt,
the Illumina small-RNA adapter and what follows it --, and a second sample of 150-nt reads at the same byte count.  Qualities look like a
sequencer's: most bases at one high value, a minority lower, falling towards the 3' end.

``--rounds`` rounds (one more in front that pays for first allocations), in every round one after the other on the same text: the parse +
trim call without an accumulator (``mirge_reads_parse_trim``: the baseline), then ``mirge_reads_parse_trim_qc`` with a fresh accumulator in
either form of the text histogram (MIRGE_QC_FORM=pos, read).  Median (min .. max), host wall clock around each call with the stream
drained.  Then the sample's collapse and cascade once, and per round the count join (``mirge_count_join``) and the class profile
(``mirge_qc_class_profile``) of that dictionary.  Last, outside the timing, one pass per form with the launches bracketed by events: the
device time of every kernel of the call.

  python tools/read_qc_time.py --rounds 5 --out profiles/read_qc.md
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
import mirge3_amd  # noqa: E402,F401
from mirge3_amd import _ffi, readqc, synth  # noqa: E402
from mirge3_amd.cascade import Cascade, EXACT_PASS, ISO_PASS  # noqa: E402
from mirge3_amd.collapse import ILLUMINA_3P  # noqa: E402

LETTERS = np.frombuffer(b"ACGT", np.uint8)
BEHIND = b"TCACATCACGATCTCGTATGCCGTCTTCTGCTTG" + b"A" * 200
FORMS = ("pos", "read")


def make_sample(rng, n_reads, cycles, n_templates, chunk=1_000_000):
    """the FASTQ text as one uint8 array"""
    lens = rng.integers(18, 31, size=n_templates) if cycles < 100 else rng.integers(60, 140, size=n_templates)
    tpl = LETTERS[rng.integers(0, 4, size=(n_templates, cycles))]
    after = np.frombuffer(ILLUMINA_3P.encode() + BEHIND, np.uint8)
    pos = np.arange(cycles, dtype=np.int16)[None, :]
    width = 3 + cycles + 3 + cycles + 1
    out = np.empty((n_reads, width), np.uint8)
    for lo in range(0, n_reads, chunk):
        n = min(chunk, n_reads - lo)
        which = np.minimum((rng.pareto(1.1, size=n) * 10).astype(np.int64), n_templates - 1)
        rel = pos - lens[which].astype(np.int16)[:, None]
        reads = np.where(rel < 0, tpl[which], after[np.clip(rel, 0, after.size - 1)])
        # qualities: 88 % at 40 ('I'), the rest between 2 and 37, more of them towards the 3' end
        u = rng.random((n, cycles), dtype=np.float32)
        low = u < (0.04 + 0.16 * np.arange(cycles, dtype=np.float32) / cycles)[None, :]
        q = np.where(low, 35 + (u * 3000).astype(np.int32) % 36, 73).astype(np.uint8)
        rec = out[lo:lo + n]
        rec[:, 0:3] = np.frombuffer(b"@r\n", np.uint8)
        rec[:, 3:3 + cycles] = reads
        rec[:, 3 + cycles:6 + cycles] = np.frombuffer(b"\n+\n", np.uint8)
        rec[:, 6 + cycles:6 + 2 * cycles] = q
        rec[:, -1] = 10
    return out.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--templates", type=int, default=20_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = _ffi.Context(0)
    rng = np.random.Generator(np.random.PCG64(2028))
    trim = _ffi.MirgeTrim.make(adapter=ILLUMINA_3P, quality_back=10, count_per_modifier=False)
    casc = Cascade(ctx, synth.make_libraries(seed=5, scale="ci").libs)
    n_mirna = len(casc.libs["mirna"])
    lines = ["# --read-qc on one MI355X (tools/read_qc_time.py)", "",
             f"`--reads {a.reads} --templates {a.templates} --rounds {a.rounds}`; -a {ILLUMINA_3P} -q 10 --minimum-length 16, counted once; the text is in host "
             "memory, every call uploads it.  Median s (min .. max) over the rounds, host wall clock, stream drained.", ""]
    n150 = a.reads * (2 * 51 + 7) // (2 * 150 + 7)
    for label, n_reads, cycles in ((f"{a.reads} records of 51 nt", a.reads, 51), (f"{n150} records of 150 nt", n150, 150)):
        text = make_sample(rng, n_reads, cycles, a.templates)
        fig = {k: [] for k in ("parse_trim_s (qc == NULL)",) + tuple(f"parse_trim_qc_s, {f}" for f in FORMS)}
        kernels, tables = {}, {}
        for rnd in range(a.rounds + 2):
            profiled = rnd == a.rounds + 1
            tm = {}
            for what in (None,) + FORMS:
                if what is not None:
                    os.environ["MIRGE_QC_FORM"] = what
                qc = _ffi.ReadQc(ctx) if what is not None else None
                ctx.sync()
                if profiled:
                    ctx.profile(True); ctx.profile_reset()
                t = time.perf_counter()
                raw, n_rec = _ffi.DeviceReads.parse_qc(ctx, text, 1, 16, trim, qc) if qc is not None else _ffi.DeviceReads.parse(ctx, text, 1, 16, trim)
                ctx.sync()
                tm["parse_trim_s (qc == NULL)" if what is None else f"parse_trim_qc_s, {what}"] = time.perf_counter() - t
                if profiled:
                    kernels["qc == NULL" if what is None else f"MIRGE_QC_FORM={what}"] = ctx.profile_records()
                    ctx.profile(False)
                kept = len(raw)
                if what is not None:
                    tables[what] = qc.fetch()[0]
                    qc.close()
                if what != FORMS[-1] or rnd <= a.rounds:
                    raw.close()
            os.environ.pop("MIRGE_QC_FORM", None)
            assert np.array_equal(tables["pos"], tables["read"])
            if 0 < rnd <= a.rounds:
                for k in fig:
                    fig[k].append(tm[k])
        e = readqc.sample_entries(tables["pos"], True)
        lines += [f"## {label} ({text.size / 1e6:.0f} MB of text; {n_rec} records, {kept} reads kept; both forms gave the same tables)", "",
                  readqc.log_line("sample", e), "", "| figure | median s | min .. max |", "|---|---|---|"]
        for k, v in fig.items():
            lines.append(f"| {k} | {statistics.median(v):.4f} | {min(v):.4f} .. {max(v):.4f} |")
        base = statistics.median(fig["parse_trim_s (qc == NULL)"])
        for f in FORMS:
            lines.append(f"| added by the flag, {f} | {statistics.median(fig[f'parse_trim_qc_s, {f}']) - base:+.4f} | "
                         f"{100 * (statistics.median(fig[f'parse_trim_qc_s, {f}']) / base - 1):+.1f} % of the call |")
        # the class profile beside the count join, on this sample's dictionary (`raw` of the last pass is still open)
        uniq, res = casc.collapse_and_run(raw)
        ctx.sync()
        jt = {"count_join_s": [], "class_profile_s": []}
        for rnd in range(a.rounds + 1):
            t = time.perf_counter()
            _ffi.count_join(ctx, uniq, res, EXACT_PASS, ISO_PASS, n_mirna)
            t1 = time.perf_counter()
            prof = _ffi.qc_class_profile(ctx, uniq, res)
            t2 = time.perf_counter()
            if rnd:
                jt["count_join_s"].append(t1 - t); jt["class_profile_s"].append(t2 - t1)
        assert int(prof[..., 0].sum()) == kept
        ctx.profile(True); ctx.profile_reset()
        _ffi.qc_class_profile(ctx, uniq, res)
        kernels["mirge_qc_class_profile"] = ctx.profile_records()
        ctx.profile(False)
        lines += ["", f"dictionary: {len(uniq)} unique reads", "", "| figure | median s | min .. max |", "|---|---|---|"]
        for k, v in jt.items():
            lines.append(f"| {k} | {statistics.median(v):.5f} | {min(v):.5f} .. {max(v):.5f} |")
        lines += ["", "device time of the kernels of one more pass (event-bracketed launches, outside the timing), ms (launches):", ""]
        for what, recs in kernels.items():
            lines += [f"{what}:", "", "| kernel | ms | launches |", "|---|---|---|"]
            lines += [f"| {name} | {ms:.3f} | {launches} |" for name, launches, ms, _ in recs]
            lines += [f"| all | {sum(r[2] for r in recs):.3f} | {sum(r[1] for r in recs)} |", ""]
        res.close(); uniq.close(); raw.close()
        del text
    text_out = "\n".join(lines)
    print(text_out)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text_out + "\n")


if __name__ == "__main__":
    main()
