#!/usr/bin/env python3
"""Time ``--trimmed-out`` on the two synthetic FASTQ samples of tools/read_qc_time.py, held in host memory: ``--reads`` records (10 M) of 51 nt
and a second sample of 150-nt reads at the same byte count.

``--rounds`` rounds (one more in front that pays for first allocations), in every round one after the other on the same text: the parse + trim
call without a writer (``mirge_reads_parse_trim_out`` with ``fq == NULL``: the baseline), then the same call with a fresh writer -- ``plain``,
``gz`` deflated on the device, ``gz`` deflated by zlib on the host (MIRGE_BGZF_DEFLATE=host) -- including ``mirge_fqout_finish``.  Median
(min .. max), host wall clock around call + finish with the stream drained.  The files go to ``--dir`` and are removed after every call.  The
three files of a round are held against each other (the same decompressed bytes); the sizes and the member forms are reported, the host
route's file being the zlib level 6 figure.  Last, outside the timing, one pass per mode with the launches bracketed by events.

  python tools/trimmed_out_time.py --rounds 5 --out profiles/trimmed_out.md
"""
import argparse
import gzip
import hashlib
import os
import statistics
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
sys.path.insert(0, HERE)
import mirge3_amd  # noqa: E402,F401
from mirge3_amd import _ffi, trimmed_out  # noqa: E402
from mirge3_amd.collapse import ILLUMINA_3P  # noqa: E402
from read_qc_time import make_sample  # noqa: E402

MODES = (("plain", "plain", None), ("gz, device", "gz", "device"), ("gz, host", "gz", "host"))


def digest_of(path, gz):
    """SHA-1 and length of the file's (decompressed) bytes, read in pieces"""
    h, n = hashlib.sha1(), 0
    with (gzip.open(path, "rb") if gz else open(path, "rb")) as fh:  # (gzip reads member after member)
        for part in iter(lambda: fh.read(1 << 24), b""):
            h.update(part); n += len(part)
    return h.hexdigest(), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--templates", type=int, default=20_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dir", default=None, help="where the files are written (default: a temporary directory)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = _ffi.Context(0)
    rng = np.random.Generator(np.random.PCG64(2028))
    trim = _ffi.MirgeTrim.make(adapter=ILLUMINA_3P, quality_back=10, count_per_modifier=False)
    lines = ["# --trimmed-out on one MI355X (tools/trimmed_out_time.py)", "",
             f"`--reads {a.reads} --templates {a.templates} --rounds {a.rounds}`; -a {ILLUMINA_3P} -q 10 --minimum-length 16, counted once; the text is in host "
             "memory, every call uploads it; call + finish, files removed after every call.  Median s (min .. max) over the rounds, host wall clock, "
             "stream drained.", ""]
    n150 = a.reads * (2 * 51 + 7) // (2 * 150 + 7)
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        for label, n_reads, cycles in ((f"{a.reads} records of 51 nt", a.reads, 51), (f"{n150} records of 150 nt", n150, 150)):
            text = make_sample(rng, n_reads, cycles, a.templates)
            fig = {k: [] for k in ("fq == NULL",) + tuple(m[0] for m in MODES)}
            kernels, stats, digests = {}, {}, {}
            for rnd in range(a.rounds + 2):
                profiled = rnd == a.rounds + 1
                for key, mode, route in (("fq == NULL", None, None),) + MODES:
                    os.environ.pop("MIRGE_BGZF_DEFLATE", None)
                    if route:
                        os.environ["MIRGE_BGZF_DEFLATE"] = route
                    w = _ffi.TrimmedOut(ctx, d, "sample", mode) if mode else None
                    ctx.sync()
                    if profiled:
                        ctx.profile(True); ctx.profile_reset()
                    t = time.perf_counter()
                    raw, n_rec = _ffi.DeviceReads.parse_out(ctx, text, 1, 16, trim, None, w)
                    st = w.finish() if w is not None else None
                    ctx.sync()
                    dt = time.perf_counter() - t
                    if profiled:
                        kernels[key] = ctx.profile_records()
                        ctx.profile(False)
                    kept = len(raw)
                    raw.close()
                    if st is not None:
                        stats[key] = st
                        if rnd == 0:
                            digests[key] = digest_of(st["path"], mode == "gz")
                        os.remove(st["path"])
                        if mode == "gz":
                            os.remove(st["path"] + ".gzi")
                    if 0 < rnd <= a.rounds:
                        fig[key].append(dt)
            os.environ.pop("MIRGE_BGZF_DEFLATE", None)
            assert len(set(digests.values())) == 1 and stats["plain"]["written"] == kept, (digests, stats, kept)
            lines += [f"## {label} ({text.size / 1e6:.0f} MB of text; {n_rec} records, {kept} reads kept; the three files hold the same {digests['plain'][1]} bytes)", "",
                      trimmed_out.log_line("sample", stats["gz, device"], "gz"), "", "| figure | median s | min .. max | added to the call |", "|---|---|---|---|"]
            base = statistics.median(fig["fq == NULL"])
            for k, v in fig.items():
                m = statistics.median(v)
                lines.append(f"| {k} | {m:.4f} | {min(v):.4f} .. {max(v):.4f} | " + ("" if k == "fq == NULL" else f"{m - base:+.4f} s, {100 * (m / base - 1):+.0f} %") + " |")
            lines += ["", "| file | bytes | of the stream | members (stored, fixed, dynamic) |", "|---|---|---|---|"]
            for k, st in stats.items():
                lines.append(f"| {k}{' (zlib level 6 per member)' if k == 'gz, host' else ''} | {st['file_bytes']} | {100 * st['file_bytes'] / max(st['stream_bytes'], 1):.1f} % | "
                             f"{st['members']} ({st['stored']}, {st['fixed']}, {st['dynamic']}) |")
            lines += ["", "device time of the kernels of one more pass (event-bracketed launches, outside the timing), ms (launches):", ""]
            for what, recs in kernels.items():
                lines += [f"{what}:", "", "| kernel | ms | launches |", "|---|---|---|"]
                lines += [f"| {name} | {ms:.3f} | {launches} |" for name, launches, ms, _ in recs]
                lines += [f"| all | {sum(r[2] for r in recs):.3f} | {sum(r[1] for r in recs)} |", ""]
            del text
    text_out = "\n".join(lines)
    print(text_out)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text_out + "\n")


if __name__ == "__main__":
    main()
