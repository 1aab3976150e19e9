#!/usr/bin/env python3
"""Time ``--unmapped-nearest``'s device call on one MI355X: ``mirge_nearest_unmapped`` at 10^5 and 10^6 synthetic unannotated unique reads of
16 to 40 nt against a hairpin library of 1 900 x 85 nt (the size of human miRBase), beside the same sample's collapse + cascade call.

The reads: half are stretches of the hairpins with 0 to 3 substituted letters, half random; none is known to the cascade's libraries (the
synthetic ``ci`` set), so every unique read is a query.  The scan is brute force, so its time does not depend on what the reads hold.
``--rounds`` rounds (one more in front that pays for first allocations), in every round one after the other on the same dictionaries: the
collapse + cascade call, ``mirge_nearest_unmapped`` as the run calls it, and the same with MIRGE_NEAR_FORCE64=1; and on a third dictionary of
10^5 reads of 16 to 32 nt, which all run in the 32-bit instance, both again: the two instances on the same queries.  Median (min .. max),
host wall clock around each call with the stream drained.  Last, outside the timing, one pass per dictionary with the launches bracketed
by events: the device time of every kernel.  No genome is at hand here, so ``--unmapped-clusters`` is not timed beside it.

  python tools/nearest_time.py --rounds 5 --out profiles/nearest.md
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
from mirge3_amd import _ffi, synth  # noqa: E402
from mirge3_amd.cascade import Cascade  # noqa: E402
from mirge3_amd.seqio import FlatSeqs  # noqa: E402

LETTERS = np.frombuffer(b"ACGT", np.uint8)


def make_reads(rng, n, lo, hi, lib_data, lib_len):
    """n distinct-looking reads of lo .. hi nt as FlatSeqs: the first half stretches of the library with 0 to 3 substitutions"""
    lens = rng.integers(lo, hi + 1, size=n).astype(np.int64)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    data = LETTERS[rng.integers(0, 4, size=int(off[-1]))]
    half = n // 2
    n_h = lib_data.size // lib_len
    src = rng.integers(0, n_h, size=half) * lib_len + rng.integers(0, lib_len - hi + 1, size=half)
    index = np.repeat(src - off[:half], lens[:half]) + np.arange(int(off[half]), dtype=np.int64)
    data[:int(off[half])] = lib_data[index]
    for _ in range(3):
        hit = np.flatnonzero(rng.random(half) < 0.6)
        at = off[hit] + (rng.random(hit.size) * lens[hit]).astype(np.int64)
        data[at] = LETTERS[rng.integers(0, 4, size=hit.size)]
    return FlatSeqs(data, off)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--hairpins", type=int, default=1900)
    ap.add_argument("--hairpin-length", type=int, default=85)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("-K", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = _ffi.Context(0)
    rng = np.random.Generator(np.random.PCG64(2031))
    casc = Cascade(ctx, synth.make_libraries(seed=5, scale="ci").libs)
    lib_data = LETTERS[rng.integers(0, 4, size=a.hairpins * a.hairpin_length)]
    targets = FlatSeqs(lib_data, np.arange(a.hairpins + 1, dtype=np.int64) * a.hairpin_length)
    sets = [(f"{n} reads of 16 .. 40 nt", n, 16, 40) for n in (int(x) for x in a.sizes.split(","))]
    sets.append((f"{int(a.sizes.split(',')[0])} reads of 16 .. 32 nt (all in the 32-bit instance)", int(a.sizes.split(",")[0]), 16, 32))
    lines = ["# --unmapped-nearest on one MI355X (tools/nearest_time.py)", "",
             f"`--sizes {a.sizes} --hairpins {a.hairpins} --hairpin-length {a.hairpin_length} --rounds {a.rounds} -K {a.K}`: {a.hairpins * a.hairpin_length} "
             "library bases.  Median s (min .. max) over the rounds, host wall clock, stream drained; the rounds interleave the calls.", ""]
    medians = {}
    for label, n, lo, hi in sets:
        reads = make_reads(rng, n, lo, hi, lib_data, a.hairpin_length)
        fig = {"collapse + cascade": [], "mirge_nearest_unmapped": [], "mirge_nearest_unmapped, MIRGE_NEAR_FORCE64=1": []}
        kernels, stats, uniq, res = None, None, None, None
        for rnd in range(a.rounds + 2):
            profiled = rnd == a.rounds + 1
            raw = _ffi.DeviceReads.pack(ctx, reads)
            ctx.sync()
            t = time.perf_counter()
            u, r = casc.collapse_and_run(raw)
            ctx.sync()
            t_casc = time.perf_counter() - t
            raw.close()
            if uniq is not None:
                res.close(); uniq.close()
            uniq, res = u, r
            tm = {"collapse + cascade": t_casc}
            for force in (None, "1"):
                os.environ.pop("MIRGE_NEAR_FORCE64", None)
                if force:
                    os.environ["MIRGE_NEAR_FORCE64"] = force
                if profiled:
                    if force:
                        continue
                    ctx.profile(True); ctx.profile_reset()
                ctx.sync()
                t = time.perf_counter()
                got, st = _ffi.nearest_unmapped(ctx, uniq, res, targets, a.K)
                ctx.sync()
                tm["mirge_nearest_unmapped" + (", MIRGE_NEAR_FORCE64=1" if force else "")] = time.perf_counter() - t
                if profiled:
                    kernels = ctx.profile_records()
                    ctx.profile(False)
                stats = stats or st
                assert st == stats  # the same numbers in every round ...
                if force is None:
                    first = got
                else:  # ... and the same rows from either instance (on one dictionary: a collapse orders its rows as it likes)
                    assert all(np.array_equal(got[k], first[k]) for k in got)
            os.environ.pop("MIRGE_NEAR_FORCE64", None)
            if 0 < rnd <= a.rounds:
                for k in fig:
                    fig[k].append(tm[k])
        cols = stats["considered"] * a.hairpins * a.hairpin_length
        lines += [f"## {label}", "", f"{len(uniq)} unique reads; " + ", ".join(f"{k} {v}" for k, v in stats.items()) + f"; {cols:.3e} column steps", "",
                  "| call | median s | min .. max | column steps / s |", "|---|---|---|---|"]
        for k, v in fig.items():
            med = statistics.median(v)
            medians[(label, k)] = (med, min(v), max(v))
            lines.append(f"| {k} | {med:.4f} | {min(v):.4f} .. {max(v):.4f} | {(cols / med):.3e} |" if "nearest" in k else f"| {k} | {med:.4f} | {min(v):.4f} .. {max(v):.4f} | |")
        lines += ["", "device time of the kernels of one more call (event-bracketed launches, outside the timing), ms (launches):", "",
                  "| kernel | ms | launches |", "|---|---|---|"]
        lines += [f"| {name} | {ms:.3f} | {launches} |" for name, launches, ms, _ in kernels]
        lines += [f"| all | {sum(r[2] for r in kernels):.3f} | {sum(r[1] for r in kernels)} |", ""]
        res.close(); uniq.close()
    # the two expectations
    small, big, narrow = (s[0] for s in sets)
    m32, m64 = medians[(narrow, "mirge_nearest_unmapped")], medians[(narrow, "mirge_nearest_unmapped, MIRGE_NEAR_FORCE64=1")]
    overlap = m32[1] <= m64[2] and m64[1] <= m32[2]
    lines += ["## The two expectations", "",
              f"1. The 32-bit instance against the 64-bit instance on the same queries of at most 32 nt: {m32[0]:.4f} s ({m32[1]:.4f} .. {m32[2]:.4f}) against "
              f"{m64[0]:.4f} s ({m64[1]:.4f} .. {m64[2]:.4f}): the ranges {'overlap' if overlap else 'do not overlap'}; the 32-bit instance is "
              f"{'not slower' if m32[0] <= m64[0] else 'SLOWER'} by the medians ({m64[0] / m32[0]:.2f} x).",
              f"2. From {small} to {big}: {medians[(small, 'mirge_nearest_unmapped')][0]:.4f} s to {medians[(big, 'mirge_nearest_unmapped')][0]:.4f} s, "
              f"{medians[(big, 'mirge_nearest_unmapped')][0] / medians[(small, 'mirge_nearest_unmapped')][0]:.2f} x the time for "
              f"{int(big.split()[0]) / int(small.split()[0]):.0f} x the reads.", ""]
    text_out = "\n".join(lines)
    print(text_out)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text_out + "\n")


if __name__ == "__main__":
    main()
