#!/usr/bin/env python3
"""Time ``--kmer-correct`` on a synthetic sample with known truth: ``--reads`` raw reads (10 M) drawn Zipf-like from ``--templates``
miRNA-like sequences of 18 .. 26 nt, every letter of every read substituted with probability ``--error`` (0.5 %).  One read per line,
no adapters.  k = ``--ks`` .. ``--ke`` (15 .. 20), H = ``--kh`` (5).

``--rounds`` rounds (one more in front that pays for first allocations), in every round one after the other: the sample's parse call
(``mirge_reads_parse``), its collapse + cascade call (``mirge_collapse_cascade`` against bench.py's synthetic libraries, ``synth.make_libraries``),
and ``mirge_kmer_correct`` alone on the sample's dictionary.  Median (min .. max), host wall clock around each call.  Then, outside
the timing: per round of k the table's slots and the suspect share, distinct reads before and after, the share of raw reads with a
planted error that end as their template, and the share of error-free raw reads that were changed (false corrections).

  python tools/kmer_correct_time.py --rounds 5 --out profiles/kmer_correct.md
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

LETTERS = np.frombuffer(b"ACGT", np.uint8)
WIDTH = 26


def sample(rng, n_reads, n_templates, error):
    """-> (text, the reads as NUL-padded rows [n, WIDTH], the same for each read's template, has a planted error [n])"""
    lens = rng.integers(18, WIDTH + 1, size=n_templates)
    tpl = LETTERS[rng.integers(0, 4, size=(n_templates, WIDTH))]
    tpl[np.arange(WIDTH)[None, :] >= lens[:, None]] = 0
    which = np.minimum((rng.pareto(1.1, size=n_reads) * 10).astype(np.int64), n_templates - 1)
    truth = tpl[which]
    wrong = (rng.random(truth.shape, dtype=np.float32) < error) & (truth != 0)
    code = np.searchsorted(LETTERS, truth)  # (padding: 0, unused)
    step = rng.integers(1, 4, size=truth.shape, dtype=np.uint8)
    reads = np.where(wrong, LETTERS[(code + step) % 4], truth).astype(np.uint8)
    lines = np.concatenate([reads, np.full((n_reads, 1), 10, np.uint8)], axis=1).reshape(-1)
    return lines[lines != 0], reads, truth, wrong.any(axis=1)


def rows_of(seqs):
    """FlatSeqs -> NUL-padded rows as fixed-width byte strings"""
    mat = np.zeros((len(seqs), WIDTH), np.uint8)
    rows = np.repeat(np.arange(len(seqs), dtype=np.int64), seqs.lengths)
    mat[rows, np.arange(int(seqs.offsets[-1]), dtype=np.int64) - seqs.offsets[:-1][rows]] = seqs.data
    return mat.view(f"S{WIDTH}").reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--templates", type=int, default=20_000)
    ap.add_argument("--error", type=float, default=0.005)
    ap.add_argument("--ks", type=int, default=15)
    ap.add_argument("--ke", type=int, default=20)
    ap.add_argument("--kh", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", default="full", choices=["ci", "small", "full"], help="size of the synthetic libraries of the cascade")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = _ffi.Context(0)
    rng = np.random.Generator(np.random.PCG64(2026))
    text, reads, truth, planted = sample(rng, a.reads, a.templates, a.error)
    casc = Cascade(ctx, synth.make_libraries(seed=20260101, scale=a.scale).libs)  # (bench.py's libraries)
    fig = {k: [] for k in ("parse_s", "collapse_cascade_s", "kmer_correct_s")}
    info, per_k = {}, []
    for rnd in range(a.rounds + 1):
        tm = {}
        t = time.perf_counter()
        raw, _ = _ffi.DeviceReads.parse(ctx, text, 3, 16, None)
        ctx.sync()
        tm["parse_s"] = time.perf_counter() - t
        if rnd == 0:
            casc.prepare(raw)
        d0 = raw.collapse()
        ctx.sync()
        t = time.perf_counter()
        out, final_of, masks = d0.kmer_correct(a.ks, a.ke, a.kh)
        tm["kmer_correct_s"] = time.perf_counter() - t
        stats = _ffi.kmer_correct_stats()
        t = time.perf_counter()
        uniq, res = casc.collapse_and_run(raw)
        ctx.sync()
        tm["collapse_cascade_s"] = time.perf_counter() - t
        res.close(); uniq.close()
        if rnd == a.rounds:  # (outside the timing) what the correction did, against the truth
            before, after = rows_of(d0.unpack()), rows_of(out.unpack())
            order = np.argsort(before)
            handle = order[np.searchsorted(before[order], reads.view(f"S{WIDTH}").reshape(-1))]
            assert len(raw) == a.reads and np.array_equal(before[handle], reads.view(f"S{WIDTH}").reshape(-1))  # every raw read found its dictionary entry
            final = after[final_of[handle]]
            is_template = final == truth.view(f"S{WIDTH}").reshape(-1)
            changed = final != reads.view(f"S{WIDTH}").reshape(-1)
            info = dict(raw_reads=a.reads, raw_reads_with_a_planted_error=int(planted.sum()), distinct_before=len(d0), distinct_after=len(out),
                        distinct_reads_changed=int((masks != 0).sum()),
                        planted_errors_restored_share=round(float(is_template[planted].mean()), 4),
                        planted_errors_changed_to_something_else_share=round(float((changed & ~is_template)[planted].mean()), 4),
                        error_free_reads_changed_share=round(float(changed[~planted].mean()), 6))
            per_k = stats
        out.close(); d0.close(); raw.close()
        if rnd:
            for k in fig:
                fig[k].append(tm[k])
    lines = ["# --kmer-correct on one MI355X (tools/kmer_correct_time.py)", "",
             f"`--reads {a.reads} --templates {a.templates} --error {a.error} --ks {a.ks} --ke {a.ke} --kh {a.kh} --rounds {a.rounds}`", "",
             ", ".join(f"{k} = {v}" for k, v in info.items()), "",
             "| figure | median s | min .. max |", "|---|---|---|"]
    for k, v in fig.items():
        lines.append(f"| {k} | {statistics.median(v):.4f} | {min(v):.4f} .. {max(v):.4f} |")
    lines += ["", "| k | table slots | eligible | suspect | suspect share | corrected | uncorrectable | unsupported | ambiguous | distinct after |",
              "|---|---|---|---|---|---|---|---|---|---|"]
    for r, st in enumerate(per_k):
        share = st["suspect"] / st["eligible"] if st["eligible"] else 0.0
        lines.append(f"| {a.ks + r} | {st['slots']} | {st['eligible']} | {st['suspect']} | {share:.4f} | {st['corrected']} | {st['uncorrectable']} | "
                     f"{st['unsupported']} | {st['ambiguous']} | {st['distinct']} |")
    lines.append("")
    text_out = "\n".join(lines)
    print(text_out)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text_out)


if __name__ == "__main__":
    main()
