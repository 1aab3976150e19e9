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

``--ratio R`` (may be given several times): in every round, behind the call without a ratio, ``mirge_kmer_correct_ratio`` with each R on
the same dictionary (interleaved: a round holds one call of each); the report then carries a time, the shares against the truth and per
round of k the k-mers above H and the dominated among them for every R, and -- from one more call each with the launches bracketed by
events, outside the timing -- the device time of every ``k_ec_*`` kernel.

  python tools/kmer_correct_time.py --rounds 5 --ratio 8 --ratio 50 --out profiles/kmer_ratio.md
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
    ap.add_argument("--ratio", type=int, action="append", default=[], help="also time mirge_kmer_correct_ratio with this R (repeatable)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = _ffi.Context(0)
    rng = np.random.Generator(np.random.PCG64(2026))
    text, reads, truth, planted = sample(rng, a.reads, a.templates, a.error)
    casc = Cascade(ctx, synth.make_libraries(seed=20260101, scale=a.scale).libs)  # (bench.py's libraries)
    fig = {k: [] for k in ("parse_s", "collapse_cascade_s", "kmer_correct_s")}
    info, per_k = {}, []
    ratio_s = {R: [] for R in a.ratio}
    ratio_info, ratio_per_k, kernel_ms = {}, {}, {}
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
        for R in a.ratio:
            t = time.perf_counter()
            o2, _, _ = d0.kmer_correct(a.ks, a.ke, a.kh, ratio=R)
            tm[R] = time.perf_counter() - t
            o2.close()
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
            for R in a.ratio:  # the same against the truth for every ratio, and the kernels' device times
                o2, f2, m2 = d0.kmer_correct(a.ks, a.ke, a.kh, ratio=R)
                ratio_per_k[R] = list(zip(_ffi.kmer_correct_stats(), _ffi.kmer_correct_ratio_stats()))
                fin2 = rows_of(o2.unpack())[f2[handle]]
                tpl2, chg2 = fin2 == truth.view(f"S{WIDTH}").reshape(-1), fin2 != reads.view(f"S{WIDTH}").reshape(-1)
                ratio_info[R] = dict(distinct_after=len(o2), distinct_reads_changed=int((m2 != 0).sum()),
                                     planted_errors_restored_share=round(float(tpl2[planted].mean()), 4),
                                     planted_errors_changed_to_something_else_share=round(float((chg2 & ~tpl2)[planted].mean()), 4),
                                     error_free_reads_changed_share=round(float(chg2[~planted].mean()), 6))
                o2.close()
            for R in ([0] + a.ratio if a.ratio else []):
                ctx.profile(True); ctx.profile_only("k_ec_"); ctx.profile_reset()
                o2, _, _ = d0.kmer_correct(a.ks, a.ke, a.kh, ratio=R)
                ctx.sync()
                kernel_ms[R] = {name: (launches, ms) for name, launches, ms, _ in ctx.profile_records()}
                ctx.profile(False); ctx.profile_only("")
                o2.close()
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
            for R in a.ratio:
                ratio_s[R].append(tm[R])
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
    if a.ratio:
        lines += ["", "## --kmer-ratio", "", "| call | median s | min .. max | planted errors restored | changed to something else | error-free reads changed | distinct after |",
                  "|---|---|---|---|---|---|---|"]
        rows = [("ratio 0", fig["kmer_correct_s"], info)] + [(f"ratio {R}", ratio_s[R], ratio_info[R]) for R in a.ratio]
        for name, v, i in rows:
            lines.append(f"| {name} | {statistics.median(v):.4f} | {min(v):.4f} .. {max(v):.4f} | {i['planted_errors_restored_share']} | "
                         f"{i['planted_errors_changed_to_something_else_share']} | {i['error_free_reads_changed_share']} | {i['distinct_after']} |")
        for R in a.ratio:
            lines += ["", f"ratio {R}:", "", "| k | k-mers above -kh (A) | dominated (D) | suspect | corrected | uncorrectable | unsupported | ambiguous | distinct after |",
                      "|---|---|---|---|---|---|---|---|---|"]
            for r, (st, rs) in enumerate(ratio_per_k[R]):
                lines.append(f"| {a.ks + r} | {rs['above']} | {rs['dominated']} | {st['suspect']} | {st['corrected']} | {st['uncorrectable']} | {st['unsupported']} | "
                             f"{st['ambiguous']} | {st['distinct']} |")
        names = sorted({n for rec in kernel_ms.values() for n in rec})
        lines += ["", "device time of the kernels over one call's rounds (event-bracketed launches, one call each, outside the timing), ms (launches):", "",
                  "| kernel | " + " | ".join(f"ratio {R}" for R in kernel_ms) + " |", "|---|" + "---|" * len(kernel_ms)]
        for n in names:
            lines.append(f"| {n} | " + " | ".join(f"{rec[n][1]:.3f} ({rec[n][0]})" if n in rec else "-" for rec in kernel_ms.values()) + " |")
    lines.append("")
    text_out = "\n".join(lines)
    print(text_out)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text_out)


if __name__ == "__main__":
    main()
