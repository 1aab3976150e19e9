#!/usr/bin/env python3
"""Time ``--umi-cluster directional`` against plain ``-udd`` on two synthetic UMI samples: a 4N library (``-umi 4,4``) and a 12-nt-UMI
library (``-umi 0,12``).  A sample: ``--molecules`` molecules, each an insert drawn Zipf-like from ``--inserts`` sequences of 18 .. 26 nt
and a random UMI; every molecule has a geometric number of PCR copies (mean 1 / ``--pcr-p``), and every UMI letter of every copy is
misread with probability ``--error`` (1 %).  One read per line, no adapters: the parse itself is not what is compared.

Per sample, ``--rounds`` rounds (one more in front that pays for first allocations), in every round one after the other: the parse call
``mirge_reads_parse_umi`` with ``dedup = 1`` (today's ``-udd`` path, byte for byte), the same with ``dedup = 2``, and ``mirge_umi_cluster``
alone on the tagged reads.  Median (min .. max), host wall clock.  Molecule counts: the truth, ``-udd``'s, the directional method's.

  python tools/umi_cluster_time.py --rounds 5 --out profiles/umi_cluster.md
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
from mirge3_amd import _ffi  # noqa: E402
from mirge3_amd.seqio import FlatSeqs  # noqa: E402

LETTERS = np.frombuffer(b"ACGT", np.uint8)


def sample(rng, f, b, molecules, n_inserts, pcr_p, error):
    """-> (text of one read per line, (distinct (insert, UMI) molecules, those of the commonest insert, that insert), reads, reads with a
    misread UMI letter)"""
    lens = rng.integers(18, 27, size=n_inserts)
    off = np.zeros(n_inserts + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    inserts = FlatSeqs(LETTERS[rng.integers(0, 4, size=int(off[-1]))], off)
    ins = np.minimum((rng.pareto(1.1, size=molecules) * 10).astype(np.int64), n_inserts - 1)  # the commonest insert holds a tenth of the molecules
    umi = rng.integers(0, 4, size=(molecules, f + b)).astype(np.uint8)
    truth = np.unique(np.concatenate([ins[:, None].astype(np.int64), umi.astype(np.int64)], axis=1), axis=0).shape[0]
    truth_top = np.unique(umi[ins == 0], axis=0).shape[0]
    copies = rng.geometric(pcr_p, size=molecules)
    mol = rng.permutation(np.repeat(np.arange(molecules, dtype=np.int64), copies))
    u = umi[mol]
    wrong = rng.random(u.shape) < error
    u = np.where(wrong, (u + rng.integers(1, 4, size=u.shape)) % 4, u).astype(np.uint8)
    n = mol.shape[0]
    col = lambda a: FlatSeqs(LETTERS[a].reshape(-1), np.arange(n + 1, dtype=np.int64) * a.shape[1])
    cols = [col(u[:, :f]), inserts.take(ins[mol]), col(u[:, f:])]
    text = np.frombuffer(FlatSeqs.join_columns(cols, b"\x00\x00\n"), dtype=np.uint8)
    return text[text != 0], (truth, truth_top, inserts.take(np.zeros(1, np.int64)).to_list()[0]), n, int(wrong.any(axis=1).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--molecules", type=int, default=1_000_000)
    ap.add_argument("--inserts", type=int, default=20_000)
    ap.add_argument("--pcr-p", type=float, default=0.4)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = _ffi.Context(0)
    lines = ["# --umi-cluster directional on one MI355X (tools/umi_cluster_time.py)", "",
             f"`--molecules {a.molecules} --inserts {a.inserts} --pcr-p {a.pcr_p} --error {a.error} --rounds {a.rounds}`", ""]
    for name, f, b in (("4N", 4, 4), ("12-nt UMI", 0, 12)):
        rng = np.random.Generator(np.random.PCG64(100 + f))
        text, (truth, truth_top, top), n_reads, n_err = sample(rng, f, b, a.molecules, a.inserts, a.pcr_p, a.error)
        fig = {k: [] for k in ("parse_udd_s", "parse_directional_s", "umi_cluster_alone_s")}
        info = {}
        for rnd in range(a.rounds + 1):
            tm = {}
            n_mol = {}
            for key, mode in (("parse_udd_s", None), ("parse_directional_s", "directional")):
                umi = _ffi.MirgeUmi.make(f, b, dedup=True, cluster=mode)
                t = time.perf_counter()
                raw, n_rec, tagged = _ffi.DeviceReads.parse_umi(ctx, text, 3, 16, None, umi)
                ctx.sync()
                tm[key] = time.perf_counter() - t
                n_mol[key] = len(raw)
                if rnd == a.rounds:  # (outside the timing) the commonest insert's molecules
                    d = raw.collapse()
                    n_mol[key + "_top"] = int(d.counts()[0][d.unpack().to_list().index(top), 0])
                    d.close()
                if mode:
                    stats = _ffi.umi_cluster_stats()
                    t = time.perf_counter()
                    flags = tagged.umi_cluster(f, b)
                    tm["umi_cluster_alone_s"] = time.perf_counter() - t
                    assert int(flags.sum()) == len(raw)
                    cnt = tagged.counts()[0][:, 0]
                    info = dict(reads=n_reads, reads_with_a_umi_error=n_err, tagged_reads=len(tagged), tagged_count_1=int((cnt == 1).sum()),
                                largest_count=int(cnt.max()), eligible=stats["eligible"], linked_count_1=stats["linked"], rounds=stats["rounds"],
                                table_slots=stats["slots"], molecules_truth=truth, molecules_udd=n_mol["parse_udd_s"], molecules_directional=len(raw),
                                commonest_insert_truth=truth_top, commonest_insert_udd=n_mol.get("parse_udd_s_top"),
                                commonest_insert_directional=n_mol.get("parse_directional_s_top"))
                raw.close(); tagged.close()
            if rnd:
                for k in fig:
                    fig[k].append(tm[k])
        lines += [f"## {name}: `-umi {f},{b} -udd`", "", ", ".join(f"{k} = {v}" for k, v in info.items()), "",
                  "| figure | median s | min .. max |", "|---|---|---|"]
        for k, v in fig.items():
            lines.append(f"| {k} | {statistics.median(v):.4f} | {min(v):.4f} .. {max(v):.4f} |")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
