#!/usr/bin/env python3
"""Generate tests/golden/unmapped/ by running the REFERENCE's own ``convert2Fasta`` and ``cluster_basedon_location``
(/root/reference/mirge/libs/novel_mir.py:41,81) on a small genome and unmapped frame made here.

Runs only where /root/reference exists (never on the GPU box, never from a test); what is committed is data: the inputs
(genome FASTA, unmapped.csv, the sorted SAM) and the files the reference wrote (the FASTA files, <sample>_clusters.tsv).
No reference source is copied.

Recipe, as in make_golden.py:
  * novel_mir.py imports scikit-learn, matplotlib, reportlab, joblib and scipy at its top for the back half of -nmir; none of
    them is touched by the two functions run here, so they are replaced by empty stand-in modules at import time (the
    stand-ins of tests/golden/stubs serve Bio / cutadapt as before);
  * the genome run is the stand-in bowtie of tests/golden/fake_bowtie, started as a child with the reference's own command
    line.  It answers genome runs in bowtie's default format only and skips -m without applying it, so its lines are turned
    into SAM lines HERE (flag 0 / 16, POS = offset + 1, the sequence as printed) and sorted stably by (reference order, POS):
    this project's "coordinate sorted" (DESIGN.md 3).  A read over -m therefore stays in the SAM: the fixture pins the
    reference's Python on a given SAM, not bowtie.

usage: python tests/golden/make_golden_unmapped.py
"""
import importlib.abc
import importlib.machinery
import os
import subprocess
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, "stubs"))
sys.path.insert(1, "/root/reference")
sys.path.insert(2, ROOT)

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

UNUSED = ("reportlab", "sklearn", "matplotlib", "joblib", "scipy", "forgi", "RNA")


class _Anything:
    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return _Anything()

    def __getattr__(self, name):
        return _Anything()


class _Empty(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything


class _UnusedModules(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path, target=None):
        if name.split(".")[0] not in UNUSED:
            return None
        return importlib.machinery.ModuleSpec(name, self, is_package=True)

    def create_module(self, spec):
        return _Empty(spec.name)

    def exec_module(self, module):
        pass


sys.meta_path.insert(0, _UnusedModules())
from mirge.libs.novel_mir import cluster_basedon_location, convert2Fasta  # noqa: E402  (the reference)

OUT = os.path.join(HERE, "unmapped")
SAMPLES = ["S1", "S2"]
MINL, MAXL, CUTOFF, MLOC, SEEDLEN, OLC = 16, 25, 2, 3, 25, 14  # mirge/libs/parse.py:130-135
_RC = str.maketrans("ACGT", "TGCA")


def rc(s):
    return s.translate(_RC)[::-1]


def make_genome(rng):
    """four references, one of them named without 'chr' (the reference skips it), an N run, a locus copied four times
    (over -m 3) and one copied twice"""
    names = ["chr1", "chr2", "scaffold_7", "chr3"]
    refs = ["".join("ACGT"[int(c)] for c in rng.integers(0, 4, size=2400)) for _ in names]
    refs[0] = refs[0][:700] + "N" * 9 + refs[0][709:]
    rep4, rep2 = refs[0][100:130], refs[1][300:330]
    r = list(refs[3])
    for k, at in enumerate((200, 600, 1000)):
        r[at:at + 30] = rep4 if k % 2 == 0 else rc(rep4)
    r[1500:1530] = rep2
    refs[3] = "".join(r)
    return names, refs


def make_frame(rng, refs):
    """the unmapped frame: piles of overlapping reads on both strands (nested reads, equal starts, overlaps at the threshold's
    edge), a second minus-strand pile on the same reference (the reference drops it), reads on the reference without 'chr', the
    repeated loci, reads too short / too long / too rare for the filter, reads that are not in the genome"""
    rows = {}

    def put(seq, c1, c2):
        if seq not in rows and "N" not in seq:
            rows[seq] = (c1, c2)

    def pile(ref, at, minus, shifts, lens):
        for sh, ln in zip(shifts, lens):
            w = refs[ref][at + sh:at + sh + ln]
            put(rc(w) if minus else w, int(rng.integers(2, 40)), int(rng.integers(0, 30)))

    pile(0, 1000, False, [0, 0, 2, 3, 5, 9, 10, 11, 12, 30], [22, 18, 20, 16, 24, 23, 22, 22, 22, 21])  # 22 - 9 + 1 = 14: the edge
    pile(0, 1400, False, [0, 4, 8, 30, 33], [20, 20, 25, 19, 22])
    pile(0, 1800, True, [0, 3, 6, 7], [22, 21, 23, 18])
    pile(0, 2100, True, [0, 2, 5], [22, 22, 20])          # second minus-strand pile of chr1
    pile(1, 500, True, [0, 1, 1, 6, 40], [24, 22, 17, 21, 22])
    pile(1, 900, False, [0, 5, 11, 12], [25, 22, 16, 25])
    pile(2, 700, False, [0, 3, 5], [22, 22, 22])          # scaffold_7
    pile(3, 200, False, [0, 3, 6], [22, 22, 22])          # four copies
    pile(1, 300, False, [0, 4, 7], [23, 21, 22])          # two copies
    pile(0, 690, False, [0, 2], [25, 24])                 # across the N run: no alignment
    put(refs[0][1000:1015], 50, 50)                       # 15 nt
    put(refs[0][1000:1026], 50, 50)                       # 26 nt
    put(refs[1][1600:1622], 1, 0)                         # sum below -c
    put(refs[1][1700:1722], 1, 1)                         # sum 2, but 1 in each sample
    for _ in range(6):
        put("".join("ACGT"[int(c)] for c in rng.integers(0, 4, size=int(rng.integers(16, 26)))), 5, 7)
    seqs = sorted(rows)  # the sorted union of several samples (digest.py:243)
    return seqs, np.array([rows[s] for s in seqs], dtype=np.int64)


def default_lines_to_sam(text, ref_order):
    """bowtie's default output (name, strand, reference, 0-based offset, sequence, ...) -> SAM lines, stably sorted"""
    recs = []
    for line in text.split("\n"):
        f = line.split("\t")
        if f == [""]:
            continue
        mm = f[7].count(":") if len(f) > 7 else 0
        recs.append((ref_order[f[2]], int(f[3]) + 1,
                     "\t".join([f[0], "0" if f[1] == "+" else "16", f[2], str(int(f[3]) + 1), "255", f"{len(f[4])}M", "*", "0", "0",
                                f[4], f[5], f"NM:i:{mm}"])))
    recs.sort(key=lambda r: (r[0], r[1]))
    return [r[2] for r in recs]


def main():
    rng = np.random.default_rng(20)
    os.makedirs(OUT, exist_ok=True)
    names, refs = make_genome(rng)
    base = os.path.join(OUT, "human_genome")
    with open(base + ".fa", "w") as fh:
        fh.write("".join(f">{n}\n{r}\n" for n, r in zip(names, refs)))
    seqs, counts = make_frame(rng, refs)
    frame = pd.DataFrame({"Sequence": seqs, "annotFlag": 0, **{s: counts[:, k] for k, s in enumerate(SAMPLES)}}).set_index("Sequence")
    frame.to_csv(os.path.join(OUT, "unmapped.csv"))
    raw, filtered = {}, {}
    convert2Fasta(frame, "unmapped.log", MINL, MAXL, CUTOFF, OUT, "human", {}, SAMPLES, raw, filtered)
    ref_order = {n: k for k, n in enumerate(names)}
    for s in SAMPLES:
        fa = os.path.join(OUT, f"unmapped_mirna_{s}.fa")
        cmd = [sys.executable, os.path.join(HERE, "fake_bowtie", "bowtie"), base, fa, "-f", "-n", "0", "--best", "-a", "--threads", "1",
               "-m", str(MLOC), "-l", str(SEEDLEN)]
        r = subprocess.run(cmd, check=True, capture_output=True, text=True)
        sam = os.path.join(OUT, f"unmapped_mirna_{s}_vs_genome_sorted.sam")
        with open(sam, "w") as fh:
            fh.write("@HD\tVN:1.0\tSO:coordinate\n" + "".join(f"@SQ\tSN:{n}\tLN:{len(x)}\n" for n, x in zip(names, refs)))
            fh.write("".join(ln + "\n" for ln in default_lines_to_sam(r.stdout, ref_order)))
        n = cluster_basedon_location(sam, OLC, s, OUT, os.path.join(OUT, f"{s}_clusters.tsv"))
        print(f"{s}: {raw[s]} raw, {filtered[s]} filtered reads, {n - 1} clusters")


if __name__ == "__main__":
    main()
