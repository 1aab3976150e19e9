"""``--read-qc``: per-sample read QC and class length profiles, from what the parse and the cascade already hold on the device.

Per sample ``<sample>.readqc.tsv``, once per run ``readqc.summary.csv``, one run.log line per sample.  No FastQC format is reproduced; the
sentences below are the specification (tests/qc_restate.py restates them byte by byte).

Views
  raw        every record of the file, with its sequence line as it stands (a trailing ``\\r`` stripped).
  trimmed    the same record's read after the LAST modifier of the chain, once per record whatever ``--trim-count`` says.  It exists only
             if its length is at least ``--minimum-length``; its quality string is the same slice of the quality line.  Without any
             modifier it is the raw view under the length filter.
  annotated  the reads as the cascade saw them (after ``--kmer-correct`` if it ran, counted per modifier under ``--trim-count
             per-modifier``): a class's sum is that class's column of annotation.report.csv, the sum over all classes is ``Trimmed Reads
             (all)``, not necessarily the trimmed view's ``reads``.

Letters and qualities
  ``A C G T`` in either case, and ``U/u`` as ``T``, are themselves; every other byte is ``N``.  The quality of a base is ``byte - phred_base``
  clamped to [0, 93]; every clamped byte counts under the scalar ``qual_clamped``.  A FASTQ record whose quality line is not as long as its
  sequence line contributes to no quality section and counts under ``qual_length_mismatch``.  FASTA and one-sequence-per-line inputs write
  no quality section and no quality scalar.

File
  First line ``#mirge3amd-readqc\\t1``, then ``section\\tview\\tk1\\tk2\\tk3\\tvalue\\n`` with ``.`` for an unused key and integer values.  A
  table line is written only for value > 0; scalars always.  Order: sections as listed, ``raw`` before ``trimmed``, then k1, k2, k3
  ascending -- numbers numerically, letters ``A C G T N``, classes in pass order with ``unmapped`` last.  A position or length of 256 or
  more is written as key 256; the ``length`` section alone is exact up to 65 535.

  reads, bases, reads_with_N, empty_reads, qual_clamped, qual_length_mismatch    scalars per view
  length               k1 = length                                              reads
  base                 k1 = min(pos, 256), k2 = letter                          bases
  qual                 k1 = min(pos, 256), k2 = quality                         bases
  meanq                k1 = floor(sum of qualities / len), len >= 1             reads
  gc                   k1 = floor(100 (G + C) / len), len counts every letter, len >= 1    reads
  first                k1 = min(len, 256), k2 = first letter, len >= 1          reads
  class_length         (view annotated) k1 = class, k2 = min(len, 256), k3 = first letter (an empty read: N)   raw reads of this sample
  class_length_unique  same keys                                                unique reads with a count > 0 in the sample

``readqc.summary.csv``: one row per (sample, view in raw, trimmed), integer columns ``reads,bases,gc_bases,n_bases,q20_bases,q30_bases`` (the
q columns empty for input without qualities), all derived on the host from the sections.

Device side: csrc/kernels_qc.hpp, csrc/native_qc.hpp (``mirge_qc``, ``mirge_reads_parse_trim_qc``, ``mirge_qc_fetch``,
``mirge_qc_class_profile``).
"""
from __future__ import annotations

import os
from pathlib import Path
from typing import Dict, List, Sequence, Tuple

import numpy as np

P = 256
NQ = 94
LEN_MAX = 65535
LETTERS = "ACGTN"
VIEWS = ("raw", "trimmed", "annotated")
SCALARS = ("reads", "bases", "reads_with_N", "empty_reads", "qual_clamped", "qual_length_mismatch")
QUAL_SCALARS = ("qual_clamped", "qual_length_mismatch")
SECTIONS = SCALARS + ("length", "base", "qual", "meanq", "gc", "first", "class_length", "class_length_unique")
HEADER = "#mirge3amd-readqc\t1\n"
SUMMARY_NAME = "readqc.summary.csv"
SUMMARY_HEADER = "sample,view,reads,bases,gc_bases,n_bases,q20_bases,q30_bases\n"
UNMAPPED = "unmapped"
# one view's tables as mirge_qc_fetch hands them out (64-bit words; include/mirge_native.h)
OFF_SCALARS, OFF_LENGTH = 0, 8
OFF_BASE = OFF_LENGTH + LEN_MAX + 1
OFF_QUAL = OFF_BASE + (P + 1) * 5
OFF_MEANQ = OFF_QUAL + (P + 1) * NQ
OFF_GC = OFF_MEANQ + NQ
OFF_FIRST = OFF_GC + 101
VIEW_WORDS = OFF_FIRST + (P + 1) * 5

Entries = Dict[Tuple, int]  # (section, view, k1, k2, k3) -> value; an unused key is None, a letter or a class its name, a number an int


def view_entries(words: np.ndarray, view: str, has_qual: bool) -> Entries:
    """one view's tables (int64 [VIEW_WORDS]) -> its entries: every scalar (the quality ones only with ``has_qual``), table cells > 0"""
    w = np.asarray(words, dtype=np.int64)
    assert w.shape == (VIEW_WORDS,)
    out: Entries = {}
    for k, name in enumerate(SCALARS):
        if has_qual or name not in QUAL_SCALARS:
            out[(name, view, None, None, None)] = int(w[OFF_SCALARS + k])
    for L in np.flatnonzero(w[OFF_LENGTH:OFF_BASE]):
        out[("length", view, int(L), None, None)] = int(w[OFF_LENGTH + L])
    tables = [("base", OFF_BASE, 5, True), ("first", OFF_FIRST, 5, True)] + ([("qual", OFF_QUAL, NQ, False)] if has_qual else [])
    for name, off, width, letters in tables:
        t = w[off:off + (P + 1) * width].reshape(P + 1, width)
        for r, c in zip(*np.nonzero(t)):
            out[(name, view, int(r), LETTERS[c] if letters else int(c), None)] = int(t[r, c])
    for name, off, n in ([("meanq", OFF_MEANQ, NQ)] if has_qual else []) + [("gc", OFF_GC, 101)]:
        for k in np.flatnonzero(w[off:off + n]):
            out[(name, view, int(k), None, None)] = int(w[off + k])
    return out


def class_entries(profile: np.ndarray, classes: Sequence[str]) -> Entries:
    """one sample's class profile (int64 [len(classes)][257][5][2], ``mirge_qc_class_profile``; the last class is ``unmapped``) -> entries"""
    t = np.asarray(profile, dtype=np.int64)
    assert t.shape == (len(classes), P + 1, 5, 2)
    out: Entries = {}
    for c, L, l, which in zip(*np.nonzero(t)):
        out[(("class_length", "class_length_unique")[which], "annotated", classes[c], int(L), LETTERS[l])] = int(t[c, L, l, which])
    return out


def class_names(n_pass: int) -> List[str]:
    from .cascade import PASSES
    return [p[0] for p in PASSES[:n_pass]] + [UNMAPPED]


def _rank(x, classes):
    if x is None:
        return (0, 0)
    if isinstance(x, str):
        return (2, classes.index(x)) if x in classes else (1, LETTERS.index(x))
    return (1, int(x))


def file_text(entries: Entries, classes: Sequence[str] = ()) -> str:
    """the bytes of ``<sample>.readqc.tsv`` for these entries, in the specified order"""
    classes = list(classes)
    keys = sorted(entries, key=lambda e: (SECTIONS.index(e[0]), VIEWS.index(e[1])) + tuple(_rank(x, classes) for x in e[2:]))
    show = lambda x: "." if x is None else str(x)
    lines = [HEADER]
    for e in keys:
        if entries[e] > 0 or e[0] in SCALARS:
            lines.append(f"{e[0]}\t{e[1]}\t{show(e[2])}\t{show(e[3])}\t{show(e[4])}\t{int(entries[e])}\n")
    return "".join(lines)


def summary_row(entries: Entries, view: str) -> List:
    """[reads, bases, gc_bases, n_bases, q20_bases, q30_bases] of a view (the q figures None for input without qualities)"""
    get = lambda name: entries.get((name, view, None, None, None), 0)
    base = {k: v for k, v in entries.items() if k[0] == "base" and k[1] == view}
    qual = {k: v for k, v in entries.items() if k[0] == "qual" and k[1] == view}
    has_qual = ("qual_clamped", view, None, None, None) in entries
    return [get("reads"), get("bases"), sum(v for k, v in base.items() if k[3] in "GC"), sum(v for k, v in base.items() if k[3] == "N"),
            sum(v for k, v in qual.items() if k[3] >= 20) if has_qual else None, sum(v for k, v in qual.items() if k[3] >= 30) if has_qual else None]


def summary_text(names: Sequence[str], per_sample: Sequence[Entries]) -> str:
    out = [SUMMARY_HEADER]
    for name, e in zip(names, per_sample):
        for view in ("raw", "trimmed"):
            out.append(",".join([str(name), view] + ["" if x is None else str(int(x)) for x in summary_row(e, view)]) + "\n")
    return "".join(out)


def modal_trimmed_length(entries: Entries) -> int:
    """the most frequent length of the trimmed view (the smallest of equals; 0 for no reads)"""
    best, at = 0, 0
    for k, v in sorted((k[2], v) for k, v in entries.items() if k[0] == "length" and k[1] == "trimmed"):
        if v > best:
            best, at = v, k
    return at


def log_line(name: str, entries: Entries) -> str:
    r, t = summary_row(entries, "raw"), summary_row(entries, "trimmed")
    return f"read qc {name}: raw {r[0]} reads, {r[1]} bases; trimmed {t[0]} reads, {t[1]} bases; modal trimmed length {modal_trimmed_length(entries)}"


def _write_whole(path: Path, text: str) -> None:
    tmp = Path(str(path) + ".tmp")
    with open(tmp, "w", newline="") as fh:
        fh.write(text)
    os.replace(tmp, path)


def write_sample(workDir, name: str, entries: Entries, classes: Sequence[str]) -> Path:
    path = Path(workDir) / f"{name}.readqc.tsv"
    _write_whole(path, file_text(entries, classes))
    return path


def write_summary(workDir, names: Sequence[str], per_sample: Sequence[Entries]) -> Path:
    path = Path(workDir) / SUMMARY_NAME
    _write_whole(path, summary_text(names, per_sample))
    return path


def sample_entries(tables: np.ndarray, has_qual: bool) -> Entries:
    """``ReadQc.fetch()`` -> the entries of the raw and the trimmed view"""
    out = view_entries(tables[0], "raw", has_qual)
    out.update(view_entries(tables[1], "trimmed", has_qual))
    return out


def write_all(ctx, workDir, names: Sequence[str], handles, uniq, res, say) -> List[Entries]:
    """after the cascade: the samples' tables from their accumulators, the class profile of the dictionary, the files and the log lines"""
    from . import _ffi
    profile = _ffi.qc_class_profile(ctx, uniq, res)
    classes = class_names(res.n_pass)
    per_sample = []
    for s, (name, h) in enumerate(zip(names, handles)):
        e = sample_entries(*h.fetch())
        h.close()
        e.update(class_entries(profile[s], classes))
        per_sample.append(e)
    for name, e in zip(names, per_sample):
        write_sample(workDir, name, e, classes)
    write_summary(workDir, names, per_sample)
    for name, e in zip(names, per_sample):
        say(log_line(name, e))
    return per_sample


def refusal(args) -> str:
    """Why this command line's ``--read-qc`` is refused, or "" (``cli.parse_args`` hands it to ``ap.error`` before anything is written).
    ``-a auto``, ``--kmer-correct`` and every exporter are legal beside the flag."""
    if not getattr(args, "read_qc", False):
        return ""
    if getattr(args, "uniq_mol_ids", None):
        return "--read-qc: not together with -umi (the UMI routes slice the reads and take the sample whole)"
    if getattr(args, "save_pkl", False) or getattr(args, "resume", False) or getattr(args, "backend", "gpu") == "bowtie":
        return "--read-qc runs on the device-resident route: not together with -spl / -rr / --backend bowtie"
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return "--read-qc is a single-process option"
    form = os.environ.get("MIRGE_QC_FORM")
    if form not in (None, "", "pos", "read"):
        return f"MIRGE_QC_FORM={form!r}: pos or read"
    return ""
