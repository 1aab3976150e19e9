"""``--unmapped-nearest [K]``: for every unique read that no pass annotated, the known miRNA precursor nearest to it by edit distance.

The cascade restates bowtie 1.x, which knows no gaps: a read one inserted or deleted base away from a hairpin, three substitutions away, or
with a tail longer than the isomiR pass trims, lands in ``unmapped.csv`` beside adapter dimers.  This report tells them apart.  It is this
project's own; there is no third-party tool to match, and the sentences below are the specification (tests/near_restate.py restates them).

Queries
  The rows of ``unmapped.csv``: the unique reads that no pass annotated, with the letters A C G T N as the parse leaves them.  A row is
  *considered* iff its length m satisfies 12 <= m <= 64; shorter and longer rows are counted for the summary and write nothing.

Targets
  The sequences of the run's hairpin library (``<org>_hairpin_<db>`` as ``seqio`` loads it), in library order, forward strand only (every
  pass is ``--norc``).  A hairpin may be empty; it then contributes nothing.

Letters
  Two letters match iff they are equal and one of A, C, G, T.  N and anything else match nothing, on either side.

Distance
  ``lev`` is the unit-cost edit distance: a substitution, an insertion and a deletion cost 1 each.  For a query q and a hairpin h,
  ``d(q, h)`` is the minimum of ``lev(q, h[s:e])`` over all NON-EMPTY substrings, 0 <= s < e <= len(h); D is the minimum of ``d(q, h)``
  over the library.  (The empty substring costs m, which the one-letter substring never exceeds, so leaving it out changes no D; it only
  keeps e >= 1 and s < e defined for a query that shares no letter with the library, where D = m.)

The hit and its ties
  Hairpin: the hairpin of lowest library index with ``d(q, h) = D``.  End: in that hairpin the smallest e such that some s gives
  ``lev(q, h[s:e]) = D``.  Start: for that e the LARGEST s with ``lev(q, h[s:e]) = D``, that is the shortest substring.

Reported
  A considered row is reported iff ``D <= min(K, m // 8)``, K in 1 .. 8 (a bare flag: 3): one edit from 12 nt, two from 16, three from
  24, so that chance hits on short reads stay rare; K = 8 becomes effective only at 64 nt.

``unmapped.nearest.csv``
  Header ``Sequence,hairpin,distance,start,end,matched,mature,<sample names...>``, then one line per reported row in the order those rows
  have in ``unmapped.csv`` (the file is a subsequence of it).  ``hairpin`` is the header's first blank-separated word; ``start`` is
  1-based and ``end`` inclusive (s + 1 and e); ``matched`` is ``h[s:e]``; the sample columns hold the row's counts as in ``unmapped.csv``.
  ``mature``: the printed names of the mature miRNAs whose canonical sequence sits on that hairpin and overlaps ``[s, e)``, joined by
  ``/`` in library order.  A canonical's position is ``gff.resolve_names``' ``start0`` with the canonical's length (for the library's last
  hairpin, whose sequence ``resolve_names`` does not see, the first occurrence in the hairpin); a canonical that is not found at its
  position is left out.  The column is empty when none overlaps, or when the run's ``<org>_<db>.gff3`` or mature FASTA is absent.

``nearest.summary.csv``
  One line per sample: ``sample,unmapped_unique,unmapped_reads,too_short,too_long,considered`` and then for d = 0 .. K ``d<d>_unique,
  d<d>_reads``, the reported unique rows and raw reads at distance d.  All integers; a row belongs to a sample iff its count there is > 0.
  ``run.log`` gets the same numbers in one line per sample.

Without a hairpin library, or with one that holds no hairpin, both files are written with their header line only and ``run.log`` says so.

Out of scope: the alignment itself (a CIGAR), the number of hairpins that tie, the reverse strand, reads beyond 64 nt, libraries other than
the hairpins, and any change to a count table.

Device side: csrc/kernels_nearest.hpp, csrc/native_nearest.hpp (``mirge_nearest_unmapped``, ``mirge_nearest_scan``).
"""
from __future__ import annotations

import os
import time
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MIN_LEN, MAX_LEN = 12, 64
MAX_K, DEFAULT_K = 8, 3
FILE_NAME = "unmapped.nearest.csv"
SUMMARY_NAME = "nearest.summary.csv"
MatureIndex = Dict[str, List[Tuple[str, int, int]]]  # hairpin name -> [(printed name, start, end)] in library order, 0-based half-open


def cap(K: int, m: int) -> int:
    """the largest distance at which a considered row of m letters is reported"""
    return min(int(K), int(m) // 8)


def header(base_names: Sequence[str]) -> str:
    return ",".join(["Sequence", "hairpin", "distance", "start", "end", "matched", "mature"] + list(base_names)) + "\n"


def summary_header(K: int) -> str:
    cols = ["sample", "unmapped_unique", "unmapped_reads", "too_short", "too_long", "considered"]
    for d in range(int(K) + 1):
        cols += [f"d{d}_unique", f"d{d}_reads"]
    return ",".join(cols) + "\n"


def mature_index(tables: Optional[dict], hp_names: Sequence[str], hp_seqs: Sequence[str]) -> MatureIndex:
    """``gff.resolve_names``' tables -> per hairpin name the canonicals that sit on it, in the miRNA library's order, each printed name once"""
    out: MatureIndex = {}
    if not tables:
        return out
    seq_of = {}
    for nm, sq in zip(hp_names, hp_seqs):
        seq_of.setdefault(nm, sq)
    seen = set()
    for r, k in enumerate(np.asarray(tables["master_of_ref"]).tolist()):
        if k < 0:
            continue
        parent = tables["parents"][int(tables["pre_of_master"][k])]
        printed = tables["printed"][int(tables["name_of_ref"][r])]
        if (parent, printed) in seen or parent not in seq_of:
            continue
        master, hseq = tables["masters"][k], seq_of[parent]
        a = int(tables["start0"][k]) - 1 if tables["pre_seqs"][int(tables["pre_of_master"][k])] != "" else hseq.find(master)
        if a < 0 or not master or hseq[a:a + len(master)] != master:
            continue
        seen.add((parent, printed))
        out.setdefault(parent, []).append((printed, a, a + len(master)))
    return out


def mature_names(index: MatureIndex, hairpin: str, s: int, e: int) -> str:
    return "/".join(nm for nm, a, b in index.get(hairpin, ()) if a < e and s < b)


def file_text(base_names: Sequence[str], seqs: Sequence[str], counts, hits: dict, hp_names: Sequence[str], hp_seqs: Sequence[str],
              index: Optional[MatureIndex] = None) -> str:
    """the bytes of ``unmapped.nearest.csv``.  ``seqs`` / ``counts``: the rows of ``unmapped.csv``; ``hits``: ``row`` (ascending indices into
    them), ``dist``, ``hairpin``, ``start``, ``end`` (0-based, half-open) of the reported rows"""
    index = index or {}
    lines = [header(base_names)]
    rows = np.asarray(hits["row"], dtype=np.int64)
    if rows.size > 1 and not (np.diff(rows) > 0).all():
        raise ValueError("the reported rows are not in the order of unmapped.csv")
    for r, d, h, s, e in zip(rows.tolist(), *(np.asarray(hits[k]).tolist() for k in ("dist", "hairpin", "start", "end"))):
        name = hp_names[h]
        lines.append(",".join([seqs[r], name, str(d), str(s + 1), str(e), hp_seqs[h][s:e], mature_names(index, name, s, e)] +
                              [str(int(x)) for x in counts[r]]) + "\n")
    return "".join(lines)


def summary_rows(base_names: Sequence[str], lengths, counts, hits: dict, K: int) -> List[List[int]]:
    """per sample [unmapped unique, unmapped reads, too short, too long, considered, then (unique, reads) for d = 0 .. K]"""
    lengths = np.asarray(lengths, dtype=np.int64)
    counts = np.asarray(counts, dtype=np.int64).reshape(lengths.shape[0], len(base_names))
    rows = np.asarray(hits["row"], dtype=np.int64)
    dist = np.asarray(hits["dist"], dtype=np.int64)
    out = []
    for s in range(len(base_names)):
        c = counts[:, s]
        here = c > 0
        row = [int(here.sum()), int(c.sum()), int((here & (lengths < MIN_LEN)).sum()), int((here & (lengths > MAX_LEN)).sum()),
               int((here & (lengths >= MIN_LEN) & (lengths <= MAX_LEN)).sum())]
        cr = c[rows] if rows.size else np.zeros(0, np.int64)
        for d in range(int(K) + 1):
            pick = (dist == d) & (cr > 0)
            row += [int(pick.sum()), int(cr[pick].sum())]
        out.append(row)
    return out


def summary_text(base_names: Sequence[str], rows: Sequence[Sequence[int]], K: int) -> str:
    return summary_header(K) + "".join(",".join([str(nm)] + [str(int(x)) for x in r]) + "\n" for nm, r in zip(base_names, rows))


def log_line(name: str, row: Sequence[int], K: int) -> str:
    per_d = ", ".join(f"d={d}: {row[5 + 2 * d]} ({row[6 + 2 * d]})" for d in range(int(K) + 1))
    return (f"unmapped nearest {name}: {row[0]} unmapped unique reads ({row[1]} raw), {row[2]} too short, {row[3]} too long, {row[4]} considered; "
            f"reported unique (raw) with K = {int(K)}: {per_d}")


def _write_whole(path: Path, text: str) -> None:
    tmp = Path(str(path) + ".tmp")
    with open(tmp, "w", newline="") as fh:
        fh.write(text)
    os.replace(tmp, path)


def write_files(workDir, base_names: Sequence[str], seqs: Sequence[str], counts, hits: dict, hp_names: Sequence[str], hp_seqs: Sequence[str],
                index: Optional[MatureIndex], K: int) -> List[List[int]]:
    """both files; -> the summary's rows"""
    workDir = Path(workDir)
    _write_whole(workDir / FILE_NAME, file_text(base_names, seqs, counts, hits, hp_names, hp_seqs, index))
    rows = summary_rows(base_names, [len(s) for s in seqs], counts, hits, K)
    _write_whole(workDir / SUMMARY_NAME, summary_text(base_names, rows, K))
    return rows


def hairpin_names(lib) -> List[str]:
    """the headers' first blank-separated words"""
    return [(h.split()[0] if h.split() else "") for h in lib.headers]


def mature_tables(libraries_path, organism: str, ref_db: str, mirna_names: Sequence[str], hairpin_lib) -> Optional[dict]:
    """``gff.resolve_names`` of the run's libraries, or None when ``<org>_<db>.gff3`` or the mature FASTA is absent"""
    from . import gff
    lp = Path(libraries_path) / organism
    fa = lp / "fasta.Libs" / (organism + "_mature_" + ref_db + ".fa")
    ann = lp / "annotation.Libs" / (organism + "_" + ref_db + ".gff3")
    if not fa.is_file() or not ann.is_file():
        return None
    return gff.resolve_names(list(mirna_names), gff.read_mature_fasta(fa), gff.read_annotation(ann, ref_db), gff.precursor_dict(hairpin_lib))


def refusal(args) -> str:
    """Why this command line's ``--unmapped-nearest`` is refused, or "" (``cli.parse_args`` hands it to ``ap.error`` before anything is
    written).  A legal K is left in ``args.unmapped_nearest`` as an int."""
    v = getattr(args, "unmapped_nearest", None)
    if v is None:
        return ""
    v = str(v)
    if not (v.isdigit() or (v[:1] in "+-" and v[1:].isdigit())):
        return "--unmapped-nearest takes an integer"
    if not 1 <= int(v) <= MAX_K:
        return f"--unmapped-nearest: 1 <= K <= {MAX_K}"
    if getattr(args, "save_pkl", False) or getattr(args, "resume", False) or getattr(args, "backend", "gpu") == "bowtie":
        return "--unmapped-nearest runs on the device-resident route: not together with -spl / -rr / --backend bowtie"
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return "--unmapped-nearest is a single-process option"
    args.unmapped_nearest = int(v)
    return ""


def _ref_db(args) -> str:
    from .cli import DB_KEYS
    return "MirGeneDB" if args.organism_name == "hamster" else DB_KEYS[str(args.mir_DB).lower()]


def run(args, workDir, base_names, casc, uniq, res, order, tm=None, ref_db: Optional[str] = None) -> dict:
    """``--unmapped-nearest`` of a single-process run, called from ``fastpath.reports`` behind the per-read CSVs.  ``order``: the row order
    of mapped.csv / unmapped.csv (handle indices)."""
    from . import _ffi
    from .unmapped import read_unmapped_csv
    tm = tm if tm is not None else {}
    t0 = time.perf_counter()
    workDir = Path(workDir)
    K = int(args.unmapped_nearest)
    base_names = list(base_names)
    with open(workDir / "run.log", "a+") as log:
        def say(msg):
            if not getattr(args, "quiet", False):
                print(msg)
            log.write(msg + "\n")
        hp = casc.libs.get("hairpin")
        if hp is None or len(hp) == 0:
            _write_whole(workDir / FILE_NAME, header(base_names))
            _write_whole(workDir / SUMMARY_NAME, summary_header(K))
            say("unmapped nearest: the run has no hairpin library (or an empty one): both files hold their header line only")
            return dict(rows=0, reported=0)
        seqs, counts = read_unmapped_csv(workDir / "unmapped.csv", base_names)
        ps, _, _, _ = res.fetch()
        order = np.asarray(order, dtype=np.int64)
        unm = order[ps[order] < 0]  # handle index of every row of unmapped.csv
        if unm.shape[0] != len(seqs):
            raise RuntimeError(f"--unmapped-nearest: unmapped.csv holds {len(seqs)} rows, the cascade left {unm.shape[0]} reads unannotated")
        t = time.perf_counter()
        got, stats = _ffi.nearest_unmapped(casc.ctx, uniq, res, hp.seqs, K)
        tm["nearest_device_s"] = time.perf_counter() - t
        if stats["unmapped"] != len(seqs):
            raise RuntimeError(f"--unmapped-nearest: the device counted {stats['unmapped']} unannotated reads, unmapped.csv holds {len(seqs)}")
        at = np.full(len(uniq), -1, dtype=np.int64)
        at[unm] = np.arange(unm.shape[0], dtype=np.int64)
        pos = at[got["row"].astype(np.int64)]
        by_file = np.argsort(pos, kind="stable")
        hits = dict(row=pos[by_file], **{k: got[k][by_file] for k in ("dist", "hairpin", "start", "end")})
        for r, e, s in zip(hits["row"][:64].tolist(), hits["end"][:64].tolist(), hits["start"][:64].tolist()):
            if r < 0 or not MIN_LEN <= len(seqs[r]) <= MAX_LEN or not 0 <= s < e:
                raise RuntimeError("--unmapped-nearest: a reported row is no considered row of unmapped.csv")
        hp_names, hp_seqs = hairpin_names(hp), hp.seqs.to_list()
        tables = mature_tables(args.libraries_path, args.organism_name, ref_db or _ref_db(args), casc.libs["mirna"].names, hp)
        if tables is None:
            say("unmapped nearest: no mature FASTA / gff3 of this database in the library directory: the mature column stays empty")
        rows = write_files(workDir, base_names, seqs, counts, hits, hp_names, hp_seqs, mature_index(tables, hp_names, hp_seqs), K)
        for name, row in zip(base_names, rows):
            say(log_line(name, row, K))
        seconds = time.perf_counter() - t0
        log.write(f"unmapped nearest: {seconds:.3f} s ({tm['nearest_device_s']:.3f} s in mirge_nearest_unmapped)\n")
    tm["unmapped_nearest_s"] = seconds
    return dict(rows=len(seqs), reported=int(hits["row"].shape[0]), stats=stats)
