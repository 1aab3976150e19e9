"""Per-sample genome coverage as bedGraph (``<sample>.bedgraph``; ``--coverage [unstranded|stranded]``) -- host side of
``mirge_coverage_write_device`` and ``mirge_coverage_runs``.

The specification (there is no bedtools in this project's world; the sentences below ARE the format, and are what ``bedtools genomecov
-bg -ibam <sample>_sorted.bam [-strand +|-]`` is documented to print):

* The intervals are exactly the rows of ``--sam-out``'s ``<sample>.sam`` (``sam_export``: same classes, same lift, same dropped
  references and classes).  One row is the 0-based half-open interval ``[START - 1, START - 1 + len(SEQ))`` on its chromosome, of
  weight c = the row's count in the sample, on the minus strand iff FLAG is 16.
* ``depth(chrom, x)`` = the summed weight of the intervals that hold x (``stranded``: per strand), a 64-bit integer.
* One line ``chrom\\tstart\\tend\\tdepth\\n`` per maximal stretch ``[start, end)`` of constant depth > 0: depth 0 writes nothing, two
  abutting stretches of equal depth are one line.  Lines are ordered by chromosome, then start; no header line; a sample without a
  kept row gets its file(s) with 0 bytes.
* Chromosome order: the ``@SQ`` order of ``--sam-header FILE`` when it holds ``@SQ`` lines (a kept row on a chromosome none of them
  names is an error); otherwise the chromosome names in byte order.
* A kept row with START < 1 or an end beyond 2^31 - 1 is an error naming the read and the reference.  Errors are raised before
  anything is written.

On the device (``csrc/kernels_cov.hpp``, ``csrc/native_cov.hpp``) a row costs two events, not work per raw read.  What stays in Python is
per chromosome: every pass's chromosome table mapped to one global rank.  ``coverage_host`` restates the depth slowly, base by base;
it is what the tests compare the device with, not a route of the product.
"""
from __future__ import annotations

import ctypes as C
import time
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _ffi, sam_export
from .cascade import PASSES
from .seqio import FlatSeqs

MAX_END = 2 ** 31 - 1


def as_intervals(rank, start, length, weight, minus) -> Dict[str, np.ndarray]:
    """the five arrays of ``mirge_coverage_runs`` with their types"""
    return dict(rank=np.ascontiguousarray(rank, dtype=np.int32), start=np.ascontiguousarray(start, dtype=np.int64),
                len=np.ascontiguousarray(length, dtype=np.int32), weight=np.ascontiguousarray(weight, dtype=np.uint32),
                minus=np.ascontiguousarray(minus, dtype=np.uint8))


def _runs_arrays(runs: Sequence[Tuple[int, int, int, int, int]]) -> Dict[str, np.ndarray]:
    cols = list(zip(*runs)) if runs else [[], [], [], [], []]
    return dict(strand=np.asarray(cols[0], dtype=np.uint8), chrom=np.asarray(cols[1], dtype=np.int32), start=np.asarray(cols[2], dtype=np.int64),
                end=np.asarray(cols[3], dtype=np.int64), depth=np.asarray(cols[4], dtype=np.int64))


def coverage_host(intervals: Dict[str, np.ndarray], stranded: bool) -> Dict[str, np.ndarray]:
    """The runs of ``intervals`` (``as_intervals``) in file order -- plus strand first, then chromosome rank, then start -- as arrays
    ``strand``, ``chrom``, ``start``, ``end``, ``depth``.  Slow on purpose: a depth per covered base of every (strand, chromosome),
    run-length encoded; no event list, no prefix sum."""
    per_base: Dict[Tuple[int, int], Dict[int, int]] = {}
    for r, s, n, w, mi in zip(intervals["rank"].tolist(), intervals["start"].tolist(), intervals["len"].tolist(),
                              intervals["weight"].tolist(), intervals["minus"].tolist()):
        if r < 0 or s < 0 or n < 1 or w < 1 or s + n > MAX_END:
            raise ValueError("coverage_host: an interval outside the contract")
        depth = per_base.setdefault((1 if (stranded and mi) else 0, r), {})
        for x in range(s, s + n):
            depth[x] = depth.get(x, 0) + w
    runs: List[Tuple[int, int, int, int, int]] = []
    for (strand, chrom) in sorted(per_base):
        depth = per_base[(strand, chrom)]
        open_at, last, d_open = None, None, 0
        for x in sorted(depth):
            d = depth[x]
            if open_at is not None and x == last + 1 and d == d_open:
                last = x
                continue
            if open_at is not None:
                runs.append((strand, chrom, open_at, last + 1, d_open))
            open_at, last, d_open = x, x, d
        if open_at is not None:
            runs.append((strand, chrom, open_at, last + 1, d_open))
    return _runs_arrays(runs)


def intervals_host(reads: Sequence[str], ps, ref, off, counts, order, sample: int, passes: Dict[int, dict], organism: str):
    """The rows of sample ``sample``'s ``<sample>.sam`` as (chromosome, 0-based start, length, weight, minus), in the file's row order
    -- ``sam_export.format_sam_host``'s loop with one entry per row instead of one line per raw read (same arguments)."""
    rows: List[Tuple[str, int, int, int, int]] = []
    for p in sam_export.CLASS_PASSES:
        if p not in passes:
            continue
        ps_ = passes[p]
        d = sam_export.header_dictionary(ps_["headers"])
        for i in order:
            i = int(i)
            c = int(counts[i][sample])
            if int(ps[i]) != p or c < 1:
                continue
            lift = sam_export.lift_of(d, ps_["names"][int(ref[i])], organism)
            if lift is None:
                continue
            chrom, minus, segs, cds = lift
            n = len(reads[i]) - ps_["trim5"] - ps_["trim3"]
            pos = int(off[i]) + 1
            start = pos
            for (s, e), (lo, hi) in zip(segs, cds):
                if s <= pos <= e:
                    start = hi - (pos - s) - n + 1 if minus else lo + (pos - s)
                    break
            rows.append((chrom, start - 1, n, c, 1 if minus else 0))
    return rows


def format_bedgraph(runs: Dict[str, np.ndarray], names: Sequence[str], strand: Optional[int] = None) -> bytes:
    """the lines of ``runs`` (of strand ``strand`` only, when given) with the chromosome names ``names[rank]``"""
    out = []
    for st, ch, s, e, d in zip(runs["strand"].tolist(), runs["chrom"].tolist(), runs["start"].tolist(), runs["end"].tolist(), runs["depth"].tolist()):
        if strand is None or st == strand:
            out.append(f"{names[ch]}\t{s}\t{e}\t{d}\n")
    return "".join(out).encode("latin-1")


def runs_device(ctx, intervals: Dict[str, np.ndarray], stranded: bool) -> Dict[str, np.ndarray]:
    """``mirge_coverage_runs``: the runs of host intervals, computed on the device"""
    iv = as_intervals(intervals["rank"], intervals["start"], intervals["len"], intervals["weight"], intervals["minus"])
    n = int(iv["rank"].size)
    if not all(a.size == n for a in iv.values()):
        raise ValueError("runs_device: the five arrays differ in length")
    cap = max(2 * n, 1)
    out = dict(strand=np.zeros(cap, np.uint8), chrom=np.zeros(cap, np.int32), start=np.zeros(cap, np.int64), end=np.zeros(cap, np.int64),
               depth=np.zeros(cap, np.int64))
    n_runs = C.c_int64(0)
    _ffi._check(_ffi.load().mirge_coverage_runs(
        ctx._h, n, *((iv[k] if n else None) for k in ("rank", "start", "len", "weight", "minus")), bool(stranded),
        out["strand"], out["chrom"], out["start"], out["end"], out["depth"], C.byref(n_runs)), "mirge_coverage_runs")
    return {k: v[:int(n_runs.value)].copy() for k, v in out.items()}


def pass_chromosomes(casc, organism: str) -> Dict[int, List[str]]:
    """pass -> its chromosome names in the order of its table (``sam_export.pass_tables``)"""
    classes, arr, keep = sam_export.pass_tables(casc, organism)
    out = {}
    for p, a in zip(classes.tolist(), keep):
        out[p] = FlatSeqs(a["chrom_data"], a["chrom_off"]).to_list() if int(arr[p].n_chrom) else []
    return out


def rank_tables(casc, organism: str, sq_names: Optional[Sequence[str]]):
    """(ranked names, flat int32 array, int64 offsets [n_pass + 1]): every pass's chromosome index -> one global rank, in the shape of
    ``bam_export.refid_tables``.  ``sq_names`` (the ``@SQ`` order) or None: the passes' names in byte order.  -1: ``sq_names`` lacks
    the name (an error only if a kept row lies there: the device call decides)."""
    per_pass = pass_chromosomes(casc, organism)
    if sq_names is None:
        names = sorted({nm for v in per_pass.values() for nm in v}, key=lambda s: s.encode("latin-1"))
    else:
        names = list(sq_names)
    rank_of = {nm: k for k, nm in enumerate(names)}
    off = np.zeros(casc.n_pass + 1, dtype=np.int64)
    for p in range(casc.n_pass):
        off[p + 1] = off[p] + len(per_pass.get(p, ()))
    flat = np.asarray([rank_of.get(nm, -1) for p in sorted(per_pass) for nm in per_pass[p]] + [0], dtype=np.int32)
    return names, flat, off


def sq_order(header: Optional[bytes]) -> Optional[List[str]]:
    """the ``@SQ`` names of a ``--sam-header`` file in file order, or None when it holds no ``@SQ`` line (a malformed one raises)"""
    if not header or not any(line.startswith(b"@SQ") for line in header.split(b"\n")):
        return None
    from .bam_export import parse_sq
    return [nm for nm, _ in parse_sq(header)]


def sample_paths(workDir, name: str, stranded: bool, bgzf_out: bool = False) -> List[Path]:
    workDir = Path(workDir)
    ext = "bedgraph.gz" if bgzf_out else "bedgraph"
    return [workDir / f"{name}.plus.{ext}", workDir / f"{name}.minus.{ext}"] if stranded else [workDir / f"{name}.{ext}"]


def _reference_name(casc, p: int, r: int) -> str:
    key = PASSES[p][1] if 0 <= p < len(PASSES) else None
    lib = casc.libs.get(key) if key is not None else None
    return lib.names[r] if lib is not None and 0 <= r < len(lib.names) else f"reference {r} of pass {p}"


def write_sample(casc, uniq, res, order: np.ndarray, sample: int, paths: Sequence, stranded: bool, organism: str,
                 sq_names: Optional[Sequence[str]] = None, bgzf_out: bool = False) -> dict:
    """One sample's file (``stranded``: its two files) through ``mirge_coverage_write_device``; -> dict(intervals, weight, lines, bytes).
    A data error -- a chromosome ``sq_names`` lacks, a row outside [1, 2^31 - 1] -- is a ValueError and leaves no file.
    ``bgzf_out``: ``paths`` are ``.bedgraph.gz`` files (``--bgzf-out``, bgzf.py), each written with its ``.gzi`` through
    ``mirge_coverage_write_device_bgzf``; the dict gains ``bgzf`` = one ``bgzf.stats_dict`` per file."""
    paths = [str(p) for p in paths]
    if len(paths) != (2 if stranded else 1):
        raise ValueError("write_sample: one path, or two when stranded")
    classes, arr, _keep = sam_export.pass_tables(casc, organism)
    order = np.ascontiguousarray(order, dtype=np.int64)
    if bgzf_out:
        from . import bgzf
        bgzf.route()
        block = bgzf.block_bytes()
    if classes.size == 0 and bgzf_out:  # no library of any class that has rows: empty streams
        gz, gzi = bgzf.write_host(b"", block)
        for p in paths:
            for q, data in ((p, gz), (bgzf.gzi_path(p), gzi)):
                with open(q, "wb") as fh:
                    fh.write(data)
        return dict(intervals=0, weight=0, lines=0, bytes=0,
                    bgzf=[dict(file_bytes=len(gz), stored=0, fixed=0, dynamic=0, members=0, stream_bytes=0) for _ in paths])
    if classes.size == 0:  # no library of any class that has rows: empty files
        for p in paths:
            open(p, "wb").close()
        return dict(intervals=0, weight=0, lines=0, bytes=0)
    names, flat, off = rank_tables(casc, organism, sq_names)
    nm = FlatSeqs.from_list(list(names))
    nm_data = np.ascontiguousarray(nm.data) if nm.data.size else np.zeros(1, np.uint8)
    nm_off = np.ascontiguousarray(nm.offsets, dtype=np.int64)
    outs = [C.c_int64(0) for _ in range(4)]
    err = np.zeros(4, dtype=np.int64)
    common = (casc.ctx._h, uniq._h, res._h, order if order.size else None, sample, classes, classes.size, arr, casc.n_pass, flat, off, len(names),
              nm_data, nm_off, bool(stranded), paths[0].encode(), paths[1].encode() if stranded else None,
              C.byref(outs[0]), C.byref(outs[1]), C.byref(outs[2]), C.byref(outs[3]), err)
    if bgzf_out:
        st = np.zeros(2 * bgzf.N_STATS, dtype=np.int64)
        rc = _ffi.load().mirge_coverage_write_device_bgzf(*common, bgzf.gzi_path(paths[0]).encode(),
                                                          bgzf.gzi_path(paths[1]).encode() if stranded else None, block, st)
    else:
        rc = _ffi.load().mirge_coverage_write_device(*common)
    if rc != 0 and int(err[0]) == 2:
        read = uniq.unpack().to_list()[int(err[1])]
        raise ValueError(f"--coverage: read {read} on reference {_reference_name(casc, int(err[2]), int(err[3]))} lies outside "
                         f"[1, 2^31 - 1] of its chromosome: a bedGraph of this project cannot hold it")
    if rc != 0 and int(err[0]) == 1:
        msg = _ffi.load().mirge_last_error().decode()
        raise ValueError("--coverage: " + msg.split(": ", 1)[-1])
    _ffi._check(rc, "mirge_coverage_write_device_bgzf" if bgzf_out else "mirge_coverage_write_device")
    out = dict(intervals=int(outs[0].value), weight=int(outs[1].value), lines=int(outs[2].value), bytes=int(outs[3].value))
    if bgzf_out:
        out["bgzf"] = [bgzf.stats_dict(st[k * bgzf.N_STATS:(k + 1) * bgzf.N_STATS]) for k in range(len(paths))]
    return out


def run(args, workDir, base_names, casc, uniq, res, order, tm: Optional[dict] = None) -> dict:
    """``--coverage``: ``<sample>.bedgraph`` (or ``.plus.`` / ``.minus.bedgraph``) for every sample of the run (fastpath.reports)"""
    workDir = Path(workDir)
    t0 = time.perf_counter()
    stranded = getattr(args, "coverage", None) == "stranded"
    header = None
    hfile = getattr(args, "sam_header", None)
    if hfile:
        with open(hfile, "rb") as fh:
            header = fh.read()
    sq_names = sq_order(header)
    files, files_bw = {}, {}
    with open(workDir / "run.log", "a+") as log:
        for s, name in enumerate(base_names):
            if getattr(args, "coverage_bigwig", False):  # first: a data error then leaves no file of this sample
                from . import bigwig
                files_bw.update(bigwig.run(args, workDir, base_names, casc, uniq, res, order, tm, sample=s))
            bgzf_out = bool(getattr(args, "bgzf_out", False))
            paths = sample_paths(workDir, str(name), stranded, bgzf_out)
            st = write_sample(casc, uniq, res, order, s, paths, stranded, args.organism_name, sq_names, bgzf_out=bgzf_out)
            files[str(name)] = dict(paths=[str(p) for p in paths], **st)
            gz = ""
            if bgzf_out:
                tot = {k: sum(f[k] for f in st["bgzf"]) for k in ("file_bytes", "members", "stored", "fixed", "dynamic")}
                gz = (f" in {tot['file_bytes']} compressed bytes, {tot['members']} members: {tot['stored']} stored, {tot['fixed']} fixed, "
                      f"{tot['dynamic']} dynamic")
            log.write(f"coverage ({'stranded' if stranded else 'unstranded'}, chromosomes in {'@SQ' if sq_names is not None else 'byte'} order) "
                      f"{name}: {st['intervals']} intervals, summed weight {st['weight']}, {st['lines']} lines, {st['bytes']} bytes{gz}\n")
    if tm is not None:
        tm["coverage_s"] = time.perf_counter() - t0 - tm.get("coverage_bigwig_s", 0.0)
    for name, v in files_bw.items():
        files[name]["bigwig"] = v
    return files
