"""Per-sample SAM alignments (``<sample>.sam``; ``--sam-out``) -- host side of ``mirge_sam_write_device``.

The reference's ``-bam`` builds each ``<sample>.sam`` in Python before it calls samtools: ``alignPlusParse`` keeps bowtie's
line of every annotated unique read in a side file per class (``mirge/libs/manifoldAlign.py:12-64``), ``bow2bam`` lifts it
from transcript to genome coordinates with what the library's header line says (``>ENST.. chr1 segs:1-9,10-981
cds:+:65565-65573,69037-70008``; ``fetchGenCor`` / ``fetch_pos_coordinate`` / ``fetch_neg_coordinate``,
``mirge/libs/bamFmt.py:9-170``) and writes it once per RAW read, ``summarize`` fixes the order of the classes
(``mirge/libs/summary.py:841-880``).  Here the cascade's result, the count matrix and the libraries are already on the device:
the lines are chosen, measured and formatted there, one call per sample (``csrc/kernels_sam.hpp``, ``csrc/native_sam.hpp``).

What stays in Python is per REFERENCE, not per read: the header lines' coordinates as flat tables (``lift_tables``).
``format_sam_host`` restates the whole file format slowly on host arrays; it is what the tests compare the device with, not
a route of the product.  The same records as a sorted, indexed BAM: ``bam_export`` (``--sorted-bam``); ``-bam`` is still refused.
"""
from __future__ import annotations

import ctypes as C
import time
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _ffi
from ._ffi import SamPass
from .cascade import PASSES
from .seqio import FlatSeqs

# the order of the classes in a sample's file (summary.py:856-878: snoRNA, rRNA, ncrna others, mRNA, then miRge3_miRNA.sam --
# every exact-miRNA line, then every isomiR line, manifoldAlign.py:21-23 -- then the hairpin miRNAs); tRNA and spike-in: no line
CLASS_PASSES = [4, 5, 6, 7, 0, 8, 1]
DEFAULT_HEADER = b"@HD\tVN:1.0\tSO:unsorted\n"  # what the reference writes for a library set it has no built-in header for


def header_dictionary(headers: Sequence[str]) -> Dict[str, str]:
    """``fetchGenCor`` on what ``bowtie-inspect -n`` prints (the header lines): the one dictionary ``bow2bam`` looks everything
    up in.  A line holding ``PATCH`` is skipped.  The line is split on single blanks; token 2 ``<a>:<list>`` is stored under
    ``name#<a>``, token 3 ``<b>:<strand>:<list>`` under ``name#<b>`` and ``name#strand``, token 1 under ``name`` -- in this order,
    and whatever is missing ends the line there (so a line that parses only in part leaves no chromosome and is dropped later)."""
    d: Dict[str, str] = {}
    for line in headers:
        if "PATCH" in line:
            continue
        tok = line.split(" ")
        if len(tok) < 4:
            continue
        name, a, b = tok[0], tok[2].split(":"), tok[3].split(":")
        if len(a) < 2:
            continue
        d[name + "#" + a[0]] = a[1]
        if len(b) < 3:
            continue
        d[name + "#" + b[0]] = b[2]
        d[name + "#strand"] = b[1]
        d[name] = tok[1]
    return d


def lift_of(d: Dict[str, str], name: str, organism: str):
    """(chromosome, minus, [(s, e)], [(lo, hi)]) of reference ``name`` or None when ``bow2bam`` writes no line for its reads: no
    chromosome, no ``segs`` / ``cds`` entry, for organism ``hamster`` no third ':' piece of token 1.  The strand is '+' only when
    the field is exactly '+'.  Deviation: a list that does not parse as ``int-int,...``, or a ``cds`` list shorter
    than the ``segs`` list, drops the reference here; the reference would stop with a ValueError or drop only some of its reads."""
    if name not in d or (name + "#strand") not in d or (name + "#segs") not in d or (name + "#cds") not in d:
        return None
    chrom = d[name]
    if organism == "hamster":
        piece = chrom.split(":")
        if len(piece) < 3:
            return None
        chrom = piece[2]
    try:
        segs = [(int(v.split("-")[0]), int(v.split("-")[1])) for v in d[name + "#segs"].split(",")]
        cds = [(int(v.split("-")[0]), int(v.split("-")[1])) for v in d[name + "#cds"].split(",")]
    except (ValueError, IndexError):
        return None
    if len(cds) < len(segs) or any(abs(x) >= 2 ** 31 for se in segs for x in se) or any(abs(x) >= 2 ** 62 for lh in cds for x in lh):
        return None
    return chrom, d[name + "#strand"] != "+", segs, cds[:len(segs)]


def lift_tables(names: Sequence[str], headers: Sequence[str], organism: str) -> dict:
    """The lift of one library as the flat arrays ``mirge_sam_write_device`` takes: ``chrom_of_ref`` (-1: no line), ``minus``,
    CSR ``seg_ptr`` into ``seg_s`` / ``seg_e`` / ``cds_lo`` / ``cds_hi``, the chromosome strings."""
    d = header_dictionary(headers)
    chrom_idx: Dict[str, int] = {}
    chrom_of_ref = np.full(len(names), -1, dtype=np.int32)
    minus = np.zeros(len(names), dtype=np.uint8)
    seg_ptr = np.zeros(len(names) + 1, dtype=np.int64)
    seg_s: List[int] = []
    seg_e: List[int] = []
    cds_lo: List[int] = []
    cds_hi: List[int] = []
    for r, nm in enumerate(names):
        lf = lift_of(d, nm, organism)
        if lf is not None:
            chrom, mi, segs, cds = lf
            chrom_of_ref[r] = chrom_idx.setdefault(chrom, len(chrom_idx))
            minus[r] = 1 if mi else 0
            seg_s += [s for s, _ in segs]; seg_e += [e for _, e in segs]
            cds_lo += [lo for lo, _ in cds]; cds_hi += [hi for _, hi in cds]
        seg_ptr[r + 1] = len(seg_s)
    chroms = FlatSeqs.from_list(list(chrom_idx))
    return dict(chrom_of_ref=chrom_of_ref, minus=minus, seg_ptr=seg_ptr, seg_s=np.asarray(seg_s, dtype=np.int32),
                seg_e=np.asarray(seg_e, dtype=np.int32), cds_lo=np.asarray(cds_lo, dtype=np.int64),
                cds_hi=np.asarray(cds_hi, dtype=np.int64), n_chrom=len(chrom_idx),
                chrom_data=np.ascontiguousarray(chroms.data) if chroms.data.size else np.zeros(1, np.uint8),
                chrom_off=np.ascontiguousarray(chroms.offsets, dtype=np.int64))


def digit_band_bytes(fixed: int, c: int) -> int:
    """Bytes of the c lines ``READ_0 .. READ_<c-1>`` of one row when a line without the digits of k takes ``fixed`` bytes: c * fixed
    plus the digits of 0 .. c-1, band by band (1 digit: 0-9, 2: 10-99, ...).  The device's closed form (``sam_digit_total``)."""
    total, lo, hi, d = c * fixed, 0, 10, 1
    while lo < c:
        total += d * (min(c, hi) - lo)
        lo, hi, d = hi, hi * 10, d + 1
    return total


_COMPLEMENT = str.maketrans("ACGTacgt", "TGCAtgca")  # anything else (N) stays what it is, as Bio.Seq.complement leaves N


def md_tag(read: str, window: str) -> str:
    out, run = [], 0
    for a, b in zip(read, window):
        if a == b:
            run += 1
        else:
            out.append(str(run) + b)
            run = 0
    return "".join(out) + str(run)


def line_suffix(read: str, p_trim5: int, p_trim3: int, name_lift, ref_seq: str, off: int, mm: int) -> str:
    """everything of a row's lines behind ``READ_k``: the stand-in bowtie's line for the (trimmed) read, lifted as ``bow2bam`` does"""
    chrom, minus, segs, cds = name_lift
    seq = read[p_trim5:len(read) - p_trim3] if p_trim5 + p_trim3 else read
    pos = off + 1
    start = pos
    for (s, e), (lo, hi) in zip(segs, cds):
        if s <= pos <= e:  # the first segment that holds POS decides; the spliced-CIGAR branch behind it can never run
            start = hi - (pos - s) - len(seq) + 1 if minus else lo + (pos - s)
            break
    out_seq = seq[::-1].translate(_COMPLEMENT) if minus else seq
    return "\t".join(["", "16" if minus else "0", chrom, str(start), "255", f"{len(seq)}M", "*", "0", "0", out_seq, "I" * len(seq),
                      f"XA:i:{mm}", "MD:Z:" + md_tag(seq, ref_seq[off:off + len(seq)]), f"NM:i:{mm}"]) + "\n"


def format_sam_host(reads: Sequence[str], ps, ref, off, mm, counts, order, sample: int, passes: Dict[int, dict], organism: str) -> bytes:
    """The body of sample ``sample``'s file (everything below the header) from host arrays: ``reads`` / ``ps`` / ``ref`` / ``off`` /
    ``mm`` per unique read, ``counts`` [U][S], ``order`` = the frame's row order, ``passes[p]`` = dict(names, headers, seqs (list of
    str), trim5, trim3) for every pass of CLASS_PASSES that has a library.  Slow on purpose: one Python string per line."""
    out: List[str] = []
    for p in CLASS_PASSES:
        if p not in passes:
            continue
        ps_ = passes[p]
        d = header_dictionary(ps_["headers"])
        lifts: Dict[int, object] = {}
        for i in order:
            i = int(i)
            c = int(counts[i][sample])
            if int(ps[i]) != p or c < 1:
                continue
            r = int(ref[i])
            if r not in lifts:
                lifts[r] = lift_of(d, ps_["names"][r], organism)
            if lifts[r] is None:
                continue
            tail = line_suffix(reads[i], ps_["trim5"], ps_["trim3"], lifts[r], ps_["seqs"][r], int(off[i]), int(mm[i]))
            head = reads[i] + "_"
            out.extend(head + str(k) + tail for k in range(c))
    return "".join(out).encode()


def host_passes(casc) -> Dict[int, dict]:
    """``format_sam_host``'s view of a cascade's libraries"""
    out = {}
    for p in CLASS_PASSES:
        if p >= casc.n_pass or PASSES[p][1] not in casc.libs:
            continue
        lib, kw = casc.libs[PASSES[p][1]], PASSES[p][3]
        out[p] = dict(names=lib.names, headers=lib.headers, seqs=lib.seqs.to_list(), trim5=int(kw.get("trim5", 0)), trim3=int(kw.get("trim3", 0)))
    return out


def pass_tables(casc, organism: str):
    """(class order, the C array of ``mirge_sam_pass``, the numpy arrays it points into) for a cascade; built once per cascade and
    organism: a human library set holds ~0.2 M header lines"""
    cached = getattr(casc, "_sam_tables", None)
    if cached is not None and cached[0] == organism:
        return cached[1]
    arr = (SamPass * casc.n_pass)()
    keep, by_key, classes = [], {}, []
    for p in CLASS_PASSES:
        key = PASSES[p][1] if p < casc.n_pass else None
        if key is None or key not in casc.libs or casc.dev_libs[p] is None:
            continue
        lib, kw = casc.libs[key], PASSES[p][3]
        if key not in by_key:  # the miRNA library serves passes 0 and 8
            by_key[key] = lift_tables(lib.names, lib.headers, organism)
        t = by_key[key]
        z32, z64, z8 = np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(1, np.uint8)
        a = dict(chrom_of_ref=t["chrom_of_ref"] if len(lib) else z32, minus=t["minus"] if len(lib) else z8, seg_ptr=t["seg_ptr"],
                 seg_s=t["seg_s"] if t["seg_s"].size else z32, seg_e=t["seg_e"] if t["seg_e"].size else z32,
                 cds_lo=t["cds_lo"] if t["cds_lo"].size else z64, cds_hi=t["cds_hi"] if t["cds_hi"].size else z64,
                 chrom_data=t["chrom_data"], chrom_off=t["chrom_off"])
        keep.append(a)
        s = arr[p]
        s.lib = casc.dev_libs[p]._h
        s.trim5, s.trim3, s.n_refs, s.n_chrom = int(kw.get("trim5", 0)), int(kw.get("trim3", 0)), len(lib), int(t["n_chrom"])
        for f, v in a.items():
            setattr(s, f, v.ctypes.data)
        classes.append(p)
    out = (np.asarray(classes, dtype=np.int32), arr, keep)
    casc._sam_tables = (organism, out)
    return out


def write_sample(casc, uniq, res, order: np.ndarray, sample: int, path, header: bytes, organism: str, bgzf_out: bool = False):
    """One sample's file through ``mirge_sam_write_device``; -> (lines below the header, their bytes).  ``bgzf_out``: ``path`` is the
    ``.sam.gz`` file (``--bgzf-out``, bgzf.py), written with its ``.gzi`` through ``mirge_sam_write_device_bgzf``; -> (lines, bytes, the
    file's numbers as ``bgzf.stats_dict`` gives them)"""
    classes, arr, _keep = pass_tables(casc, organism)
    order = np.ascontiguousarray(order, dtype=np.int64)
    if bgzf_out:
        from . import bgzf
        bgzf.route()
        block = bgzf.block_bytes()
        if classes.size == 0:  # no library of any class that writes lines: the header alone
            gz, gzi = bgzf.write_host(header, block)
            for p, data in ((str(path), gz), (bgzf.gzi_path(path), gzi)):
                with open(p, "wb") as fh:
                    fh.write(data)
            ms = bgzf.members(gz)
            return 0, 0, dict(file_bytes=len(gz), stored=sum(m["btype"] == 0 for m in ms), fixed=sum(m["btype"] == 1 for m in ms),
                              dynamic=sum(m["btype"] == 2 for m in ms), members=len(ms), stream_bytes=len(header))
        n_lines, n_bytes, st = C.c_int64(0), C.c_int64(0), np.zeros(bgzf.N_STATS, dtype=np.int64)
        _ffi._check(_ffi.load().mirge_sam_write_device_bgzf(
            casc.ctx._h, uniq._h, res._h, order if order.size else None, sample, classes, classes.size, arr, casc.n_pass, str(path).encode(),
            header, len(header), C.byref(n_lines), C.byref(n_bytes), bgzf.gzi_path(path).encode(), block, st), "mirge_sam_write_device_bgzf")
        return int(n_lines.value), int(n_bytes.value), bgzf.stats_dict(st)
    if classes.size == 0:  # no library of any class that writes lines: the header alone
        with open(path, "wb") as fh:
            fh.write(header)
        return 0, 0
    n_lines, n_bytes = C.c_int64(0), C.c_int64(0)
    _ffi._check(_ffi.load().mirge_sam_write_device(
        casc.ctx._h, uniq._h, res._h, order if order.size else None, sample, classes, classes.size, arr, casc.n_pass, str(path).encode(),
        header, len(header), C.byref(n_lines), C.byref(n_bytes)), "mirge_sam_write_device")
    return int(n_lines.value), int(n_bytes.value)


def run(args, workDir, base_names, casc, uniq, res, order, tm: Optional[dict] = None) -> dict:
    """``--sam-out``: ``<sample>.sam`` for every sample of the run, beside the other per-read reports (fastpath.reports)"""
    workDir = Path(workDir)
    t0 = time.perf_counter()
    hfile = getattr(args, "sam_header", None)
    if hfile:
        with open(hfile, "rb") as fh:
            header = fh.read()
    else:
        header = DEFAULT_HEADER
        with open(workDir / "run.log", "a+") as log:
            log.write("NOTE: --sam-out without --sam-header: every <sample>.sam starts with '@HD VN:1.0 SO:unsorted' alone; put the @SQ "
                      "lines of the genome the libraries were built on in front (or pass them with --sam-header FILE) before samtools "
                      "view / sort / index\n")
    t_tables = time.perf_counter()
    pass_tables(casc, args.organism_name)
    t_tables = time.perf_counter() - t_tables
    files = {}
    bgzf_out = bool(getattr(args, "bgzf_out", False))
    for s, name in enumerate(base_names):
        path = workDir / (str(name) + (".sam.gz" if bgzf_out else ".sam"))
        if bgzf_out:
            n_lines, n_bytes, st = write_sample(casc, uniq, res, order, s, path, header, args.organism_name, bgzf_out=True)
            files[str(name)] = dict(path=str(path), lines=n_lines, bytes=n_bytes, bgzf=st)
            with open(workDir / "run.log", "a+") as log:
                log.write(f"sam-out (bgzf) {name}: {n_lines} lines, {st['stream_bytes']} bytes of text in {st['file_bytes']} compressed bytes, "
                          f"{st['members']} members: {st['stored']} stored, {st['fixed']} fixed, {st['dynamic']} dynamic\n")
            continue
        n_lines, n_bytes = write_sample(casc, uniq, res, order, s, path, header, args.organism_name)
        files[str(name)] = dict(path=str(path), lines=n_lines, bytes=n_bytes)
    if tm is not None:
        tm["sam_out_s"] = time.perf_counter() - t0
        tm["sam_lift_tables_s"] = round(t_tables, 4)
    return files
