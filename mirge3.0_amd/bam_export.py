"""Per-sample sorted BAM and index (``<sample>_sorted.bam`` / ``<sample>_sorted.bai``; ``--sorted-bam``) -- host side of
``mirge_bam_write_device``.

The reference's ``-bam`` ends in ``createBAM`` (``mirge/libs/bamFmt.py:173-205``): ``samtools view -bS``, ``sort`` and ``index`` on the
``<sample>.sam`` it wrote.  Here the records of that file (``sam_export``: same rows, same lift, same dropped classes) are encoded as
BAM v1, sorted by (refID, pos, reverse flag), BGZF-compressed and indexed on the device, one call per sample
(``csrc/kernels_bam.hpp``, ``csrc/native_bam.hpp``).  The sort is stable with respect to the ``.sam`` file's row order and a row's copies
follow in ``k`` order; there is no samtools in this project's world to confirm ``samtools sort``'s tie rule, so this rule is the
specification.

What stays in Python is per reference: the ``@SQ`` dictionary of ``--sam-header FILE`` (the reference's literal per-organism headers
are program text and are not carried), the header text with ``SO:coordinate``, each pass's chromosome -> refID table.
``format_bam_host`` restates the whole format slowly -- records, sort, BGZF through ``zlib``, the index per record -- and is what the
tests compare the device with, not a route of the product.

The index (SAM specification 5.2), as both builders write it: per reference the bins in ascending order, each with the maximal runs
of consecutive records of that bin as its chunks; the pseudo-bin 37450 last (virtual offsets of the reference's first record and of
the end of its last, then mapped and unmapped counts); the 16 kb linear index up to the last window touched, an entry being the
virtual offset of the first record that overlaps the window, empty windows taking the entry to their right; ``n_no_coor`` = 0.  The
virtual offset of stream byte u is (file offset of the member that holds block u // block_bytes) << 16 | u % block_bytes; the end
of the stream is the start of the EOF block (a position on a member boundary belongs to the member that follows).
"""
from __future__ import annotations

import ctypes as C
import struct
import time
import zlib
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _ffi, sam_export
from .seqio import FlatSeqs

BLOCK_BYTES = 65280  # uncompressed bytes of a BGZF block (htslib's BGZF_BLOCK_SIZE)
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
MAX_POS = 1 << 29    # where the binning index ends
_CODE = {"A": 1, "C": 2, "G": 4, "T": 8}


def parse_sq(header: bytes) -> List[Tuple[str, int]]:
    """(name, length) of the ``@SQ`` lines in file order = refID order; a line without SN: / LN:, a name twice or no line at all
    is a ValueError"""
    refs: List[Tuple[str, int]] = []
    for line in header.decode("latin-1").split("\n"):
        if not line.startswith("@SQ"):
            continue
        f = {x[:2]: x[3:] for x in line.rstrip("\r").split("\t")[1:] if len(x) >= 3 and x[2] == ":"}
        if "SN" not in f or not f.get("LN", "").isdigit() or not 0 < int(f["LN"]) < 2 ** 31:
            raise ValueError(f"--sam-header: an @SQ line needs SN: and LN: ({line!r})")
        if f["SN"] in dict(refs):
            raise ValueError(f"--sam-header: @SQ SN:{f['SN']} twice")
        refs.append((f["SN"], int(f["LN"])))
    if not refs:
        raise ValueError("--sorted-bam: the --sam-header file holds no @SQ line (a BAM needs the references' names and lengths)")
    return refs


def header_text(header: bytes) -> bytes:
    """FILE verbatim with one change: a first line ``@HD`` gets ``SO:coordinate`` (replaced, or appended if absent); without one,
    ``@HD VN:1.0 SO:coordinate`` is put in front"""
    if not header.startswith(b"@HD"):
        return b"@HD\tVN:1.0\tSO:coordinate\n" + header
    first, nl, rest = header.partition(b"\n")
    cr = b"\r" if first.endswith(b"\r") else b""
    fields = first[:len(first) - len(cr)].split(b"\t")
    if any(f.startswith(b"SO:") for f in fields):
        fields = [b"SO:coordinate" if f.startswith(b"SO:") else f for f in fields]
    else:
        fields.append(b"SO:coordinate")
    return b"\t".join(fields) + cr + nl + rest


def header_blob(header: bytes) -> Tuple[bytes, List[Tuple[str, int]]]:
    """the front of the uncompressed stream: magic, l_text, text, n_ref, (l_name, name NUL, l_ref) per reference"""
    refs = parse_sq(header)
    text = header_text(header)
    out = [b"BAM\1", struct.pack("<i", len(text)), text, struct.pack("<i", len(refs))]
    for name, length in refs:
        nm = name.encode("latin-1") + b"\0"
        out += [struct.pack("<i", len(nm)), nm, struct.pack("<i", length)]
    return b"".join(out), refs


def reg2bin(beg: int, end: int) -> int:
    """SAM specification 5.3; [beg, end) 0-based"""
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def encode_record(line: str, refid_of: Dict[str, int]) -> Tuple[Tuple[int, int, int], bytes, int, int, int]:
    """one line of ``<sample>.sam`` -> ((refID, pos, reverse), the BAM record with its block_size, refID, pos, end)"""
    f = line.split("\t")
    qname, flag, rname, start, seq = f[0], int(f[1]), f[2], int(f[3]), f[9]
    tags = dict((x[:2], x[5:]) for x in f[11:])
    if rname not in refid_of:
        raise ValueError(f"--sorted-bam: reads lie on '{rname}', which no @SQ line of the header names")
    if len(qname) > 254:
        raise ValueError(f"--sorted-bam: the QNAME of a read of {len(qname.rsplit('_', 1)[0])} nt exceeds 254 characters (BAM's l_read_name is one byte)")
    n, pos, refid = len(seq), start - 1, refid_of[rname]
    if pos < 0 or pos + n > MAX_POS:
        raise ValueError("--sorted-bam: a read lies outside [1, 2^29] of its reference: a BAM index cannot hold it")
    assert f[5] == f"{n}M" and f[10] == "I" * n and f[4] == "255" and flag in (0, 16)
    codes = [_CODE.get(ch, 15) for ch in seq] + [0]
    packed = bytes((codes[2 * k] << 4) | codes[2 * k + 1] for k in range((n + 1) // 2))
    body = struct.pack("<iiBBHHHiiii", refid, pos, len(qname) + 1, 255, reg2bin(pos, pos + n), 1, flag, n, -1, -1, 0)
    body += qname.encode() + b"\0" + struct.pack("<I", n << 4) + packed + bytes([40]) * n
    body += b"XAC" + bytes([int(tags["XA"])]) + b"MDZ" + tags["MD"].encode() + b"\0" + b"NMC" + bytes([int(tags["NM"])])
    return (refid, pos, 1 if flag & 16 else 0), struct.pack("<i", len(body)) + body, refid, pos, pos + n


def bgzf_member(data: bytes, level: int = 6) -> bytes:
    z = zlib.compressobj(level, zlib.DEFLATED, -15)
    cdata = z.compress(data) + z.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(cdata) + 25) + cdata +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def build_bai(n_ref: int, records: Sequence[Tuple[int, int, int, int, int]]) -> bytes:
    """The index from the records in file order: (refID, pos, end, virtual offset of the record, virtual offset of its end)."""
    out = [b"BAI\1", struct.pack("<i", n_ref)]
    per_ref: List[List[Tuple[int, int, int, int]]] = [[] for _ in range(n_ref)]
    for refid, pos, end, vb, ve in records:
        per_ref[refid].append((pos, end, vb, ve))
    for recs in per_ref:
        bins: Dict[int, List[List[int]]] = {}
        lin: List[int] = []
        prev = -1
        for pos, end, vb, ve in recs:
            b = reg2bin(pos, end)
            ch = bins.setdefault(b, [])
            if ch and (b == prev or ch[-1][1] == vb):
                ch[-1][1] = ve
            else:
                ch.append([vb, ve])
            prev = b
            w1 = (end - 1) >> 14
            lin += [-1] * (w1 + 1 - len(lin))
            for w in range(pos >> 14, w1 + 1):
                if lin[w] < 0:
                    lin[w] = vb
        for w in range(len(lin) - 2, -1, -1):
            if lin[w] < 0:
                lin[w] = lin[w + 1]
        out.append(struct.pack("<i", len(bins) + (1 if recs else 0)))
        for b in sorted(bins):
            out.append(struct.pack("<Ii", b, len(bins[b])) + b"".join(struct.pack("<QQ", *c) for c in bins[b]))
        if recs:
            out.append(struct.pack("<IiQQQQ", 37450, 2, recs[0][2], recs[-1][3], len(recs), 0))
        out.append(struct.pack("<i", len(lin)) + b"".join(struct.pack("<Q", v) for v in lin))
    out.append(struct.pack("<Q", 0))
    return b"".join(out)


def format_bam_host(sam_body: bytes, header: bytes, block_bytes: int = BLOCK_BYTES, level: int = 6) -> Tuple[bytes, bytes]:
    """(``<sample>_sorted.bam``, ``<sample>_sorted.bai``) from the lines of ``<sample>.sam`` below its header (``sam_export.
    format_sam_host``) and the ``--sam-header`` file's bytes.  Slow on purpose: one Python object per record."""
    blob, refs = header_blob(header)
    refid_of = {name: k for k, (name, _) in enumerate(refs)}
    recs = [encode_record(line, refid_of) for line in sam_body.decode().split("\n") if line]
    recs.sort(key=lambda r: r[0])  # (stable: ties keep the file's row order, a row's copies their k order)
    stream = blob + b"".join(r[1] for r in recs)
    members, coff, at = [], [], 0
    for u in range(0, len(stream), block_bytes):
        coff.append(at)
        members.append(bgzf_member(stream[u:u + block_bytes], level))
        at += len(members[-1])
    coff.append(at)  # the EOF block
    voff = lambda u: (coff[u // block_bytes] << 16) | (u % block_bytes) if u < len(stream) else coff[-1] << 16
    table, u = [], len(blob)
    for _, rec, refid, pos, end in recs:
        table.append((refid, pos, end, voff(u), voff(u + len(rec))))
        u += len(rec)
    return b"".join(members) + BGZF_EOF, build_bai(len(refs), table)


def refid_tables(casc, organism: str, refs: Sequence[Tuple[str, int]]):
    """(flat int32 array, int64 offsets [n_pass + 1]): every pass's chromosome index (``sam_export.pass_tables``) -> refID, -1 when
    no ``@SQ`` names the chromosome (an error only if a kept row lies there: the device call decides)"""
    classes, arr, keep = sam_export.pass_tables(casc, organism)
    refid_of = {name: k for k, (name, _) in enumerate(refs)}
    per_pass: Dict[int, np.ndarray] = {}
    for p, a in zip(classes.tolist(), keep):
        n_chrom = int(arr[p].n_chrom)
        names = FlatSeqs(a["chrom_data"], a["chrom_off"]).to_list() if n_chrom else []
        per_pass[p] = np.asarray([refid_of.get(nm, -1) for nm in names], dtype=np.int32)
    off = np.zeros(casc.n_pass + 1, dtype=np.int64)
    for p in range(casc.n_pass):
        off[p + 1] = off[p] + (per_pass[p].size if p in per_pass else 0)
    flat = np.concatenate([per_pass[p] for p in sorted(per_pass)] + [np.zeros(1, np.int32)]).astype(np.int32)
    return flat, off


def write_sample(casc, uniq, res, order: np.ndarray, sample: int, bam_path, bai_path, header: bytes, organism: str,
                 threads: Optional[int] = None):
    """One sample's pair of files through ``mirge_bam_write_device``; -> (records, uncompressed bytes, bytes of the .bam).
    ``MIRGE_BAM_DEFLATE``, read per call, names the route: ``device`` (the default), ``dynamic``, ``tight`` or ``host``"""
    blob, refs = header_blob(header)
    classes, arr, _keep = sam_export.pass_tables(casc, organism)
    order = np.ascontiguousarray(order, dtype=np.int64)
    if classes.size == 0:  # no library of any class that writes records: the header alone
        bam, bai = format_bam_host(b"", header)
        Path(bam_path).write_bytes(bam)
        Path(bai_path).write_bytes(bai)
        return 0, len(blob), len(bam)
    flat, off = refid_tables(casc, organism, refs)
    n_rec, n_stream, n_file = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    _ffi._check(_ffi.load().mirge_bam_write_device(
        casc.ctx._h, uniq._h, res._h, order if order.size else None, sample, classes, classes.size, arr, casc.n_pass, flat, off, len(refs),
        str(bam_path).encode(), str(bai_path).encode(), blob, len(blob), threads if threads else _ffi.gz_threads(), C.byref(n_rec),
        C.byref(n_stream), C.byref(n_file)), "mirge_bam_write_device")
    return int(n_rec.value), int(n_stream.value), int(n_file.value)


def run(args, workDir, base_names, casc, uniq, res, order, tm: Optional[dict] = None) -> dict:
    """``--sorted-bam``: ``<sample>_sorted.bam`` and ``<sample>_sorted.bai`` for every sample of the run (fastpath.reports)"""
    workDir = Path(workDir)
    t0 = time.perf_counter()
    hfile = getattr(args, "sam_header", None)
    if not hfile:
        raise ValueError("--sorted-bam requires --sam-header FILE with the @SQ lines of the genome the libraries were built on")
    with open(hfile, "rb") as fh:
        header = fh.read()
    parse_sq(header)
    files = {}
    for s, name in enumerate(base_names):
        bam, bai = workDir / (str(name) + "_sorted.bam"), workDir / (str(name) + "_sorted.bai")
        n_rec, n_stream, n_file = write_sample(casc, uniq, res, order, s, bam, bai, header, args.organism_name)
        files[str(name)] = dict(bam=str(bam), bai=str(bai), records=n_rec, stream_bytes=n_stream, bytes=n_file)
    if tm is not None:
        tm["sorted_bam_s"] = time.perf_counter() - t0
    return files
