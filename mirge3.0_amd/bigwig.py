"""Per-sample genome coverage as bigWig (``<sample>.bw``, or ``<sample>.plus.bw`` / ``<sample>.minus.bw``; ``--coverage-bigwig`` beside
``--coverage``) -- host side of ``mirge_bigwig_write_device`` and ``mirge_bigwig_from_intervals``.

The specification (there is no kent tool and no pyBigWig in this project's world; the sentences below ARE the format):

* bigWig version 4, little-endian, one file per strand.  The intervals are exactly the runs of ``--coverage`` (``coverage``): one
  bedGraph item ``(chromId, start, end, float32(depth))`` per run, neighbours that round to one float stay separate.  ``float32`` rounds
  to nearest even from the 64-bit depth.
* Chromosomes: ALL ``@SQ`` names of ``--sam-header FILE``, sorted by bytes; ``chromId`` = position in that order (not the ``@SQ`` order
  of the bedGraph).  Sizes are the ``LN`` values, at most 2^32 - 1; a run that ends beyond its ``LN`` is an error.
* Layout in file order:
    1. header, 64 bytes: magic 0x888FFC26 u32, version 4 u16, zoomLevels u16, chromosomeTreeOffset u64, fullDataOffset u64,
       fullIndexOffset u64, fieldCount 0 u16, definedFieldCount 0 u16, autoSqlOffset 0 u64, totalSummaryOffset u64, uncompressBufSize
       u32, extensionOffset 0 u64
    2. zoom headers, 24 bytes per kept level: reductionLevel u32, reserved 0 u32, dataOffset u64, indexOffset u64
    3. total summary, 40 bytes: basesCovered u64, minVal, maxVal, sumData, sumSquares as doubles
    4. chromosome B+ tree: header 32 bytes (magic 0x78CA8C91, blockSize B = min(256, n), keySize = longest name, valSize 8, itemCount n
       u64, reserved 0 u64); node = isLeaf u8, reserved u8, count u16, items; leaf item = key NUL-padded to keySize, chromId u32,
       chromSize u32; inner item = first key of the child, child file offset u64.  Leaves are level 0, a node of level l covers
       B^(l+1) consecutive items, as many levels as one root needs; levels root first, each in key order, every node zero-padded to B
       items
    5. data: u64 section count, then the sections in (chromId, start) order.  A section = up to S = 1024 consecutive runs of ONE
       chromosome (``MIRGE_BW_SECTION_ITEMS``: 1 .. 1024): 24-byte header (chromId, chromStart, chromEnd, itemStep 0, itemSpan 0 as
       u32, type 1 u8, reserved 0 u8, itemCount u16) and the items (start u32, end u32, value float32)
    6. data index (R-tree): header 48 bytes (magic 0x2468ACE0, blockSize 256 u32, itemCount u64, startChromIx, startBase, endChromIx,
       endBase u32 -- the first section's start and the largest (chromId, end); zeros without a section --, endFileOffset u64 = where
       the indexed data ends, itemsPerSlot 1 u32, reserved 0 u32); node = isLeaf u8, reserved u8, count u16; leaf item 32 bytes = the
       section's four bounds, dataOffset u64, dataSize u64; inner item 24 bytes = the bounds over the child (start of its first item,
       lexicographic maximum of (chromId, end)), child offset u64.  Bulk-loaded: a leaf holds 256 consecutive sections, a node of level
       l 256^(l+1); levels root first, leaves last; every node padded to 256 items; without a section one empty leaf
    7. per kept zoom level: at dataOffset a u32 record count and blocks of up to S records of one chromosome; at indexOffset an R-tree
       of the same kind over the blocks
    8. the magic once more, u32
  A sample without a run: header, total summary of zeros, tree, section count 0, the empty index, magic; zoomLevels 0.
* Blocks (sections and zoom blocks alike).  Compressed, a block is one zlib stream: 0x78 0x01, ONE deflate block (fixed Huffman, or
  stored when that is not smaller), the Adler-32 of the uncompressed bytes big-endian.  ``uncompressBufSize`` = the largest
  uncompressed block.  ``MIRGE_BW_DEFLATE=none`` writes the blocks raw and ``uncompressBufSize`` 0; any value but ``device`` / ``none``
  is an error.
* Zoom level k has reduction R_k = base * 4^k for k < 8 and R_k <= 2^20 (``MIRGE_BW_ZOOM_BASE``, default 64).  Bin j of a chromosome is
  [j R, min((j + 1) R, LN)); a bin writes a record iff some run overlaps it: chromId, start, end (the bin's bounds), validCount (the
  overlapped bases) u32, minVal, maxVal, sumData, sumSquares float32.  With ov the overlap and v the item's float as a double, over the
  overlapping runs in ascending order in doubles: sum += ov * v; sq += ov * (v * v); every product and every sum rounded on its own (no
  fused multiply-add), cast to float32 at the end.  Level k is kept iff 2 n_k <= n_(k-1) (n_(-1) = the file's runs); the levels end
  at the first that fails.
* Total summary: per section one pass in item order accumulates the same two sums with ov = the item's length, min, max and bases;
  the sections' partials are added in section order in doubles.

``write_host`` is the slow NumPy / struct writer of that file (compressed: Python's zlib, so only ``none`` is byte-comparable with the
device); the device route is ``csrc/kernels_bw.hpp`` + ``csrc/native_bw.hpp`` with the host bookkeeping of ``csrc/bw_layout.hpp``.
"""
from __future__ import annotations

import os
import struct
import time
import zlib
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MAGIC, TREE_MAGIC, INDEX_MAGIC = 0x888FFC26, 0x78CA8C91, 0x2468ACE0
MAX_LN = 2 ** 32 - 1
MAX_SECTION, RTREE_BLOCK, MAX_LEVELS, MAX_REDUCTION = 1024, 256, 8, 1 << 20


def env_settings(section_items: Optional[int] = None, zoom_base: Optional[int] = None, deflate: Optional[str] = None) -> Tuple[int, int, str]:
    """(S, zoom base, deflate route) from the arguments or ``MIRGE_BW_SECTION_ITEMS`` / ``MIRGE_BW_ZOOM_BASE`` / ``MIRGE_BW_DEFLATE``"""
    S = int(os.environ.get("MIRGE_BW_SECTION_ITEMS", MAX_SECTION)) if section_items is None else int(section_items)
    base = int(os.environ.get("MIRGE_BW_ZOOM_BASE", 64)) if zoom_base is None else int(zoom_base)
    mode = os.environ.get("MIRGE_BW_DEFLATE", "device") if deflate is None else deflate
    if not 1 <= S <= MAX_SECTION:
        raise ValueError("MIRGE_BW_SECTION_ITEMS: 1 to 1024")
    if not 1 <= base <= MAX_REDUCTION:
        raise ValueError("MIRGE_BW_ZOOM_BASE: 1 to 2^20")
    if mode not in ("device", "none"):
        raise ValueError(f"MIRGE_BW_DEFLATE: device or none, not {mode!r}")
    return S, base, mode


def chrom_ids(names: Sequence[str], sizes: Sequence[int]) -> np.ndarray:
    """rank -> chromId: the position of ``names[rank]`` among all names sorted by bytes; refuses a name twice and a size beyond 2^32 - 1"""
    keys = [n.encode("latin-1") for n in names]
    if len(set(keys)) != len(keys):
        raise ValueError("bigWig: a chromosome name twice")
    if len(keys) != len(sizes) or any(not 0 <= int(s) <= MAX_LN for s in sizes):
        raise ValueError("bigWig: one size of at most 2^32 - 1 per chromosome")
    order = sorted(range(len(keys)), key=lambda r: keys[r])
    cid = np.zeros(len(keys), dtype=np.int64)
    cid[order] = np.arange(len(keys))
    return cid


def parse_sizes(header: Optional[bytes]) -> List[Tuple[str, int]]:
    """(name, LN) of the ``@SQ`` lines in file order; no line, a line without SN: / LN:, an LN above 2^32 - 1 or a name twice raise"""
    refs: List[Tuple[str, int]] = []
    seen = set()
    for line in (header or b"").decode("latin-1").split("\n"):
        if not line.startswith("@SQ"):
            continue
        f = {x[:2]: x[3:] for x in line.rstrip("\r").split("\t")[1:] if len(x) >= 3 and x[2] == ":"}
        if "SN" not in f or not f.get("LN", "").isdigit() or int(f["LN"]) < 1:
            raise ValueError(f"--coverage-bigwig: an @SQ line needs SN: and LN: ({line!r})")
        if int(f["LN"]) > MAX_LN:
            raise ValueError(f"--coverage-bigwig: @SQ SN:{f['SN']} has LN:{f['LN']}, above 2^32 - 1: a bigWig cannot hold it")
        if f["SN"] in seen:
            raise ValueError(f"--coverage-bigwig: @SQ SN:{f['SN']} twice")
        seen.add(f["SN"])
        refs.append((f["SN"], int(f["LN"])))
    if not refs:
        raise ValueError("--coverage-bigwig needs --sam-header FILE with @SQ SN:/LN: lines (the chromosome sizes come from there)")
    return refs


# ---- the slow writer
def _chrom_tree(keys: List[bytes], sizes: List[int], at: int) -> bytes:
    """the B+ tree over the sorted names ``keys`` (chromId = index), placed at file offset ``at``"""
    n = len(keys)
    B, ks = min(256, n), max(len(k) for k in keys)
    out = [struct.pack("<IIIIQQ", TREE_MAGIC, B, ks, 8, n, 0)]
    counts = [(n + B - 1) // B]
    while counts[-1] > 1:
        counts.append((counts[-1] + B - 1) // B)
    node = 4 + B * (ks + 8)
    start = {}  # level -> file offset of its first node
    pos = at + 32
    for lv in range(len(counts) - 1, -1, -1):
        start[lv] = pos
        pos += counts[lv] * node
    for lv in range(len(counts) - 1, -1, -1):
        span = B ** (lv + 1)
        for k in range(counts[lv]):
            lo, hi = k * span, min(n, (k + 1) * span)
            if lv == 0:
                items = [keys[i].ljust(ks, b"\0") + struct.pack("<II", i, sizes[i]) for i in range(lo, hi)]
            else:
                sub = span // B
                items = [keys[i].ljust(ks, b"\0") + struct.pack("<Q", start[lv - 1] + (i // sub) * node) for i in range(lo, hi, sub)]
            out.append((struct.pack("<BBH", 1 if lv == 0 else 0, 0, len(items)) + b"".join(items)).ljust(node, b"\0"))
    return b"".join(out)


def _rtree(blocks: List[Tuple[int, int, int, int, int]], at: int, data_end: int) -> bytes:
    """the R-tree over ``blocks`` = (chromId, start, end, file offset, bytes), placed at file offset ``at``"""
    n = len(blocks)
    if n:
        top = max((b[0], b[2]) for b in blocks)
        head = struct.pack("<IIQIIIIQII", INDEX_MAGIC, RTREE_BLOCK, n, blocks[0][0], blocks[0][1], top[0], top[1], data_end, 1, 0)
    else:
        head = struct.pack("<IIQIIIIQII", INDEX_MAGIC, RTREE_BLOCK, 0, 0, 0, 0, 0, data_end, 1, 0)
    counts = [max(1, (n + RTREE_BLOCK - 1) // RTREE_BLOCK)]
    while counts[-1] > 1:
        counts.append((counts[-1] + RTREE_BLOCK - 1) // RTREE_BLOCK)
    size = lambda lv: 4 + RTREE_BLOCK * (32 if lv == 0 else 24)
    start, pos = {}, at + 48
    for lv in range(len(counts) - 1, -1, -1):
        start[lv] = pos
        pos += counts[lv] * size(lv)
    out = [head]
    for lv in range(len(counts) - 1, -1, -1):
        span = RTREE_BLOCK ** (lv + 1)
        for k in range(counts[lv]):
            lo, hi = k * span, min(n, (k + 1) * span)
            items = []
            if lv == 0:
                for b in blocks[lo:hi]:
                    items.append(struct.pack("<IIIIQQ", b[0], b[1], b[0], b[2], b[3], b[4]))
            else:
                sub = span // RTREE_BLOCK
                for i in range(lo, hi, sub):
                    part = blocks[i:min(n, i + sub)]
                    top = max((b[0], b[2]) for b in part)
                    items.append(struct.pack("<IIIIQ", part[0][0], part[0][1], top[0], top[1], start[lv - 1] + (i // sub) * size(lv - 1)))
            out.append((struct.pack("<BBH", 1 if lv == 0 else 0, 0, len(items)) + b"".join(items)).ljust(size(lv), b"\0"))
    return b"".join(out)


def _pack(payload: bytes, compress: bool, level: int) -> bytes:
    return zlib.compress(payload, level) if compress else payload


def zoom_records(cid: int, ln: int, start: Sequence[int], end: Sequence[int], val: Sequence[float], R: int) -> List[tuple]:
    """the records of one chromosome's runs (ascending, values as Python floats of the float32) at reduction R:
    (chromId, bin start, bin end, validCount, min, max, sum, sq) with min .. sq as float32"""
    recs: List[list] = []
    cur = -1
    for s, e, v in zip(start, end, val):
        for j in range(s // R, (e - 1) // R + 1):
            b0, b1 = j * R, min((j + 1) * R, ln)
            ov = min(e, b1) - max(s, b0)
            if j != cur:
                recs.append([cid, b0, b1, 0, v, v, 0.0, 0.0])
                cur = j
            r = recs[-1]
            r[3] += ov
            r[4], r[5] = min(r[4], v), max(r[5], v)
            r[6] = r[6] + float(ov) * v
            r[7] = r[7] + float(ov) * (v * v)
    return [(r[0], r[1], r[2], r[3], np.float32(r[4]), np.float32(r[5]), np.float32(r[6]), np.float32(r[7])) for r in recs]


def write_host(runs: Dict[str, np.ndarray], names: Sequence[str], sizes: Sequence[int], strand: Optional[int] = None,
               section_items: Optional[int] = None, zoom_base: Optional[int] = None, compress: bool = False, level: int = 6) -> bytes:
    """The bigWig file of ``runs`` (``coverage.coverage_host``'s arrays; of strand ``strand`` only, when given) with the chromosome
    names and sizes in rank order.  ``compress``: zlib streams of Python's zlib at ``level``, else raw blocks (MIRGE_BW_DEFLATE=none)."""
    S, base, _ = env_settings(section_items, zoom_base, "none")
    cid_of = chrom_ids(names, sizes)
    keys = sorted(n.encode("latin-1") for n in names)
    size_by_cid = [0] * len(names)
    for r, c in enumerate(cid_of.tolist()):
        size_by_cid[c] = int(sizes[r])
    if not names:
        raise ValueError("bigWig: at least one chromosome")
    pick = np.ones(runs["chrom"].size, bool) if strand is None else (runs["strand"] == strand)
    ch = cid_of[runs["chrom"][pick].astype(np.int64)] if pick.any() else np.zeros(0, np.int64)
    st, en = runs["start"][pick].astype(np.int64), runs["end"][pick].astype(np.int64)
    val32 = runs["depth"][pick].astype(np.int64).astype(np.float32)
    order = np.lexsort((st, ch))
    ch, st, en, val32 = ch[order], st[order], en[order], val32[order]
    for c, e in zip(ch.tolist(), en.tolist()):
        if e > size_by_cid[c]:
            raise ValueError(f"bigWig: a run on '{keys[c].decode('latin-1')}' ends at {e}, beyond its LN {size_by_cid[c]}")
    n_runs = int(ch.size)
    per_chrom = []  # (chromId, lo, hi) of the chromosomes with runs, in chromId order
    if n_runs:
        cut = np.flatnonzero(np.diff(ch)) + 1
        for lo, hi in zip(np.concatenate([[0], cut]).tolist(), np.concatenate([cut, [n_runs]]).tolist()):
            per_chrom.append((int(ch[lo]), lo, hi))
    # ---- sections with their partial summaries
    sections = []  # (chromId, start, end, payload)
    bases, vmin, vmax, ssum, ssq = 0, 0.0, 0.0, 0.0, 0.0
    for c, lo, hi in per_chrom:
        for a in range(lo, hi, S):
            b = min(hi, a + S)
            body = np.zeros(b - a, dtype=[("s", "<u4"), ("e", "<u4"), ("v", "<f4")])
            body["s"], body["e"], body["v"] = st[a:b], en[a:b], val32[a:b]
            head = struct.pack("<IIIIIBBH", c, int(st[a]), int(en[b - 1]), 0, 0, 1, 0, b - a)
            sections.append((c, int(st[a]), int(en[b - 1]), head + body.tobytes()))
            p_b, p_min, p_max, p_s, p_q = 0, float(val32[a]), float(val32[a]), 0.0, 0.0
            for s_, e_, v_ in zip(st[a:b].tolist(), en[a:b].tolist(), val32[a:b].tolist()):
                p_b += e_ - s_
                p_min, p_max = min(p_min, v_), max(p_max, v_)
                p_s = p_s + float(e_ - s_) * v_
                p_q = p_q + float(e_ - s_) * (v_ * v_)
            if not bases:
                vmin, vmax = p_min, p_max
            bases += p_b
            vmin, vmax, ssum, ssq = min(vmin, p_min), max(vmax, p_max), ssum + p_s, ssq + p_q
    # ---- zoom levels
    levels = []  # (R, records, blocks as (chromId, start, end, payload))
    prev = n_runs
    for k in range(MAX_LEVELS if n_runs else 0):
        R = base * 4 ** k
        if R > MAX_REDUCTION:
            break
        recs_by_chrom = [zoom_records(c, size_by_cid[c], st[lo:hi].tolist(), en[lo:hi].tolist(), val32[lo:hi].tolist(), R) for c, lo, hi in per_chrom]
        n_k = sum(len(r) for r in recs_by_chrom)
        if 2 * n_k > prev:
            break
        blocks = []
        for recs in recs_by_chrom:
            for a in range(0, len(recs), S):
                part = recs[a:a + S]
                blocks.append((part[0][0], part[0][1], part[-1][2], b"".join(struct.pack("<IIIIffff", *r) for r in part)))
        levels.append((R, n_k, blocks))
        prev = n_k
    # ---- the file
    Z = len(levels)
    tree_at = 64 + 24 * Z + 40
    tree = _chrom_tree(keys, size_by_cid, tree_at)
    data_at = tree_at + len(tree)
    out = [struct.pack("<Q", len(sections))]
    pos = data_at + 8
    placed, largest = [], 0
    for c, s_, e_, payload in sections:
        blob = _pack(payload, compress, level)
        placed.append((c, s_, e_, pos, len(blob)))
        out.append(blob)
        pos += len(blob)
        largest = max(largest, len(payload))
    index_at = pos
    idx = _rtree(placed, index_at, index_at)
    out.append(idx)
    pos += len(idx)
    zoom_heads = []
    for R, n_k, blocks in levels:
        z_at = pos
        out.append(struct.pack("<I", n_k))
        pos += 4
        placed = []
        for c, s_, e_, payload in blocks:
            blob = _pack(payload, compress, level)
            placed.append((c, s_, e_, pos, len(blob)))
            out.append(blob)
            pos += len(blob)
            largest = max(largest, len(payload))
        idx = _rtree(placed, pos, pos)
        zoom_heads.append(struct.pack("<IIQQ", R, 0, z_at, pos))
        out.append(idx)
        pos += len(idx)
    out.append(struct.pack("<I", MAGIC))
    header = struct.pack("<IHHQQQHHQQIQ", MAGIC, 4, Z, tree_at, data_at, index_at, 0, 0, 0, 64 + 24 * Z, largest if compress else 0, 0)
    summary = struct.pack("<Qdddd", bases, vmin, vmax, ssum, ssq)
    return header + b"".join(zoom_heads) + summary + tree + b"".join(out)


# ---- the device routes
def sample_paths(workDir, name: str, stranded: bool) -> List[Path]:
    workDir = Path(workDir)
    return [workDir / f"{name}.plus.bw", workDir / f"{name}.minus.bw"] if stranded else [workDir / f"{name}.bw"]


def _name_arrays(names: Sequence[str]):
    from .seqio import FlatSeqs
    nm = FlatSeqs.from_list(list(names))
    data = np.ascontiguousarray(nm.data) if nm.data.size else np.zeros(1, np.uint8)
    return data, np.ascontiguousarray(nm.offsets, dtype=np.int64)


def _stats(st: np.ndarray, n_files: int) -> List[dict]:
    out = []
    for f in range(n_files):
        v = st[f * 16:(f + 1) * 16].tolist()
        out.append(dict(sections=v[0], items=v[1], levels=v[2], bytes=v[3], max_depth=v[4], zoom_records=v[5:5 + v[2]]))
    return out


def _raise(rc: int, err: np.ndarray, names: Sequence[str], what: str):
    from . import _ffi
    if rc != 0 and int(err[0]) == 3:
        raise ValueError(f"--coverage-bigwig: a run on '{names[int(err[1])]}' ends at {int(err[2])}, beyond its LN {int(err[3])}")
    _ffi._check(rc, what)


def from_intervals(ctx, intervals: Dict[str, np.ndarray], names: Sequence[str], sizes: Sequence[int], stranded: bool, paths: Sequence) -> List[dict]:
    """``mirge_bigwig_from_intervals``: host intervals (``coverage.as_intervals``) -> one file, or two when stranded; per file
    dict(sections, items, levels, bytes, max_depth, zoom_records)"""
    from . import _ffi
    from .coverage import as_intervals
    iv = as_intervals(intervals["rank"], intervals["start"], intervals["len"], intervals["weight"], intervals["minus"])
    n = int(iv["rank"].size)
    paths = [str(p) for p in paths]
    if len(paths) != (2 if stranded else 1):
        raise ValueError("from_intervals: one path, or two when stranded")
    cid = np.ascontiguousarray(chrom_ids(names, sizes), dtype=np.int32)
    ln = np.ascontiguousarray(np.asarray(sizes, dtype=np.int64))
    nm_data, nm_off = _name_arrays(names)
    st, err = np.zeros(32, dtype=np.int64), np.zeros(4, dtype=np.int64)
    rc = _ffi.load().mirge_bigwig_from_intervals(
        ctx._h, n, *((iv[k] if n else None) for k in ("rank", "start", "len", "weight", "minus")), bool(stranded), len(names), nm_data, nm_off,
        ln, cid, paths[0].encode(), paths[1].encode() if stranded else None, st, err)
    _raise(rc, err, names, "mirge_bigwig_from_intervals")
    return _stats(st, len(paths))


def write_sample(casc, uniq, res, order: np.ndarray, sample: int, paths: Sequence, stranded: bool, organism: str,
                 sq: Sequence[Tuple[str, int]]) -> List[dict]:
    """One sample's file (``stranded``: its two files) through ``mirge_bigwig_write_device``; ``sq`` = (name, LN) in ``@SQ`` order, the
    chromosome order of ``coverage.write_sample``.  A data error is a ValueError and leaves no file."""
    from . import _ffi, coverage, sam_export
    paths = [str(p) for p in paths]
    if len(paths) != (2 if stranded else 1):
        raise ValueError("write_sample: one path, or two when stranded")
    sq_names, sizes = [n for n, _ in sq], [s for _, s in sq]
    classes, arr, _keep = sam_export.pass_tables(casc, organism)
    order = np.ascontiguousarray(order, dtype=np.int64)
    if classes.size == 0:  # no library of any class that has rows: empty files
        empty = dict(strand=np.zeros(0, np.uint8), chrom=np.zeros(0, np.int32), start=np.zeros(0, np.int64), end=np.zeros(0, np.int64),
                     depth=np.zeros(0, np.int64))
        _, _, mode = env_settings()
        for p in paths:
            with open(p, "wb") as fh:
                fh.write(write_host(empty, sq_names, sizes, compress=mode == "device"))
        return [dict(sections=0, items=0, levels=0, bytes=os.path.getsize(p), max_depth=0, zoom_records=[]) for p in paths]
    names, flat, off = coverage.rank_tables(casc, organism, sq_names)
    cid = np.ascontiguousarray(chrom_ids(sq_names, sizes), dtype=np.int32)
    ln = np.ascontiguousarray(np.asarray(sizes, dtype=np.int64))
    nm_data, nm_off = _name_arrays(names)
    st, err = np.zeros(32, dtype=np.int64), np.zeros(4, dtype=np.int64)
    rc = _ffi.load().mirge_bigwig_write_device(
        casc.ctx._h, uniq._h, res._h, order if order.size else None, sample, classes, classes.size, arr, casc.n_pass, flat, off, len(names),
        nm_data, nm_off, ln, cid, bool(stranded), paths[0].encode(), paths[1].encode() if stranded else None, st, err)
    if rc != 0 and int(err[0]) == 2:
        read = uniq.unpack().to_list()[int(err[1])]
        raise ValueError(f"--coverage-bigwig: read {read} on reference {coverage._reference_name(casc, int(err[2]), int(err[3]))} lies "
                         f"outside [1, 2^31 - 1] of its chromosome")
    if rc != 0 and int(err[0]) == 1:
        msg = _ffi.load().mirge_last_error().decode()
        raise ValueError("--coverage-bigwig: " + msg.split(": ", 1)[-1])
    _raise(rc, err, names, "mirge_bigwig_write_device")
    return _stats(st, len(paths))


def log_line(name: str, path, st: dict) -> str:
    zoom = ", ".join(str(n) for n in st["zoom_records"]) or "none"
    note = "; depths of 2^24 and above are rounded to float32" if st["max_depth"] >= 2 ** 24 else ""
    return (f"coverage-bigwig {name} {Path(path).name}: {st['sections']} sections, {st['items']} items, {st['levels']} zoom levels "
            f"(records: {zoom}), {st['bytes']} bytes{note}\n")


def run(args, workDir, base_names, casc, uniq, res, order, tm: Optional[dict] = None, sample: Optional[int] = None) -> dict:
    """``--coverage-bigwig``: the ``.bw`` file(s) of every sample (``sample``: of that one), called per sample BEFORE its bedGraph call
    (fastpath.reports through ``coverage.run``'s loop), so that a data error leaves no file of that sample"""
    workDir = Path(workDir)
    t0 = time.perf_counter()
    stranded = getattr(args, "coverage", None) == "stranded"
    with open(args.sam_header, "rb") as fh:
        sq = parse_sizes(fh.read())
    files = {}
    with open(workDir / "run.log", "a+") as log:
        for s, name in enumerate(base_names):
            if sample is not None and s != sample:
                continue
            paths = sample_paths(workDir, str(name), stranded)
            stats = write_sample(casc, uniq, res, order, s, paths, stranded, args.organism_name, sq)
            files[str(name)] = dict(paths=[str(p) for p in paths], files=stats)
            for p, st in zip(paths, stats):
                log.write(log_line(str(name), p, st))
    if tm is not None:
        tm["coverage_bigwig_s"] = tm.get("coverage_bigwig_s", 0.0) + time.perf_counter() - t0
    return files
