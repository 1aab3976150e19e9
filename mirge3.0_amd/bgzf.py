"""``--bgzf-out``: the text of ``--sam-out`` and ``--coverage`` written as BGZF -- host side of ``mirge_bgzf_write``,
``mirge_sam_write_device_bgzf`` and ``mirge_coverage_write_device_bgzf`` (csrc/kernels_bgzf.hpp, csrc/native_bgzf.hpp).

There is no htslib here.  The sentences below are this project's specification of the files, as ``bam_export.py`` is for the ``.bai``.

**The switch.**  ``--bgzf-out`` is a flag, legal only with ``--sam-out`` and/or ``--coverage``.  Without it every byte of every output is
what it was.  With it every text file those two switches write is written as BGZF instead -- ``<sample>.sam.gz``;
``<sample>.bedgraph.gz``, or ``<sample>.plus.bedgraph.gz`` and ``<sample>.minus.bedgraph.gz`` -- and the plain file is not written.  Each
file gets a block index beside it, ``<name>.gz.gzi``.  bigWig and BAM outputs are untouched.

**Stream.**  S is the exact byte sequence the plain route writes to that file, the SAM header included.  B is the block size: 65280 by
default, ``MIRGE_BGZF_BLOCK_BYTES`` accepts 64 .. 65280 (for tests).

- Member b holds ``S[b*B : (b+1)*B]``; the last member may be short.
- The 28-byte BGZF EOF block follows the last member.
- An empty S gives a file of the EOF block alone.
- The file is a function of S and B only: it does not depend on ``MIRGE_SAM_CHUNK_BYTES``, ``MIRGE_COV_CHUNK_BYTES``, the tile sizes or
  timing.  With the flag a chunk therefore holds a whole number of blocks.
- In a stranded run each file is a stream of its own: the minus file's block 0 starts at the minus text's byte 0, wherever the plus
  strand's text ends inside a chunk.

**Member.**  One deflate block (RFC 1951) in a gzip member (RFC 1952) with the ``BC`` extra field: 18 bytes of header (magic 1f 8b, CM 8,
FLG 4, XLEN 6, ``B`` ``C``, SLEN 2, BSIZE = member bytes - 1), the block, CRC-32 and ISIZE.

- Each member is stored, fixed-Huffman or dynamic-Huffman.
- The rule is that of ``MIRGE_BAM_DEFLATE=dynamic``: the dynamic form is taken if and only if it is strictly smaller than the better of
  stored and fixed.
- No member exceeds ``n + 31`` bytes for its n bytes of S.
- Text has a skewed alphabet, so the code of the block's own is the default here and not an option.  The tight parse uses BAM's record
  structure and is out of scope.

**``.gzi``.**  Little-endian: a ``uint64`` count, then that many pairs of ``uint64`` (compressed offset, uncompressed offset), one pair per
member after the first and none for the EOF block.  This is the author's recollection of the layout ``bgzip -i`` writes; it is
UNCHECKED against htslib.

**Routes.**  ``MIRGE_BGZF_DEFLATE=device`` is the default.  ``host`` copies the text out as without the switch and deflates each block
with zlib level 6 on the threads ``MIRGE_GZ_THREADS`` sizes: the A/B route and the tests' second implementation; its members differ, its
decompressed bytes and its ``.gzi`` uncompressed offsets do not.  Any other value is an error, raised before a file is opened.

**Files.**  Every file is written as ``<name>.tmp`` and renamed when all files of the call are whole -- both strands and their
indexes; a failed call leaves nothing behind.  ``run.log``'s line per sample gains the compressed bytes and the count of members that
are stored, fixed and dynamic.

**Refusals**, raised before anything is written: the flag without ``--sam-out`` or ``--coverage``; the flag together with what those two
already refuse (``-spl``, ``-rr``, ``--backend bowtie``, a sharded run).  ``--sam-header``, ``--coverage-bigwig`` and ``--sorted-bam``
beside it behave as before.
"""
import ctypes as C
import os
import struct
import zlib
from typing import Dict, List, Tuple

import numpy as np

from . import _ffi

BLOCK_BYTES = 65280
EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
N_STATS = 8  # per file, of the native calls: file bytes, members stored, fixed, dynamic, members, stream bytes, 0, 0


def block_bytes() -> int:
    """B of this process: ``MIRGE_BGZF_BLOCK_BYTES`` or 65280; a value outside 64 .. 65280 is a ValueError"""
    v = os.environ.get("MIRGE_BGZF_BLOCK_BYTES")
    if not v:
        return BLOCK_BYTES
    try:
        b = int(v)
    except ValueError:
        b = -1
    if not 64 <= b <= BLOCK_BYTES:
        raise ValueError(f"MIRGE_BGZF_BLOCK_BYTES={v}: a BGZF block holds 64 .. {BLOCK_BYTES} bytes")
    return b


def route() -> str:
    """``MIRGE_BGZF_DEFLATE``: 'device' (the default) or 'host'; anything else is a ValueError"""
    v = os.environ.get("MIRGE_BGZF_DEFLATE") or "device"
    if v not in ("device", "host"):
        raise ValueError(f"MIRGE_BGZF_DEFLATE={v}: 'device' or 'host'")
    return v


def gz_path(path) -> str:
    return str(path) + ".gz"


def gzi_path(path) -> str:
    """the index beside a ``.gz`` file"""
    return str(path) + ".gzi"


def stats_dict(st) -> Dict[str, int]:
    """one file's eight numbers of a native call"""
    return dict(file_bytes=int(st[0]), stored=int(st[1]), fixed=int(st[2]), dynamic=int(st[3]), members=int(st[4]), stream_bytes=int(st[5]))


def members(data: bytes) -> List[dict]:
    """The structure of a BGZF file, checked: every member's magic, ``BC`` field, BSIZE, a deflate stream that ends with the member,
    CRC-32 and ISIZE; the EOF block last and nowhere else.  -> per member (the EOF block not among them) dict(offset, bsize, single,
    btype, payload, crc, isize); ``single``: the first deflate block is the final one (the device's members; zlib may write several),
    ``btype`` is that first block's."""
    data = bytes(data)
    out, at = [], 0
    while at < len(data):
        if len(data) - at < 28:
            raise ValueError(f"{len(data) - at} bytes at offset {at}: shorter than a BGZF member")
        hd = data[at:at + 18]
        if hd[:4] != b"\x1f\x8b\x08\x04" or hd[10:16] != b"\x06\x00BC\x02\x00":
            raise ValueError(f"no BGZF member at offset {at}")
        bsize = struct.unpack_from("<H", hd, 16)[0] + 1
        if bsize < 28 or at + bsize > len(data):
            raise ValueError(f"member at offset {at}: BSIZE {bsize} does not fit the file")
        cdata = data[at + 18:at + bsize - 8]
        crc, isize = struct.unpack_from("<II", data, at + bsize - 8)
        z = zlib.decompressobj(-15)
        payload = z.decompress(cdata)
        if not z.eof or z.unused_data:
            raise ValueError(f"member at offset {at}: its deflate stream does not end with its bytes")
        if len(payload) != isize or zlib.crc32(payload) != crc:
            raise ValueError(f"member at offset {at}: CRC-32 or ISIZE do not fit its bytes")
        out.append(dict(offset=at, bsize=bsize, single=bool(cdata[0] & 1), btype=(cdata[0] >> 1) & 3, payload=payload, crc=crc, isize=isize))
        at += bsize
    if not out or data[out[-1]["offset"]:] != EOF_BLOCK:
        raise ValueError("the file does not end with the BGZF EOF block")
    out.pop()
    if any(m["isize"] == 0 for m in out):
        raise ValueError("an empty member in front of the EOF block")
    return out


def read_gzi(data: bytes) -> List[Tuple[int, int]]:
    """the pairs (compressed offset, uncompressed offset) of a ``.gzi`` file"""
    data = bytes(data)
    if len(data) < 8:
        raise ValueError("a .gzi file holds at least its count")
    n = struct.unpack_from("<Q", data, 0)[0]
    if len(data) != 8 + 16 * n:
        raise ValueError(f".gzi: {n} pairs announced, {len(data)} bytes")
    v = struct.unpack_from(f"<{2 * n}Q", data, 8)
    return [(v[2 * k], v[2 * k + 1]) for k in range(n)]


def check_index(gz: bytes, gzi: bytes) -> List[dict]:
    """the invariant that holds a ``.gzi`` to its file: one pair per member after the first, each compressed offset on that member's
    magic, each uncompressed offset the summed ISIZE in front of it.  -> ``members(gz)``"""
    ms = members(gz)
    pairs = read_gzi(gzi)
    if len(pairs) != max(len(ms) - 1, 0):
        raise ValueError(f".gzi: {len(pairs)} pairs for {len(ms)} members")
    u = 0
    for k, m in enumerate(ms):
        if k and pairs[k - 1] != (m["offset"], u):
            raise ValueError(f".gzi: pair {k - 1} is {pairs[k - 1]}, member {k} lies at {(m['offset'], u)}")
        u += m["isize"]
    return ms


def write_host(stream: bytes, block: int = BLOCK_BYTES, level: int = 6) -> Tuple[bytes, bytes]:
    """The layout reference, with Python's zlib: ``stream`` in blocks of ``block`` bytes -> (the .gz file, its .gzi).  The members'
    deflate bytes are zlib's, so only the layout -- the blocks, the EOF block, the index -- is what the device writes."""
    stream = bytes(stream)
    if not 64 <= block <= BLOCK_BYTES:
        raise ValueError(f"a BGZF block holds 64 .. {BLOCK_BYTES} bytes")
    out, pairs = bytearray(), []
    for at in range(0, len(stream), block):
        part = stream[at:at + block]
        z = zlib.compressobj(level, zlib.DEFLATED, -15)
        cdata = z.compress(part) + z.flush()
        if len(cdata) > len(part) + 5:  # (zlib stores what it cannot shrink, but in blocks of its own choosing: one stored block here)
            cdata = b"\x01" + struct.pack("<HH", len(part), len(part) ^ 0xFFFF) + part
        if at:
            pairs.append((len(out), at))
        out += b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(cdata) + 25) + cdata
        out += struct.pack("<II", zlib.crc32(part), len(part))
    out += EOF_BLOCK
    gzi = struct.pack("<Q", len(pairs)) + b"".join(struct.pack("<QQ", c, u) for c, u in pairs)
    return bytes(out), gzi


def write_device(ctx, data, path, block: int = 0) -> Dict[str, int]:
    """``mirge_bgzf_write``: host bytes -> ``path`` and ``path + '.gzi'`` by the kernels of ``--bgzf-out`` (``block`` 0:
    ``MIRGE_BGZF_BLOCK_BYTES``); -> the file's numbers (``stats_dict``)"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    st = np.zeros(N_STATS, dtype=np.int64)
    _ffi._check(_ffi.load().mirge_bgzf_write(ctx._h, buf if buf.size else None, buf.size, int(block), str(path).encode(),
                                             gzi_path(path).encode(), st), "mirge_bgzf_write")
    return stats_dict(st)
