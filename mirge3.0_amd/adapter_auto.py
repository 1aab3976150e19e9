"""``-a auto``: every sample's 3' adapter inferred from its own reads, before any sample is parsed.

The head of the FASTQ (``head_text``: the first MIRGE_ADAPTER_HEAD_READS records, host work of a few tens of MB) is parsed on the
device WITHOUT trimming and without a length filter, collapsed there into distinct reads with counts, and ``mirge_adapter_infer``
(csrc/native_adapter.hpp, csrc/kernels_adapter.hpp) reads the adapter off the k-mer spectrum with start positions: README,
"`-a auto`: the 3' adapter, inferred from the reads".  Independent of the streams of collapse.py.
"""
from __future__ import annotations

import os
import zlib
from pathlib import Path
from typing import List, Sequence

import numpy as np

from . import _ffi

HEAD_READS_DEFAULT = 1 << 18
HEAD_READS_MAX = 1 << 24
CSV_NAME = "adapter.auto.csv"
CSV_HEADER = "Sample,Adapter,Length,Support,Eligible,Records,Distinct\n"


def head_reads() -> int:
    """MIRGE_ADAPTER_HEAD_READS: records of a sample's head that ``-a auto`` looks at (default 2^18; 1 .. 2^24, else ValueError)"""
    v = os.environ.get("MIRGE_ADAPTER_HEAD_READS")
    if v is None or v == "":
        return HEAD_READS_DEFAULT
    if not v.isdigit() or not 1 <= int(v) <= HEAD_READS_MAX:
        raise ValueError(f"MIRGE_ADAPTER_HEAD_READS={v!r}: an integer from 1 to 2^24")
    return int(v)


def _cut(pieces: List[bytes], lines: int) -> bytes:
    """the pieces' text up to and with its ``lines``-th newline (all of it when it has fewer)"""
    text = b"".join(pieces)
    if text.count(b"\n") < lines:
        return text
    nl = np.flatnonzero(np.frombuffer(text, np.uint8) == 10)
    return text[:int(nl[lines - 1]) + 1]


def head_text(path, n: int, chunk: int = 1 << 20) -> bytes:
    """The first ``n`` FASTQ records (4 n lines; LF or CRLF) of a plain or ``.gz`` file, fewer when the file has fewer.  A ``.gz`` may be one
    member, several, or BGZF; it is inflated member by member only until the lines are there.  A ``.gz`` that ends inside a member
    gives what could be inflated."""
    lines, have, pieces = 4 * int(n), 0, []
    gz = str(path).endswith(".gz")
    with open(path, "rb") as fh:
        d = zlib.decompressobj(31) if gz else None
        while have < lines:
            raw = fh.read(chunk)
            if not raw:
                break
            if not gz:
                pieces.append(raw)
                have += raw.count(b"\n")
                continue
            while raw and have < lines:
                try:
                    out = d.decompress(raw)
                except zlib.error:  # (damaged behind what was inflated: the head so far)
                    raw, lines = b"", have
                    break
                if out:
                    pieces.append(out)
                    have += out.count(b"\n")
                raw = b""
                if d.eof:  # the next member, if there is one (a BGZF file has thousands)
                    raw = d.unused_data
                    d = zlib.decompressobj(31)
    return _cut(pieces, 4 * int(n))


def infer_sample(ctx: "_ffi.Context", path, n: int = None) -> dict:
    """-> the fields of ``mirge_adapter`` (``seq`` empty: no adapter) plus ``records`` (FASTQ records looked at) and ``distinct`` (reads of
    their dictionary)"""
    text = head_text(path, head_reads() if n is None else n)
    raw, n_rec = _ffi.DeviceReads.parse(ctx, text, 1, 0, None)
    uniq = None
    try:
        uniq = raw.collapse()
        res = uniq.adapter_infer()
        res["records"], res["distinct"] = int(n_rec), len(uniq)
        return res
    finally:
        if uniq is not None:
            uniq.close()
        raw.close()


def csv_text(names: Sequence[str], results: Sequence[dict]) -> str:
    """``adapter.auto.csv``: one line per sample in ``-s`` order; a sample without an adapter has an empty ``Adapter`` field"""
    return CSV_HEADER + "".join(f"{name},{r['seq']},{r['len']},{r['support']},{r['eligible']},{r['records']},{r['distinct']}\n"
                                for name, r in zip(names, results))


def log_line(name: str, r: dict) -> str:
    return f"adapter auto {name}: {r['seq']} (support {r['support']} of {r['eligible']} eligible reads in the first {r['records']} records)"


def infer_all(ctx: "_ffi.Context", files: Sequence[str], names: Sequence[str], workDir, say) -> List[str]:
    """All samples, before any of them is parsed: writes ``adapter.auto.csv`` and one run.log line per sample (``say``); a sample without
    an adapter ends the run (SystemExit) with a message that names it and its T."""
    results = [infer_sample(ctx, f) for f in files]
    with open(Path(workDir) / CSV_NAME, "w") as fh:
        fh.write(csv_text(names, results))
    for name, r in zip(names, results):
        if r["seq"]:
            say(log_line(name, r))
    bad = [(name, r) for name, r in zip(names, results) if not r["seq"]]
    if bad:
        name, r = bad[0]
        raise SystemExit(f"ERROR: -a auto found no adapter in sample {name} (T = {r['eligible']} eligible reads in the first {r['records']} records, "
                         f"{r['candidates']} seed candidates): give the 3' adapter with -a SEQ, or no -a for reads that carry none"
                         + (f"; also without an adapter: {', '.join(n for n, _ in bad[1:])}" if len(bad) > 1 else ""))
    return [r["seq"] for r in results]


def refusal(args) -> str:
    """Why this command line's use of the literal ``auto`` is refused, or "" (``cli.parse_args`` hands it to ``ap.error`` before anything is
    written).  Legal: ``-a auto`` as the only ``-a``, optionally followed by one ``-g SEQ``."""
    adapters = [tuple(a) if isinstance(a, (tuple, list)) else ("back", a) for a in (getattr(args, "adapters", None) or [])]
    for kind, q in adapters:
        parts = str(q).replace("^", "").replace("$", "").split("...")
        if q != "auto" and "auto" in parts:
            return "-a auto is a plain 3' adapter: not together with '^', '$' or a linked form (A...B)"
    where = [i for i, (kind, q) in enumerate(adapters) if q == "auto"]
    if not where:
        return ""
    if any(adapters[i][0] == "front" for i in where):
        return "-g auto: only the 3' adapter is inferred (-a auto)"
    if sum(1 for kind, _ in adapters if kind == "back") > 1:
        return "-a auto is the only -a of a run (every sample gets its own sequence)"
    if where[0] != 0:
        return "-a auto comes first: a -g SEQ may follow it, not precede it"
    if len(adapters) > 2:
        return "-a auto takes at most one -g SEQ behind it"
    if getattr(args, "save_pkl", False) or getattr(args, "resume", False) or getattr(args, "backend", "gpu") == "bowtie":
        return "-a auto runs on the device-resident route: not together with -spl / -rr / --backend bowtie"
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return "-a auto is a single-process option"
    try:
        head_reads()
    except ValueError as e:
        return str(e)
    return ""


def wanted(args) -> bool:
    return any((tuple(a) if isinstance(a, (tuple, list)) else ("back", a))[1] == "auto" for a in (getattr(args, "adapters", None) or []))
