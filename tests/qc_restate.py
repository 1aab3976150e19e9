"""A slow, per-byte restatement of the ``--read-qc`` specification (the docstring of mirge3_amd/readqc.py), independent of the kernels: the
records of a text, the bounds the modifier chain leaves of each (restated here with the oracle's index functions and held against
``oracle.trim_stages``, which the trim tests trust), and the entries of the ``raw`` and ``trimmed`` views, in the form
``readqc.view_entries`` gives the device's tables: {(section, view, k1, k2, k3): value}."""
import numpy as np

import oracle

P, QMAX, LETTERS = 256, 93, "ACGTN"


def letter(byte: int) -> str:
    ch = chr(byte)
    if ch in "Aa":
        return "A"
    if ch in "Cc":
        return "C"
    if ch in "Gg":
        return "G"
    if ch in "TtUu":
        return "T"
    return "N"


def records(text: bytes, fmt: int):
    """[(b, e, qb, qe)]: the byte bounds of every record's sequence line and quality line (qb = qe = None without qualities) in ``text`` as
    the parser sees it -- blank space at the end of the file is no line, but as many empty lines as complete the last record are; a '\\r' at
    a line's end is still inside these bounds"""
    period, phase = {1: (4, 1), 2: (2, 1), 3: (1, 0)}[fmt]
    body = text.rstrip(b"\n\r \t")
    if not body:
        return []
    spare = max(0, min(text[len(body):].count(b"\n"), 8) - 1) if fmt != 3 else 0
    bounds, at = [], 0
    for line in body.split(b"\n"):
        bounds.append((at, at + len(line)))
        at += len(line) + 1
    while len(bounds) % period and spare:
        bounds.append((at, at))
        at += 1
        spare -= 1
    assert len(bounds) % period == 0, "not whole records"
    out = []
    for r in range(len(bounds) // period):
        b, e = bounds[r * period + phase]
        qb, qe = bounds[r * period + 3] if fmt == 1 else (None, None)
        out.append((b, e, qb, qe))
    return out


def device_text(text: bytes) -> bytes:
    """the bytes the bounds of ``records`` index: the text with the line ends that close its last record"""
    return text.rstrip(b"\n\r \t") + b"\n" * 8


def strip_cr(buf: bytes, b: int, e: int) -> int:
    return e - 1 if e > b and buf[e - 1] == 13 else e


def trimmed_bounds(seq: str, qual, opts: dict):
    """(lo, hi) of the read the chain leaves of ``seq``: quality trimming, a 3' adapter, N ends, cuts, in the chain's order (each step as
    ``oracle.trim_stages`` takes it); checked against that function's last stage"""
    lo, hi = 0, len(seq)
    base = opts.get("base", 33)
    if opts.get("q_back") is not None and qual is not None:
        a, b = oracle.quality_trim_index(qual, opts.get("q_front", 0), opts["q_back"], base)
        lo, hi = a, b
    if opts.get("adapter"):
        hit = oracle.adapter_locate_back(opts["adapter"], seq[lo:hi].upper(), opts.get("error_rate", 0.12), opts.get("overlap", 3))
        if hit is not None:
            hi = lo + hit[2]
    if opts.get("trim_n"):
        while lo < hi and seq[lo] in "Nn":
            lo += 1
        while hi > lo and seq[hi - 1] in "Nn":
            hi -= 1
    for c in opts.get("cut", []):
        if c > 0:
            lo = min(lo + c, hi)
        elif c < 0:
            hi = max(hi + c, lo)
    stages = oracle.trim_stages(seq, qual, opts)
    if stages:
        assert seq[lo:hi] == stages[-1], (seq, opts, seq[lo:hi], stages[-1])
    return lo, hi


def n_stages(opts, has_qual: bool) -> int:
    """modifiers in the chain (= virtual records per record under --trim-count per-modifier)"""
    if not opts:
        return 0
    return int(opts.get("q_back") is not None and has_qual) + int(bool(opts.get("adapter"))) + int(bool(opts.get("trim_n"))) + \
        sum(1 for c in opts.get("cut", []) if c)


def views(text: bytes, fmt: int, min_len: int = 0, opts: dict = None):
    """-> (buf, [per record: dict(line=(b, e), qline=(qb, qe) or None, trimmed=(vb, ve))]): byte bounds in ``buf`` = device_text(text), the
    lines after '\\r' stripping, qline None for a record without a usable quality line, trimmed = the read after the last modifier"""
    buf = device_text(text)
    out = []
    for b, e, qb, qe in records(text, fmt):
        e = strip_cr(buf, b, e)
        mismatch = False
        qline = None
        if qb is not None:
            qe = strip_cr(buf, qb, qe)
            mismatch = qe - qb != e - b
            qline = None if mismatch else (qb, qe)
        lo, hi = 0, e - b
        if opts and n_stages(opts, fmt == 1):
            qual = buf[qline[0]:qline[1]].decode("latin-1") if qline else None
            lo, hi = trimmed_bounds(buf[b:e].decode("latin-1"), qual, opts if fmt == 1 else {k: v for k, v in opts.items() if k != "q_back"})
        out.append(dict(line=(b, e), qline=qline, mismatch=mismatch, has_q=qb is not None, trimmed=(b + lo, b + hi)))
    return buf, out


def entries(text: bytes, fmt: int, min_len: int = 0, opts: dict = None):
    """the entries of the raw and the trimmed view of this text (scalars always, the quality ones only for FASTQ; table cells > 0)"""
    buf, recs = views(text, fmt, min_len, opts)
    base = (opts or {}).get("base", 33)
    out = {}
    scal = ["reads", "bases", "reads_with_N", "empty_reads"] + (["qual_clamped", "qual_length_mismatch"] if fmt == 1 else [])
    for view in ("raw", "trimmed"):
        for s in scal:
            out[(s, view, None, None, None)] = 0

    def add(section, view, k1=None, k2=None, k3=None, v=1):
        key = (section, view, k1, k2, k3)
        out[key] = out.get(key, 0) + v

    for rec in recs:
        for view in ("raw", "trimmed"):
            b, e = rec["line"] if view == "raw" else rec["trimmed"]
            L = e - b
            if view == "trimmed" and L < min_len:
                continue
            add("reads", view)
            add("bases", view, v=L)
            add("length", view, L)
            if rec["mismatch"]:
                add("qual_length_mismatch", view)
            if L == 0:
                add("empty_reads", view)
                continue
            ls = [letter(buf[p]) for p in range(b, e)]
            for p, l in enumerate(ls):
                add("base", view, min(p, P), l)
            if "N" in ls:
                add("reads_with_N", view)
            add("gc", view, (100 * (ls.count("G") + ls.count("C"))) // L)
            add("first", view, min(L, P), ls[0])
            if rec["qline"]:
                q0 = rec["qline"][0] + (b - rec["line"][0])
                total = 0
                for p in range(L):
                    q = buf[q0 + p] - base
                    if q < 0 or q > QMAX:
                        add("qual_clamped", view)
                        q = min(max(q, 0), QMAX)
                    total += q
                    add("qual", view, min(p, P), q)
                add("meanq", view, total // L)
    return {k: v for k, v in out.items() if v > 0 or k[2] is None}


def class_profile(passes, lengths, letters, counts, n_pass: int) -> np.ndarray:
    """NumPy restatement of ``mirge_qc_class_profile``: int64 [S][n_pass + 1][257][5][2] from per-read pass (-1: none), length, first letter
    (0 .. 4) and counts [n][S]"""
    counts = np.asarray(counts, dtype=np.int64)
    S = counts.shape[1]
    out = np.zeros((S, n_pass + 1, P + 1, 5, 2), dtype=np.int64)
    cls = np.where(np.asarray(passes) >= 0, passes, n_pass)
    lk = np.minimum(np.asarray(lengths), P)
    for s in range(S):
        np.add.at(out[s, :, :, :, 0], (cls, lk, letters), counts[:, s])
        np.add.at(out[s, :, :, :, 1], (cls, lk, letters), (counts[:, s] > 0).astype(np.int64))
    return out


def identities(e: dict) -> None:
    """what must hold of any expected or computed result"""
    for view in ("raw", "trimmed"):
        tot = lambda name: sum(v for k, v in e.items() if k[0] == name and k[1] == view and k[2] is not None)
        get = lambda name: e.get((name, view, None, None, None), 0)
        assert tot("length") == get("reads"), view
        assert tot("base") == get("bases"), view
        if ("qual_clamped", view, None, None, None) in e and get("qual_length_mismatch") == 0:
            assert tot("qual") == get("bases"), view
        assert tot("first") + get("empty_reads") == get("reads"), view
        assert tot("gc") == tot("first"), view
