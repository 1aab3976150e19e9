"""A slow restatement of the ``--trimmed-out`` specification (the docstring of mirge3_amd/trimmed_out.py), independent of the kernels: the
stream S of a text, built record by record from ``qc_restate.views`` (its ``trimmed`` bounds, ``line``, ``qline``, ``mismatch``) plus the
header bounds, which follow from the line bounds of ``qc_restate.records``."""
import qc_restate


class QualityLengthMismatch(ValueError):
    pass


def header_bounds(text: bytes, fmt: int):
    """[(hb, he)] per record in ``qc_restate.device_text(text)``: the header line without its line end, a trailing '\\r' stripped (format 3:
    an empty stretch)"""
    buf = qc_restate.device_text(text)
    out, prev_end = [], -1  # the last line end of the record before
    for b, e, qb, qe in qc_restate.records(text, fmt):
        if fmt == 3:
            out.append((b, b))
        else:
            hb = prev_end + 1
            out.append((hb, qc_restate.strip_cr(buf, hb, b - 1)))
        prev_end = qe if fmt == 1 else e
    return out


def written_records(text: bytes, fmt: int, min_len: int = 0, opts: dict = None):
    """-> (n_records, [bytes of every written record, in file order]); raises QualityLengthMismatch on a record whose quality line is not as
    long as its sequence line"""
    buf, recs = qc_restate.views(text, fmt, min_len, opts)
    heads = header_bounds(text, fmt)
    assert len(heads) == len(recs)
    out = []
    for (hb, he), rec in zip(heads, recs):
        if rec["mismatch"]:
            raise QualityLengthMismatch("a record's quality line is not as long as its sequence line")
        ts, te = rec["trimmed"]
        if te - ts < min_len:
            continue
        seq = buf[ts:te]
        if fmt == 1:
            q0 = rec["qline"][0] + (ts - rec["line"][0])
            out.append(buf[hb:he] + b"\n" + seq + b"\n+\n" + buf[q0:q0 + (te - ts)] + b"\n")
        elif fmt == 2:
            out.append(buf[hb:he] + b"\n" + seq + b"\n")
        else:
            out.append(seq + b"\n")
    return len(recs), out


def stream(text: bytes, fmt: int, min_len: int = 0, opts: dict = None) -> bytes:
    """S of this text"""
    return b"".join(written_records(text, fmt, min_len, opts)[1])


def stats(text: bytes, fmt: int, min_len: int = 0, opts: dict = None) -> dict:
    """records, written and stream_bytes as ``mirge_fqout_finish`` reports them"""
    n, recs = written_records(text, fmt, min_len, opts)
    return dict(records=n, written=len(recs), stream_bytes=sum(len(r) for r in recs))
