"""The named cases of the ``--trimmed-out`` tests (host simulation and GPU alike): every case of ``qc_cases.all_cases()`` except the one with a
quality line of the wrong length, which is the error case here, plus the smallest shapes at which the kernels of csrc/kernels_fq.hpp can
still go wrong.  A case is a ``qc_cases`` case: dict(text, fmt, min_len, opts, per_modifier).  ``expected(name)`` is the restatement's
stream, computed once."""
import functools

import numpy as np

import fq_restate
import qc_cases
from qc_cases import ADAPTER, _case, _rand_qual, _rand_seq

ERROR_CASE = "quality_line_of_the_wrong_length"
random_text = qc_cases.random_text
trim_kwargs = qc_cases.trim_kwargs


def _fastq(recs, eol="\n"):
    """recs: (header with its '@', sequence, third line, qualities)"""
    return "".join(f"{h}{eol}{s}{eol}{p}{eol}{q}{eol}" for h, s, p, q in recs).encode("latin-1")


@functools.lru_cache(maxsize=None)
def all_cases():
    rng = np.random.default_rng(23)
    c = {k: v for k, v in qc_cases.all_cases().items() if k != ERROR_CASE}
    recs = []
    for n in (1, 15, 16, 17, 255, 300, 1, 16):  # header bytes, the '@' included: around the 16 bytes a lane stores, and past a small tile
        s = _rand_seq(rng, int(rng.integers(18, 40)))
        recs.append(("@" + "".join(chr(int(x)) for x in rng.integers(48, 123, n - 1)), s, "+", _rand_qual(rng, len(s), 20, 41)))
    c["header_lengths"] = _case(_fastq(recs), min_len=16)
    recs = [("@a 1:N:0", "ACGTACGTACGTACGTAC", "+a 1:N:0", "I" * 18), ("@b", "TTGCATTGCATTGCATTGCA" + ADAPTER, "+b", "I" * (20 + len(ADAPTER))),
            ("@c", "ACGT", "+c", "IIII")]
    c["third_line_with_a_name"] = _case(_fastq(recs), min_len=5, opts=dict(adapter=ADAPTER))
    c["crlf_with_names"] = _case(_fastq(recs, eol="\r\n"), min_len=5, opts=dict(adapter=ADAPTER))
    c["every_record_dropped"] = _case(qc_cases.fastq([(_rand_seq(rng, n), "I" * n) for n in (5, 9, 0, 15, 12)]), min_len=16)
    # one read of 5 000 nt behind a 300-byte header: a record that spans many tiles, between two short ones
    long_seq = _rand_seq(rng, 4980) + ADAPTER + "ACG"
    recs = [("@s", "ACGTACGTACGTACGTACGT", "+", "I" * 20), ("@" + "h" * 299, long_seq, "+", _rand_qual(rng, len(long_seq) - 10, 25, 41) + "#" * 10),
            ("@t", "TTTTGGGGCCCCAAAATTTT", "+", "I" * 20)]
    c["a_long_read_behind_a_long_header"] = _case(_fastq(recs), min_len=16, opts=dict(q_back=10, adapter=ADAPTER))
    # format 3 with -m 0: 600 records of ONE byte (a read cut to nothing writes its line end), then records of one to four bytes
    c["six_hundred_one_byte_records"] = _case(("".join("C\n" if rng.integers(0, 2) else "\n" for _ in range(599)) + "C\n").encode(), fmt=3, min_len=0,
                                              opts=dict(cut=[1]))
    c["tiny_records_and_empty_reads"] = _case(("".join(["", "A", "AC", "ACG"][int(rng.integers(0, 4))] + "\n" for _ in range(599)) + "T\n").encode(), fmt=3,
                                              min_len=0)
    recs = []
    for i in range(60):
        n = int(rng.integers(20, 50))
        recs.append((_rand_seq(rng, n), _rand_qual(rng, n - 6, 25, 41) + _rand_qual(rng, 6, 2, 25)))
    c["a_cut_and_a_quality_trim"] = _case(qc_cases.fastq(recs), min_len=16, opts=dict(q_back=20, cut=[3, -2]))
    c["fasta_with_empty_sequences"] = _case(qc_cases.fasta(["ACGTACGT", "", "acgun", "", "GGGGCCCC", ""]), fmt=2, min_len=0)
    return c


def error_case():
    return qc_cases.all_cases()[ERROR_CASE]


def restated(case) -> bytes:
    return fq_restate.stream(case["text"], case["fmt"], case["min_len"], case["opts"])


@functools.lru_cache(maxsize=None)
def expected(name: str) -> bytes:
    return restated(all_cases()[name])
