"""The named cases of the ``--read-qc`` tests (host simulation and GPU alike) and the generator of random small texts: the smallest shapes at
which the kernels of csrc/kernels_qc.hpp can still go wrong.  A case = dict(text, fmt (1 FASTQ, 2 FASTA, 3 one sequence per line), min_len,
opts (the chain as ``oracle.trim_stages`` takes it, or None), per_modifier).  ``expected(name)`` is the restatement's answer, computed once."""
import functools

import numpy as np

import qc_restate

ADAPTER = "TGGAATTCTCGGGTGCC"


def fastq(recs, eol="\n"):
    return "".join(f"@r{i}{eol}{s}{eol}+{eol}{q}{eol}" for i, (s, q) in enumerate(recs)).encode("latin-1")


def fasta(seqs, eol="\n"):
    return "".join(f">r{i}{eol}{s}{eol}" for i, s in enumerate(seqs)).encode("latin-1")


def _rand_seq(rng, n, letters="ACGT"):
    return "".join(letters[i] for i in rng.integers(0, len(letters), n))


def _rand_qual(rng, n, lo=2, hi=41, base=33):
    return "".join(chr(base + int(q)) for q in rng.integers(lo, hi + 1, n))


def _case(text, fmt=1, min_len=0, opts=None, per_modifier=False):
    return dict(text=text, fmt=fmt, min_len=min_len, opts=opts, per_modifier=per_modifier)


@functools.lru_cache(maxsize=None)
def all_cases():
    rng = np.random.default_rng(11)
    c = {}
    c["empty_text"] = _case(b"")
    c["one_record"] = _case(fastq([("TGAGGTAGTAGGTTGTATAGTT", "IIIIIIIIIIIIIIIIIIIIII")]), min_len=16)
    c["empty_sequence_lines"] = _case(fastq([("ACGT", "IIII"), ("", ""), ("GGCA", "!I~I"), ("", "")]))
    c["lengths_around_the_wave_and_the_overflow_row"] = _case(
        fastq([(_rand_seq(rng, n), _rand_qual(rng, n)) for n in (1, 63, 64, 65, 255, 256, 257, 300, 300, 1)]), min_len=16)
    c["crlf"] = _case(fastq([("ACGTNACGTTGCA", "IIIIIHHHHH###"), ("", ""), ("TTTTGGGGCCCCAAAAT", "ABCDEFGHIJKLMNOPQ")], eol="\r\n"), min_len=5,
                      opts=dict(q_back=10))
    c["lower_case_u_iupac_and_dot"] = _case(fastq([("acgtuUNnRYSWKMBDHV.ACGT", "IIIIIIIIIIIIIIIIIIIIIII"), ("uuuACGTryk...", "5555566666777"),
                                                   ("n", "I"), (".", "#")]))
    c["qualities_at_both_ends"] = _case(fastq([("ACGTACGT", "!~!~!~!~"), ("GGGG", "~~~~"), ("CCCC", "!!!!"), ("ACGT", "I\x7fI\x7f")]))
    c["phred64_with_bytes_below_the_base"] = _case(fastq([("ACGTACGTACGTACGTACGT", "hhhhhhhhhh;;hhhhhh@B"), ("TTGCATTGCATTGCA", "h5h5h5hhhhhhhhh")]),
                                                   min_len=4, opts=dict(base=64))
    c["phred64_trimmed"] = _case(fastq([("ACGTACGTACGTACGTACGT", "hhhhhhhhhhhhhhhh;;@B"), ("TTGCATTGCATTGCA", "h5h5h5hhhhhhhhh")]),
                                 min_len=4, opts=dict(base=64, q_back=20))
    c["quality_line_of_the_wrong_length"] = _case(fastq([("ACGTACGT", "IIIIIIII"), ("ACGTACGTAA", "IIIIIIII"), ("GGGTTT", "IIIIIIII"), ("CCCC", "5555")]),
                                                  min_len=5)
    # about 1 000 records: several workgroups of either kernel, and the grid stride of k_qc_pos (16 reads per workgroup and step)
    recs = []
    for i in range(1000):
        n = int(rng.integers(15, 45))
        s = (_rand_seq(rng, n, "ACGTACGTACGTN" if i % 7 == 0 else "ACGT") + ADAPTER + _rand_seq(rng, 8))[:int(rng.integers(20, 61))]
        recs.append((s, _rand_qual(rng, len(s), 2, 41)))
    c["a_thousand_records"] = _case(fastq(recs), min_len=16, opts=dict(q_back=10, adapter=ADAPTER))
    c["trimmed_to_length_zero"] = _case(fastq([(ADAPTER + "ACGT", "I" * (len(ADAPTER) + 4)), ("ACGTTGCAACGTTGCAACGT" + ADAPTER[:9], "I" * 29),
                                               ("NNNN", "IIII"), ("ACGT", "####")]), min_len=0, opts=dict(q_back=10, adapter=ADAPTER, trim_n=True))
    c["reads_under_the_minimum_length"] = _case(fastq([("ACGTACGTACGTACG", "I" * 15), ("ACGTACGTACGTACGT", "I" * 16), ("ACG", "III"),
                                                       ("ACGTACGTACGTACGTACGTAC" + ADAPTER, "I" * (22 + len(ADAPTER))), ("ACGTACGTACGTAC" + ADAPTER, "I" * (14 + len(ADAPTER)))]),
                                                min_len=16, opts=dict(adapter=ADAPTER))
    recs = []
    for i in range(40):
        n = int(rng.integers(18, 30))
        s = "N" * int(rng.integers(0, 3)) + _rand_seq(rng, n) + "NN"[:int(rng.integers(0, 3))] + ADAPTER[:int(rng.integers(0, len(ADAPTER) + 1))]
        recs.append((s, _rand_qual(rng, len(s) - 4, 20, 41) + _rand_qual(rng, 4, 2, 30)))
    c["chain_counted_per_modifier"] = _case(fastq(recs), min_len=16, opts=dict(q_back=15, adapter=ADAPTER, trim_n=True, cut=[2, -1]), per_modifier=True)
    c["fasta"] = _case(fasta(["ACGTACGTACGTACGTACGTAC" + ADAPTER, "acgtnACGU", "", "GGGGCCCCGGGGCCCCAAAA", "TTTT" + ADAPTER]), fmt=2, min_len=8,
                       opts=dict(q_back=10, adapter=ADAPTER))
    c["one_sequence_per_line"] = _case(b"ACGTACGTACGTACGTACGT\nacgu\n\nGGGGNNNN\n", fmt=3, min_len=5)
    return c


def random_text(seed: int):
    """a small text with everything left to chance: format, line ends, letters, qualities, the chain, the minimum length"""
    rng = np.random.default_rng(1000 + seed)
    fmt = int(rng.choice([1, 1, 1, 2, 3]))
    eol = "\r\n" if rng.integers(0, 4) == 0 else "\n"
    letters = ["ACGT", "ACGTN", "ACGTacgtNRY."][int(rng.integers(0, 3))]  # (U: the named case; the chain's own letter rules are not under test here)
    seqs = []
    for _ in range(int(rng.integers(0, 14))):
        n = int(rng.choice([0, 1, 5, 17, 22, 30, 51, 64, 65, 70, 130, 256, 257, 290], p=[.05, .05, .1, .15, .2, .1, .1, .05, .05, .05, .04, .02, .02, .02]))
        s = _rand_seq(rng, n, letters)
        if rng.integers(0, 3) == 0:
            s += ADAPTER[:int(rng.integers(3, len(ADAPTER) + 1))]
        seqs.append(s)
    if fmt == 3:
        seqs = [s or "A" for s in seqs]
    opts = None
    if rng.integers(0, 4):
        opts = {}
        if rng.integers(0, 2):
            opts["q_back"] = int(rng.choice([10, 20]))
        if rng.integers(0, 2):
            opts["adapter"] = ADAPTER
        if rng.integers(0, 3) == 0:
            opts["trim_n"] = True
        if rng.integers(0, 3) == 0:
            opts["cut"] = [[2], [-3], [1, -1]][int(rng.integers(0, 3))]
        if rng.integers(0, 5) == 0:
            opts["base"] = 64
    base = (opts or {}).get("base", 33)
    if fmt == 1:
        text = fastq([(s, _rand_qual(rng, len(s), 0, 93 if base == 33 else 62, base) if rng.integers(0, 5) else _rand_qual(rng, len(s), 30, 41, base)) for s in seqs], eol)
    elif fmt == 2:
        text = fasta(seqs, eol)
    else:
        text = "".join(s + eol for s in seqs).encode("latin-1")
    return _case(text, fmt, int(rng.choice([0, 5, 16])), opts, bool(rng.integers(0, 2)))


def trim_kwargs(case):
    """the arguments of ``_ffi.MirgeTrim.make`` for this case's chain (None: no trim struct at all)"""
    o = case["opts"]
    if o is None:
        return None
    return dict(adapter=o.get("adapter"), quality_back=o["q_back"] if o.get("q_back") is not None else -1, quality_front=o.get("q_front", 0),
                phred_base=o.get("base", 33), trim_n=bool(o.get("trim_n")), cut=o.get("cut", []), count_per_modifier=case["per_modifier"])


def restated(case):
    e = qc_restate.entries(case["text"], case["fmt"], case["min_len"], case["opts"])
    qc_restate.identities(e)
    return e


@functools.lru_cache(maxsize=None)
def expected(name: str):
    return restated(all_cases()[name])
