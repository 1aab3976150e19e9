"""``--kmer-correct`` on the MI355X: ``mirge_kmer_correct`` (csrc/native_ec.hpp, csrc/kernels_ec.hpp) through the C ABI on the cases of
tests/ec_cases.py and on a random set of about 20 000 distinct reads -- inputs built with ``DeviceReads.pack`` + ``collapse(weights=counts)``
so that counts are free to choose --, again with the hashes cut to 6 bits, on dictionaries that ``mirge_collapse`` made of
65 536 raw reads and more (its partitioned route), then the command line on two synthetic samples, with the switch and without.  Sequences,
counts, first indices, ``final_of``, ``rounds_mask`` and the tallies of every round are compared exactly with the restatement
(tests/ec_restate.py)."""
import os

import numpy as np
import pytest

import ec_cases
import ec_restate
from helpers import GoldenCase, ORG
import mirge3_amd  # noqa: F401
from mirge3_amd import _ffi
from mirge3_amd.seqio import FlatSeqs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


def correct(ctx, case):
    """-> what ``ec_restate.correct`` returns, from the device"""
    reads, counts = case["reads"], case["counts"]
    raw = _ffi.DeviceReads.pack(ctx, FlatSeqs.from_list(list(reads)))
    d0 = raw.collapse(weights=np.asarray(counts, dtype=np.uint32))
    out = None
    try:
        assert len(d0) == len(reads)
        out, final_of, mask = d0.kmer_correct(case["ks"], case["ke"], case["H"])
        stats = _ffi.kmer_correct_stats()
        assert len(stats) == case["ke"] - case["ks"] + 1
        tallies = [{k: st[k] for k in ec_restate.TALLIES} for st in stats]
        if not len(reads):
            assert len(out) == 0
            return {"entries": [], "final": [], "rounds": [], "tallies": tallies}
        _, first0 = d0.counts()
        assert np.array_equal(np.sort(first0), np.arange(len(reads)))  # a read's first index is its position in `reads`
        cnt, first = out.counts()
        seqs = out.unpack().to_list()
        order = np.argsort(first, kind="stable")
        entries = [(seqs[h], int(cnt[h, 0]), int(first[h])) for h in order]
        final, rounds = [None] * len(reads), [None] * len(reads)
        for h0, i in enumerate(first0.tolist()):
            final[i] = seqs[int(final_of[h0])]
            rounds[i] = [case["ks"] + b for b in range(32) if (int(mask[h0]) >> b) & 1]
        for st in stats:
            assert st["slots"] >= 256 and st["slots"] & (st["slots"] - 1) == 0
        return {"entries": entries, "final": final, "rounds": rounds, "tallies": tallies}
    finally:
        if out is not None:
            out.close()
        d0.close(); raw.close()


def same(got, want, name):
    assert got["tallies"] == want["tallies"], name
    bad = [i for i, (a, b) in enumerate(zip(got["final"], want["final"])) if a != b]
    assert not bad, (name, bad[:5])
    assert got["rounds"] == want["rounds"], name
    assert got["entries"] == want["entries"], name


@pytest.mark.parametrize("name", sorted(ec_cases.all_cases()))
def test_cases_equal_the_restatement(ctx, name):
    same(correct(ctx, ec_cases.all_cases()[name]), ec_cases.expected(name), name)


@pytest.fixture(scope="module")
def big():
    case = ec_cases.big_set()
    want = ec_restate.correct(case["reads"], case["counts"], case["ks"], case["ke"], case["H"])
    assert 18000 < len(case["reads"]) < 22000 and want["tallies"][0]["corrected"] > 5000 and want["tallies"][0]["unsupported"] > 500
    return case, want


@pytest.fixture(scope="module")
def ties():
    """many small two- and four-letter sets side by side (each behind a prefix of its own, so that they share no k-mer): ties, merges,
    reads corrected in both rounds"""
    reads, counts = [], []
    rng = np.random.default_rng(5)
    for seed in range(300):
        c = ec_cases.random_set(seed, letters="AC" if seed % 3 == 0 else "ACGT", lengths=(12, 18), ks=10, ke=11)
        prefix = "G" + ec_cases.rand_seq(rng, 14, "GT") + "G"
        reads += [prefix + r for r in c["reads"]]
        counts += c["counts"]
    keep = {}
    for r, c in zip(reads, counts):
        keep.setdefault(r, c)
    case = {"reads": list(keep), "counts": list(keep.values()), "ks": 10, "ke": 11, "H": 2}
    want = ec_restate.correct(case["reads"], case["counts"], 10, 11, 2)
    assert sum(t["ambiguous"] for t in want["tallies"]) > 20 and sum(t["corrected"] for t in want["tallies"]) > 100
    return case, want


def test_a_large_random_set_equals_the_restatement(ctx, big):
    same(correct(ctx, big[0]), big[1], "big")


def test_tied_sets_equal_the_restatement(ctx, ties):
    same(correct(ctx, ties[0]), ties[1], "ties")


def test_collisions_change_nothing(ctx, big, ties, monkeypatch):
    monkeypatch.setenv("MIRGE_TEST_EC_HASH_BITS", "6")
    try:
        for name in sorted(ec_cases.all_cases()):
            same(correct(ctx, ec_cases.all_cases()[name]), ec_cases.expected(name), name)
        same(correct(ctx, big[0]), big[1], "big")
        same(correct(ctx, ties[0]), ties[1], "ties")
    finally:
        monkeypatch.delenv("MIRGE_TEST_EC_HASH_BITS")


def _from_raw_reads(ctx, reads, ks, ke, H):
    """raw reads through ``mirge_collapse`` (65 536 reads of up to 31 nt and more take its partitioned route, whose handle order is
    unspecified) -> (sequences of the dictionary in handle order, counts, first, sequences of the corrected one, its counts, its
    first indices, final_of, masks)"""
    raw = _ffi.DeviceReads.pack(ctx, FlatSeqs.from_list(reads))
    d0 = raw.collapse()
    out = None
    try:
        out, final_of, mask = d0.kmer_correct(ks, ke, H)
        c0, f0 = d0.counts()
        c1, f1 = out.counts()
        return d0.unpack().to_list(), c0[:, 0], f0, out.unpack().to_list(), c1[:, 0], f1, final_of, mask, _ffi.kmer_correct_stats()
    finally:
        if out is not None:
            out.close()
        d0.close(); raw.close()


def test_an_unchanged_dictionary_of_raw_reads_keeps_its_handles(ctx):
    """72 000 raw reads (12 000 distinct ones of 20 .. 30 nt, six copies each: nothing is suspect at H = 5) collapsed by
    ``mirge_collapse``: every read of the input names itself in the output"""
    rng = np.random.default_rng(11)
    distinct = list(dict.fromkeys(ec_cases.rand_seq(rng, int(rng.integers(20, 31))) for _ in range(12000)))
    reads = [distinct[i] for i in rng.permutation(np.repeat(np.arange(len(distinct)), 6))]
    assert len(reads) >= 65536
    s0, c0, f0, s1, c1, f1, final_of, mask, stats = _from_raw_reads(ctx, reads, 15, 17, 5)
    assert len(s0) == len(distinct) == len(s1) and not mask.any()
    assert all(st["suspect"] == 0 and st["eligible"] == len(distinct) and st["distinct"] == len(distinct) for st in stats)
    assert [s1[h] for h in final_of.tolist()] == s0
    assert np.array_equal(c1[final_of], c0) and np.array_equal(f1[final_of], f0) and (c0 == 6).all()
    assert sorted(final_of.tolist()) == list(range(len(s0)))


def test_a_dictionary_of_raw_reads_equals_the_restatement(ctx):
    """the same route with planted errors: 12 000 templates of six copies and 6 000 single copies with one substitution"""
    rng = np.random.default_rng(12)
    distinct = list(dict.fromkeys(ec_cases.rand_seq(rng, int(rng.integers(20, 31))) for _ in range(12000)))
    errors = [ec_cases.mutate(distinct[2 * i], int(rng.integers(0, len(distinct[2 * i]))), int(rng.integers(1, 4))) for i in range(6000)]
    pool = distinct * 6 + errors
    reads = [pool[i] for i in rng.permutation(len(pool))]
    dreads, dcounts = _dictionary(reads)
    want = ec_restate.correct(dreads, dcounts, 15, 16, 5)
    assert want["tallies"][0]["corrected"] > 5000
    s0, c0, f0, s1, c1, f1, final_of, mask, stats = _from_raw_reads(ctx, reads, 15, 16, 5)
    assert [{k: st[k] for k in ec_restate.TALLIES} for st in stats] == want["tallies"]
    final = dict(zip(dreads, want["final"]))
    rounds = dict(zip(dreads, want["rounds"]))
    assert [s1[h] for h in final_of.tolist()] == [final[r] for r in s0]
    assert [[15 + b for b in range(2) if (int(m) >> b) & 1] for m in mask] == [rounds[r] for r in s0]
    first_raw = {}
    for i, r in enumerate(reads):
        first_raw.setdefault(r, i)
    order = np.argsort(f1, kind="stable")
    assert [(s1[h], int(c1[h])) for h in order] == [(e[0], e[1]) for e in want["entries"]]
    assert [int(f1[h]) for h in order] == [first_raw[dreads[e[2]]] for e in want["entries"]]  # the earliest contributor's raw index


def test_bad_ranges_and_handles_are_refused(ctx):
    raw = _ffi.DeviceReads.pack(ctx, FlatSeqs.from_list(["ACGTACGTACGTACGTACGTAC", "ACGTACGTACGTACGTACGTAA"]))
    d0 = raw.collapse()
    try:
        for ks, ke, h in ((7, 9, 5), (10, 32, 5), (11, 10, 5), (10, 10, 0)):
            with pytest.raises(RuntimeError):
                d0.kmer_correct(ks, ke, h)
        with pytest.raises(RuntimeError):
            raw.kmer_correct(10, 10, 5)  # no collapse result
    finally:
        d0.close(); raw.close()


def _fastq(reads):
    return "".join(f"@r{i}\n{r}\n+\n{'I' * len(r)}\n" for i, r in enumerate(reads)).encode()


def _sample(templates, seed):
    """(this wrote tests/golden/kmer_correct_off/S1.fastq and S2.fastq: templates[0:40] with seed 100, templates[20:60] with seed 101)"""
    rng = np.random.default_rng(seed)
    reads = []
    for t in templates:
        reads += [t] * int(rng.integers(8, 30))
        for _ in range(int(rng.integers(2, 7))):
            reads.append(ec_cases.mutate(t, int(rng.integers(0, len(t))), int(rng.integers(1, 4))))
    return [reads[i] for i in rng.permutation(len(reads))]


def _dictionary(reads):
    d = {}
    for r in reads:
        d[r] = d.get(r, 0) + 1
    return list(d), list(d.values())


OFF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmer_correct_off")
OFF_FILES = ("miR.Counts.csv", "miR.RPM.csv", "annotation.report.csv", "mapped.csv", "unmapped.csv", "S1.trim.collapse.fa", "S2.trim.collapse.fa")


def _log_without_times(text):
    """run.log without its first line (the command line, with the run's paths) and with every decimal number -- the times -- as T"""
    import re
    return re.sub(r"\d+\.\d+", "T", text.split("\n", 1)[1])


@pytest.mark.parametrize("n_samples", [2, 1], ids=["two_samples", "one_sample"])
def test_command_line(tmp_path, n_samples):
    """two samples (the sorted union of their reads; the committed input of tests/golden/kmer_correct_off) and one (rows in the order of
    first appearance): the run with --kmer-correct writes the tables the unchanged pipeline writes when it is fed the restatement's
    corrected reads (every raw read replaced by its final sequence); its per-sample file and log lines are the restatement's.  The
    two-sample input WITHOUT the switch writes, byte for byte, the files the commit before this feature wrote for it
    (tests/golden/kmer_correct_off: tables, -tcf files, run.log without times)."""
    from test_gpu_parity import _run_cli
    case = GoldenCase("case2_two_samples")
    ks, ke, H = 12, 14, 5
    files, fixed_files, wants, dicts = [], [], [], []
    for s in range(n_samples):
        with open(os.path.join(OFF, f"S{s + 1}.fastq")) as fh:
            reads = fh.read().split("\n")[1::4]
        dreads, dcounts = _dictionary(reads)
        want = ec_restate.correct(dreads, dcounts, ks, ke, H)
        becomes = dict(zip(dreads, want["final"]))
        assert sum(t["corrected"] for t in want["tallies"]) > 20
        q = tmp_path / "fixed" / f"S{s + 1}.fastq"
        q.parent.mkdir(exist_ok=True)
        q.write_bytes(_fastq([becomes[r] for r in reads]))
        files.append(os.path.join(OFF, f"S{s + 1}.fastq")); fixed_files.append(str(q)); wants.append(want); dicts.append((dreads, dcounts))
    common = ["-lib", case.libdir, "-on", ORG, "-db", "miRBase", "-o", str(tmp_path), "-shh", "-tcf"]
    _run_cli(["-s", ",".join(files), "-dn", "ec", "--kmer-correct", "-ks", str(ks), "-ke", str(ke), "-kh", str(H)] + common)
    _run_cli(["-s", ",".join(fixed_files), "-dn", "fixed_in", "-ks", "3", "-kh", "x"] + common)
    for name in ("miR.Counts.csv", "miR.RPM.csv", "annotation.report.csv", "mapped.csv", "unmapped.csv") + tuple(f"S{s + 1}.trim.collapse.fa" for s in range(n_samples)):
        assert (tmp_path / "ec" / name).read_bytes() == (tmp_path / "fixed_in" / name).read_bytes(), name
    log = (tmp_path / "ec" / "run.log").read_text()
    for s, (want, (dreads, dcounts)) in enumerate(zip(wants, dicts)):
        assert (tmp_path / "ec" / f"S{s + 1}_kmerCorrected.csv").read_text() == ec_restate.csv_text(dreads, dcounts, want)
        for line in ec_restate.log_lines(f"S{s + 1}", ks, want):
            assert line + "\n" in log
        assert not (tmp_path / "fixed_in" / f"S{s + 1}_kmerCorrected.csv").exists()
    assert "kmer-correct" not in (tmp_path / "fixed_in" / "run.log").read_text()
    if n_samples == 2:
        _run_cli(["-s", ",".join(files), "-dn", "off"] + common)
        for name in OFF_FILES:
            with open(os.path.join(OFF, name), "rb") as fh:
                assert (tmp_path / "off" / name).read_bytes() == fh.read(), name
        with open(os.path.join(OFF, "run.log")) as fh:
            assert _log_without_times((tmp_path / "off" / "run.log").read_text()) == fh.read()
        assert not list((tmp_path / "off").glob("*_kmerCorrected.csv"))
