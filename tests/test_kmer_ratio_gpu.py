"""``--kmer-ratio`` on the MI355X: ``mirge_kmer_correct_ratio`` (csrc/native_ec.hpp; k_ec_dominate and k_ec_fold of csrc/kernels_ec.hpp)
through the C ABI on the cases of tests/ec_ratio_cases.py, its small random sets side by side and its set of about 20 000 distinct
reads, again with the hashes cut to 6 bits; without a ratio against the old entry point; then the command line on two synthetic samples
with deep templates.  Sequences, counts, first indices, ``final_of``, ``rounds_mask``, the tallies of every round and per round the
k-mers above H and the dominated among them are compared exactly with the restatement (tests/ec_ratio_restate.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import ec_cases
import ec_ratio_cases
import ec_ratio_restate as rr
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


def _old_entry_point(d0, ks, ke, H):
    """``mirge_kmer_correct`` itself, not through ``DeviceReads.kmer_correct``"""
    n = len(d0)
    final_of, mask = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
    h = C.c_void_p()
    rc = _ffi.load().mirge_kmer_correct(d0.ctx._h, d0._h, C.c_int32(ks), C.c_int32(ke), C.c_int32(H), C.byref(h), C.c_void_p(final_of.ctypes.data),
                                        C.c_void_p(mask.ctypes.data))
    assert rc == 0
    return _ffi.DeviceReads(d0.ctx, h), final_of[:n], mask[:n]


def correct(ctx, case, ratio=None, old=False):
    """-> what ``ec_ratio_restate.correct`` returns, from the device"""
    reads, counts = case["reads"], case["counts"]
    raw = _ffi.DeviceReads.pack(ctx, FlatSeqs.from_list(list(reads)))
    d0 = raw.collapse(weights=np.asarray(counts, dtype=np.uint32))
    out = None
    try:
        assert len(d0) == len(reads)
        if old:
            out, final_of, mask = _old_entry_point(d0, case["ks"], case["ke"], case["H"])
        else:
            out, final_of, mask = d0.kmer_correct(case["ks"], case["ke"], case["H"], ratio=case["R"] if ratio is None else ratio)
        stats, rstats = _ffi.kmer_correct_stats(), _ffi.kmer_correct_ratio_stats()
        assert len(stats) == len(rstats) == case["ke"] - case["ks"] + 1
        res = {"tallies": [{k: st[k] for k in ec_restate.TALLIES} for st in stats], "above": [st["above"] for st in rstats],
               "dominated": [st["dominated"] for st in rstats]}
        if not len(reads):
            assert len(out) == 0
            return dict(res, entries=[], final=[], rounds=[])
        _, first0 = d0.counts()
        assert np.array_equal(np.sort(first0), np.arange(len(reads)))  # a read's first index is its position in `reads`
        cnt, first = out.counts()
        seqs = out.unpack().to_list()
        order = np.argsort(first, kind="stable")
        final, rounds = [None] * len(reads), [None] * len(reads)
        for h0, i in enumerate(first0.tolist()):
            final[i] = seqs[int(final_of[h0])]
            rounds[i] = [case["ks"] + b for b in range(32) if (int(mask[h0]) >> b) & 1]
        return dict(res, entries=[(seqs[h], int(cnt[h, 0]), int(first[h])) for h in order], final=final, rounds=rounds)
    finally:
        if out is not None:
            out.close()
        d0.close(); raw.close()


def same(got, want, name):
    assert got["tallies"] == want["tallies"], name
    assert (got["above"], got["dominated"]) == (want["above"], want["dominated"]), name
    bad = [i for i, (a, b) in enumerate(zip(got["final"], want["final"])) if a != b]
    assert not bad, (name, bad[:5])
    assert got["rounds"] == want["rounds"], name
    assert got["entries"] == want["entries"], name


@pytest.mark.parametrize("name", sorted(ec_ratio_cases.all_cases()))
def test_cases_equal_the_restatement(ctx, name):
    ec_ratio_cases.holds(name)
    same(correct(ctx, ec_ratio_cases.all_cases()[name]), ec_ratio_cases.expected(name), name)


@pytest.mark.parametrize("R", ec_ratio_cases.RANDOM_RATIOS)
def test_small_random_sets_equal_the_restatement(ctx, R):
    case, want = ec_ratio_cases.random_sets_side_by_side()[R]
    same(correct(ctx, case), want, f"small sets, R = {R}")


def test_a_large_random_set_equals_the_restatement(ctx):
    case, want, _ = ec_ratio_cases.big_set()
    same(correct(ctx, case), want, "big")


def test_collisions_change_nothing(ctx, monkeypatch):
    monkeypatch.setenv("MIRGE_TEST_EC_HASH_BITS", "6")
    try:
        for name in sorted(ec_ratio_cases.all_cases()):
            same(correct(ctx, ec_ratio_cases.all_cases()[name]), ec_ratio_cases.expected(name), name)
        for R, (case, want) in ec_ratio_cases.random_sets_side_by_side().items():
            same(correct(ctx, case), want, f"small sets, R = {R}")
        case, want, _ = ec_ratio_cases.big_set()
        same(correct(ctx, case), want, "big")
    finally:
        monkeypatch.delenv("MIRGE_TEST_EC_HASH_BITS")


@pytest.mark.parametrize("name", sorted(ec_cases.all_cases()))
def test_ratio_0_is_the_old_entry_point(ctx, name):
    case = ec_cases.all_cases()[name]
    zeros = [0] * (case["ke"] - case["ks"] + 1)
    want = dict(ec_cases.expected(name), above=zeros, dominated=zeros)
    with_0, old = correct(ctx, case, ratio=0), correct(ctx, case, old=True)
    assert with_0 == old
    same(with_0, want, name)


def test_the_ratio_stats_are_zeros_after_a_call_without_a_ratio(ctx):
    case = ec_ratio_cases.all_cases()["deep_template"]
    assert correct(ctx, case)["dominated"] == [10]
    assert correct(ctx, case, old=True)["dominated"] == [0] and correct(ctx, case, ratio=0)["above"] == [0]


def test_bad_ratios_are_refused(ctx):
    raw = _ffi.DeviceReads.pack(ctx, FlatSeqs.from_list(["ACGTACGTACGTACGTACGTAC", "ACGTACGTACGTACGTACGTAA"]))
    d0 = raw.collapse()
    try:
        for ratio in (1, -1, -2 ** 31, 2 ** 31):
            with pytest.raises(RuntimeError):
                d0.kmer_correct(10, 10, 5, ratio=ratio)
        out, _, _ = d0.kmer_correct(10, 10, 5, ratio=2 ** 31 - 1)
        out.close()
    finally:
        d0.close(); raw.close()


def _fastq(reads):
    return "".join(f"@r{i}\n{r}\n+\n{'I' * len(r)}\n" for i, r in enumerate(reads)).encode()


def _deep_sample(templates, seed):
    """tests/test_kmer_correct_gpu.py's ``_sample`` with deeper templates, whose errors come in copies: 120 .. 200 copies of a template and
    three to five substitution variants of it, 1 .. 12 copies each (8 * 12 <= 120: every variant seen more than -kh 5 times is
    dominated at R = 8).  (this wrote tests/golden/kmer_ratio/S1.fastq and S2.fastq: the 10 first and the 10 last of the 15 most
    frequent reads of tests/golden/kmer_correct_off/S1.fastq in sorted order, with seeds 200 and 201)"""
    rng = np.random.default_rng(seed)
    reads = []
    for t in templates:
        reads += [t] * int(rng.integers(120, 201))
        for _ in range(int(rng.integers(3, 6))):
            reads += [ec_cases.mutate(t, int(rng.integers(0, len(t))), int(rng.integers(1, 4)))] * int(rng.integers(1, 13))
    return [reads[i] for i in rng.permutation(len(reads))]


def _dictionary(reads):
    d = {}
    for r in reads:
        d[r] = d.get(r, 0) + 1
    return list(d), list(d.values())


DEEP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmer_ratio")
OFF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmer_correct_off")


def test_the_committed_input_of_kmer_correct_has_no_deep_template():
    """why tests/golden/kmer_ratio exists: on the FASTQs of tests/golden/kmer_correct_off R = 8 changes no read's final sequence"""
    for s in (1, 2):
        with open(os.path.join(OFF, f"S{s}.fastq")) as fh:
            dreads, dcounts = _dictionary(fh.read().split("\n")[1::4])
        assert rr.correct(dreads, dcounts, 12, 14, 5, 8)["final"] == ec_restate.correct(dreads, dcounts, 12, 14, 5)["final"]


def test_command_line(tmp_path):
    """two samples with deep templates (tests/golden/kmer_ratio): the run with --kmer-correct --kmer-ratio 8 writes the tables the unchanged
    pipeline writes when it is fed the restatement's corrected reads; its per-sample file and both kinds of log line are the
    restatement's, a sample's ratio line behind the line of its k"""
    from test_gpu_parity import _run_cli
    case = GoldenCase("case2_two_samples")
    ks, ke, H, R = 12, 14, 5, 8
    files, fixed_files, wants, dicts = [], [], [], []
    for s in range(2):
        with open(os.path.join(DEEP, f"S{s + 1}.fastq")) as fh:
            reads = fh.read().split("\n")[1::4]
        dreads, dcounts = _dictionary(reads)
        want = rr.correct(dreads, dcounts, ks, ke, H, R)
        plain = ec_restate.correct(dreads, dcounts, ks, ke, H)
        assert sum(a != b for a, b in zip(want["final"], plain["final"])) >= 10  # R = 8 changes reads that R = 0 leaves
        assert sum(want["dominated"]) > 50
        becomes = dict(zip(dreads, want["final"]))
        q = tmp_path / "fixed" / f"S{s + 1}.fastq"
        q.parent.mkdir(exist_ok=True)
        q.write_bytes(_fastq([becomes[r] for r in reads]))
        files.append(os.path.join(DEEP, f"S{s + 1}.fastq")); fixed_files.append(str(q)); wants.append(want); dicts.append((dreads, dcounts))
    common = ["-lib", case.libdir, "-on", ORG, "-db", "miRBase", "-o", str(tmp_path), "-shh", "-tcf"]
    _run_cli(["-s", ",".join(files), "-dn", "ec", "--kmer-correct", "--kmer-ratio", str(R), "-ks", str(ks), "-ke", str(ke), "-kh", str(H)] + common)
    _run_cli(["-s", ",".join(fixed_files), "-dn", "fixed_in"] + common)
    for name in ("miR.Counts.csv", "miR.RPM.csv", "annotation.report.csv", "mapped.csv", "unmapped.csv", "S1.trim.collapse.fa", "S2.trim.collapse.fa"):
        assert (tmp_path / "ec" / name).read_bytes() == (tmp_path / "fixed_in" / name).read_bytes(), name
    log = (tmp_path / "ec" / "run.log").read_text()
    for s, (want, (dreads, dcounts)) in enumerate(zip(wants, dicts)):
        assert (tmp_path / "ec" / f"S{s + 1}_kmerCorrected.csv").read_text() == ec_restate.csv_text(dreads, dcounts, want)
        for line, extra in zip(ec_restate.log_lines(f"S{s + 1}", ks, want), rr.ratio_log_lines(f"S{s + 1}", ks, R, want)):
            assert line + "\n" + extra + "\n" in log
    assert "kmer-correct" not in (tmp_path / "fixed_in" / "run.log").read_text()
