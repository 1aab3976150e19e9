"""``--kmer-ratio`` without a GPU: the restatement of sentences 2a and 2b (tests/ec_ratio_restate.py) against the hand-written
expectations of the named cases (tests/ec_ratio_cases.py) and, without a ratio, against tests/ec_restate.py; the conditions of the
random sets; the equivalence the kernels rest on (a dominated sum set to 0 decides every read as 2a and 2b do); the command line's
refusals; the text of the second ``run.log`` line."""
import pytest

import ec_cases
import ec_ratio_cases
import ec_ratio_restate as rr
import ec_restate


@pytest.mark.parametrize("name", sorted(ec_ratio_cases.all_cases()))
def test_restatement_gives_what_the_case_was_written_for(name):
    ec_ratio_cases.holds(name)


def test_the_deep_template_needs_the_ratio():
    """what the flag is for: the error of a deep template, seen 20 times, is solid by count and stays without a ratio"""
    cases = ec_ratio_cases.all_cases()
    with_r, without = cases["deep_template"], cases["deep_template_no_ratio"]
    assert with_r["reads"] == without["reads"] and with_r["counts"] == without["counts"] == [1000, 20]
    t, v = with_r["reads"]
    assert ec_ratio_cases.expected("deep_template")["final"] == [t, t]
    assert ec_ratio_cases.expected("deep_template_no_ratio")["final"] == [t, v]
    assert ec_restate.correct([t, v], [1000, 20], 10, 10, 5)["final"] == [t, v]


def test_the_edge_of_2a_in_exact_integers():
    S = {"ACGTACGTAC": 10, "ACGAACGTAC": 80, "CCGTACGTAC": 79}
    assert rr.dominated(S, 10, 5, 8) == {"ACGTACGTAC"}
    del S["ACGAACGTAC"]
    assert rr.dominated(S, 10, 5, 8) == set()
    sx, sy = ec_ratio_cases.wrap_sums()
    x, y = "ACGTACGTAC", "ACGTCCGTAC"
    assert (ec_ratio_cases.RMAX * sx) % 2 ** 64 <= sy and rr.dominated({x: sx, y: sy}, 10, 5, ec_ratio_cases.RMAX) == set()
    assert sy // ec_ratio_cases.RMAX < sx  # the form that cannot wrap says the same


@pytest.mark.parametrize("name", sorted(ec_cases.all_cases()))
def test_without_a_ratio_it_is_the_restatement_of_kmer_correct(name):
    c, want = ec_cases.all_cases()[name], ec_cases.expected(name)
    got = rr.correct(c["reads"], c["counts"], c["ks"], c["ke"], c["H"], 0)
    zeros = [0] * (c["ke"] - c["ks"] + 1)
    assert got == dict(want, above=zeros, dominated=zeros)


def test_the_random_sets_reach_the_relative_threshold():
    """the builders assert it: D > 0 in at least half of the 300 small sets and a result other than without a ratio in at least a
    third; on the big set D >= 1000 and at least 1000 corrections more than without"""
    assert len(ec_ratio_cases.random_sets()) == 300
    assert {c["R"] for c, _ in ec_ratio_cases.random_sets()} == {2, 3, 8}
    ec_ratio_cases.random_sets_side_by_side()
    ec_ratio_cases.big_set()


def zeroing_decides_alike(case):
    """every round of the case: ``ec_restate.outcome`` on the spectrum with the dominated sums at 0 == the outcome by 2a and 2b, for
    every eligible read, and a valid candidate's score is no zeroed sum -> the number of reads compared"""
    entries = sorted(zip(case["reads"], case["counts"], range(len(case["reads"]))), key=lambda e: e[2])
    n = 0
    for k in range(case["ks"], case["ke"] + 1):
        S = ec_restate.spectrum(entries, k)
        dom = rr.dominated(S, k, case["H"], case["R"])
        Z = rr.zeroed(S, dom)
        for read, _, _ in entries:
            if ec_restate.eligible(read, k):
                assert ec_restate.outcome(read, k, Z, case["H"]) == rr.outcome(read, k, S, case["H"], dom), (read, k)
                n += 1
        entries = rr.one_round(entries, k, case["H"], case["R"])[0]
    return n


@pytest.mark.parametrize("name", sorted(ec_ratio_cases.all_cases()))
def test_zeroed_sums_decide_as_2a_and_2b_on_the_cases(name):
    zeroing_decides_alike(ec_ratio_cases.all_cases()[name])


def test_zeroed_sums_decide_as_2a_and_2b_on_the_random_sets():
    assert sum(zeroing_decides_alike(c) for c, _ in ec_ratio_cases.random_sets()) > 3000
    for c, _ in ec_ratio_cases.random_sets_side_by_side().values():
        zeroing_decides_alike(c)
    assert zeroing_decides_alike(ec_ratio_cases.big_set()[0]) > 30000


BASE = ["-s", "x.fastq", "-lib", "/nowhere", "-on", "human"]


@pytest.mark.parametrize("extra, message", [
    (["--kmer-ratio", "8"], "--kmer-ratio requires --kmer-correct"),
    (["--kmer-correct", "--kmer-ratio", "0"], "--kmer-ratio: 2 <= R <= 2^31 - 1"),
    (["--kmer-correct", "--kmer-ratio", "1"], "--kmer-ratio: 2 <= R <= 2^31 - 1"),
    (["--kmer-correct", "--kmer-ratio", "-3"], "--kmer-ratio: 2 <= R <= 2^31 - 1"),
    (["--kmer-correct", "--kmer-ratio", str(2 ** 31)], "--kmer-ratio: 2 <= R <= 2^31 - 1"),
    (["--kmer-correct", "--kmer-ratio", "x"], "--kmer-ratio takes an integer"),
    (["--kmer-correct", "--kmer-ratio", "2.5"], "--kmer-ratio takes an integer"),
    (["--kmer-correct", "--kmer-ratio", "8", "-umi", "4,4"], "--kmer-correct is not run together with -umi"),
    (["--kmer-correct", "--kmer-ratio", "8", "-spl"], "--kmer-correct runs on the device-resident route"),
])
def test_the_command_line_refuses(extra, message, capsys):
    from mirge3_amd.cli import parse_args
    with pytest.raises(SystemExit):
        parse_args(BASE + extra)
    assert message in capsys.readouterr().err


def test_the_command_line_accepts():
    from mirge3_amd.cli import parse_args
    a = parse_args(BASE + ["--kmer-correct"])
    assert a.kmer_ratio is None and a.kmer_range == (15, 20, 5)
    a = parse_args(BASE + ["--kmer-correct", "--kmer-ratio", "8"])
    assert a.kmer_ratio == 8 and a.kmer_range == (15, 20, 5)
    a = parse_args(BASE + ["--kmer-correct", "-ks", "8", "-ke", "31", "-kh", "1", "--kmer-ratio", str(2 ** 31 - 1), "-ai", "-gff"])
    assert a.kmer_ratio == 2 ** 31 - 1 and a.kmer_range == (8, 31, 1)
    a = parse_args(BASE + ["--kmer-correct", "--kmer-ratio", "2"])
    assert a.kmer_ratio == 2
    assert parse_args(BASE).kmer_ratio is None


def test_log_lines_from_restated_numbers():
    from mirge3_amd.collapse import kmer_ratio_log_lines
    for name in ("two_errors_two_rounds", "deep_template", "empty"):
        c, res = ec_ratio_cases.all_cases()[name], ec_ratio_cases.expected(name)
        stats = [{"above": a, "dominated": d} for a, d in zip(res["above"], res["dominated"])]
        assert kmer_ratio_log_lines("S1", c["ks"], c["R"], stats) == rr.ratio_log_lines("S1", c["ks"], c["R"], res)
    res = ec_ratio_cases.expected("deep_template")
    assert rr.ratio_log_lines("S1", 10, 8, res) == ["kmer-correct S1 k=10 ratio 8: k-mers above -kh 25, dominated 10"]
