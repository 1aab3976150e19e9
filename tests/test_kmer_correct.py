"""``--kmer-correct`` without a GPU: the restatement (tests/ec_restate.py) against the hand-written expectations of the named cases
(tests/ec_cases.py), conservation of the total count, a property run over random small sets, the command line's refusals, and the text
of ``<sample>_kmerCorrected.csv`` and of the ``run.log`` lines from restated arrays."""
import numpy as np
import pytest

import ec_cases
import ec_restate


@pytest.mark.parametrize("name", sorted(ec_cases.all_cases()))
def test_restatement_gives_what_the_case_was_written_for(name):
    ec_cases.holds(name)


@pytest.mark.parametrize("name", sorted(ec_cases.all_cases()))
def test_total_count_is_conserved_and_first_indices_are_minima(name):
    c, res = ec_cases.all_cases()[name], ec_cases.expected(name)
    assert sum(e[1] for e in res["entries"]) == sum(c["counts"])
    assert len({e[0] for e in res["entries"]}) == len(res["entries"])
    by_final = {}
    for i, (fin, cnt) in enumerate(zip(res["final"], c["counts"])):
        n, f = by_final.get(fin, (0, i))
        by_final[fin] = (n + cnt, min(f, i))
    assert sorted(res["entries"], key=lambda e: e[2]) == res["entries"]
    assert {e[0]: (e[1], e[2]) for e in res["entries"]} == by_final
    assert all(len(a) == len(b) for a, b in zip(c["reads"], res["final"]))


def test_no_corrected_read_keeps_a_weak_window_where_it_changed():
    """a few thousand random sets (four- and two-letter alphabets: ties): after a round every window of a corrected read that covers
    the changed letter was solid in THAT round's spectrum, the read differs from what it was in exactly one letter inside
    [max W, min W + k - 1], the count is conserved, and a read that is not eligible never changes"""
    seen = dict.fromkeys(("corrected", "ambiguous", "unsupported", "uncorrectable"), 0)
    for seed in range(3000):
        case = ec_cases.random_set(seed, letters="AC" if seed % 3 == 0 else "ACGT")
        k, H = case["ks"], case["H"]
        entries = sorted(zip(case["reads"], case["counts"], range(len(case["reads"]))), key=lambda e: e[2])
        S = ec_restate.spectrum(entries, k)
        out, becomes, fixed, tally = ec_restate.one_round(entries, k, H)
        assert sum(e[1] for e in out) == sum(case["counts"])
        for key in seen:
            seen[key] += tally[key]
        assert tally["suspect"] == tally["corrected"] + tally["uncorrectable"] + tally["unsupported"] + tally["ambiguous"]
        for (read, count, _), new, fx in zip(entries, becomes, fixed):
            assert fx == (new != read)
            if not ec_restate.eligible(read, k) or count > H:
                assert new == read
            if fx:
                diff = [p for p in range(len(read)) if read[p] != new[p]]
                W = ec_restate.weak_starts(read, k, S, H)
                assert len(diff) == 1 and max(W) <= diff[0] <= min(W) + k - 1
                p = diff[0]
                assert all(S.get(new[i:i + k], 0) > H for i in range(max(0, p - k + 1), min(p, len(read) - k) + 1))
    assert min(seen.values()) > 50, seen


BASE = ["-s", "x.fastq", "-lib", "/nowhere", "-on", "human"]


@pytest.mark.parametrize("extra, message", [
    (["-kh", "0"], "--kmer-correct: -kh is at least 1"),
    (["-ks", "7"], "--kmer-correct: 8 <= -ks <= -ke <= 31"),
    (["-ke", "32"], "--kmer-correct: 8 <= -ks <= -ke <= 31"),
    (["-ks", "20", "-ke", "19"], "--kmer-correct: 8 <= -ks <= -ke <= 31"),
    (["-kh", "five"], "--kmer-correct: -kh takes an integer"),
    (["-ks", "15.5"], "--kmer-correct: -ks takes an integer"),
    (["-ke", "2e1"], "--kmer-correct: -ke takes an integer"),
    (["-umi", "4,4"], "--kmer-correct is not run together with -umi"),
    (["-spl"], "--kmer-correct runs on the device-resident route: not together with -spl / -rr / --backend bowtie"),
    (["-rr"], "--kmer-correct runs on the device-resident route: not together with -spl / -rr / --backend bowtie"),
    (["--backend", "bowtie"], "--kmer-correct runs on the device-resident route: not together with -spl / -rr / --backend bowtie"),
])
def test_the_command_line_refuses(extra, message, capsys):
    from mirge3_amd.cli import parse_args
    with pytest.raises(SystemExit):
        parse_args(BASE + ["--kmer-correct"] + extra)
    assert message in capsys.readouterr().err


def test_a_sharded_run_is_refused(monkeypatch, capsys):
    from mirge3_amd.cli import parse_args
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        parse_args(BASE + ["--kmer-correct"])
    assert "--kmer-correct is a single-process option" in capsys.readouterr().err


def test_the_command_line_accepts_and_mEC_stays_refused(capsys):
    from mirge3_amd.cli import parse_args
    a = parse_args(BASE + ["--kmer-correct"])
    assert a.kmer_correct and a.kmer_range == (15, 20, 5)
    a = parse_args(BASE + ["--kmer-correct", "-ks", "8", "-ke", "31", "-kh", "1", "-ai", "-gff", "-tcf", "-ie"])
    assert a.kmer_range == (8, 31, 1)
    a = parse_args(BASE + ["-ks", "3", "-ke", "99", "-kh", "x"])  # without the switch the three stay accepted and ignored
    assert not a.kmer_correct and a.kmer_range is None
    with pytest.raises(SystemExit):
        parse_args(BASE + ["-mEC"])


def test_csv_and_log_text_from_restated_arrays():
    from mirge3_amd.collapse import kmer_corrected_csv, kmer_correct_log_lines
    from mirge3_amd.seqio import FlatSeqs
    for name in ("two_rounds", "higher_wins", "nothing_suspect", "empty", "word_boundaries"):
        c, res = ec_cases.all_cases()[name], ec_cases.expected(name)
        masks = np.array([sum(1 << (k - c["ks"]) for k in ks) for ks in res["rounds"]], dtype=np.uint32)
        got = kmer_corrected_csv(FlatSeqs.from_list(c["reads"]), FlatSeqs.from_list(res["final"]), np.array(c["counts"], dtype=np.uint32), masks, c["ks"])
        assert got.decode() == ec_restate.csv_text(c["reads"], c["counts"], res), name
        stats = [dict(t) for t in res["tallies"]]
        assert kmer_correct_log_lines("S1", c["ks"], stats) == ec_restate.log_lines("S1", c["ks"], res)
    c, res = ec_cases.all_cases()["two_rounds"], ec_cases.expected("two_rounds")
    assert ec_restate.csv_text(c["reads"], c["counts"], res) == f"Original,Corrected,Count,Rounds\n{c['reads'][1]},{c['reads'][0]},1,8;9\n"
    assert ec_restate.log_lines("S1", 8, res)[1] == ("kmer-correct S1 k=9: eligible 3, suspect 1, corrected 1, uncorrectable 0, unsupported 0, ambiguous 0, "
                                                    "distinct reads after the round 2")
