"""CPU tests of ``--unmapped-nearest``: the restatement (tests/near_restate.py) against the definition -- an exhaustive ``lev`` over every
substring -- and against the hand-made expectations of the named cases (tests/near_cases.py); the column step of the kernels'
recurrence in Python integers of 32 and 64 bits against the same DP, m = W included; the writers of ``mirge3_amd/nearest.py`` on hand-made
rows; every refusal of the command line; the ``mature`` column on the libraries of tests/golden/case4_gff_a2i."""
import os
import random

import numpy as np
import pytest

import near_cases
import near_restate
import mirge3_amd  # noqa: F401
from mirge3_amd import nearest, seqio

HERE = os.path.dirname(os.path.abspath(__file__))
LIBS4 = os.path.join(HERE, "golden", "case4_gff_a2i", "libs")


def test_restatement_equals_the_exhaustive_definition():
    rng = random.Random(3)
    n = 0
    for trial in range(120):
        hairpins = [near_cases.rnd_seq(rng, rng.randint(0, 20), "ACGTN" if trial % 5 == 0 else ("AC" if trial % 3 == 0 else "ACGT"))
                    for _ in range(rng.randint(1, 4))]
        for _ in range(3):
            fit = [h for h in hairpins if len(h) >= 12]
            if fit and rng.random() < 0.7:
                h = rng.choice(fit)
                m = rng.randint(12, min(14, len(h)))
                at = rng.randrange(len(h) - m + 1)
                q = near_cases.edit(rng, h[at:at + m], rng.randint(0, 3))[:14]
            else:
                q = near_cases.rnd_seq(rng, rng.randint(11, 14), "AC" if trial % 3 == 0 else "ACGT")
            assert near_restate.nearest(q, hairpins) == near_restate.nearest_exhaustive(q, hairpins), (q, hairpins)
            n += 1
    assert n == 360
    # the tie rules by hand: lowest hairpin, smallest end, largest start; N matches nothing
    assert near_restate.nearest("ACGTACGTACGT", ["TTTT", "GGACGTACGTACGTGG", "ACGTACGTACGT"]) == (0, 1, 2, 14)
    assert near_restate.nearest("ACGTACGTACGT", ["ACGTACGTACGTACGT"]) == (0, 0, 0, 12)
    assert near_restate.nearest("TACGTACGTACGA", ["GGCACGTACGTACGAGG"]) == (1, 0, 3, 15)
    assert near_restate.nearest("ACGTACNTACGT", ["ACGTACNTACGT"]) == (1, 0, 0, 12)
    assert near_restate.nearest("ACGTACGTACG", ["ACGTACGTACGT"]) == (-1, -1, -1, -1) == near_restate.nearest("ACGTACGTACGT", ["", ""])
    assert near_restate.lev("ACGT", "AGT") == 1 and near_restate.lev("", "ACG") == 3 and near_restate.lev("AN", "AN") == 1


@pytest.mark.parametrize("case", near_cases.CASES, ids=lambda c: c["name"])
def test_named_cases_give_what_the_specification_says(case):
    got = near_restate.nearest_all(case["queries"], case["hairpins"])
    assert case["expect"], case["name"]
    for i, want in case["expect"].items():
        r = tuple(int(got[k][i]) for k in ("dist", "hairpin", "start", "end"))
        assert want(r) if callable(want) else r == want, (case["name"], i, r)


def test_side_by_side_form_of_the_restatement_equals_the_one_query_form():
    """``nearest_many`` (the GPU tests' thousands of queries) is the same DP: equal on every named case and on the random set"""
    sets = [(c["hairpins"], c["queries"]) for c in near_cases.CASES if c["name"] != "long_hairpin"] + near_cases.random_sets()
    for hairpins, queries in sets:
        one, many = near_restate.nearest_all(queries, hairpins), near_restate.nearest_many(queries, hairpins)
        for k in one:
            assert np.array_equal(one[k], many[k]), (k, queries, hairpins)


def test_cap_cases_sit_on_both_sides_of_the_bound():
    (case,) = [c for c in near_cases.CASES if c["name"] == "caps"]
    got = near_restate.nearest_all(case["queries"], case["hairpins"])
    seen = {}
    for q, d in zip(case["queries"], got["dist"].tolist()):
        for K in (3, 8):
            seen.setdefault((len(q), K), []).append((d, near_restate.reported(q, d, K), d <= nearest.cap(K, len(q))))
    assert sorted(seen) == [(m, K) for m in (16, 23, 24, 64) for K in (3, 8)]
    for (m, K), rows in seen.items():
        c = nearest.cap(K, m)
        assert c == {(16, 3): 2, (23, 3): 2, (24, 3): 3, (64, 3): 3, (16, 8): 2, (23, 8): 2, (24, 8): 3, (64, 8): 8}[(m, K)]
        assert (c, True, True) in rows and (c + 1, False, False) in rows, (m, K, rows)


def test_random_set_reports_between_a_quarter_and_three_quarters_of_its_random_queries():
    sets = near_cases.random_sets()
    assert len(sets) == 30 and sum(len(q) for _, q in sets) == 300
    assert all(1 <= len(h) <= 6 and all(1 <= len(x) <= 120 for x in h) for h, _ in sets)
    n = rep = 0
    for hairpins, queries in sets:
        got = near_restate.nearest_all(queries, hairpins)
        n += len(queries)
        rep += sum(near_restate.reported(q, d, nearest.DEFAULT_K) for q, d in zip(queries, got["dist"].tolist()))
    print(f"random set: {rep} of {n} queries reported by the restatement ({100.0 * rep / n:.1f} %)")
    assert n // 4 <= rep <= 3 * n // 4


def _myers(q: str, h: str, W: int, anchored: bool):
    """the kernels' column step in Python integers cut to W bits -> D[m][1 .. len(h)]"""
    mask, m = (1 << W) - 1, len(q)
    peq = {c: sum(1 << i for i, x in enumerate(q) if x == c) for c in "ACGT"}
    Pv, Mv, score, out = mask, 0, m, []
    for ch in h:
        Eq = peq.get(ch, 0)
        Xv = Eq | Mv
        Xh = ((((Eq & Pv) + Pv) & mask) ^ Pv) | Eq
        Ph = Mv | (~(Xh | Pv) & mask)
        Mh = Pv & Xh
        score += (Ph >> (m - 1)) & 1
        score -= (Mh >> (m - 1)) & 1
        Ph = ((Ph << 1) | (1 if anchored else 0)) & mask
        Mh = (Mh << 1) & mask
        Pv = Mh | (~(Xv | Ph) & mask)
        Mv = Ph & Xv
        out.append(score)
    return out


@pytest.mark.parametrize("W", [32, 64])
def test_the_column_step_equals_the_plain_dp(W):
    rng = random.Random(W)
    for trial in range(60):
        m = W if trial % 4 == 0 else rng.randint(1, W)
        q = near_cases.rnd_seq(rng, m, "ACGTN" if trial % 7 == 0 else "ACGT")
        h = near_cases.edit(rng, q, rng.randint(0, 6)) + near_cases.rnd_seq(rng, rng.randint(0, 30)) if trial % 2 else near_cases.rnd_seq(rng, rng.randint(1, 90))
        for anchored in (False, True):
            want = near_restate._row_m(near_restate._codes(q), near_restate._codes(h), anchored)[1:].tolist()
            assert _myers(q, h, W, anchored) == want, (q, h, anchored)


# ------------------------------------------------------------------------------------------------------------------ writers
def test_writers_on_hand_made_rows(tmp_path):
    names = ["S1", "S2"]
    seqs = ["ACGTACGTACGTA", "TTTTTTTTTT", "G" * 70, "ACGTACGTACGTACGTACGTACGTA", "CCCCCCCCCCCCCCCC"]
    counts = np.array([[3, 0], [1, 1], [0, 2], [5, 7], [0, 4]])
    hp_names, hp_seqs = ["hsa-mir-a", "hsa-mir-b"], ["GGACGTACGTACGTAGG", "TTACGTACGTACGTACGTACGTACGTATT"]
    hits = dict(row=np.array([0, 3]), dist=np.array([0, 1]), hairpin=np.array([0, 1]), start=np.array([2, 2]), end=np.array([15, 27]))
    index = {"hsa-mir-a": [("hsa-miR-a-5p", 0, 2), ("hsa-miR-a-3p", 14, 17)], "hsa-mir-b": [("hsa-miR-b-5p", 0, 3), ("hsa-miR-b-3p", 26, 29), ("hsa-miR-c", 27, 29)]}
    text = nearest.file_text(names, seqs, counts, hits, hp_names, hp_seqs, index)
    assert text == ("Sequence,hairpin,distance,start,end,matched,mature,S1,S2\n"
                    "ACGTACGTACGTA,hsa-mir-a,0,3,15,ACGTACGTACGTA,hsa-miR-a-3p,3,0\n"
                    "ACGTACGTACGTACGTACGTACGTA,hsa-mir-b,1,3,27,ACGTACGTACGTACGTACGTACGTA,hsa-miR-b-5p/hsa-miR-b-3p,5,7\n")
    assert nearest.file_text(names, seqs, counts, hits, hp_names, hp_seqs).split("\n")[1] == "ACGTACGTACGTA,hsa-mir-a,0,3,15,ACGTACGTACGTA,,3,0"
    with pytest.raises(ValueError):
        nearest.file_text(names, seqs, counts, dict(hits, row=np.array([3, 0])), hp_names, hp_seqs)
    rows = nearest.summary_rows(names, [len(s) for s in seqs], counts, hits, 2)
    #        unique reads short long considered d0 d1 d2
    assert rows == [[3, 9, 1, 0, 2, 1, 3, 1, 5, 0, 0], [4, 14, 1, 1, 2, 0, 0, 1, 7, 0, 0]]
    assert nearest.summary_text(names, rows, 2) == ("sample,unmapped_unique,unmapped_reads,too_short,too_long,considered,d0_unique,d0_reads,d1_unique,d1_reads,"
                                                   "d2_unique,d2_reads\nS1,3,9,1,0,2,1,3,1,5,0,0\nS2,4,14,1,1,2,0,0,1,7,0,0\n")
    assert nearest.log_line("S1", rows[0], 2) == ("unmapped nearest S1: 3 unmapped unique reads (9 raw), 1 too short, 0 too long, 2 considered; "
                                                  "reported unique (raw) with K = 2: d=0: 1 (3), d=1: 1 (5), d=2: 0 (0)")
    got = nearest.write_files(tmp_path, names, seqs, counts, hits, hp_names, hp_seqs, index, 2)
    assert got == rows and (tmp_path / nearest.FILE_NAME).read_text() == text
    assert (tmp_path / nearest.SUMMARY_NAME).read_text() == nearest.summary_text(names, rows, 2)
    assert sorted(p.name for p in tmp_path.iterdir()) == [nearest.SUMMARY_NAME, nearest.FILE_NAME]
    # no rows at all
    none = dict(row=np.zeros(0, np.int64), dist=np.zeros(0, np.int64), hairpin=np.zeros(0, np.int64), start=np.zeros(0, np.int64), end=np.zeros(0, np.int64))
    assert nearest.file_text(names, [], np.zeros((0, 2)), none, hp_names, hp_seqs) == nearest.header(names)
    assert nearest.summary_rows(names, [], np.zeros((0, 2)), none, 1) == [[0] * 9, [0] * 9]
    assert [nearest.cap(3, m) for m in (12, 15, 16, 23, 24, 31, 32, 64)] == [1, 1, 2, 2, 3, 3, 3, 3] and nearest.cap(8, 64) == 8 and nearest.cap(8, 63) == 7


# ------------------------------------------------------------------------------------------------------------------ command line
def test_switch_parsing_and_every_refusal(capsys, monkeypatch):
    from mirge3_amd.cli import parse_args
    base = ["-s", "a.fq", "-lib", "/x", "-on", "human"]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert parse_args(base).unmapped_nearest is None
    assert parse_args(base + ["--unmapped-nearest"]).unmapped_nearest == 3
    assert parse_args(["--unmapped-nearest"] + base).unmapped_nearest == 3
    for k in range(1, 9):
        assert parse_args(base + ["--unmapped-nearest", str(k)]).unmapped_nearest == k
    both = parse_args(base + ["--unmapped-nearest", "2", "--unmapped-clusters", "--read-qc"])  # independent of the genome route
    assert both.unmapped_nearest == 2 and both.unmapped_clusters
    for bad, word in ((["--unmapped-nearest", "0"], "1 <= K <= 8"), (["--unmapped-nearest", "9"], "1 <= K <= 8"), (["--unmapped-nearest", "-1"], "1 <= K <= 8"),
                      (["--unmapped-nearest", "x"], "takes an integer"), (["--unmapped-nearest", "2.5"], "takes an integer"),
                      (["--unmapped-nearest", "-spl"], "-spl / -rr / --backend bowtie"), (["--unmapped-nearest", "4", "-rr"], "-spl / -rr / --backend bowtie"),
                      (["--unmapped-nearest", "--backend", "bowtie"], "-spl / -rr / --backend bowtie")):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
        assert word in capsys.readouterr().err, bad
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        parse_args(base + ["--unmapped-nearest"])
    assert "single-process" in capsys.readouterr().err
    parse_args(base)  # the sharded run without the switch is not this module's business


# ------------------------------------------------------------------------------------------------------------------ the mature column
def test_mature_column_on_the_case4_libraries():
    libs = seqio.load_library_dir(LIBS4, "human", "miRBase")
    hp = libs["hairpin"]
    hp_names, hp_seqs = nearest.hairpin_names(hp), hp.seqs.to_list()
    tables = nearest.mature_tables(LIBS4, "human", "miRBase", libs["mirna"].names, hp)
    assert tables is not None
    index = nearest.mature_index(tables, hp_names, hp_seqs)
    # hsa-mir-1 carries hsa-miR-1-5p at 10 .. 29 and hsa-miR-46-3p at 54 .. 76 (1-based: the gff3's 10010-10028 and 10054-10075 on 10000)
    seq_of = dict(zip(hp_names, hp_seqs))
    on1 = index["hsa-mir-1"]
    assert [nm for nm, _, _ in on1][:1] == ["hsa-miR-1-5p"] and on1[0][1:] == (10, 29)
    for hairpin, entries in index.items():
        assert len({nm for nm, _, _ in entries}) == len(entries)
        for nm, a, b in entries:
            assert 0 <= a < b <= len(seq_of[hairpin])
    assert len(index) >= 40  # nearly every one of the 48 hairpins carries a canonical, the last one included
    assert hp_names[-1] in index
    assert nearest.mature_names(index, "hsa-mir-1", 0, 10) == "" and nearest.mature_names(index, "hsa-mir-1", 0, 11) == "hsa-miR-1-5p"
    assert nearest.mature_names(index, "hsa-mir-1", 28, 29) == "hsa-miR-1-5p" and nearest.mature_names(index, "hsa-mir-1", 29, 40) == ""
    both = nearest.mature_names(index, "hsa-mir-1", 0, len(seq_of["hsa-mir-1"]))
    assert both.split("/")[0] == "hsa-miR-1-5p" and len(both.split("/")) == len(on1) >= 2
    assert nearest.mature_names(index, "no-such-hairpin", 0, 5) == ""
    # a query cut from a hairpin over a canonical, through the writers
    s, e = on1[0][1] - 3, on1[0][2] + 2
    hits = dict(row=np.array([0]), dist=np.array([0]), hairpin=np.array([0]), start=np.array([s]), end=np.array([e]))
    line = nearest.file_text(["S1"], [hp_seqs[0][s:e]], np.array([[4]]), hits, hp_names, hp_seqs, index).split("\n")[1]
    assert line == f"{hp_seqs[0][s:e]},hsa-mir-1,0,{s + 1},{e},{hp_seqs[0][s:e]},hsa-miR-1-5p,4"
    # a library directory without the gff3 or the mature FASTA: no tables, an empty column
    case1 = os.path.join(HERE, "golden", "case1_single", "libs")
    assert nearest.mature_tables(case1, "human", "miRBase", libs["mirna"].names, hp) is None
    assert nearest.mature_index(None, hp_names, hp_seqs) == {}
