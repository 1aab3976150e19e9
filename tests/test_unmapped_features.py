"""``--unmapped-features`` (mirge3_amd/unmapped_features.py; ``mirge_cluster_diagonals``, ``mirge_cluster_pileup``,
``mirge_genome_fetch``): the host text against the files the reference's own ``generate_featureFiles`` / ``get_precursors`` wrote
(tests/golden/unmapped_features, make_golden_unmapped_features.py) from pile-up arrays restated by brute force in this file, the
Smith-Waterman twin against the committed stand-in, the window bounds against Python slicing, the device route on the fixture
and the switch end to end."""
import filecmp
import os
import shutil
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import mirge3_amd  # noqa: F401
from helpers import GOLDEN, GoldenCase, ORG
from mirge3_amd import unmapped_features as uf

FIX = os.path.join(GOLDEN, "unmapped_features")
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SAMPLES = ["S1", "S2"]
OUTPUTS = ["{s}_features.tsv", "{s}_cluster.txt", "{s}_precursor.fa"]
# what make_golden_unmapped_features.py printed: entries of the table (S1: 34 names, two of them twice), in _cluster.txt, feature
# rows, precursors
COUNTS = dict(S1=(36, 26, 24, 44), S2=(8, 8, 8, 16))
# and the kinds it counted on S1 (it asserts at least two of each)
KINDS = {'plus': 13, 'minus': 11, 'low_count': 2, 'few_rows': 2, 'near_start': 2, 'near_end': 2, 'no_stable': 2, 'short_stable': 2,
         'head_pad': 19, 'head_no_pad': 5, 'tail_pad': 22, 'tail_no_pad': 2, 'tail_minus1': 11, 'overhang_head': 2, 'overhang_tail': 2,
         'mismatch': 4, 'read_N': 2, 'base_tie': 2, 'majority_tie': 2, 'Good': 2, 'Bad_strand': 2, 'Bad_distance': 8, 'Null': 13,
         'clamped_precursor': 2, 'repeated_name': 2}
_RC = str.maketrans("ACGTN", "TGCAN")


def genome():
    names, seqs = [], []
    for line in open(os.path.join(FIX, "genome.fa")):
        if line[0] == ">":
            names.append(line[1:].strip())
        else:
            seqs.append(line.strip())
    return names, seqs


def slicing_fetch(chrom_seq):
    """``fetch`` of write_features from Python strings: the reference's own expressions"""
    def fetch(windows):
        out = []
        for chrom, start, length, minus, rna in windows:
            s = chrom_seq[chrom][start:start + length]
            s = s.translate(_RC)[::-1] if minus else s
            out.append(s.replace("T", "U") if rna else s)
        return out
    return fetch


def brute_row(cluster, read):
    """every ungapped local alignment of ``read`` on ``cluster``: -> (diagonal, score, identity on that diagonal) of the best one,
    equal scores by (end in the cluster, end in the read)"""
    best = None
    for d in range(-(len(read) - 1), len(cluster)):
        cells = [(i, i - d) for i in range(max(0, d), min(len(cluster), len(read) + d))]
        same = sum(1 for i, j in cells if cluster[i] == read[j] and cluster[i] in "ACGT")
        for a in range(len(cells)):
            s = 0
            for i, j in cells[a:]:
                s += 2 if (cluster[i] == read[j] and cluster[i] in "ACGT") else -1
                key = (-s, i, j)
                if s > 0 and (best is None or key < best[0]):
                    best = (key, d, s, same)
    return (0, 0, 0) if best is None else best[1:]


def brute_arrays(ctx, clusters, tm=None):
    """``device_arrays`` by brute force: the same dictionary"""
    diag, score, ident, flag, head, tail, tally, col_off, row_start = [], [], [], [], [], [], [], [0], [0]
    for cseq, reads, counts in clusters:
        rows = [brute_row(cseq, r) for r in reads]
        h = max([0] + [-d for d, _, _ in rows])
        t = max([0] + [len(r) + d - len(cseq) for r, (d, _, _) in zip(reads, rows)])
        tab = np.zeros((h + len(cseq) + t, 5), dtype=np.int64)
        for r, n, (d, s, same) in zip(reads, counts, rows):
            for j, ch in enumerate(r):
                tab[h + d + j, "ATCG".find(ch) if ch in "ATCG" else 4] += n
            diag.append(d); score.append(s); ident.append(same)
            flag.append((0 if s > 2 * min(len(r), len(cseq)) - 20 else 1) | (0 if s > 0 else 2))
        head.append(h); tail.append(t); tally.append(tab)
        col_off.append(col_off[-1] + tab.shape[0]); row_start.append(row_start[-1] + len(reads))
    return dict(diag=np.array(diag, np.int32), score=np.array(score, np.int32), identity=np.array(ident, np.int32),
                flag=np.array(flag, np.uint8), head=np.array(head, np.int32), tail=np.array(tail, np.int32),
                col_off=np.array(col_off, np.int64), tally=np.concatenate(tally) if tally else np.zeros((0, 5), np.int64),
                row_start=np.array(row_start, np.int64))


def host_route(tmp_path, sample, arrays_fn=brute_arrays, table=None):
    names, seqs = genome()
    shutil.copy(table or os.path.join(FIX, f"{sample}_modified_selected_sorted.tsv"), tmp_path / f"{sample}_modified_selected_sorted.tsv")

    def pile_fn(clusters):
        assert all(uf.device_eligible(c[0], c[1]) for c in clusters)
        return uf.piles_from_arrays(clusters, arrays_fn(None, clusters))
    return uf.write_features(sample, tmp_path, {n: len(s) for n, s in zip(names, seqs)}, pile_fn, slicing_fetch(dict(zip(names, seqs))))


# ------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("sample", SAMPLES)
def test_host_text_reproduces_the_reference_files(tmp_path, sample):
    res = host_route(tmp_path, sample)
    for f in OUTPUTS:
        assert filecmp.cmp(tmp_path / f.format(s=sample), os.path.join(FIX, f.format(s=sample)), shallow=False), f
    assert (res["clusters"], res["detailed"], res["rows"], res["precursors"]) == COUNTS[sample]
    assert res["flagged"] == 0 and res["fallback"] == 0
    if sample == "S1":  # the quirks the fixture was built for (make_golden_unmapped_features.py asserts at least two of each)
        text = (tmp_path / "S1_cluster.txt").read_text()
        assert "\t0\t" in text or ": 0\t" in text  # a padded column's integer 0 among the float ratios
        feat = [ln.split("\t") for ln in (tmp_path / "S1_features.tsv").read_text().split("\n")[1:] if ln]
        assert {f[-3] for f in feat} == {"Good", "Bad", "Null"} and "None" in {f[-1] for f in feat} | {f[-2] for f in feat}
        names = [f[5] for f in feat]
        assert (sum(n[-1] == "+" for n in names), sum(n[-1] == "-" for n in names)) == (KINDS["plus"], KINDS["minus"])
        assert [sum(f[-3] == k for f in feat) for k in ("Good", "Null")] == [KINDS["Good"], KINDS["Null"]]
        k_hu, k_tu = uf.HEADER.split("\t").index("headUnstableLength"), uf.HEADER.split("\t").index("tailUnstableLength")
        assert sum(int(f[k_hu]) < 3 for f in feat) == KINDS["head_pad"] and sum(int(f[k_tu]) < 6 for f in feat) == KINDS["tail_pad"]
        assert sum(int(f[k_tu]) == 0 for f in feat) == KINDS["tail_minus1"]
        assert res["clusters"] - res["passed"] == sum(KINDS[k] for k in ("low_count", "few_rows", "near_start", "near_end"))
        assert res["passed"] - res["detailed"] == KINDS["no_stable"] and res["detailed"] - res["rows"] == KINDS["short_stable"]
        assert len(names) - len(set(names)) == KINDS["repeated_name"]  # two names come twice; the precursors name each once
        assert res["passed"] == 36 - 8 and res["precursors"] == 2 * len(set(names))


def test_all_string_route_writes_the_same_files(tmp_path):
    """every cluster through ``string_pile`` (the reference's route over the Smith-Waterman twin): the same bytes"""
    def all_flagged(ctx, clusters, tm=None):
        a = brute_arrays(ctx, clusters)
        a["flag"][:] = 1
        return a
    res = host_route(tmp_path, "S1", all_flagged)
    for f in OUTPUTS:
        assert filecmp.cmp(tmp_path / f.format(s="S1"), os.path.join(FIX, f.format(s="S1")), shallow=False), f
    assert res["flagged"] == res["fallback"] > 0


def test_no_detailed_cluster_leaves_half_a_header(tmp_path):
    lines = [ln for ln in open(os.path.join(FIX, "S1_modified_selected_sorted.tsv")) if ":chr10:30" in ln or ":chr10:33" in ln]
    assert lines
    (tmp_path / "in.tsv").write_text("".join(lines))  # the two clusters whose counts sum to less than 10
    res = host_route(tmp_path, "S9", table=tmp_path / "in.tsv")
    assert (tmp_path / "S9_features.tsv").read_text() == uf.HEADER and not uf.HEADER.endswith("\n")
    assert (tmp_path / "S9_cluster.txt").read_text() == "" and (tmp_path / "S9_precursor.fa").read_text() == ""
    assert res["passed"] == 0 and res["precursors"] == 0


def test_smith_waterman_twin_equals_the_stand_in():
    sys.path.insert(0, os.path.join(GOLDEN, "stubs"))
    try:
        from Bio import pairwise2
    finally:
        sys.path.pop(0)
    rng = np.random.default_rng(17)

    def rand(n):
        return "".join("ACGT"[int(c)] for c in rng.integers(0, 4, n))
    gapped = 0
    for k in range(400):
        a = rand(int(rng.integers(16, 41)))
        i = int(rng.integers(0, 8))
        b = a[i:i + int(rng.integers(8, 26))]
        if k % 4 == 0:
            a = rand(40)
            b = a[1:14] + a[15 + k % 2:29]  # two segments of more than ten matches around an indel: the gap wins
        elif k % 4 == 1:
            b = "".join(rng.choice(list("ACGTN")) for _ in range(20))
        elif k % 4 == 2:
            u = rand(8)
            a, b = u + u + u, u + u[:4]  # tandem: equal scores on several diagonals
        want = pairwise2.align.localms(a, b, 2, -1, -20, -20)
        got = uf.localms_first(a, b)
        if not want:
            assert got is None
            continue
        assert got == (want[0].seqA, want[0].seqB, want[0].score), (a, b)
        gapped += "-" in got[0].strip("-") or "-" in got[1].strip("-")
        d, s, same = brute_row(a, b)
        if s > 2 * min(len(a), len(b)) - 20:  # the bound of DESIGN.md: the ungapped diagonal IS the answer
            assert got[2] == s and uf.head_dashes(got[1]) - uf.head_dashes(got[0]) == d
            assert uf.calculate_identity(got[0], got[1]) == same
    assert gapped >= 50


def test_window_bounds_are_python_slices():
    s = "".join("ACGT"[k % 4] for k in range(50))
    for a in (None, -60, -7, -1, 0, 3, 49, 50, 70):
        for b in (None, -60, -3, 0, 5, 50, 90):
            lo, n = uf.slice_bounds(a, b, len(s))
            assert s[lo:lo + n] == s[a:b], (a, b)
    # get_precursors: a start that clamps to 0 takes the [:end] branch
    head = uf.HEADER + "\t".join(uf.POSITION_LABELS) + "\tneighborState\tupstreamDistance\tdownstreamDistance\n"
    row = ["Null", "Null", "chr3", "40", "63", "S:miRCluster_1_24:chr3:40_63+", "x", "x", "x", "-" + "A" * 24 + "--"] + ["x"] * 6 + ["2", "1"]
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "f.tsv"), "w") as fh:
            fh.write(head + "\t".join(row + ["x"] * 63 + ["Null", "None", "None"]) + "\n")
        w = uf.precursor_windows(os.path.join(d, "f.tsv"))
    # start 40 - 1 dash + 2 = 41, end 63 + 2 - 1 = 64
    assert w == [("S:miRCluster_1_24:chr3:40_63+:precusor_1", "chr3", None, 84, "+"), ("S:miRCluster_1_24:chr3:40_63+:precusor_2", "chr3", 20, 134, "+")]


def test_switch_parsing_implication_and_refusals():
    from mirge3_amd.cli import parse_args
    base = ["-s", "a.fq", "-lib", "/x", "-on", "human"]
    off = parse_args(base + ["--unmapped-align"])
    assert off.unmapped_features is False
    on = parse_args(base + ["--unmapped-features"])
    assert on.unmapped_features is True and on.unmapped_align is True and on.unmapped_clusters is True
    parse_args(base + ["--unmapped-features", "-clc", "26"])
    for bad in (["--unmapped-features", "--backend", "bowtie"], ["--unmapped-features", "-spl"], ["--unmapped-features", "-rr"],
                ["--unmapped-features", "-clc", "x"], ["--unmapped-features", "-nmir"], ["-nmir"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gctx():
    from mirge3_amd import _ffi
    ctx = _ffi.Context(0)
    yield ctx
    ctx.close()


def device_genome(ctx):
    from mirge3_amd import _ffi
    from mirge3_amd.seqio import FlatSeqs
    names, seqs = genome()
    g = _ffi.DeviceGenome(ctx, seqs=FlatSeqs.from_list(seqs))
    g.ref_names, g.ref_lens = names, [len(s) for s in seqs]
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("sample", SAMPLES)
def test_device_route_writes_the_reference_files(tmp_path, gctx, sample):
    g = device_genome(gctx)
    shutil.copy(os.path.join(FIX, f"{sample}_modified_selected_sorted.tsv"), tmp_path)
    log = []
    res = uf.features_sample(gctx, sample, tmp_path, g, log)
    g.close()
    for f in OUTPUTS:
        assert filecmp.cmp(tmp_path / f.format(s=sample), os.path.join(FIX, f.format(s=sample)), shallow=False), f
    assert res["flagged"] == 0 and res["fallback"] == 0
    assert (res["clusters"], res["detailed"], res["rows"], res["precursors"]) == COUNTS[sample]
    assert log and log[0].startswith(f"unmapped features, {sample}: ")


@pytest.mark.gpu
def test_genome_fetch_equals_python_slicing(gctx):
    from mirge3_amd import _ffi
    from mirge3_amd.seqio import FlatSeqs
    rng = np.random.default_rng(5)
    refs = ["".join("ACGT"[int(c)] for c in rng.integers(0, 4, n)) for n in (700, 90, 1300)]
    refs[0] = "NN" + refs[0][2:300] + "N" * 11 + refs[0][311:690] + "RYNNNNNNNN"
    refs[2] = refs[2][:640] + "n" + refs[2][641:]
    refs[1] = refs[1].lower()
    g = _ffi.DeviceGenome(gctx, seqs=FlatSeqs.from_list(refs))
    wins = [(0, 0, 40), (0, 280, 60), (0, 650, 50), (0, 699, 1), (0, 700, 0), (1, 0, 90), (1, 85, 5), (2, 600, 100), (2, 0, 1300), (2, 1299, 1)]
    wins += [(int(r), int(a), int(rng.integers(0, 150))) for r, a in zip(rng.integers(0, 3, 200), rng.integers(0, 1300, 200))]
    wins = [(r, a, min(n, len(refs[r]) - a)) for r, a, n in wins if a <= len(refs[r])]
    minus = [k % 2 for k in range(len(wins))]
    rna = [(k // 2) % 2 for k in range(len(wins))]
    got = g.fetch([w[0] for w in wins], [w[1] for w in wins], [w[2] for w in wins], minus, rna)
    g.close()
    for (r, a, n), m, u, text in zip(wins, minus, rna, got):
        want = "".join(ch if ch in "ACGT" else "N" for ch in refs[r][a:a + n].upper())
        want = want.translate(_RC)[::-1] if m else want
        assert text == (want.replace("T", "U") if u else want), (r, a, n, m, u)
    assert any("N" in t and len(t) > 11 for t in got)


@pytest.mark.gpu
def test_cli_switch_adds_its_files_and_they_agree_with_features_sample(tmp_path, gctx):
    case = GoldenCase("case4_gff_a2i")
    from test_unmapped_clusters import _fastq_files
    from mirge3_amd import a2i
    files = _fastq_files(tmp_path, case)
    # the case's own unannotated reads make no cluster of three reads and ten counts, so piles are planted on its genome: at five
    # places per chromosome a 24-nt window twelve times and two 22-nt windows of it three times each, alternately on either strand
    # (a window the cascade annotates, or one beside a repeat, is lost; the rest become clusters with a stable head and tail)
    planted = []
    for k, line in enumerate(ln.strip() for ln in open(os.path.join(case.libdir, ORG, "index.Libs", f"{ORG}_genome.fa")) if ln[0] != ">"):
        for at in range(500, 5500, 1000):
            w = line[at:at + 24].upper()
            if set(w) <= set("ACGT"):
                w = w.translate(_RC)[::-1] if (at // 1000 + k) % 2 else w
                planted += [w] * 12 + [w[:22]] * 3 + [w[2:]] * 3
    for f in files:
        with open(f, "a") as fh:
            fh.write("".join(f"@p\n{q}\n+\n{'I' * len(q)}\n" for q in planted))
    r = subprocess.run([sys.executable, "-m", "mirge3_amd.cli", "-s", ",".join(files), "-lib", case.libdir, "-on", ORG, "-db", "miRBase",
                        "-o", str(tmp_path / "run"), "-ai", "--genome-filter", "gpu", "-gff", "-shh", "--unmapped-features", "-c", "1"],
                       cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    (run,) = [d for d in (tmp_path / "run").iterdir() if d.is_dir()]
    log = (run / "run.log").read_text()
    assert "unmapped align:" in log and "unmapped features:" in log
    through = [s for s in case.samples if f"unmapped align, {s}:" in log]
    assert through
    args = SimpleNamespace(libraries_path=case.libdir, organism_name=ORG)
    g = a2i.load_genome(gctx, str(a2i.genome_base(args)))
    n_rows = n_pre = 0
    for s in case.samples:
        d = run / "unmapped_tmp"
        assert all((d / f.format(s=s)).exists() for f in OUTPUTS) == (s in through)
        if s not in through:
            continue
        assert f"unmapped features, {s}: " in log
        n_rows += (d / f"{s}_features.tsv").read_text().count("\n") - 1
        n_pre += (d / f"{s}_precursor.fa").read_text().count(">")
        head = (d / f"{s}_features.tsv").read_text().split("\n")[0].split("\t")
        assert head[:3] == ["realMicRNA", "realMicRNAName", "chr"] and (len(head) in (19, 18 + 63 + 3))
        fa = (d / f"{s}_precursor.fa").read_text().split("\n")
        assert all(set(x) <= set("ACGUN") for x in fa[1::2])
        again = tmp_path / f"again_{s}"
        again.mkdir()
        shutil.copy(d / f"{s}_modified_selected_sorted.tsv", again)
        uf.features_sample(gctx, s, again, g)
        for f in OUTPUTS:
            assert filecmp.cmp(again / f.format(s=s), d / f.format(s=s), shallow=False), f
    assert n_rows >= 1 and n_pre >= 2  # the run reaches feature rows and genome windows, not only the half header
