"""``--unmapped-clusters`` (mirge3_amd/unmapped.py, ``mirge_loci_cluster``): the clustering rule against a sequential restatement,
the host half against fixtures the reference's own ``convert2Fasta`` / ``cluster_basedon_location`` wrote
(tests/golden/unmapped, make_golden_unmapped.py), the device kernel, and the switch end to end."""
import filecmp
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import mirge3_amd  # noqa: F401
from helpers import GOLDEN, GoldenCase, ORG
from mirge3_amd import unmapped

FIX = os.path.join(GOLDEN, "unmapped")
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SAMPLES = ["S1", "S2"]


def sequential_clusters(ref, off, strand, length, ref_skip, threshold, minus_first_only=True):
    """The reference's rule read record by record (novel_mir.py:98-132): per reference one list of clusters per strand; a record
    joins the LAST cluster of its list iff its start lies inside it and the overlap is at least the threshold, and then
    stretches it; otherwise it opens a cluster -- except on the minus strand, where (the last `else` binding to the outer
    `if`) it is dropped.  Clusters are numbered when written: per reference in order of appearance, '+' list then '-' list.
    -> (cluster id per record or -1, table rows (ref, strand, start1, end1, members))"""
    lists, where = {}, []
    for i in range(len(ref)):
        r, s = int(ref[i]), int(strand[i])
        if ref_skip[r]:
            where.append(None)
            continue
        start, end = int(off[i]) + 1, int(off[i]) + int(length[i])
        pair = lists.setdefault(r, ([], []))
        cur = pair[s]
        if not cur:
            cur.append([start, end, [i]])
            where.append((r, s, 0))
            continue
        last = cur[-1]
        if start >= last[0] and start <= last[1] and last[1] - start + 1 >= threshold:
            last[1] = max(last[1], end)
            last[2].append(i)
            where.append((r, s, len(cur) - 1))
        elif s == 0 or not minus_first_only:
            cur.append([start, end, [i]])
            where.append((r, s, len(cur) - 1))
        else:
            where.append(None)
    ids, rows = {}, []
    for r in lists:  # insertion order = order of appearance
        for s in (0, 1):
            for k, c in enumerate(lists[r][s]):
                ids[(r, s, k)] = len(rows)
                rows.append((r, s, c[0], c[1], len(c[2])))
    return np.array([-1 if w is None else ids[w] for w in where], dtype=np.int64), rows


def random_records(rng, n, n_refs=4, span=400, lens=(8, 31)):
    ref = np.sort(rng.integers(0, n_refs, n))
    off = np.zeros(n, dtype=np.int64)
    for r in range(n_refs):
        m = ref == r
        off[m] = np.sort(rng.integers(0, span, int(m.sum())))
    return ref, off, rng.integers(0, 2, n), rng.integers(lens[0], lens[1], n)


ADVERSARIAL = {
    # (ref, off, strand, length) rows, threshold 14 unless the name says otherwise; reference 2 is named without 'chr'
    "nested": [(0, 10, 0, 30), (0, 12, 0, 10), (0, 14, 0, 20), (0, 26, 0, 22), (0, 27, 0, 22)],
    "equal_starts_short_first": [(0, 5, 0, 10), (0, 5, 0, 25), (0, 5, 0, 12), (0, 16, 0, 20)],
    "equal_starts_long_first": [(0, 5, 0, 25), (0, 5, 0, 10), (0, 17, 0, 20)],
    "edge_minus_1": [(0, 100, 0, 22), (0, 108, 0, 22)],   # overlap 14: joins
    "edge_exact": [(0, 100, 0, 22), (0, 109, 0, 22)],     # overlap 13: opens
    "edge_plus_1": [(0, 100, 0, 22), (0, 110, 0, 22)],
    "long_then_far_short": [(0, 0, 0, 30), (0, 1, 0, 8), (0, 2, 0, 8), (0, 17, 0, 20), (0, 25, 0, 20), (0, 40, 0, 20)],
    "minus_non_joiners": [(0, 10, 1, 22), (0, 12, 1, 22), (0, 300, 1, 22), (0, 302, 1, 22), (0, 305, 0, 22), (1, 5, 1, 20),
                          (1, 200, 1, 20), (1, 201, 1, 20)],
    "minus_far_end_after_drop": [(0, 10, 1, 20), (0, 100, 1, 30), (0, 110, 1, 20), (0, 111, 0, 20)],
    "no_chr": [(1, 5, 0, 22), (2, 5, 0, 22), (2, 6, 0, 22), (2, 7, 1, 22), (3, 5, 1, 22)],
    "interleaved_strands": [(0, 10, 0, 22), (0, 11, 1, 22), (0, 12, 0, 22), (0, 13, 1, 22), (0, 40, 0, 22), (0, 41, 1, 22)],
}
SKIP = np.array([0, 0, 1, 0], dtype=np.uint8)


def _cols(rows):
    return tuple(np.array([r[k] for r in rows], dtype=np.int64) for k in range(4))


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_segmented_running_maximum_equals_the_sequential_rule():
    """the formulation the kernel implements (unmapped.cluster_scan) against the rule read record by record: random layouts,
    thresholds around the read lengths, both treatments of the minus strand, and the adversarial layouts"""
    rng = np.random.default_rng(1)
    n_clusters = 0
    for trial in range(300):
        n = int(rng.integers(1, 120))
        ref, off, strand, length = random_records(rng, n, span=int(rng.choice([60, 400, 3000])))
        thr = int(rng.choice([0, 1, 5, 14, 20, 40]))
        for mfo in (True, False):
            exp, rows = sequential_clusters(ref, off, strand, length, SKIP, thr, mfo)
            got = unmapped.cluster_scan(ref, off, strand, length, SKIP, thr, mfo)
            assert np.array_equal(got, exp), (trial, thr, mfo)
            n_clusters += len(rows)
    assert n_clusters > 3000
    for name, rows in ADVERSARIAL.items():
        for thr in (13, 14, 15):
            exp, _ = sequential_clusters(*_cols(rows), SKIP, thr)
            assert np.array_equal(unmapped.cluster_scan(*_cols(rows), SKIP, thr), exp), (name, thr)
    # what the layouts are there for
    assert sequential_clusters(*_cols(ADVERSARIAL["edge_minus_1"]), SKIP, 14)[0].tolist() == [0, 0]
    assert sequential_clusters(*_cols(ADVERSARIAL["edge_exact"]), SKIP, 14)[0].tolist() == [0, 1]
    assert sequential_clusters(*_cols(ADVERSARIAL["minus_non_joiners"]), SKIP, 14)[0].tolist() == [1, 1, -1, -1, 0, 2, -1, -1]
    assert sequential_clusters(*_cols(ADVERSARIAL["no_chr"]), SKIP, 14)[0].tolist() == [0, -1, -1, -1, 1]


def test_fasta_files_equal_the_references(tmp_path):
    """convert2Fasta's four files from unmapped.csv, byte for byte (names mir<row>_<count>, the per-sample second filter)"""
    seqs, counts = unmapped.read_unmapped_csv(os.path.join(FIX, "unmapped.csv"), SAMPLES)
    per, raw_n, filt_n = unmapped.convert2fasta(seqs, counts, SAMPLES, 16, 25, 2, tmp_path)
    for f in ["unmapped_mirna_raw.fa", "unmapped_mirna.fa"] + [f"unmapped_mirna_{s}.fa" for s in SAMPLES]:
        assert filecmp.cmp(os.path.join(FIX, f), tmp_path / f, shallow=False), f
    assert raw_n["S1"] > filt_n["S1"] > 30 and len(per["S2"][0]) == filt_n["S2"]
    # a row with enough reads in all but too few in each sample is in unmapped_mirna.fa and in no sample's file
    joint = open(os.path.join(FIX, "unmapped_mirna.fa")).read().count(">")
    assert joint > max(filt_n.values())


@pytest.mark.parametrize("sample", SAMPLES)
def test_cluster_file_equals_the_references(tmp_path, sample):
    """<sample>_clusters.tsv from the sorted SAM, byte for byte what cluster_basedon_location wrote: the append rule of the
    sequences, the minus strand's single cluster per reference, the reference without 'chr' left out"""
    out = tmp_path / "c.tsv"
    n = unmapped.clusters_from_sam(os.path.join(FIX, f"unmapped_mirna_{sample}_vs_genome_sorted.sam"), sample, 14, out)
    want = open(os.path.join(FIX, f"{sample}_clusters.tsv")).read()
    assert out.read_text() == want
    assert n == want.count("\n") - 1 >= 10
    assert "scaffold_7" not in want and "scaffold_7" in open(os.path.join(FIX, f"unmapped_mirna_{sample}_vs_genome_sorted.sam")).read()
    minus = [ln.split("\t")[1] for ln in want.split("\n")[1:] if ln and ln.split("\t")[2] == "-"]
    assert len(minus) == len(set(minus)) >= 2  # one minus-strand cluster per reference, though chr1 has two piles


def test_switch_parsing_defaults_and_refusals(capsys):
    from mirge3_amd.cli import parse_args
    base = ["-s", "a.fq", "-lib", "/x", "-on", "human"]
    off = parse_args(base + ["-minl", "18", "-olc", "12"])
    assert off.unmapped_clusters is False
    on = parse_args(base + ["--unmapped-clusters"])
    assert unmapped.settings(on) == dict(minl=16, maxl=25, c=2, mloc=3, sl=25, olc=14)
    on = parse_args(base + ["--unmapped-clusters", "-minl", "18", "-maxl", "30", "-c", "5", "-mloc", "7", "-sl", "20", "-olc", "12"])
    assert unmapped.settings(on) == dict(minl=18, maxl=30, c=5, mloc=7, sl=20, olc=12)
    for bad in (["--unmapped-clusters", "--backend", "bowtie"], ["--unmapped-clusters", "-spl"], ["--unmapped-clusters", "-olc", "x"],
                ["-nmir"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
    # what the genome scan refuses is refused here, before a file is written: a seed below bowtie's floor, reads past two words
    for ok in (["-sl", "5"], ["-maxl", "64"]):
        parse_args(base + ["--unmapped-clusters"] + ok)
    for bad, word in ((["-sl", "4"], "at least 5"), (["-sl", "0"], "at least 5"), (["-sl", "-3"], "at least 5"), (["-maxl", "65"], "64 nt")):
        with pytest.raises(SystemExit):
            parse_args(base + ["--unmapped-clusters"] + bad)
        assert word in capsys.readouterr().err, bad
        parse_args(base + bad)  # read only with the switch, as before


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gctx():
    from mirge3_amd import _ffi
    ctx = _ffi.Context(0)
    yield ctx
    ctx.close()


def device_clusters(ctx, ref, off, strand, length, skip, thr, mfo=True, qcount=None):
    """every record its own query (lengths and read counts per record)"""
    from mirge3_amd import _ffi
    n = len(ref)
    qcount = np.arange(1, n + 1, dtype=np.int64) if qcount is None else qcount
    return _ffi.loci_cluster(ctx, ref, off, strand, np.arange(n), length, qcount, skip, thr, mfo), qcount


def check_device(ctx, ref, off, strand, length, skip, thr, mfo=True):
    tab, qcount = device_clusters(ctx, ref, off, strand, length, skip, thr, mfo)
    exp, rows = sequential_clusters(ref, off, strand, length, skip, thr, mfo)
    assert np.array_equal(tab["cluster"].astype(np.int64), exp)
    assert len(tab["ref"]) == len(rows)
    for c, (r, s, start, end, members) in enumerate(rows):
        assert (int(tab["ref"][c]), int(tab["strand"][c]), int(tab["start"][c]) + 1, int(tab["end"][c]), int(tab["members"][c])) == \
            (r, s, start, end, members), c
        assert int(tab["reads"][c]) == int(qcount[exp == c].sum())
    return len(rows)


@pytest.mark.gpu
def test_device_clusters_equal_the_sequential_rule(gctx):
    """adversarial layouts at the threshold and one off, random layouts, and the alignments of a synthetic genome"""
    import test_genome_filter as gf
    for name, rows in ADVERSARIAL.items():
        for thr in (13, 14, 15):
            check_device(gctx, *_cols(rows), SKIP, thr)
    rng = np.random.default_rng(2)
    total = 0
    for trial in range(40):
        ref, off, strand, length = random_records(rng, int(rng.integers(1, 3000)), span=int(rng.choice([200, 5000, 100000])))
        total += check_device(gctx, ref, off, strand, length, SKIP, int(rng.choice([0, 1, 14, 25])), bool(trial % 2))
    assert total > 2000
    # loci of a genome with repeats on both strands: reads tiled over a few regions, -n 0 -l 25
    refs = gf.random_genome(rng, [3000, 2000, 2500, 1200])
    qs = []
    for r, at in ((0, 400), (0, 1500), (1, 800), (2, 300), (3, 500), (1, 237), (3, 274)):
        for sh in rng.integers(0, 40, 25).tolist():
            w = refs[r][at + sh:at + sh + int(rng.integers(18, 26))].replace("N", "A")
            qs.append(w if rng.random() < 0.5 else gf._rc(w))
    genome = gf._genome(gctx, refs)
    loci = genome.align_loci(gf._flat(qs), 0, 25, 2, 0, 0, 0)
    assert len(loci["query"]) >= len(qs)
    length = np.array([len(q) for q in qs])[loci["query"]]
    skip = np.array([0, 0, 1, 0], dtype=np.uint8)
    assert check_device(gctx, loci["ref"].astype(np.int64), loci["off"].astype(np.int64), loci["strand"].astype(np.int64), length, skip, 14) >= 5


@pytest.mark.gpu
def test_device_route_writes_the_fixture_cluster_files(tmp_path, gctx):
    """the fixture's genome and FASTA files through the device (-m off: the fixture's SAM holds every alignment): the same
    <sample>_clusters.tsv as the reference wrote, and a SAM whose aligned lines are the fixture's up to the order of ties"""
    from types import SimpleNamespace
    from mirge3_amd import a2i
    lib = tmp_path / "libs" / ORG / "index.Libs"
    lib.mkdir(parents=True)
    shutil.copy(os.path.join(FIX, "human_genome.fa"), lib / f"{ORG}_genome.fa")
    work = tmp_path / "out"
    work.mkdir()
    shutil.copy(os.path.join(FIX, "unmapped.csv"), work / "unmapped.csv")
    args = SimpleNamespace(libraries_path=str(tmp_path / "libs"), organism_name=ORG, ignored_mloc="0")
    g = a2i.GpuGenome(gctx, a2i.load_genome(gctx, str(a2i.genome_base(args))))
    tm = {}
    res = unmapped.run(args, gctx, work, SAMPLES, g, tm)
    assert tm["unmapped_loci_s"] > 0 and "unmapped clusters, S1" in (work / "run.log").read_text()
    for s in SAMPLES:
        assert (work / "unmapped_tmp" / f"{s}_clusters.tsv").read_text() == open(os.path.join(FIX, f"{s}_clusters.tsv")).read(), s
        body = lambda p: sorted(ln.split("\t")[:4] + [ln.split("\t")[9]] for ln in open(p) if ln[0] != "@" and ln.split("\t")[1] != "4")
        assert body(work / "unmapped_tmp" / f"unmapped_mirna_{s}_vs_genome_sorted.sam") == \
            body(os.path.join(FIX, f"unmapped_mirna_{s}_vs_genome_sorted.sam"))
        assert res[s]["clusters"] >= 10
    # -m 3, the default: the locus copied four times reports nothing
    args.ignored_mloc = None
    res3 = unmapped.run(args, gctx, work, SAMPLES, g, {})
    assert res3["S1"]["capped"] == 3 and res3["S1"]["alignments"] < res["S1"]["alignments"]


def _fastq_files(tmp_path, case):
    files = []
    for k, nm in enumerate(case.samples):
        p = tmp_path / f"{nm}.fastq"
        with open(p, "w") as fh:
            for seq, row in zip(case.seqs, case.counts):
                fh.write(f"@r\n{seq}\n+\n{'I' * len(seq)}\n" * int(row[k]))
        files.append(str(p))
    return files


@pytest.mark.gpu
@pytest.mark.parametrize("case_name", ["case4_gff_a2i", "case6_gff_a2i"])
def test_cli_switch_adds_five_kinds_of_files_and_moves_nothing_else(tmp_path, case_name):
    case = GoldenCase(case_name)
    files = _fastq_files(tmp_path, case)
    env = dict(os.environ, PYTHONPATH=ROOT)
    runs = {}
    for tag, extra in (("plain", []), ("clusters", ["--unmapped-clusters", "-c", "1"])):
        r = subprocess.run([sys.executable, "-m", "mirge3_amd.cli", "-s", ",".join(files), "-lib", case.libdir, "-on", ORG, "-db", "miRBase",
                            "-o", str(tmp_path / tag), "-ai", "--genome-filter", "gpu", "-gff", "-shh"] + extra, cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        (runs[tag],) = [d for d in (tmp_path / tag).iterdir() if d.is_dir()]
    plain = sorted(p.name for p in runs["plain"].iterdir())
    assert sorted(p.name for p in runs["clusters"].iterdir()) == sorted(plain + ["unmapped_tmp"])
    for f in plain:
        if f != "run.log":
            assert filecmp.cmp(runs["plain"] / f, runs["clusters"] / f, shallow=False), f
    for f in ("a2IEditing.report.csv", "mapped.csv", "unmapped.csv"):
        assert (runs["clusters"] / f).read_text() == case.text(f), f
    made = sorted(p.name for p in (runs["clusters"] / "unmapped_tmp").iterdir())
    want = ["unmapped_mirna_raw.fa", "unmapped_mirna.fa"]
    for s in case.samples:
        want += [f"unmapped_mirna_{s}.fa", f"unmapped_mirna_{s}_vs_genome_sorted.sam", f"{s}_clusters.tsv"]
    assert made == sorted(want)
    log = (runs["clusters"] / "run.log").read_text()
    assert "unmapped clusters:" in log and "unmapped clusters" not in (runs["plain"] / "run.log").read_text()
    # the files agree with each other: the SAM's aligned lines clustered on the host give the cluster file
    for s in case.samples:
        out = tmp_path / f"{s}.tsv"
        unmapped.clusters_from_sam(runs["clusters"] / "unmapped_tmp" / f"unmapped_mirna_{s}_vs_genome_sorted.sam", s, 14, out)
        assert out.read_text() == (runs["clusters"] / "unmapped_tmp" / f"{s}_clusters.tsv").read_text()
