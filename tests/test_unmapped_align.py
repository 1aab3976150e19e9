"""``--unmapped-align`` (mirge3_amd/unmapped_align.py, ``mirge_genome_align_loci_strata``): the host functions against the files the
reference's own ``preTrimClusteredSeq`` / processSam.py wrote (tests/golden/unmapped_align, make_golden_unmapped_align.py), the
best-stratum call against a brute-force restatement in this file, the device route on the fixture inputs, and the switch end
to end."""
import filecmp
import hashlib
import os
import pickle
import shutil
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import mirge3_amd  # noqa: F401
from helpers import GOLDEN, GoldenCase, ORG
from mirge3_amd import unmapped_align as ua

FIX = os.path.join(GOLDEN, "unmapped_align")
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SAMPLES = ["S1", "S2"]
P = dict(minl=16, maxl=25, c=2, mloc=3, sl=25, olc=14, clc=30)
INPUTS = ["unmapped_mirna_{s}.fa", "unmapped_mirna_{s}_vs_genome_sorted.sam", "{s}_clusters.tsv"]
TEXT_OUT = ["{s}clusters_trimmed.tsv", "{s}_clusters_trimmed_orig.fa", "{s}_imperfectMath2Cluster.fa", "{s}_modified_selected_sorted.tsv",
            "{s}_modified_selected_reverseKept_sorted.tsv"]
SAM_OUT = ["{s}_tmp1.sam", "{s}_tmp2.sam", "{s}.sam", "{s}_modified.sam", "{s}_RepSeq_modified.sam", "{s}_selected.tsv",
           "{s}_selected_reverseKept.tsv"]


def fix(name, s=None):
    return os.path.join(FIX, name.format(s=s))


SUMS = dict(reversed(ln.split()) for ln in open(os.path.join(FIX, "derived.sha256")))  # the long derived files: SHA-256, not text
KEPT, ALIGNED2 = dict(S1=21, S2=10), dict(S1=25, S2=12)  # what make_golden_unmapped_align.py printed


def same(path, name, s):
    """the bytes of ``path`` are the fixture's: the committed file, or the committed sum of a file that is not committed as text"""
    name = name.format(s=s)
    if name in SUMS:
        return hashlib.sha256(open(path, "rb").read()).hexdigest() == SUMS[name]
    return filecmp.cmp(path, os.path.join(FIX, name), shallow=False)


def repeat_table():
    """the table of <org>_genome_repeats.pckl from the committed interval list: {chromosome: [[k-d tree], [(start, end, name)]]}"""
    from scipy.spatial import cKDTree
    table = {}
    for line in open(fix("repeats.txt")):
        c, a, b, n = line.rstrip("\n").split("\t")
        table.setdefault(c, [[], []])[1].append((int(a), int(b), n))
    for c in table:
        table[c][0] = [cKDTree([(e[0], 0) for e in table[c][1]])]
    return table


def loci_of_sam(path, q_names, c_names, mloc=0):
    """a cluster SAM of the fixture read back as the arrays the device hands out (any order)"""
    qi, ci = {n: k for k, n in enumerate(q_names)}, {n: k for k, n in enumerate(c_names)}
    q, r, o, mm = [], [], [], []
    capped = np.zeros(len(q_names), dtype=bool)
    for line in open(path):
        if line[0] == "@":
            continue
        f = line.rstrip("\n").split("\t")
        if f[1] == "0":
            q.append(qi[f[0]]); r.append(ci[f[2]]); o.append(int(f[3]) - 1); mm.append(int(f[11].split(":")[2]))
        elif f[11] == "XM:i:1":
            capped[qi[f[0]]] = True
    order = np.random.default_rng(3).permutation(len(q))
    return dict(query=np.array(q, dtype=np.uint32)[order], ref=np.array(r, dtype=np.uint32)[order], off=np.array(o, dtype=np.uint64)[order],
                mm=np.array(mm, dtype=np.uint8)[order], capped=capped)


# ------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("sample", SAMPLES)
def test_host_functions_reproduce_every_fixture_file(tmp_path, sample):
    s, out = sample, lambda f: tmp_path / f.format(s=sample)
    names, seqs = ua.read_fasta(fix("unmapped_mirna_{s}.fa", s))
    c_names, c_seqs = ua.pretrim_clusters(repeat_table(), fix("{s}_clusters.tsv", s), 30, out("{s}clusters_trimmed.tsv"),
                                          out("{s}_clusters_trimmed_orig.fa"))
    assert (c_names, c_seqs) == ua.read_fasta(fix("{s}_clusters_trimmed_orig.fa", s)) and len(c_names) == KEPT[s]
    flags = [ln.split("\t")[2:4] for ln in open(fix("{s}clusters_trimmed.tsv", s)).read().split("\n")[1:] if ln]
    assert {f for f, _ in flags} == {"0", "1"}
    if s == "S1":  # the names of the nearest, the second nearest and the only element, and '*'
        assert len({n for _, n in flags}) == 6
    c_lens = [len(x) for x in c_seqs]
    # the two cluster SAMs from their own records, whatever order those come in
    l1 = loci_of_sam(fix("{s}_tmp1.sam", s), names, c_names)
    assert l1["capped"].sum() == 3
    out("{s}_tmp1.sam").write_text(ua.cluster_sam_text(names, seqs, l1, c_names, c_lens, "-f -n 0 --best -a --norc -m 3 -l 25 -S"))
    i_names, i_seqs = ua.split_fasta_from_sam(out("{s}_tmp1.sam"), names, seqs, out("{s}_imperfectMath2Cluster.fa"))
    assert {names[i] for i in np.nonzero(l1["capped"])[0]} <= set(i_names)  # over -m in run 1: run 2 sees them
    l2 = loci_of_sam(fix("{s}_tmp2.sam", s), i_names, c_names)
    out("{s}_tmp2.sam").write_text(ua.cluster_sam_text(i_names, i_seqs, l2, c_names, c_lens,
                                                       "-f -n 1 -l 15 -5 1 -3 3 --best --strata -a --norc -S", 1, 3))
    ua.combine_sam(out("{s}_tmp1.sam"), out("{s}_tmp2.sam"), out("{s}.sam"))
    read_seqs = dict(zip(names, seqs))
    ua.decorate_sam(out("{s}.sam"), read_seqs, out("{s}_modified.sam"), dict(zip(c_names, c_seqs)))
    ua.decorate_sam(fix("unmapped_mirna_{s}_vs_genome_sorted.sam", s), read_seqs, out("{s}_RepSeq_modified.sam"))
    ua.parse_refine_sam(out("{s}_modified.sam"), out("{s}_selected.tsv"), out("{s}_selected_reverseKept.tsv"))
    ua.sort_tsv(out("{s}_selected.tsv"), out("{s}_modified_selected_sorted.tsv"))
    ua.sort_tsv(out("{s}_selected_reverseKept.tsv"), out("{s}_modified_selected_reverseKept_sorted.tsv"))
    for f in TEXT_OUT + SAM_OUT:
        assert same(out(f), f, s), f


def test_byte_order_sort_equals_the_fixture_on_shuffled_input(tmp_path, sample="S1"):
    rng = np.random.default_rng(8)
    want = open(fix("{s}_modified_selected_sorted.tsv", sample), "rb").read()
    lines = want.split(b"\n")[:-1]
    keys = [(ln.split(b"\t")[5], ln.split(b"\t")[0]) for ln in lines]
    assert any(a == b for a, b in zip(keys, keys[1:]))  # a pair only the whole line orders
    for _ in range(5):
        (tmp_path / "in.tsv").write_bytes(b"".join(lines[i] + b"\n" for i in rng.permutation(len(lines))))
        ua.sort_tsv(tmp_path / "in.tsv", tmp_path / "out.tsv")
        assert (tmp_path / "out.tsv").read_bytes() == want
        assert same(tmp_path / "out.tsv", "{s}_modified_selected_reverseKept_sorted.tsv", sample)  # every run is --norc: the same lines


def test_a_missing_repeat_table_means_no_repeats(tmp_path):
    assert ua.load_repeats(tmp_path / "human_genome_repeats.pckl") == {}
    with open(tmp_path / "human_genome_repeats.pckl", "wb") as fh:
        pickle.dump(repeat_table(), fh)
    table = ua.load_repeats(tmp_path / "human_genome_repeats.pckl")
    assert sorted(table) == ["chr1", "chr2", "chr3"] and len(table["chr3"][1]) == 1
    kept, _ = ua.pretrim_clusters({}, fix("{s}_clusters.tsv", "S1"), 30, tmp_path / "t.tsv", tmp_path / "t.fa")
    with_table, _ = ua.pretrim_clusters(table, fix("{s}_clusters.tsv", "S1"), 30, tmp_path / "t.tsv", tmp_path / "t.fa")
    assert len(kept) == len(with_table) + 5  # four clusters on elements of chr1 / chr2, one on chr3's only element


def test_switch_parsing_defaults_implication_and_refusals():
    from mirge3_amd.cli import parse_args
    base = ["-s", "a.fq", "-lib", "/x", "-on", "human"]
    off = parse_args(base + ["-clc", "25"])
    assert off.unmapped_align is False and off.unmapped_clusters is False
    only = parse_args(base + ["--unmapped-clusters"])
    assert only.unmapped_align is False and only.unmapped_clusters is True
    on = parse_args(base + ["--unmapped-align"])
    assert on.unmapped_align is True and on.unmapped_clusters is True
    assert ua.settings(on) == P
    on = parse_args(base + ["--unmapped-align", "-clc", "26", "-mloc", "5", "-sl", "20"])
    assert ua.settings(on) == dict(P, clc=26, mloc=5, sl=20)
    for bad in (["--unmapped-align", "--backend", "bowtie"], ["--unmapped-align", "-spl"], ["--unmapped-align", "-rr"],
                ["--unmapped-align", "-clc", "x"], ["--unmapped-align", "-olc", "x"], ["--unmapped-align", "-nmir"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
    parse_args(base + ["--unmapped-clusters", "-clc", "x"])  # -clc is read only with --unmapped-align, as before


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gctx():
    from mirge3_amd import _ffi
    ctx = _ffi.Context(0)
    yield ctx
    ctx.close()


CODE = np.full(256, 4, dtype=np.uint8)
for _k, _ch in enumerate("ACGT"):
    CODE[ord(_ch)] = _k
_RC = str.maketrans("ACGT", "TGCA")


def brute_strata(refs, queries, n_mm, seedlen, maxtotal, trim5, trim3, norc):
    """per query every valid alignment as (reference, offset, strand, total mismatches, seed mismatches): every window of every
    reference compared base by base, the policy of include/mirge_native.h restated"""
    width = max(len(r) for r in refs)
    text = np.full((len(refs), width), 5, dtype=np.uint8)  # 5: past the reference's end
    for k, r in enumerate(refs):
        text[k, :len(r)] = CODE[np.frombuffer(r.encode(), dtype=np.uint8)]
    out = []
    for q in queries:
        s = q[trim5:len(q) - trim3]
        L, recs = len(s), []
        if L >= 1 and L > n_mm:
            sl = min(seedlen, L)
            for strand in ((0,) if norc else (0, 1)):
                pat = CODE[np.frombuffer((s if strand == 0 else s.translate(_RC)[::-1]).encode(), dtype=np.uint8)]
                in_seed = (np.arange(L) < sl) if strand == 0 else (np.arange(L) >= L - sl)
                for o in range(width - L + 1):
                    w = text[:, o:o + L]
                    mis = w != pat[None, :]
                    tot, sd = mis.sum(axis=1), (mis & in_seed[None, :]).sum(axis=1)
                    ok = (w < 4).all(axis=1) & (tot <= maxtotal) & (sd <= n_mm)
                    recs += [(int(r), o, strand, int(tot[r]), int(sd[r])) for r in np.nonzero(ok)[0]]
        out.append(recs)
    return out


def strata_case(rng, n_refs=260, n_reads=420, ref_len=(20, 30), read_len=(16, 25), past=(17, 19)):
    """random references of ref_len nt, some of them copies or near copies of others (one base changed inside the first 15, or
    two past them, at ``past``), and reads of read_len nt cut from either end of them with 0 to 3 changes, on both strands"""
    def rand(n):
        return "".join("ACGT"[int(c)] for c in rng.integers(0, 4, n))

    def change(s, at):
        return s[:at] + "ACGT"[("ACGT".index(s[at]) + 1 + int(rng.integers(0, 3))) % 4] + s[at + 1:]
    refs, pairs = [], []
    while len(refs) < n_refs:
        r = rand(int(rng.integers(ref_len[0], ref_len[1] + 1)))
        refs.append(r)
        k = rng.random()
        if k < 0.08:
            refs.append(r)
        elif k < 0.15:  # three or four copies: over max_loci = 2 in the best stratum
            refs += [r] * int(rng.integers(2, 4))
        elif k < 0.22:  # one copy and two near copies: over max_loci in all, not in the best stratum
            refs += [change(r, int(rng.integers(2, 8))), change(r, int(rng.integers(8, 14)))]
        elif k < 0.35:
            refs.append(change(r, int(rng.integers(2, 14))))
        elif k < 0.55:
            refs.append(change(change(r, past[0]), past[1]))
        elif k < 0.65:
            refs.append(change(change(change(r, past[0]), past[1]), int(rng.integers(2, 14))))
            pairs.append((r, refs[-1]))
    reads = []
    for _ in range(n_reads):
        r = refs[int(rng.integers(0, len(refs)))]
        L = int(rng.integers(read_len[0], min(len(r), read_len[1]) + 1))
        s = r[:L] if rng.random() < 0.7 else r[len(r) - L:]
        for _ in range(int(rng.choice([0, 0, 1, 1, 2, 3]))):
            s = change(s, int(rng.integers(0, L)))
        if rng.random() < 0.1:
            s = rand(L)
        reads.append(s if rng.random() < 0.7 else s.translate(_RC)[::-1])
    for r, v in pairs:  # against r: two mismatches past the seed; against its variant: one, in the seed
        if len(r) >= past[1] + 4:
            s = r[:past[0]] + v[past[0]] + r[past[0] + 1:past[1]] + v[past[1]] + r[past[1] + 1:]
            reads.append(s[:int(rng.integers(max(past[1] + 4, read_len[0]), min(len(r), read_len[1]) + 1))])
    return refs, reads


@pytest.mark.gpu
def test_strata_call_equals_brute_force(gctx):
    """-n 1 -l 15 -5 1 -3 3 (the third run's policy) and -n 2 -l 12: only the best seed stratum is reported, -m counts it alone,
    totals count everything, and strata=0 is the existing call record for record"""
    from mirge3_amd import _ffi, a2i
    from mirge3_amd.seqio import FlatSeqs
    rng = np.random.default_rng(41)
    refs, reads = strata_case(rng)
    dev = _ffi.DeviceGenome(gctx, seqs=FlatSeqs.from_list(refs))
    g = a2i.GpuGenome(gctx, dev)
    flat = FlatSeqs.from_list(reads)
    seen = dict(best0=0, best1=0, dropped=0, two_best=0, total_in_worse=0, unaligned=0, capped=0, over_in_all_only=0)
    for n_mm, seedlen, trim5, trim3 in ((1, 15, 1, 3), (2, 12, 0, 2)):
        for norc in (True, False):
            every = brute_strata(refs, reads, n_mm, seedlen, 2, trim5, trim3, norc)
            lens = {len(q) - trim5 - trim3 for q, e in zip(reads, every) if e}
            assert n_mm != 1 or (min(lens), max(lens)) == (12, 21)
            for max_loci in (0, 2):
                got = g.loci(flat, n_mm=n_mm, seedlen=seedlen, maxtotal=2, trim5=trim5, trim3=trim3, max_loci=max_loci, norc=norc, strata=True)
                key = list(zip(got["ref"].tolist(), got["off"].tolist(), got["query"].tolist(), got["strand"].tolist()))
                assert key == sorted(key)
                mine = {}
                for q, r, o, st, mm in zip(got["query"].tolist(), got["ref"].tolist(), got["off"].tolist(), got["strand"].tolist(),
                                           got["mm"].tolist()):
                    mine.setdefault(q, []).append((r, o, st, mm))
                assert got["totals"].tolist() == [len(e) for e in every]
                for q, e in enumerate(every):
                    best = min((x[4] for x in e), default=None)
                    want = sorted(x[:4] for x in e if x[4] == best)
                    if max_loci and len(want) > max_loci:
                        want = []
                        seen["capped"] += 1
                    elif max_loci and len(e) > max_loci:
                        seen["over_in_all_only"] += 1  # -m counts the best stratum alone: reported
                    assert sorted(mine.get(q, [])) == want, (n_mm, norc, max_loci, q, reads[q])
                    if max_loci == 0 and n_mm == 1 and norc:
                        worse = [x for x in e if x[4] != best]
                        seen["best0"] += best == 0
                        seen["best1"] += best == 1
                        seen["dropped"] += bool(worse)
                        seen["two_best"] += len(want) >= 2
                        seen["total_in_worse"] += bool(worse) and min(x[3] for x in worse) < min(x[3] for x in want)
                        seen["unaligned"] += best is None
                plain = g.loci(flat, n_mm=n_mm, seedlen=seedlen, maxtotal=2, trim5=trim5, trim3=trim3, max_loci=max_loci, norc=norc)
                zero = g.loci(flat, n_mm=n_mm, seedlen=seedlen, maxtotal=2, trim5=trim5, trim3=trim3, max_loci=max_loci, norc=norc, strata=False)
                for k in ("query", "ref", "off", "strand", "mm", "totals"):
                    assert np.array_equal(plain[k], zero[k]), k
                if max_loci == 0:
                    assert sorted(zip(plain["query"].tolist(), plain["ref"].tolist(), plain["off"].tolist(), plain["strand"].tolist(),
                                      plain["mm"].tolist())) == sorted((q,) + x[:4] for q, e in enumerate(every) for x in e)
                    assert len(got["query"]) < len(plain["query"])
    dev.close()
    print(f"\n[strata] {len(refs)} references, {len(reads)} reads: {seen}")
    assert all(v >= 3 for v in seen.values()), seen


def _stage(tmp_path, clc=None):
    lib = tmp_path / "libs" / ORG / "annotation.Libs"
    lib.mkdir(parents=True)
    with open(lib / f"{ORG}_genome_repeats.pckl", "wb") as fh:
        pickle.dump(repeat_table(), fh)
    work = tmp_path / "out"
    (work / "unmapped_tmp").mkdir(parents=True)
    for s in SAMPLES:
        for f in INPUTS:
            shutil.copy(fix(f, s), work / "unmapped_tmp" / f.format(s=s))
    return SimpleNamespace(libraries_path=str(tmp_path / "libs"), organism_name=ORG, ignored_clc=clc), work


def _aligned(path):
    return sorted(ln for ln in open(path) if ln[0] != "@" and "\t4\t*\t" not in ln)


@pytest.mark.gpu
def test_device_route_writes_the_fixture_files(tmp_path, gctx):
    args, work = _stage(tmp_path)
    tm = {}
    res = ua.run(args, gctx, work, SAMPLES, tm)
    log = (work / "run.log").read_text()
    assert tm["unmapped_align_s"] > 0 and "unmapped align, S1" in log and "unmapped align:" in log
    for s in SAMPLES:
        for f in SAM_OUT[:2]:  # the aligned lines as sets, before the whole files in this project's line order
            assert _aligned(work / "unmapped_tmp" / f.format(s=s)) == _aligned(fix(f, s)), f
        for f in TEXT_OUT + SAM_OUT:
            assert same(work / "unmapped_tmp" / f.format(s=s), f, s), f
        assert (res[s]["capped"], res[s]["kept"], res[s]["aligned2"]) == (3, KEPT[s], ALIGNED2[s])


@pytest.mark.gpu
def test_a_sample_without_a_kept_cluster_ends_cleanly(tmp_path, gctx):
    args, work = _stage(tmp_path, clc="10")
    res = ua.run(args, gctx, work, SAMPLES, {})
    assert all(res[s]["kept"] == 0 for s in SAMPLES)
    log = (work / "run.log").read_text()
    for s in SAMPLES:
        assert f"No cluster sequences are generated and prediction is aborted for {s}." in log
        made = {p.name for p in (work / "unmapped_tmp").iterdir()} - {f.format(s=x) for f in INPUTS for x in SAMPLES}
        assert (work / "unmapped_tmp" / f"{s}_clusters_trimmed_orig.fa").read_text() == ""
        assert made == {f.format(s=x) for f in TEXT_OUT[:2] for x in SAMPLES}


@pytest.mark.gpu
@pytest.mark.parametrize("case_name", ["case4_gff_a2i", "case6_gff_a2i"])
def test_cli_switch_adds_its_files_and_moves_nothing_else(tmp_path, case_name):
    case = GoldenCase(case_name)
    from test_unmapped_clusters import _fastq_files
    files = _fastq_files(tmp_path, case)
    env = dict(os.environ, PYTHONPATH=ROOT)
    runs = {}
    for tag, extra in (("clusters", ["--unmapped-clusters", "-c", "1"]), ("align", ["--unmapped-align", "-c", "1"])):
        r = subprocess.run([sys.executable, "-m", "mirge3_amd.cli", "-s", ",".join(files), "-lib", case.libdir, "-on", ORG, "-db", "miRBase",
                            "-o", str(tmp_path / tag), "-ai", "--genome-filter", "gpu", "-gff", "-shh"] + extra, cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        (runs[tag],) = [d for d in (tmp_path / tag).iterdir() if d.is_dir()]
    before = sorted(p.name for p in runs["clusters"].iterdir())
    assert sorted(p.name for p in runs["align"].iterdir()) == before
    for f in before:
        if f not in ("run.log", "unmapped_tmp"):
            assert filecmp.cmp(runs["clusters"] / f, runs["align"] / f, shallow=False), f
    old = sorted(p.name for p in (runs["clusters"] / "unmapped_tmp").iterdir())
    for f in old:
        assert filecmp.cmp(runs["clusters"] / "unmapped_tmp" / f, runs["align"] / "unmapped_tmp" / f, shallow=False), f
    made = sorted(p.name for p in (runs["align"] / "unmapped_tmp").iterdir())
    log = (runs["align"] / "run.log").read_text()
    want = list(old)
    for s in case.samples:
        want += [f.format(s=s) for f in TEXT_OUT[:2]]
        if f"prediction is aborted for {s}." not in log:
            want += [f.format(s=s) for f in TEXT_OUT[2:] + SAM_OUT]
    assert made == sorted(want)
    assert "unmapped align:" in log and "unmapped align" not in (runs["clusters"] / "run.log").read_text()
    # case 4 keeps clusters and goes through both runs; case 6's clusters are all filtered out: the abort line, through the CLI
    through = [s for s in case.samples if f"unmapped align, {s}:" in log]
    assert bool(through) == (case_name == "case4_gff_a2i"), log
    # the files agree with each other: the host functions on the run's own SAMs give the run's tables
    for s in case.samples:
        d = runs["align"] / "unmapped_tmp"
        if not (d / f"{s}_tmp1.sam").exists():
            continue
        ua.combine_sam(d / f"{s}_tmp1.sam", d / f"{s}_tmp2.sam", tmp_path / "c.sam")
        assert filecmp.cmp(tmp_path / "c.sam", d / f"{s}.sam", shallow=False)
        ua.parse_refine_sam(d / f"{s}_modified.sam", tmp_path / "a.tsv", tmp_path / "b.tsv")
        ua.sort_tsv(tmp_path / "a.tsv", tmp_path / "a_sorted.tsv")
        assert filecmp.cmp(tmp_path / "a_sorted.tsv", d / f"{s}_modified_selected_sorted.tsv", shallow=False)
