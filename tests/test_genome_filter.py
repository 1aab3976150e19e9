"""The A-to-I report's genome filter on the device (``mirge_genome_align_counts``, ``a2i.GpuGenome``): the two whole-genome
bowtie runs of mirge2_tRF_a2i.py:1056-1096,1297-1316 under the policy of the bowtie stand-in (tests/golden/fake_bowtie,
``default_output``), checked against the stand-in itself, an independent numpy restatement and the golden A-to-I files."""
import contextlib
import importlib.machinery
import importlib.util
import io
import os
import shutil
import subprocess
import sys
import time
from types import SimpleNamespace

import numpy as np
import pytest

import mirge3_amd  # noqa: F401
from helpers import GOLDEN, GoldenCase, ORG

FAKE = os.path.join(GOLDEN, "fake_bowtie")
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CODE = np.full(256, 4, dtype=np.uint8)
for _k, _c in enumerate(b"ACGT"):
    CODE[_c] = _k
COMP = np.array([3, 2, 1, 0, 4], dtype=np.uint8)


def _stand_in():
    loader = importlib.machinery.SourceFileLoader("fake_bowtie_mod", os.path.join(FAKE, "bowtie"))
    spec = importlib.util.spec_from_loader("fake_bowtie_mod", loader)
    mod = importlib.util.module_from_spec(spec)
    loader.exec_module(mod)
    return mod


def stand_in_counts(refs, queries, n_mm):
    """[n, 3] from the stand-in's default-format lines (`-n N -f -a -3 2`, both strands), grouped by record name as the
    reference's dictionary groups them: a sequence given k times gets every line k times"""
    mod = _stand_in()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        mod.default_output([], dict(mode=0, mm=n_mm, seedlen=28, maxtotal=2, trim3=2), [f"r{i}" for i in range(len(refs))], refs,
                           list(queries), list(queries))
    per = {}
    for row in buf.getvalue().split("\n"):
        f = row.split("\t")
        if f != [""]:
            per.setdefault(f[0], [0, 0, 0])[f[-1].count(":")] += 1
    return np.array([per.get(q, [0, 0, 0]) for q in queries], dtype=np.int64)


def np_counts(refs, queries, n_mm, seedlen=28, maxtotal=2, trim3=2):
    """the same policy restated with numpy over every window of every reference (small genomes)"""
    out = np.zeros((len(queries), 3), dtype=np.int64)
    g = [CODE[np.frombuffer(r.encode(), dtype=np.uint8)] for r in refs]
    bad_cache = {}
    for qi, q in enumerate(queries):
        s = q[:len(q) - trim3]
        L = len(s)
        if L < 1 or L <= n_mm:
            continue
        qc = CODE[np.frombuffer(s.encode(), dtype=np.uint8)]
        seed = min(seedlen, L)
        for strand in (0, 1):
            pat = qc if strand == 0 else COMP[qc][::-1]
            smask = np.zeros(L, dtype=bool)
            if strand == 0:
                smask[:seed] = True
            else:
                smask[L - seed:] = True
            for ri, gc in enumerate(g):
                if gc.shape[0] < L:
                    continue
                W = np.lib.stride_tricks.sliding_window_view(gc, L)
                if (ri, L) not in bad_cache:
                    bad_cache[(ri, L)] = (W == 4).any(axis=1)
                mm = (W != pat) | (pat == 4)
                tot = mm.sum(axis=1)
                ok = ~bad_cache[(ri, L)] & (tot <= maxtotal) & (mm[:, smask].sum(axis=1) <= n_mm)
                out[qi] += np.bincount(tot[ok], minlength=3)[:3]
    return out


def _rc(s):
    return s.translate(str.maketrans("ACGTN", "TGCAN"))[::-1]


def random_genome(rng, sizes, n_runs=4):
    refs = []
    for n in sizes:
        r = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()
        for _ in range(n_runs):  # N runs, one of them at an end of the reference now and then
            a = int(rng.integers(0, n - 30)) if rng.random() < 0.7 else (0 if rng.random() < 0.5 else n - 12)
            r[a:a + int(rng.integers(1, 12))] = ord("N")
        refs.append(r.tobytes().decode())
    # repeat families: one segment copied across references, on both strands, a few copies with one change
    seg = refs[0][100:160].replace("N", "A")
    for k in range(1, len(refs)):
        r = list(refs[k])
        at = 200 + 37 * k
        ins = seg if k % 2 else _rc(seg)
        if k % 3 == 0:
            ins = ins[:20] + ("A" if ins[20] != "A" else "C") + ins[21:]
        if at + len(ins) > len(r):
            continue
        r[at:at + len(ins)] = ins
        refs[k] = "".join(r)
    return refs


def mutate(rng, s, k):
    s = list(s)
    for p in rng.choice(len(s), size=min(k, len(s)), replace=False):
        s[p] = "ACGT"[("ACGT".index(s[p]) + int(rng.integers(1, 4))) % 4] if s[p] in "ACGT" else "A"
    return "".join(s)


def query_set(rng, refs, n):
    """reads of 3..40 nt: windows of the genome (both strands, 0..3 changes inside and outside the seed), windows at reference
    ends and across two references, over N runs, reads holding N, palindromes, random reads, duplicates"""
    qs = []
    joined = "".join(refs)
    while len(qs) < n:
        kind = rng.integers(0, 9)
        L = int(rng.integers(3, 41)) if rng.random() < 0.3 else int(rng.integers(16, 33))
        r = refs[int(rng.integers(0, len(refs)))]
        if kind <= 2:
            a = int(rng.integers(0, len(r) - L))
            s = r[a:a + L].replace("N", "G")
            s = mutate(rng, s, int(rng.integers(0, 4)))
            qs.append(s if kind != 2 else _rc(s))
        elif kind == 3:  # reference edges, with the 2 trimmed bases behind
            qs.append((r[:L] if rng.random() < 0.5 else r[len(r) - L + 2:] + "AC").replace("N", "C"))
        elif kind == 4:  # across a reference boundary
            b = len(refs[0])
            qs.append(joined[b - L // 2:b - L // 2 + L].replace("N", "T"))
        elif kind == 5:  # holds an N
            a = int(rng.integers(0, len(r) - L))
            s = list(r[a:a + L].replace("N", "A"))
            s[int(rng.integers(0, L))] = "N"
            qs.append("".join(s))
        elif kind == 6:  # palindrome (+ 2 bases the trim removes)
            h = r[int(rng.integers(0, 1000)):][:max(2, L // 2)].replace("N", "A")
            qs.append(h + _rc(h) + "TT")
        elif kind == 7 and qs:
            qs.append(qs[int(rng.integers(0, len(qs)))])  # duplicate
        else:
            qs.append("".join("ACGT"[x] for x in rng.integers(0, 4, L)))
    return qs


def plant_palindromes(refs, qs):
    """put every palindromic query into the genome once, so that its '+' and '-' hits at one offset are both there"""
    r = list(refs[-1])
    at = 50
    for q in qs:
        s = q[:-2]
        if len(s) >= 4 and s == _rc(s) and at + len(s) < len(r) - 50:
            r[at:at + len(s)] = s
            at += len(s) + 31
    refs[-1] = "".join(r)
    return refs


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_numpy_restatement_equals_the_stand_in():
    """the test's own restatement (used at sizes the pure-Python stand-in cannot take) against the stand-in"""
    rng = np.random.default_rng(3)
    refs = random_genome(rng, [1500, 900, 1100])
    qs = query_set(rng, refs, 60)
    refs = plant_palindromes(refs, qs)
    mult = np.array([qs.count(q) for q in qs])[:, None]  # the stand-in's grouping by name: k copies, every line k times
    assert mult.max() > 1
    for n_mm in (0, 1):
        assert np.array_equal(np_counts(refs, qs, n_mm) * mult, stand_in_counts(refs, qs, n_mm)), n_mm


def test_genome_filter_flag_parsing_and_refusals():
    from mirge3_amd.cli import parse_args
    base = ["-s", "a.fq", "-lib", "/x", "-on", "human", "-ai"]
    assert parse_args(base).genome_filter == "auto"
    assert parse_args(base + ["--genome-filter", "gpu"]).genome_filter == "gpu"
    assert parse_args(base + ["--genome-filter", "bowtie", "-pbwt", "/opt/b"]).genome_filter == "bowtie"
    assert parse_args(base + ["--genome-filter", "bowtie", "--genome-retained", "r.txt"]).genome_retained == "r.txt"
    for bad in (["--genome-filter", "gpu", "--genome-retained", "r.txt"], ["--genome-filter", "cpu"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)


def test_genome_route_auto_rule(monkeypatch):
    from mirge3_amd import a2i
    ns = lambda **k: SimpleNamespace(**dict(dict(genome_filter="auto", bowtie_path=None, genome_retained=None), **k))
    monkeypatch.setattr(shutil, "which", lambda name: None)
    assert a2i.genome_route(ns()) == "gpu"  # no bowtie anywhere: what raised before
    assert a2i.genome_route(SimpleNamespace()) == "gpu"
    assert a2i.genome_route(ns(bowtie_path="/opt/bowtie")) == "bowtie"
    assert a2i.genome_route(ns(genome_retained="r.txt")) == "listed"
    assert a2i.genome_route(ns(genome_retained="r.txt", bowtie_path="/opt/bowtie")) == "listed"
    assert a2i.genome_route(ns(genome_filter="bowtie")) == "bowtie"
    assert a2i.genome_route(ns(genome_filter="gpu", bowtie_path="/opt/bowtie")) == "gpu"
    assert a2i.genome_route(ns(genome_predicate=object())) == "predicate"
    monkeypatch.setattr(shutil, "which", lambda name: "/usr/bin/bowtie" if name == "bowtie" else None)
    assert a2i.genome_route(ns()) == "bowtie"
    assert a2i.genome_route(ns(genome_filter="gpu")) == "gpu"


@pytest.mark.parametrize("large", [False, True])
def test_ebwt_records_are_the_upload_layout_of_the_text(tmp_path, large):
    """what the genome upload takes from .3/.4.ebwt[l] (records + packed bytes, undecoded) lays out ebwt.py's decoded text and
    the FASTA it was written from: bases at bits 2*(i & 3), stretches after `off` ambiguous characters, `first` per reference"""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from ebwt_writer import write_ebwt
    from mirge3_amd import ebwt
    rng = np.random.default_rng(11)
    refs = random_genome(rng, [700, 333, 1201, 64])
    refs[1] = "NNN" + refs[1][3:-4] + "NNNN"
    base = str(tmp_path / "g")
    write_ebwt(base, [f"c{i} x" for i in range(len(refs))], refs, large=large)
    packed, off, ln, first = ebwt.read_records(base)
    assert packed.dtype == np.uint8 and int(first.sum()) == len(refs)
    total = int(ln.sum())
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[(packed[np.arange(total) >> 2] >> (2 * (np.arange(total) & 3))) & 3]
    text, at, cur = [], 0, None
    for o, n, f in zip(off.tolist(), ln.tolist(), first.tolist()):
        if f:
            if cur is not None:
                text.append(cur)
            cur = ""
        cur += "N" * o + bases[at:at + n].tobytes().decode()
        at += n
    text.append(cur)
    decoded, _ = ebwt.read_sequences(base)
    assert text == decoded.to_list()
    assert [t.ljust(len(r), "N") for t, r in zip(text, refs)] == refs


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gctx():
    from mirge3_amd import _ffi
    ctx = _ffi.Context(0)
    yield ctx
    ctx.close()


def _flat(qs):
    from mirge3_amd.seqio import FlatSeqs
    return FlatSeqs.from_list(qs)


def _genome(ctx, refs):
    from mirge3_amd import _ffi
    return _ffi.DeviceGenome(ctx, seqs=_flat(refs))


def _lib_dir(tmp_path, refs):
    d = tmp_path / "libs" / ORG / "index.Libs"
    d.mkdir(parents=True)
    with open(d / f"{ORG}_genome.fa", "w") as fh:
        fh.write("".join(f">chr{i} test\n{r}\n" for i, r in enumerate(refs)))
    return str(tmp_path / "libs")


@pytest.mark.gpu
def test_counts_equal_the_stand_in(tmp_path, gctx):
    """(0, 1, 2)-mismatch counts of every query under -n 0 and -n 1 equal the stand-in's lines; unique_best / aligned equal
    BowtieGenome(stand-in)'s (small genome: the stand-in is pure Python)"""
    from mirge3_amd import a2i
    rng = np.random.default_rng(7)
    refs = random_genome(rng, [2500, 1200, 1800, 700])
    qs = query_set(rng, refs, 70)
    refs = plant_palindromes(refs, qs)
    genome = _genome(gctx, refs)
    for n_mm in (0, 1):
        got = genome.align_counts(_flat(qs), n_mm).astype(np.int64)
        exp = stand_in_counts(refs, qs, n_mm)
        # the stand-in groups duplicates under one name: k copies -> k times every line; the device answers per record
        mult = {q: qs.count(q) for q in qs}
        per_record = exp // np.array([mult[q] for q in qs])[:, None]
        assert np.array_equal(got, per_record), [(q, g.tolist(), e.tolist()) for q, g, e in zip(qs, got, per_record) if (g != e).any()][:5]
    lib = _lib_dir(tmp_path, refs)
    args = SimpleNamespace(libraries_path=lib, organism_name=ORG, bowtie_path=FAKE, threads=1)
    bt = a2i.BowtieGenome(args, str(tmp_path))
    gg = a2i.GpuGenome(gctx, genome)
    assert gg.unique_best(qs) == bt.unique_best(qs)
    assert gg.aligned(qs) == bt.aligned(qs)


@pytest.mark.gpu
def test_counts_equal_the_numpy_restatement(gctx):
    """a few hundred kb over several references: every query, -n 0 and -n 1"""
    rng = np.random.default_rng(21)
    refs = random_genome(rng, [90000, 60000, 75000, 40000, 35000], n_runs=12)
    qs = query_set(rng, refs, 90)
    refs = plant_palindromes(refs, qs)
    genome = _genome(gctx, refs)
    for n_mm in (0, 1):
        got = genome.align_counts(_flat(qs), n_mm).astype(np.int64)
        exp = np_counts(refs, qs, n_mm)
        assert np.array_equal(got, exp), [(q, g.tolist(), e.tolist()) for q, g, e in zip(qs, got, exp) if (g != e).any()][:5]


@pytest.mark.gpu
def test_ebwt_and_ebwtl_give_the_fasta_counts(tmp_path, gctx):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from ebwt_writer import write_ebwt
    from mirge3_amd import a2i
    rng = np.random.default_rng(5)
    refs = random_genome(rng, [30000, 20000, 12000], n_runs=8)
    refs[1] = "NNNNN" + refs[1][5:-3] + "NNN"
    qs = query_set(rng, refs, 80)
    lib = _lib_dir(tmp_path, refs)
    fa = a2i.load_genome(gctx, os.path.join(lib, ORG, "index.Libs", f"{ORG}_genome"))
    want = {n: fa.align_counts(_flat(qs), n) for n in (0, 1)}
    assert want[1].any()
    for large in (False, True):
        d = tmp_path / ("l" if large else "s")
        d.mkdir()
        write_ebwt(str(d / "g"), [f"chr{i}" for i in range(len(refs))], refs, large=large)
        tm = {}
        g = a2i.load_genome(gctx, str(d / "g"), tm)
        assert tm["genome_load_s"] > 0 and a2i.load_genome(gctx, str(d / "g")) is g  # loaded once, kept
        for n in (0, 1):
            assert np.array_equal(g.align_counts(_flat(qs), n), want[n]), (large, n)


@pytest.mark.gpu
def test_a_query_planted_200000_times(gctx):
    """one query 200 000 times in the genome, half on each strand: exact counts (the wave-level merge of the hits), and the
    scan's kernel time"""
    rng = np.random.default_rng(9)
    q = "TGAGGTAGTAGGTTGTATAGTT"
    body = q[:-2]
    n_copies, spacer = 200000, 18
    gap = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n_copies, spacer))]
    ins = np.array([list((body if k % 2 == 0 else _rc(body)).encode()) for k in range(2)], dtype=np.uint8)
    rows = np.concatenate([ins[np.arange(n_copies) % 2], gap], axis=1)
    text = rows.tobytes().decode()
    refs = [text[:len(text) // 2], text[len(text) // 2:]]
    genome = _genome(gctx, refs)
    gctx.profile(True)
    gctx.profile_reset()
    got = genome.align_counts(_flat([q]), 1).astype(np.int64)
    recs = {name: ms for name, _, ms, _ in gctx.profile_records()}
    gctx.profile(False)
    exp = np.zeros_like(got)
    for r in refs:  # one query at a time against 8.0 Mb: the windows of the restatement
        exp += np_counts([r], [q], 1)
    assert exp[0, 0] == n_copies
    assert np.array_equal(got, exp), (got, exp)
    print(f"\n[genome filter] {len(text)} bases, query x {n_copies}: k_genome_scan {recs.get('k_genome_scan', float('nan')):.3f} ms")


_KMERS = {}


def _kmer_restatement(gcodes, starts, qs, n_mm, k=12, seedlen=28, maxtotal=2, trim3=2):
    """independent of the kernel's index: a sorted array of the genome's k-mers, pigeonhole pieces of every query's seed looked
    up in it by their first k bases (every piece must be >= k long), every candidate window verified in full, duplicates of
    (query, strand, window) dropped"""
    G = gcodes.shape[0]
    if (id(gcodes), k) not in _KMERS:
        km = np.zeros(G - k + 1, dtype=np.int64)
        badk = np.zeros(G - k + 1, dtype=bool)
        for j in range(k):
            c = gcodes[j:G - k + 1 + j]
            km = km * 4 + np.minimum(c, 3)
            badk |= c == 4
        pos = np.nonzero(~badk)[0]
        order = np.argsort(km[pos], kind="stable")
        _KMERS[(id(gcodes), k)] = (km[pos][order], pos[order])
    skm, spos = _KMERS[(id(gcodes), k)]
    P = n_mm + 1
    lens = np.array([len(q) - trim3 for q in qs], dtype=np.int64)
    Lmax = int(lens.max())
    pats = np.full((2 * len(qs), Lmax), 4, dtype=np.uint8)
    keys, los, owners = [], [], []
    for qi, q in enumerate(qs):
        L = int(lens[qi])
        qc = CODE[np.frombuffer(q[:L].encode(), dtype=np.uint8)]
        sl = min(seedlen, L)
        for strand in (0, 1):
            pat = qc if strand == 0 else COMP[qc][::-1]
            pats[2 * qi + strand, :L] = pat
            s0 = 0 if strand == 0 else L - sl
            for j in range(P):
                lo, hi = s0 + (j * sl) // P, s0 + ((j + 1) * sl) // P
                assert hi - lo >= k
                if (pat[lo:lo + k] == 4).any():
                    continue
                key = 0
                for c in pat[lo:lo + k].tolist():
                    key = key * 4 + c
                keys.append(key); los.append(lo); owners.append(2 * qi + strand)
    keys, los, owners = (np.array(x, dtype=np.int64) for x in (keys, los, owners))
    a, b = np.searchsorted(skm, keys, "left"), np.searchsorted(skm, keys, "right")
    n = b - a
    idx = np.repeat(np.arange(keys.shape[0]), n)
    within = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    ws = spos[a[idx] + within] - los[idx]
    qsi = owners[idx]
    comb = np.unique(qsi * (G + 64) + (ws + 32))
    qsi, ws = comb // (G + 64), comb % (G + 64) - 32
    out = np.zeros((len(qs), 3), dtype=np.int64)
    for L in np.unique(lens).tolist():
        sel = (lens[qsi >> 1] == L) & (ws >= 0) & (ws + L <= G)
        sq, sw = qsi[sel], ws[sel]
        same_ref = np.searchsorted(starts, sw, "right") == np.searchsorted(starts, sw + L - 1, "right")
        W = gcodes[sw[:, None] + np.arange(L)]
        pat = pats[sq, :L]
        mm = (W != pat) | (pat == 4)
        sl = min(seedlen, L)
        sd = np.where((sq & 1) == 0, mm[:, :sl].sum(axis=1), mm[:, L - sl:].sum(axis=1))
        tot = mm.sum(axis=1)
        ok = same_ref & ~(W == 4).any(axis=1) & (tot <= maxtotal) & (sd <= n_mm)
        np.add.at(out, (sq[ok] >> 1, tot[ok]), 1)
    return out


@pytest.mark.gpu
def test_scale_32mb_20000_queries(gctx):
    """32 Mb over eight references with N runs and a planted repeat family, 2 x 10^4 queries of 26..31 nt drawn from it with
    0..3 changes (pieces of at least 12 nt for the k = 12 restatement), -n 1 and -n 0"""
    rng = np.random.default_rng(2024)
    sizes = [4_000_000] * 8
    g = rng.integers(0, 4, sum(sizes)).astype(np.uint8)
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    for a in rng.integers(0, g.shape[0] - 500, 400):
        g[a:a + int(rng.integers(1, 300))] = 4
    fam = rng.integers(0, 4, 300).astype(np.uint8)
    for a in rng.integers(0, g.shape[0] - 300, 3000):  # a repeat family: 3000 copies of one 300-mer with ~1 % divergence
        c = fam.copy()
        c[rng.integers(0, 300, 3)] = rng.integers(0, 4, 3)
        g[a:a + 300] = c
    text = np.frombuffer(b"ACGTN", dtype=np.uint8)[g].tobytes().decode()
    refs = [text[a:a + n] for a, n in zip(starts, sizes)]
    n_q = 20000
    qs = []
    for _ in range(n_q):
        L = int(rng.integers(26, 32))
        a = int(rng.integers(0, g.shape[0] - L))
        s = text[a:a + L].replace("N", "A")
        if rng.random() < 0.02:
            s = "".join("ACGT"[x] for x in fam[:L]) if rng.random() < 0.5 else s
        s = mutate(rng, s, int(rng.integers(0, 4)))
        qs.append(s if rng.random() < 0.5 else _rc(s))
    genome = _genome(gctx, refs)
    for n_mm in (1, 0):
        t = time.perf_counter()
        got = genome.align_counts(_flat(qs), n_mm).astype(np.int64)
        t_gpu = time.perf_counter() - t
        t = time.perf_counter()
        exp = _kmer_restatement(g, starts, qs, n_mm)
        print(f"\n[genome filter] 32 Mb, {n_q} queries, -n {n_mm}: device call {t_gpu:.3f} s, restatement {time.perf_counter() - t:.1f} s")
        assert exp.sum() > n_q // 2
        assert np.array_equal(got, exp), int((got != exp).any(axis=1).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("case_name", ["case4_gff_a2i", "case6_gff_a2i"])
def test_golden_a2i_files_through_the_device_filter(tmp_path, case_name):
    """-ai with --genome-filter gpu and no bowtie: the three A-to-I files byte for byte the committed fixtures (made with the
    stand-in's genome runs against <ORG>_genome.fa)"""
    from mirge3_amd import fastpath
    case = GoldenCase(case_name)
    files = []
    for s, nm in enumerate(case.samples):
        p = tmp_path / f"{nm}.fastq"
        with open(p, "w") as fh:
            for seq, row in zip(case.seqs, case.counts):
                if row[s]:
                    fh.write(f"@r\n{seq}\n+\n{'I' * len(seq)}\n" * int(row[s]))
        files.append(str(p))
    work = tmp_path / "out"
    work.mkdir()
    args = SimpleNamespace(libraries_path=case.libdir, organism_name=ORG, spikeIn=False, quiet=True, minimum_length=16,
                           crThreshold="0.1", device=0, isoform_entropy=False, threads=1, bowtieVersion="True", phred64=False,
                           bowtie_path=None, genome_filter="gpu", AtoI=True)
    tm = {}
    fastpath.run(args, files, case.samples, str(work), "miRBase", timings=tm)
    for f in ("a2IEditing.report.csv", "a2IEditing.report.newform.csv", "a2IEditing.detail.txt"):
        assert (work / f).read_text() == case.text(f), f
    assert "genome_filter_s" in tm and "genome_load_s" in tm
    assert "A-to-I genome filter: gpu" in (work / "run.log").read_text()


@pytest.mark.gpu
def test_cli_ai_without_bowtie_on_path(tmp_path):
    """`python -m mirge3_amd.cli ... -ai` on a copy of golden case 4's directory with no bowtie anywhere: auto takes the device"""
    case = GoldenCase("case4_gff_a2i")
    lib = tmp_path / "libs"
    shutil.copytree(case.libdir, lib)
    files = []
    for k, nm in enumerate(case.samples):
        p = tmp_path / f"{nm}.fastq"
        with open(p, "w") as fh:
            for seq, row in zip(case.seqs, case.counts):
                fh.write(f"@r\n{seq}\n+\n{'I' * len(seq)}\n" * int(row[k]))
        files.append(str(p))
    path = os.pathsep.join(d for d in os.environ.get("PATH", "").split(os.pathsep) if not os.path.exists(os.path.join(d, "bowtie")))
    assert shutil.which("bowtie", path=path) is None
    env = dict(os.environ, PATH=path, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "mirge3_amd.cli", "-s", ",".join(files), "-lib", str(lib),
                        "-on", ORG, "-db", "miRBase", "-o", str(tmp_path / "out"), "-ai", "-shh"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    (run,) = [d for d in (tmp_path / "out").iterdir() if d.is_dir()]
    for f in ("a2IEditing.report.csv", "a2IEditing.report.newform.csv", "a2IEditing.detail.txt"):
        assert (run / f).read_text() == case.text(f), f
    assert "A-to-I genome filter: gpu" in (run / "run.log").read_text()
