"""Genome alignments with positions (``mirge_genome_align_loci``, ``a2i.GpuGenome.loci``): every record against a brute-force
restatement in this file, against the ``-a`` lines of the bowtie stand-in (tests/golden/fake_bowtie, a child process) and
against ``mirge_genome_align_counts``; the ``-m`` cap, bowtie's own index files, and the sizes of test_genome_filter.py."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import mirge3_amd  # noqa: F401
import test_genome_filter as gf

CODE, COMP = gf.CODE, gf.COMP


def brute_loci(ref_codes, queries, n_mm, seedlen=28, maxtotal=2, trim5=0, trim3=0, norc=False, only=None):
    """{(query, reference, offset, strand, mismatches)} of every valid alignment: each window of each reference compared base
    by base (one vector operation per base of the query), the policy of include/mirge_native.h restated"""
    recs = set()
    n_before = [np.concatenate(([0], np.cumsum(g == 4))) for g in ref_codes]  # ambiguous bases in front of each position
    for qi in (range(len(queries)) if only is None else only):
        s = queries[qi][trim5:len(queries[qi]) - trim3]
        L = len(s)
        if L < 1 or L <= n_mm:
            continue
        qc = CODE[np.frombuffer(s.encode(), dtype=np.uint8)]
        sl = min(seedlen, L)
        for strand in ((0,) if norc else (0, 1)):
            pat = qc if strand == 0 else COMP[qc][::-1]
            in_seed = (np.arange(L) < sl) if strand == 0 else (np.arange(L) >= L - sl)
            for ri, g in enumerate(ref_codes):
                n = g.shape[0] - L + 1
                if n <= 0:
                    continue
                tot = np.zeros(n, dtype=np.int16)
                sd = np.zeros(n, dtype=np.int16)
                bad = (n_before[ri][L:] - n_before[ri][:n]) > 0
                for j in range(L):
                    col = g[j:j + n]
                    m = (col != pat[j]) if pat[j] != 4 else np.ones(n, dtype=bool)
                    tot += m
                    if in_seed[j]:
                        sd += m
                ok = ~bad & (tot <= maxtotal) & (sd <= n_mm)
                for o in np.nonzero(ok)[0].tolist():
                    recs.add((qi, ri, o, strand, int(tot[o])))
    return recs


def codes(refs):
    return [CODE[np.frombuffer(r.encode(), dtype=np.uint8)] for r in refs]


def record_set(loci):
    out = list(zip(loci["query"].tolist(), loci["ref"].tolist(), loci["off"].tolist(), loci["strand"].tolist(), loci["mm"].tolist()))
    assert len(set(out)) == len(out), "a record is reported twice"
    return set(out)


def assert_sorted(loci):
    key = list(zip(loci["ref"].tolist(), loci["off"].tolist(), loci["query"].tolist(), loci["strand"].tolist()))
    assert key == sorted(key)


def stand_in_records(tmp_path, refs, queries, n_mm, trim3):
    """the stand-in as a child process: `bowtie <index> -n N -f -a -3 T q.fa`, its default-format lines as records"""
    base = str(tmp_path / f"g{n_mm}")
    with open(base + ".fa", "w") as fh:
        fh.write("".join(f">r{i} x\n{r}\n" for i, r in enumerate(refs)))
    with open(base + ".q.fa", "w") as fh:
        fh.write("".join(f">q{i}\n{q}\n" for i, q in enumerate(queries)))
    r = subprocess.run([sys.executable, os.path.join(gf.FAKE, "bowtie"), base, "-n", str(n_mm), "-f", "-a", "-3", str(trim3),
                        base + ".q.fa"], capture_output=True, text=True, timeout=900, check=True)
    recs = set()
    for line in r.stdout.split("\n"):
        f = line.split("\t")
        if f != [""]:
            recs.add((int(f[0][1:]), int(f[2][1:]), int(f[3]), 0 if f[1] == "+" else 1, f[7].count(":")))
    return recs


def check_against_counts(genome, flat, loci, n_mm, seedlen, maxtotal, trim5, trim3, capped=None):
    """(c): per uncapped query, its records per mismatch stratum are what mirge_genome_align_counts counts; totals likewise"""
    counts = genome.align_counts(flat, n_mm, seedlen, maxtotal, trim5, trim3).astype(np.int64)
    n = counts.shape[0]
    assert np.array_equal(loci["totals"].astype(np.int64), counts.sum(axis=1))
    per = np.zeros((n, 3), dtype=np.int64)
    np.add.at(per, (loci["query"].astype(np.int64), loci["mm"].astype(np.int64)), 1)
    keep = np.ones(n, dtype=bool) if capped is None else ~capped
    assert np.array_equal(per[keep], counts[keep])
    assert not per[~keep].any()
    return counts


@pytest.fixture(scope="module")
def gctx():
    from mirge3_amd import _ffi
    ctx = _ffi.Context(0)
    yield ctx
    ctx.close()


def small_case(seed, sizes, n_q):
    rng = np.random.default_rng(seed)
    refs = gf.random_genome(rng, sizes)
    qs = gf.query_set(rng, refs, n_q)
    refs = gf.plant_palindromes(refs, qs)
    return refs, qs


@pytest.mark.gpu
@pytest.mark.parametrize("n_mm", [0, 1, 2])
def test_loci_equal_brute_force_stand_in_and_counts(tmp_path, gctx, n_mm):
    """N runs, four references, repeats across references on both strands, palindromes, reads with N; -3 2"""
    from mirge3_amd import a2i
    refs, qs = small_case(31, [1500, 900, 1100, 600], 60)
    genome = gf._genome(gctx, refs)
    loci = a2i.GpuGenome(gctx, genome).loci(qs, n_mm=n_mm, trim3=2)
    got = record_set(loci)
    assert_sorted(loci)
    assert len(got) > 40 and {r[3] for r in got} == {0, 1}
    assert got == brute_loci(codes(refs), qs, n_mm, trim3=2)                       # (a), every query
    assert got == stand_in_records(tmp_path, refs, qs, n_mm, 2)                     # (b), every query
    check_against_counts(genome, gf._flat(qs), loci, n_mm, 28, 2, 0, 2)             # (c), every query


@pytest.mark.gpu
def test_loci_seed_rule_trims_forward_only_and_batches(gctx):
    """a seed shorter than the read (mismatches past it), -5, --norc, and the same call split over many batches of queries"""
    refs, qs = small_case(32, [4000, 2500, 1500], 120)
    genome = gf._genome(gctx, refs)
    flat = gf._flat(qs)
    seen_mm = set()
    for n_mm, seedlen, maxtotal, trim5, trim3, norc in ((0, 10, 2, 0, 0, False), (1, 12, 2, 1, 2, False), (0, 25, 2, 0, 0, True),
                                                         (2, 28, 2, 0, 2, True), (0, 8, 1, 0, 0, False)):
        loci = genome.align_loci(flat, n_mm, seedlen, maxtotal, trim5, trim3, 0, norc)
        got = record_set(loci)
        assert_sorted(loci)
        assert got == brute_loci(codes(refs), qs, n_mm, seedlen, maxtotal, trim5, trim3, norc)
        if not norc:
            check_against_counts(genome, flat, loci, n_mm, seedlen, maxtotal, trim5, trim3)
        else:
            assert not loci["strand"].any()
        seen_mm |= {(n_mm, r[4]) for r in got}
    assert (0, 1) in seen_mm and (0, 2) in seen_mm  # -n 0 alignments that carry mismatches past the seed
    whole = genome.align_loci(flat, 1, 28, 2, 0, 2, 2)
    os.environ["MIRGE_LOCI_BATCH"] = "7"
    try:
        split = genome.align_loci(flat, 1, 28, 2, 0, 2, 2)
    finally:
        del os.environ["MIRGE_LOCI_BATCH"]
    for k in ("query", "ref", "off", "strand", "mm", "totals"):
        assert np.array_equal(whole[k], split[k]), k


@pytest.mark.gpu
def test_max_loci_reports_all_or_none(gctx):
    """-m: a query planted max_loci times reports them all; planted max_loci + 1 times it reports none and its total says why"""
    rng = np.random.default_rng(33)
    max_loci = 3
    g = ["".join("ACGT"[x] for x in rng.integers(0, 4, 3000)) for _ in range(2)]
    a, b = "TGAGGTAGTAGGTTGTATAGTT", "ACCGTTAGGCATCGATTGCAAGGT"
    r0, r1 = list(g[0]), list(g[1])
    for k, at in enumerate((100, 900, 1700)):         # a: three times, one of them on the minus strand
        (r0 if k < 2 else r1)[at:at + len(a)] = a if k != 1 else gf._rc(a)
    for k, at in enumerate((300, 1200, 2100, 2600)):  # b: four times
        (r0 if k % 2 else r1)[at:at + len(b)] = b if k != 2 else gf._rc(b)
    refs = ["".join(r0), "".join(r1)]
    qs = [a, b, "ACGTACGTTTGACCAGTACAGT"]
    genome = gf._genome(gctx, refs)
    loci = genome.align_loci(gf._flat(qs), 0, 25, 2, 0, 0, max_loci)
    assert loci["totals"].tolist() == [3, 4, 0]
    assert sorted(loci["query"].tolist()) == [0, 0, 0]
    assert record_set(loci) == {r for r in brute_loci(codes(refs), qs, 0, 25) if r[0] == 0}
    free = genome.align_loci(gf._flat(qs), 0, 25, 2, 0, 0, 0)
    assert record_set(free) == brute_loci(codes(refs), qs, 0, 25) and np.bincount(free["query"], minlength=3).tolist() == [3, 4, 0]
    check_against_counts(genome, gf._flat(qs), loci, 0, 25, 2, 0, 0, capped=loci["totals"] > max_loci)


@pytest.mark.gpu
def test_ebwt_and_ebwtl_give_the_fasta_records(tmp_path, gctx):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from ebwt_writer import write_ebwt
    from mirge3_amd import a2i
    rng = np.random.default_rng(5)
    refs = gf.random_genome(rng, [30000, 20000, 12000], n_runs=8)
    refs[1] = "NNNNN" + refs[1][5:-3] + "NNN"
    qs = gf.query_set(rng, refs, 80)
    lib = gf._lib_dir(tmp_path, refs)
    fa = a2i.load_genome(gctx, os.path.join(lib, gf.ORG, "index.Libs", f"{gf.ORG}_genome"))
    assert fa.ref_names == [f"chr{i}" for i in range(len(refs))]
    want = {n: fa.align_loci(gf._flat(qs), n, 28, 2, 0, 2) for n in (0, 1)}
    assert len(want[1]["query"]) > 30 and record_set(want[1]) == brute_loci(codes(refs), qs, 1, trim3=2)
    for large in (False, True):
        d = tmp_path / ("l" if large else "s")
        d.mkdir()
        write_ebwt(str(d / "g"), [f"chr{i} x" for i in range(len(refs))], refs, large=large)
        g = a2i.load_genome(gctx, str(d / "g"))
        assert g.ref_names == fa.ref_names
        for n in (0, 1):
            got = g.align_loci(gf._flat(qs), n, 28, 2, 0, 2)
            for k in ("query", "ref", "off", "strand", "mm", "totals"):
                assert np.array_equal(got[k], want[n][k]), (large, n, k)


@pytest.mark.gpu
def test_a_query_planted_200000_times(gctx):
    """200 000 copies, half on each strand: every record, and the fill pass's kernel time beside the count pass's"""
    rng = np.random.default_rng(9)
    q = "TGAGGTAGTAGGTTGTATAGTT"
    body = q[:-2]
    n_copies, spacer = 200000, 18
    gap = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n_copies, spacer))]
    ins = np.array([list((body if k % 2 == 0 else gf._rc(body)).encode()) for k in range(2)], dtype=np.uint8)
    rows = np.concatenate([ins[np.arange(n_copies) % 2], gap], axis=1)
    text = rows.tobytes().decode()
    refs = [text[:len(text) // 2], text[len(text) // 2:]]
    genome = gf._genome(gctx, refs)
    gctx.profile(True)
    gctx.profile_reset()
    loci = genome.align_loci(gf._flat([q]), 1, 28, 2, 0, 2)
    recs = {name: ms for name, _, ms, _ in gctx.profile_records()}
    gctx.profile(False)
    print(f"\n[genome loci] {len(text)} bases, query x {n_copies}: count pass {recs.get('k_genome_scan', float('nan')):.3f} ms, "
          f"fill pass {recs.get('k_genome_scan_fill', float('nan')):.3f} ms")
    assert_sorted(loci)
    got = record_set(loci)
    assert sum(1 for r in got if r[4] == 0) == n_copies
    assert got == brute_loci(codes(refs), [q], 1, trim3=2)                          # (a) in full: one query
    check_against_counts(genome, gf._flat([q]), loci, 1, 28, 2, 0, 2)               # (c)


@pytest.mark.gpu
def test_scale_32mb_20000_queries(gctx):
    """the 32 Mb genome and 2 x 10^4 queries of test_genome_filter.py: (c) for every query, (a) for a seeded sample of them"""
    rng = np.random.default_rng(2024)
    sizes = [4_000_000] * 8
    g = rng.integers(0, 4, sum(sizes)).astype(np.uint8)
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    for a in rng.integers(0, g.shape[0] - 500, 400):
        g[a:a + int(rng.integers(1, 300))] = 4
    fam = rng.integers(0, 4, 300).astype(np.uint8)
    for a in rng.integers(0, g.shape[0] - 300, 3000):
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
        s = gf.mutate(rng, s, int(rng.integers(0, 4)))
        qs.append(s if rng.random() < 0.5 else gf._rc(s))
    genome = gf._genome(gctx, refs)
    flat = gf._flat(qs)
    ref_codes = [g[a:a + n] for a, n in zip(starts, sizes)]
    pick = np.random.default_rng(77)
    for n_mm in (1, 0):
        t = time.perf_counter()
        loci = genome.align_loci(flat, n_mm, 28, 2, 0, 2)
        t_loci = time.perf_counter() - t
        t = time.perf_counter()
        counts = check_against_counts(genome, flat, loci, n_mm, 28, 2, 0, 2)
        t_counts = time.perf_counter() - t
        assert_sorted(loci)
        got = record_set(loci)
        assert len(got) > n_q // 2
        # the sample: queries with many alignments (the repeat family), with one, with none
        many, some, none = (np.nonzero(m)[0] for m in (counts.sum(axis=1) > 100, (counts.sum(axis=1) > 0) & (counts.sum(axis=1) <= 100),
                                                        counts.sum(axis=1) == 0))
        sample = np.concatenate([pick.choice(many, min(2, many.size), replace=False), pick.choice(some, 5, replace=False),
                                 pick.choice(none, 1, replace=False)]).tolist()
        t = time.perf_counter()
        exp = brute_loci(ref_codes, qs, n_mm, trim3=2, only=sample)
        print(f"\n[genome loci] 32 Mb, {n_q} queries, -n {n_mm}: {len(got)} records, loci call {t_loci:.3f} s, counts call + checks "
              f"{t_counts:.3f} s, brute force of {len(sample)} queries {time.perf_counter() - t:.1f} s")
        in_sample = set(sample)
        assert {r for r in got if r[0] in in_sample} == exp
