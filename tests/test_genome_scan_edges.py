"""The genome scan (``k_genome_queries`` / ``k_genome_index`` / ``k_genome_scan``, csrc/kernels_genome.hpp) where the other genome
tests do not reach: queries held in two words (39 to 64 nt, seeds past 32), more hits in one 32-position strip than a lane
stashes, key tables of 12 and 13 bases, streams that end inside the first words, and a seed shorter than its pieces.  Every
comparison is exact and against the brute forces of test_genome_loci.py / test_unmapped_align.py; every test asserts from its
inputs (or from the brute force's answer, never from the device's) that it reaches the branch it exists for."""
import os
import time

import numpy as np
import pytest

import mirge3_amd  # noqa: F401
import test_genome_filter as gf
from test_genome_filter import _flat, _genome, _rc, mutate
from test_genome_loci import assert_sorted, brute_loci, check_against_counts, codes, record_set
from test_unmapped_align import brute_strata, strata_case

MAXLEN, STASH, STRIP = 64, 4, 32  # MIRGE_GENOME_MAXLEN, MIRGE_GENOME_STASH, MIRGE_GENOME_STRIP
KEYS = ("query", "ref", "off", "strand", "mm", "totals")


@pytest.fixture(scope="module")
def gctx():
    from mirge3_amd import _ffi
    ctx = _ffi.Context(0)
    yield ctx
    ctx.close()


def rand_seq(rng, n):
    return "".join("ACGT"[int(c)] for c in rng.integers(0, 4, n))


def change(rng, s, at):
    return s[:at] + "ACGT"[("ACGT".index(s[at]) + int(rng.integers(1, 4))) % 4] + s[at + 1:]


def table_k(n_queries, n_mm):
    """genome_tables_build's rule restated: the least k >= 8 with 4^k >= 32 x keys, at most 13; keys = 2 strands x (n_mm + 1)
    pieces per query"""
    keys = 2 * n_queries * (n_mm + 1)
    k = 8
    while k < 13 and 4 ** k < 32 * keys:
        k += 1
    return k


def seed_cut(L, strand, n_mm, seedlen):
    """k_genome_queries' cut restated, on the forward text ('-': the seed is the END of the reverse complement):
    the seed's [s0, s1) and its pieces [(lo, plen)] with lo = s0 + j * sl / P"""
    P, sl = n_mm + 1, min(seedlen, L)
    s0 = 0 if strand == 0 else L - sl
    cut = [s0 + j * sl // P for j in range(P + 1)]
    return (s0, s0 + sl), [(cut[j], cut[j + 1] - cut[j]) for j in range(P)]


def per_query(recs, n):
    out = np.zeros(n, dtype=np.int64)
    for r in recs:
        out[r[0]] += 1
    return out


# ------------------------------------------------------------------------------------------------- A1: two-word queries
POLICIES = [(0, 28, 2, 0, 0), (1, 28, 2, 0, 2), (2, 28, 2, 0, 2), (1, 40, 2, 1, 0), (0, 64, 2, 0, 0), (2, 64, 2, 0, 0), (1, 15, 2, 1, 3)]
TWO_WORD_SIZES = [1500, 1400, 1600, 1450]
REACH = ("piece_in_second_word_minus", "piece_across_the_words", "mismatch_past_32_in_seed", "mismatch_past_32_outside_seed")


def two_word_genome():
    return gf.random_genome(np.random.default_rng(611), TWO_WORD_SIZES)


def two_word_queries(rng, refs, trim5, trim3):
    """per trimmed length 30..64 seven windows of the genome, on either strand: a change at the first base, at the last, at base
    31, 32 or 33, at 32 and 33, 0..3 changes anywhere, an N in the second word (where L has one), none; trim5 / trim3 random
    bases around them"""
    qs = []
    for L in range(30, MAXLEN + 1):
        for kind in range(7):
            while True:
                r = refs[int(rng.integers(0, len(refs)))]
                a = int(rng.integers(0, len(r) - L + 1))
                s = r[a:a + L]
                if "N" not in s:
                    break
            for p in ([0], [L - 1], [31 + L % 3], [32, 33], [], [], [])[kind]:
                if p < L:
                    s = change(rng, s, p)
            if kind == 4:
                s = mutate(rng, s, int(rng.integers(0, 4)))
            if kind == 5:
                p = int(rng.integers(32, L)) if L > 32 else int(rng.integers(0, L))
                s = s[:p] + "N" + s[p + 1:]
            if (kind + L) % 2:  # positions above are on the forward text: a '-' read carries them mirrored
                s = _rc(s)
            qs.append(rand_seq(rng, trim5) + s + rand_seq(rng, trim3))
    return qs


def two_word_possible(policy, kmax):
    """which of REACH the policy admits at some L of 30..64, from the cut rule alone"""
    n_mm, seedlen, maxtotal = policy[:3]
    out = dict.fromkeys(REACH, False)
    for L in range(30, MAXLEN + 1):
        for strand in (0, 1):
            (s0, s1), pieces = seed_cut(L, strand, n_mm, seedlen)
            out[REACH[0]] |= strand == 1 and any(lo >= 32 for lo, _ in pieces)
            out[REACH[1]] |= any(lo < 32 < lo + min(pl, kmax) for lo, pl in pieces)
            out[REACH[2]] |= n_mm >= 1 and maxtotal >= 1 and s1 > 32
            out[REACH[3]] |= maxtotal >= 1 and L > 32 and (s0 > 32 or s1 < L)
    return out


def two_word_reached(ref_codes, qs, recs, policy, kmax):
    """which of REACH the brute force's records show"""
    n_mm, seedlen, _, trim5, trim3 = policy
    out = dict.fromkeys(REACH, False)
    for q, r, o, strand, mm in recs:
        s = qs[q][trim5:len(qs[q]) - trim3]
        (s0, s1), pieces = seed_cut(len(s), strand, n_mm, seedlen)
        out[REACH[0]] |= strand == 1 and any(lo >= 32 for lo, _ in pieces)
        out[REACH[1]] |= any(lo < 32 < lo + min(pl, kmax) for lo, pl in pieces)
        if mm:
            qc = gf.CODE[np.frombuffer(s.encode(), dtype=np.uint8)]
            pat = qc if strand == 0 else gf.COMP[qc][::-1]
            for p in np.nonzero((ref_codes[r][o:o + len(s)] != pat) | (pat == 4))[0].tolist():
                if p >= 32:
                    out[REACH[2 if s0 <= p < s1 else 3]] = True
    return out


def two_word_case(policy):
    """-> references, queries, the brute force's records; asserts that they reach what the policy admits"""
    n_mm, seedlen, maxtotal, trim5, trim3 = policy
    refs = two_word_genome()
    qs = two_word_queries(np.random.default_rng(700 + POLICIES.index(policy)), refs, trim5, trim3)
    assert sorted({len(q) - trim5 - trim3 for q in qs}) == list(range(30, MAXLEN + 1))
    want = brute_loci(codes(refs), qs, n_mm, seedlen, maxtotal, trim5, trim3)
    kmax = table_k(len(qs), n_mm)
    possible, reached = two_word_possible(policy, kmax), two_word_reached(codes(refs), qs, want, policy, kmax)
    assert {r[3] for r in want} == {0, 1} and len(want) > len(qs) // 8
    for k in REACH:
        assert reached[k] == possible[k], (policy, k, possible, reached)
    between = [two_word_possible(p, kmax) for p in POLICIES]
    assert all(any(b[k] for b in between) for k in REACH)       # the policies reach every branch between them,
    assert between[POLICIES.index((1, 28, 2, 0, 2))][REACH[0]]  # -n 1 -l 28 the second word from L = 46 on
    return refs, qs, want, possible


@pytest.mark.gpu
@pytest.mark.parametrize("policy", POLICIES, ids=lambda p: "n{}_l{}_e{}_5p{}_3p{}".format(*p))
def test_two_word_queries_every_length(gctx, policy):
    """30..64 nt after trimming, changes at both ends and around the word boundary, N in the second word, seeds of 15 to 64:
    the records and the counts, both strands and --norc"""
    n_mm, seedlen, maxtotal, trim5, trim3 = policy
    refs, qs, want, _ = two_word_case(policy)
    genome = _genome(gctx, refs)
    flat = _flat(qs)
    for norc in (False, True):
        exp = {r for r in want if r[3] == 0} if norc else want
        loci = genome.align_loci(flat, n_mm, seedlen, maxtotal, trim5, trim3, 0, norc)
        assert_sorted(loci)
        assert record_set(loci) == exp, (policy, norc)
        assert np.array_equal(loci["totals"].astype(np.int64), per_query(exp, len(qs)))
        if not norc:
            check_against_counts(genome, flat, loci, n_mm, seedlen, maxtotal, trim5, trim3)
    genome.close()


@pytest.mark.gpu
def test_a_query_of_65_nt_is_refused_until_trimmed(gctx):
    refs = two_word_genome()
    long = refs[2][700:765]
    assert len(long) == MAXLEN + 1 and "N" not in long
    qs = [refs[0][100:130].replace("N", "A"), long]
    genome = _genome(gctx, refs)
    for call in (lambda **k: genome.align_loci(_flat(qs), 1, 28, 2, **k), lambda **k: genome.align_counts(_flat(qs), 1, 28, 2, **k)):
        with pytest.raises(RuntimeError, match="longer than 64"):
            call(trim5=0, trim3=0)
    loci = genome.align_loci(_flat(qs), 1, 28, 2, 0, 1)
    want = brute_loci(codes(refs), qs, 1, 28, 2, 0, 1)
    assert (1, 2, 700, 0, 0) in want and record_set(loci) == want
    check_against_counts(genome, _flat(qs), loci, 1, 28, 2, 0, 1)
    genome.close()


# ------------------------------------------------------------------------------------------------- A2: strata, long reads
def long_strata_case():
    """strata_case with references of 70..90 nt and reads of 49..68 nt (45..64 after -5 1 -3 3), cut from either end; a near copy
    differs by one base inside the seed's first 15, or by two past it: at 17 and, in the second word, at 40"""
    return strata_case(np.random.default_rng(43), n_refs=150, n_reads=240, ref_len=(70, 90), read_len=(49, 68), past=(17, 40))


def strata_expectation(every, max_loci, seen):
    """per query what --best --strata reports of the brute force's alignments under -m max_loci; adds to the counters of
    test_strata_call_equals_brute_force"""
    wants = []
    for e in every:
        best = min((x[4] for x in e), default=None)
        want = sorted(x[:4] for x in e if x[4] == best)
        worse = [x for x in e if x[4] != best]
        if not max_loci:
            seen["best0"] += best == 0
            seen["best1"] += best == 1
            seen["dropped"] += bool(worse)
            seen["two_best"] += len(want) >= 2
            seen["total_in_worse"] += bool(worse) and min(x[3] for x in worse) < min(x[3] for x in want)
            seen["unaligned"] += best is None
        if max_loci and len(want) > max_loci:
            want = []
            seen["capped"] += 1
        elif max_loci and len(e) > max_loci:
            seen["over_in_all_only"] += 1  # -m counts the best stratum alone: reported
        wants.append(want)
    return wants


@pytest.mark.gpu
def test_strata_on_reads_of_45_to_64_nt(gctx):
    """-n 1 -l 15 -5 1 -3 3 --best --strata on reads that fill the second word: the best seed stratum only, -m on it alone"""
    from mirge3_amd import a2i
    refs, reads = long_strata_case()
    n_mm, seedlen, trim5, trim3 = 1, 15, 1, 3
    dev = _genome(gctx, refs)
    g = a2i.GpuGenome(gctx, dev)
    flat = _flat(reads)
    seen = dict(best0=0, best1=0, dropped=0, two_best=0, total_in_worse=0, unaligned=0, capped=0, over_in_all_only=0)
    for norc in (True, False):
        every = brute_strata(refs, reads, n_mm, seedlen, 2, trim5, trim3, norc)
        lens = {len(q) - trim5 - trim3 for q, e in zip(reads, every) if e}
        assert (min(lens), max(lens)) == (45, MAXLEN)
        for max_loci in (0, 2):
            wants = strata_expectation(every, max_loci, seen)
            got = g.loci(flat, n_mm=n_mm, seedlen=seedlen, maxtotal=2, trim5=trim5, trim3=trim3, max_loci=max_loci, norc=norc, strata=True)
            key = list(zip(got["ref"].tolist(), got["off"].tolist(), got["query"].tolist(), got["strand"].tolist()))
            assert key == sorted(key)
            mine = {}
            for q, r, o, st, mm in zip(got["query"].tolist(), got["ref"].tolist(), got["off"].tolist(), got["strand"].tolist(), got["mm"].tolist()):
                mine.setdefault(q, []).append((r, o, st, mm))
            assert got["totals"].tolist() == [len(e) for e in every]
            for q, want in enumerate(wants):
                assert sorted(mine.get(q, [])) == want, (norc, max_loci, q, reads[q])
    dev.close()
    assert all(v >= 3 for v in seen.values()), seen


# ------------------------------------------------------------------------------------------------- A3: dense hits
def dense_case():
    """one reference of runs with no N in it (stream position = offset), a second with the same runs reverse-complemented behind
    an N run; queries that hit a run at every position of it"""
    rng = np.random.default_rng(52)
    r0 = (rand_seq(rng, 40) + "A" * 200 + rand_seq(rng, 30) + "AC" * 80 + rand_seq(rng, 30) + "ACG" * 60 + rand_seq(rng, 30) + "T" * 70)
    assert "N" not in r0 and r0.endswith("T" * 70)
    refs = [r0, "NNNNN" + _rc(r0)]
    window = r0[8:30]
    qs = ["A" * 20, "A" * 33, "A" * 64, "AC" * 12, "CA" * 12, "ACG" * 8, "A" * 19 + "C", "A" * 10 + "N" + "A" * 10] + [window] * 6
    return refs, qs


def strip_load(recs):
    """from records: the most records that start in one 32-aligned strip of reference 0, and the most queries in one strip"""
    per, who = {}, {}
    for q, r, o, _, _ in recs:
        if r == 0:
            per[o // STRIP] = per.get(o // STRIP, 0) + 1
            who.setdefault(o // STRIP, set()).add(q)
    return max(per.values()), max(len(w) for w in who.values())


@pytest.mark.gpu
@pytest.mark.parametrize("n_mm", [0, 1, 2])
def test_more_than_four_hits_in_one_strip(gctx, n_mm):
    """poly-A, dinucleotide and trinucleotide runs: a lane meets more hits in a trip than it stashes, of several queries"""
    refs, qs = dense_case()
    want = brute_loci(codes(refs), qs, n_mm, 28, 2)
    most, queries = strip_load(want)
    assert most > STASH and queries >= 2, (most, queries)
    genome = _genome(gctx, refs)
    flat = _flat(qs)
    loci = genome.align_loci(flat, n_mm, 28, 2)
    assert_sorted(loci)
    assert record_set(loci) == want
    totals = per_query(want, len(qs))
    assert np.array_equal(loci["totals"].astype(np.int64), totals)
    check_against_counts(genome, flat, loci, n_mm, 28, 2, 0, 0)
    # -m 50: all or none per query
    capped = totals > 50
    assert capped.any() and (~capped & (totals > 0)).any()
    few = genome.align_loci(flat, n_mm, 28, 2, 0, 0, 50)
    assert_sorted(few)
    assert record_set(few) == {r for r in want if not capped[r[0]]}
    assert np.array_equal(few["totals"].astype(np.int64), totals)
    check_against_counts(genome, flat, few, n_mm, 28, 2, 0, 0, capped=capped)
    # the same call over batches of three queries
    os.environ["MIRGE_LOCI_BATCH"] = "3"
    try:
        split = genome.align_loci(flat, n_mm, 28, 2)
        split_few = genome.align_loci(flat, n_mm, 28, 2, 0, 0, 50)
    finally:
        del os.environ["MIRGE_LOCI_BATCH"]
    for k in KEYS:
        assert np.array_equal(loci[k], split[k]), k
        assert np.array_equal(few[k], split_few[k]), k
    genome.close()


# ------------------------------------------------------------------------------------------------- A4: key tables of 12 and 13
_ASCII = np.frombuffer(b"ACGTN", dtype=np.uint8)
KEY_SIZES = {40000: 12, 140000: 13}
_KEY_GENOME = {}


def key_table_genome():
    if not _KEY_GENOME:
        refs = gf.random_genome(np.random.default_rng(88), [16000] * 4, n_runs=3)
        _KEY_GENOME["refs"], _KEY_GENOME["codes"] = refs, codes(refs)
    return _KEY_GENOME["refs"], _KEY_GENOME["codes"]


def key_table_queries(n_q, seed):
    """n_q distinct windows of 28..31 nt of the genome as reads of either strand with 0..2 substitutions; a read that equals an
    earlier one takes one more substitution past the seed's 28 bases (a 28-nt one is drawn again).
    -> queries, and per query its place (reference, offset, strand) and its changes in the seed and in all"""
    rng = np.random.default_rng(seed)
    refs, rc = key_table_genome()
    g = np.concatenate(rc)
    size = len(refs[0])
    n_before = np.concatenate(([0], np.cumsum(g == 4)))
    L, ref, off, strand = (np.zeros(n_q, dtype=np.int64) for _ in range(4))
    q0 = np.zeros((n_q, 31), dtype=np.uint8)  # the window as the read holds it, before any change
    col = np.arange(31)

    def draw(rows, min_len):
        todo = rows
        while todo.size:
            L[todo] = rng.integers(min_len, 32, todo.size)
            ref[todo] = rng.integers(0, len(refs), todo.size)
            off[todo] = rng.integers(0, size - L[todo] + 1)
            a = ref[todo] * size + off[todo]
            todo = todo[(n_before[a + L[todo]] - n_before[a]) > 0]  # over an N run: again
        strand[rows] = rng.integers(0, 2, rows.size)
        at = (ref[rows] * size + off[rows])[:, None] + np.where(strand[rows, None] == 0, col[None, :], L[rows, None] - 1 - col[None, :])
        w = g[np.clip(at, 0, g.shape[0] - 1)]
        w = np.where(strand[rows, None] == 1, 3 - w, w)
        w[col[None, :] >= L[rows, None]] = 0
        q0[rows] = w
    draw(np.arange(n_q), 28)
    q = q0.copy()
    n_sub = rng.integers(0, 3, n_q)
    for k in range(2):
        rows = np.nonzero(n_sub > k)[0]
        p = rng.integers(0, L[rows])
        q[rows, p] = (q[rows, p] + rng.integers(1, 4, rows.size)) % 4
    for _ in range(50):
        key = (q.astype(np.uint64) << (2 * col).astype(np.uint64)[None, :]).sum(axis=1, dtype=np.uint64) | ((L - 28).astype(np.uint64) << np.uint64(62))
        _, first = np.unique(key, return_index=True)
        dup = np.setdiff1d(np.arange(n_q), first)
        if not dup.size:
            break
        short = dup[L[dup] == 28]  # no base past the seed: another window, one that has such a base
        draw(short, 29)
        q[short] = q0[short]
        p = rng.integers(28, L[dup])
        q[dup, p] = (q[dup, p] + rng.integers(1, 4, dup.size)) % 4
    else:
        raise AssertionError("the queries did not become distinct")
    diff = (q != q0) & (col[None, :] < L[:, None])
    text = _ASCII[q]
    qs = [text[i, :L[i]].tobytes().decode() for i in range(n_q)]
    return qs, ref, off, strand, diff[:, :28].sum(axis=1), diff.sum(axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("n_q", sorted(KEY_SIZES))
def test_key_tables_of_length_12_and_13(gctx, n_q):
    """-n 1 -l 28 with enough queries for the 4^12 and the 4^13 table (nothing but the query count selects k)"""
    n_mm, seedlen = 1, 28
    assert table_k(n_q, n_mm) == KEY_SIZES[n_q] and table_k(20000, n_mm) == 11
    for L in range(28, 32):
        for strand in (0, 1):
            assert [pl for _, pl in seed_cut(L, strand, n_mm, seedlen)[1]] == [14, 14]  # >= 13: both pieces go into the longest table
    refs, ref_codes = key_table_genome()
    t = time.perf_counter()
    qs, ref, off, strand, seed_changes, changes = key_table_queries(n_q, 90 + KEY_SIZES[n_q])
    t_make = time.perf_counter() - t
    assert len(set(qs)) == n_q
    genome = _genome(gctx, refs)
    flat = _flat(qs)
    t = time.perf_counter()
    loci = genome.align_loci(flat, n_mm, seedlen, 2)
    t_loci = time.perf_counter() - t
    assert_sorted(loci)
    got = record_set(loci)
    # necessary: a read cut with <= 1 change in the seed and <= 2 in all is reported where it was cut
    own = (seed_changes <= n_mm) & (changes <= 2)
    assert own.sum() > n_q // 2 and (~own).sum() > n_q // 100
    mine = set(zip(np.nonzero(own)[0].tolist(), ref[own].tolist(), off[own].tolist(), strand[own].tolist(), changes[own].tolist()))
    assert mine <= got, len(mine - got)
    # exact for a sample, and every query's strata against the count pass
    sample = np.random.default_rng(5).choice(n_q, 300, replace=False).tolist()
    t = time.perf_counter()
    exp = brute_loci(ref_codes, qs, n_mm, seedlen, 2, only=sample)
    t_brute = time.perf_counter() - t
    in_sample = set(sample)
    assert len(exp) > 150 and {r for r in got if r[0] in in_sample} == exp
    check_against_counts(genome, flat, loci, n_mm, seedlen, 2, 0, 0)
    print(f"\n[genome scan edges] k = {KEY_SIZES[n_q]}: {n_q} queries made in {t_make:.2f} s, loci call {t_loci:.3f} s, {len(got)} records, "
          f"brute force of {len(sample)} queries {t_brute:.2f} s")
    genome.close()


# ------------------------------------------------------------------------------------------------- A5: stream ends
def end_queries(refs):
    qs = []
    for r in refs:
        for L in range(1, min(MAXLEN, len(r)) + 1):
            qs += [r[:L], r[len(r) - L:], _rc(r[:L]), _rc(r[len(r) - L:])]
    return qs


def tiny_genomes():
    rng = np.random.default_rng(17)
    out = {f"{n}_bases": [rand_seq(rng, n)] for n in (1, 31, 32, 33, 64)}
    # every stretch (at most 9 bases) shorter than the queries added below; the references' own ends hold N
    short = ["ACGTTGCAN" + "GGATC" + "NN" + "TTGACAGTA", "N" + rand_seq(rng, 9) + "N" + rand_seq(rng, 7)]
    out["short_stretches"] = short
    out["all_N"] = ["NNNNNNN", "N"]
    # stream positions 32 and 64 start a stretch: a reference's end, and an N
    out["boundaries_at_32_and_64"] = [rand_seq(rng, 32), rand_seq(rng, 32) + "N" + rand_seq(rng, 36)]
    return out


@pytest.mark.gpu
def test_stream_ends_and_tiny_genomes(gctx):
    """genomes that end inside the first text words, stretches that start on a word boundary, stretches too short for any query,
    no base at all: the first and last L bases of every reference on both strands, -n 0"""
    seen = 0
    for name, refs in tiny_genomes().items():
        qs = end_queries(refs)
        if name == "short_stretches":
            qs += [refs[0].replace("N", "A")[:12], "ACGTTGCAGG", _rc("GGATCTTTGA"), refs[1][1:10] + "A" + refs[1][11:]]
            assert max(len(s) for r in refs for s in r.split("N")) < min(len(q) for q in qs[-4:])
        genome = _genome(gctx, refs)
        flat = _flat(qs)
        want = brute_loci(codes(refs), qs, 0, 28, 2)
        loci = genome.align_loci(flat, 0, 28, 2)
        assert_sorted(loci)
        assert record_set(loci) == want, name
        assert np.array_equal(loci["totals"].astype(np.int64), per_query(want, len(qs))), name
        check_against_counts(genome, flat, loci, 0, 28, 2, 0, 0)
        if name in ("all_N",):
            assert not want and not loci["totals"].any()
        elif name.endswith("_bases"):
            n = len(refs[0])
            assert {(r[2], r[2] + len(qs[r[0]])) for r in want} >= {(0, L) for L in range(1, min(n, MAXLEN) + 1)} | {(n - 1, n)}
        elif name.startswith("boundaries"):
            assert {(1, 0, 0), (1, 33, 0)} <= {r[1:4] for r in want}  # windows that start at stream positions 32 and 64
            assert not any(r[1] == 1 and r[2] <= 32 < r[2] + len(qs[r[0]]) for r in want)
        seen += len(want)
        genome.close()
    assert seen > 500


# ------------------------------------------------------------------------------------------------- A6: the seed's floor
@pytest.mark.gpu
def test_seed_shorter_than_its_pieces(gctx):
    """a seed of fewer bases than pieces would leave a piece empty: refused (bowtie's own floor for -l is 5); 5 is served"""
    rng = np.random.default_rng(23)
    refs = two_word_genome()
    qs = gf.query_set(rng, refs, 40)
    genome = _genome(gctx, refs)
    flat = _flat(qs)
    assert brute_loci(codes(refs), qs, 2, 2, 2, 0, 2)  # there is something to miss
    for seedlen, n_mm in ((1, 1), (2, 2), (1, 2), (4, 2)):
        with pytest.raises(RuntimeError, match="floor of 5"):
            genome.align_loci(flat, n_mm, seedlen, 2, 0, 2)
        with pytest.raises(RuntimeError, match="floor of 5"):
            genome.align_counts(flat, n_mm, seedlen, 2, 0, 2)
    assert [pl for _, pl in seed_cut(20, 1, 2, 5)[1]] == [1, 2, 2]
    want = brute_loci(codes(refs), qs, 2, 5, 2, 0, 2)
    loci = genome.align_loci(flat, 2, 5, 2, 0, 2)
    assert_sorted(loci)
    assert len(want) > 40 and record_set(loci) == want
    check_against_counts(genome, flat, loci, 2, 5, 2, 0, 2)
    genome.close()
