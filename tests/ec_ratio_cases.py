"""The cases of ``--kmer-ratio`` (k_ec_dominate, k_ec_fold: csrc/kernels_ec.hpp), shared by the CPU test (tests/test_kmer_ratio.py), the
host build (tests/test_kmer_ratio_hostsim.py) and the GPU test (tests/test_kmer_ratio_gpu.py); no test in here.  A case is a case of
tests/ec_cases.py with ``R`` and, by hand, ``want`` (the final read of every input read), ``ad`` (``{round: (A, D)}``) and ``tally``.
``expected(name)`` is the restatement's answer (tests/ec_ratio_restate.py), computed once per case; ``holds(name)`` asserts that the
case contains what it was written for.  The random sets assert their own conditions when they are built."""
import functools

import numpy as np

import ec_ratio_restate as rr
import ec_restate
from ec_cases import rand_seq, mutate

H = 5
K = 10
MAXC = 2 ** 32 - 1
RMAX = 2 ** 31 - 1


def case(reads, counts, ks, ke, R, want, ad=None, tally=None, h=H):
    assert len(set(reads)) == len(reads) == len(counts) == len(want)
    return {"reads": list(reads), "counts": [int(c) for c in counts], "ks": ks, "ke": ke, "H": h, "R": R, "want": list(want), "ad": ad or {},
            "tally": tally or {}}


def wrap_sums():
    """S(x), S(y) with (R S(x)) mod 2^64 <= S(y) < R S(x) at R = 2^31 - 1 and S(y) = 3 (2^32 - 1): the smallest such S(x)"""
    sy = 3 * MAXC
    sx = 2 ** 64 // RMAX
    while not (RMAX * sx) % 2 ** 64 <= sy < RMAX * sx:
        sx += 1
    return sx, sy


def _cases():
    rng = np.random.default_rng(21)
    out = {}
    k = K
    # a deep template and one of its errors, seen 20 times: solid by count, dominated at R = 8
    t = rand_seq(rng, 24)
    v = mutate(t, 12)
    out["deep_template"] = case([t, v], [1000, 20], k, k, 8, [t, t], {0: (25, 10)}, {0: {"suspect": 1, "corrected": 1, "distinct": 1}})
    out["deep_template_no_ratio"] = case([t, v], [1000, 20], k, k, 0, [t, v], {0: (0, 0)}, {0: {"suspect": 0}})
    # the edge of 2a on single windows: 80 >= 8 * 10, 79 < 8 * 10
    x = rand_seq(rng, k)
    y = mutate(x, 3, 2)
    out["edge_80"] = case([x, y], [10, 80], k, k, 8, [y, y], {0: (2, 1)}, {0: {"suspect": 1, "corrected": 1}})
    out["edge_79"] = case([x, y], [10, 79], k, k, 8, [x, y], {0: (2, 0)}, {0: {"suspect": 0}})
    # 2a applies above H only: x (H + 1 copies) is dominated, z (H copies) is weak by count and in neither A nor D
    x, z = rand_seq(rng, k), rand_seq(rng, k)
    y, w = mutate(x, 3), mutate(z, 3)
    out["h_plus_1"] = case([x, y, z, w], [H + 1, 8 * (H + 1), H, 1000], k, k, 8, [y, y, w, w], {0: (3, 1)}, {0: {"suspect": 2, "corrected": 2}})
    # r's only candidate that is solid by count is c, and c is dominated by t: unsupported with the ratio, corrected without
    t = rand_seq(rng, k)
    c = mutate(t, 2)
    r = mutate(c, 7)
    out["dominated_target"] = case([t, c, r], [1000, 20, 1], k, k, 8, [t, t, r], {0: (2, 1)}, {0: {"suspect": 2, "corrected": 1, "unsupported": 1}})
    out["dominated_target_no_ratio"] = case([t, c, r], [1000, 20, 1], k, k, 0, [t, c, c], {0: (0, 0)}, {0: {"suspect": 1, "corrected": 1}})
    # two errors over two rounds.  r = t with errors at 3 and 25; i = t with the error at 25, seen 20 times.  At k = 8 a helper of 200
    # copies holds every window over letter 25 (221 copies: 1000 < 8 * 221), so r loses its first error and becomes i.  At k = 9 the
    # window that starts at 17 is not the helper's: 21 copies against t's 1000, dominated, and i -- with r inside -- becomes t.
    while True:
        t, q = rand_seq(rng, 30), rand_seq(rng, 10)
        if q[-1] != t[17]:
            break
    i = mutate(t, 25)
    r = mutate(i, 3)
    helper = q + r[18:]
    out["two_errors_two_rounds"] = case([t, i, r, helper], [1000, 20, 1, 200], 8, 9, 8, [t, t, t, helper], {},
                                        {0: {"suspect": 1, "corrected": 1, "distinct": 3}, 1: {"suspect": 1, "corrected": 1, "distinct": 2}})
    out["two_errors_two_rounds_no_ratio"] = case([t, i, r, helper], [1000, 20, 1, 200], 8, 9, 0, [t, i, i, helper], {},
                                                 {0: {"suspect": 1, "corrected": 1}, 1: {"suspect": 0}})
    # a family: two templates one letter apart at 1000 : 200
    t = rand_seq(rng, 24)
    u = mutate(t, 12, 2)
    out["family_r8"] = case([t, u], [1000, 200], k, k, 8, [t, u], {0: (25, 0)}, {0: {"suspect": 0}})
    out["family_r4"] = case([t, u], [1000, 200], k, k, 4, [t, t], {0: (25, 10)}, {0: {"suspect": 1, "corrected": 1, "distinct": 1}})
    # reads that contribute to no sum dominate nothing: the k-mers one letter from a's are held, 100 000 times each, by a read with an N
    # and by a read of 257 nt only
    a = rand_seq(rng, 20)
    b = mutate(a, 5)
    bn = b + "N" + rand_seq(rng, 4)
    blong = b + rand_seq(rng, 237)
    assert len(blong) == 257
    out["non_contributors"] = case([a, bn, blong], [20, 100000, 100000], k, k, 8, [a, bn, blong], {0: (11, 0)}, {0: {"eligible": 1, "suspect": 0}})
    # a neighbour at every letter of a 31-letter word: substitutions at read letters 0, 15, 30 and the last one, reads of 31 .. 65 nt
    reads, counts, want = [], [], []
    for L in (31, 32, 33, 64, 65):
        t = rand_seq(rng, L)
        spots = sorted({0, 15, 30, L - 1})
        reads += [t] + [mutate(t, p, 1 + n % 3) for n, p in enumerate(spots)]
        counts += [1000] + [20] * len(spots)
        want += [t] * (1 + len(spots))
    out["every_letter_k31"] = case(reads, counts, 31, 31, 8, want, {}, {0: {"suspect": 19, "corrected": 19, "distinct": 5}})
    # a 64-bit product that wraps: S(x) a little above 2^33 in three reads x + A / C / G, S(y) = 3 (2^32 - 1) likewise
    sx, sy = wrap_sums()
    x = rand_seq(rng, k)
    y = mutate(x, 4)
    cx = [sx // 3, sx // 3, sx - 2 * (sx // 3)]
    reads = [x + e for e in "ACG"] + [y + e for e in "ACG"]
    out["wrap"] = case(reads, cx + [MAXC] * 3, k, k, RMAX, reads, {0: (8, 0)}, {0: {"eligible": 6, "suspect": 0}})
    out["empty"] = case([], [], k, 12, 8, [], {0: (0, 0), 2: (0, 0)})
    reads = [rand_seq(rng, k) for _ in range(4)]
    reads.append(mutate(reads[0], 2))
    out["nothing_above_h"] = case(reads, [H, 1, 3, H, 2], k, k, 2, reads, {0: (0, 0)}, {0: {"suspect": 5, "unsupported": 5}})
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    return _cases()


@functools.lru_cache(maxsize=None)
def expected(name):
    c = all_cases()[name]
    return rr.correct(c["reads"], c["counts"], c["ks"], c["ke"], c["H"], c["R"])


def _spectrum(c):
    return ec_restate.spectrum(list(zip(c["reads"], c["counts"], range(len(c["reads"])))), c["ks"])


def holds(name):
    """the restatement gives what the case was written for"""
    c, res = all_cases()[name], expected(name)
    assert res["final"] == c["want"], name
    for r, part in c["tally"].items():
        for key, v in part.items():
            assert res["tallies"][r][key] == v, (name, r, key, res["tallies"][r])
    for r, (a, d) in c["ad"].items():
        assert (res["above"][r], res["dominated"][r]) == (a, d), (name, r, res["above"], res["dominated"])
    if name == "wrap":
        S = _spectrum(c)
        sx, sy = S[c["reads"][0][:K]], S[c["reads"][3][:K]]
        assert (sx, sy) == wrap_sums() and (RMAX * sx) % 2 ** 64 <= sy < RMAX * sx and max(c["counts"]) <= MAXC
    if name == "two_errors_two_rounds":
        assert res["rounds"] == [[], [9], [8, 9], []] and res["dominated"] == [0, 1]
    if name == "two_errors_two_rounds_no_ratio":
        assert res["rounds"] == [[], [], [8], []]
    if name == "non_contributors":
        S = _spectrum(c)
        for b in c["reads"][1:]:  # were they counted, every k-mer of a over letter 5 would be dominated
            for i in range(11):
                S[b[i:i + K]] = S.get(b[i:i + K], 0) + 100000
        assert len(rr.dominated(S, K, H, 8)) == 6
    if name == "dominated_target":
        assert res["entries"] == [(c["reads"][0], 1020, 0), (c["reads"][2], 1, 2)]


RANDOM_RATIOS = (2, 3, 8)


@functools.lru_cache(maxsize=None)
def random_set(seed, n_templates=6, lengths=(10, 16), ks=8, ke=9, h=2):
    """tests/ec_cases.py's random_set with skewed counts: one template of the set has 50 .. 500 times a count of the others' kind, and an
    error is seen 1 .. 8 times (tie-rich: two letters in a third of the sets) -> a case without ``want``, R = 2, 3, 8 in turn"""
    rng = np.random.default_rng(1000 + seed)
    letters = "AC" if seed % 3 == 0 else "ACGT"
    deep = int(rng.integers(0, n_templates))
    seen = {}
    for ti in range(n_templates):
        t = rand_seq(rng, int(rng.integers(lengths[0], lengths[1] + 1)), letters)
        c = int(rng.integers(1, 40))
        seen.setdefault(t, c * int(rng.integers(50, 501)) if ti == deep else c)
        for _ in range(int(rng.integers(0, 6))):
            e = t
            for _ in range(int(rng.integers(1, 3))):
                p = int(rng.integers(0, len(e)))
                e = e[:p] + letters[int(rng.integers(0, len(letters)))] + e[p + 1:]
            seen.setdefault(e, int(rng.integers(1, 9)))
    if seed % 7 == 0:
        seen.setdefault(rand_seq(rng, 9, letters) + "N" + rand_seq(rng, 5, letters), 2)
    reads = list(seen)
    return {"reads": reads, "counts": [seen[r] for r in reads], "ks": ks, "ke": ke, "H": h, "R": RANDOM_RATIOS[(seed // 3) % 3]}


N_RANDOM = 300


@functools.lru_cache(maxsize=None)
def random_sets():
    """-> [(case, the restatement's answer)]; asserts that the sets reach the relative threshold often enough"""
    out, with_d, differ = [], 0, 0
    for seed in range(N_RANDOM):
        c = random_set(seed)
        want = rr.correct(c["reads"], c["counts"], c["ks"], c["ke"], c["H"], c["R"])
        plain = ec_restate.correct(c["reads"], c["counts"], c["ks"], c["ke"], c["H"])
        with_d += sum(want["dominated"]) > 0
        differ += want["final"] != plain["final"]
        out.append((c, want))
    assert 2 * with_d >= N_RANDOM and 3 * differ >= N_RANDOM, (with_d, differ)
    return out


@functools.lru_cache(maxsize=None)
def random_sets_side_by_side():
    """for the device: the small sets of one R side by side, each behind a random 16-letter prefix of its own (the sets share no k-mer that
    holds a letter of theirs, and hardly one of the prefixes'); the expectation is the restatement's on the whole -> {R: (case, the restatement's answer)}"""
    rng = np.random.default_rng(6)
    prefixes = [rand_seq(rng, 16) for _ in range(N_RANDOM)]
    assert len(set(prefixes)) == N_RANDOM
    out = {}
    for R in RANDOM_RATIOS:
        keep = {}
        for seed in range(N_RANDOM):
            c = random_set(seed)
            if c["R"] == R:
                for r, n in zip(c["reads"], c["counts"]):
                    keep.setdefault(prefixes[seed] + r, n)
        case_ = {"reads": list(keep), "counts": list(keep.values()), "ks": 10, "ke": 11, "H": 2, "R": R}
        want = rr.correct(case_["reads"], case_["counts"], 10, 11, 2, R)
        plain = ec_restate.correct(case_["reads"], case_["counts"], 10, 11, 2)
        assert sum(want["dominated"]) > 50 and sum(t["corrected"] for t in want["tallies"]) > 50
        assert sum(a != b for a, b in zip(want["final"], plain["final"])) > 50
        out[R] = (case_, want)
    return out


@functools.lru_cache(maxsize=None)
def big_set(n_distinct=20000, seed=78, R=8):
    """about n_distinct distinct reads of 18 to 30 nt: Zipf counts over templates, and every template's errors (one or two substitutions)
    seen in proportion to its depth -> (case, the restatement's answer, the answer without a ratio)"""
    rng = np.random.default_rng(seed)
    seen = {}
    n_templates = n_distinct // 8
    for ti in range(n_templates):
        t = rand_seq(rng, int(rng.integers(18, 31)))
        depth = int(1 + 20000 // (1 + ti % 200))
        seen.setdefault(t, depth)
        for _ in range(7):
            e = mutate(t, int(rng.integers(0, len(t))), int(rng.integers(1, 4)))
            if rng.random() < 0.2:
                e = mutate(e, int(rng.integers(0, len(e))), int(rng.integers(1, 4)))
            seen.setdefault(e, int(1 + depth * rng.uniform(0.002, 0.02)))
    reads = list(seen)
    c = {"reads": reads, "counts": [seen[r] for r in reads], "ks": 15, "ke": 17, "H": 5, "R": R}
    want = rr.correct(c["reads"], c["counts"], c["ks"], c["ke"], c["H"], R)
    plain = ec_restate.correct(c["reads"], c["counts"], c["ks"], c["ke"], c["H"])
    assert 18000 < len(reads) < 22000
    assert sum(want["dominated"]) >= 1000
    assert sum(t["corrected"] for t in want["tallies"]) >= 1000 + sum(t["corrected"] for t in plain["tallies"])
    return c, want, plain
