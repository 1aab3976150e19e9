"""The cases of the ``--kmer-correct`` kernels, shared by the CPU test (tests/test_kmer_correct.py), the host build
(tests/test_kmer_correct_hostsim.py) and the GPU test (tests/test_kmer_correct_gpu.py); no test in here.  A case is a dict: ``reads``
(distinct, in the order they first appeared), ``counts``, ``ks``, ``ke``, ``H``, and what it was written for, by hand: ``want`` (the final
read of every input read) and ``tally`` (some of the tallies of named rounds, ``{round: {name: number}}``).  ``expected(name)`` is the
restatement's answer (tests/ec_restate.py), computed once per case; ``holds(name)`` asserts that the case contains what it is for."""
import functools

import numpy as np

import ec_restate

H = 5
BIG = 100


def rand_seq(rng, n, letters="ACGT"):
    return "".join(letters[x] for x in rng.integers(0, len(letters), n))


def mutate(s, p, step=1):
    return s[:p] + "ACGT"[("ACGT".index(s[p]) + step) % 4] + s[p + 1:]


def case(reads, counts, ks, ke, want, tally=None, h=H):
    assert len(set(reads)) == len(reads) == len(counts) == len(want)
    return {"reads": list(reads), "counts": [int(c) for c in counts], "ks": ks, "ke": ke, "H": h, "want": list(want), "tally": tally or {}}


def _cases():
    rng = np.random.default_rng(20)
    out = {}
    k = 10
    # len = k: a single window; the corrected read merges into the template, which appeared AFTER it: counts add, the first index is the minimum
    t = rand_seq(rng, k)
    out["single_window_merge"] = case([mutate(t, 4), t], [1, BIG], k, k, [t, t], {0: {"eligible": 2, "suspect": 1, "corrected": 1, "distinct": 1}})
    t = rand_seq(rng, k + 1)
    out["len_k_plus_1"] = case([t, mutate(t, 5)], [BIG, 2], k, k, [t, t], {0: {"suspect": 1, "corrected": 1}})
    # an error in the first letter, the last letter and the middle
    t = rand_seq(rng, 24)
    out["first_last_middle"] = case([t, mutate(t, 0), mutate(t, 23), mutate(t, 12)], [BIG, 1, 2, 3], k, k, [t] * 4, {0: {"suspect": 3, "corrected": 3, "distinct": 1}})
    # two errors more than k apart: no letter lies in all weak windows
    t = rand_seq(rng, 30)
    far = mutate(mutate(t, 2), 20)
    out["two_errors_apart"] = case([t, far], [BIG, 1], k, k, [t, far], {0: {"suspect": 1, "uncorrectable": 1, "corrected": 0}})
    # two errors closer than k (both in the first window): lo <= hi, but no single substitution makes every window solid
    near = mutate(mutate(t, 2), 6)
    near_end = mutate(mutate(t, 27), 23)
    out["two_errors_close"] = case([t, near, near_end], [BIG, 1, 1], k, k, [t, near, near_end], {0: {"suspect": 2, "unsupported": 2, "uncorrectable": 0}})
    # a sum of exactly H is weak, H + 1 is solid (single windows)
    a, b = rand_seq(rng, k), rand_seq(rng, k)
    out["threshold"] = case([a, mutate(a, 3), b, mutate(b, 3)], [H, 1, H + 1, 1], k, k, [a, mutate(a, 3), b, b],
                            {0: {"suspect": 3, "unsupported": 2, "corrected": 1}})
    # two candidates at the largest score: ambiguous; different scores: the higher wins
    t = rand_seq(rng, k)
    t = t[:3] + "A" + t[4:]
    c_, g_, t_ = (t[:3] + x + t[4:] for x in "CGT")
    out["tie"] = case([t, c_, g_], [50, 50, 1], k, k, [t, c_, g_], {0: {"suspect": 1, "ambiguous": 1}})
    out["higher_wins"] = case([t, c_, g_, t_], [50, 80, 1, 2], k, k, [t, c_, c_, c_], {0: {"suspect": 2, "corrected": 2, "distinct": 2}})
    # four suspect reads corrected to one sequence that was not in the dictionary: every window of it is held by two of the others
    t = rand_seq(rng, 20)
    e = [mutate(t, p) for p in (0, 19, 15, 4)]
    out["new_sequence"] = case(e, [3, 3, 3, 3], k, k, [t] * 4, {0: {"suspect": 4, "corrected": 4, "distinct": 1}})
    # a read with N is untouched and absent from the spectrum.  s makes a's windows from 1 on solid; a's first window has 3 copies.  Were
    # the windows of `an` (N at 15: starts 0 .. 5 are free of it) counted, that window would be solid, a clean and e corrected to a.
    a = rand_seq(rng, 20)
    an, e, s = a[:15] + "N" + a[16:], mutate(a, 0), a[1:] + "C"
    t = rand_seq(rng, 20)
    tn = t[:3] + "N" + t[4:]
    out["with_n"] = case([a, an, e, s, t, mutate(t, 7), tn], [3, 10, 1, BIG, BIG, 1, 1], k, k, [a, an, e, s, t, t, tn],
                         {0: {"eligible": 5, "suspect": 3, "unsupported": 2, "corrected": 1}})
    # the packing's word boundaries: an error in the last letter of a word and in the first letter of the next
    reads, counts, want = [], [], []
    for L in (31, 32, 33, 63, 64, 65):
        t = rand_seq(rng, L)
        spots = [p for p in (30, 31, 32, 62, 63, 64) if p < L and (p in (31, 32, 63, 64) or p == L - 1)]
        reads += [t] + [mutate(t, p) for p in spots]
        counts += [BIG] + [1] * len(spots)
        want += [t] * (1 + len(spots))
    out["word_boundaries"] = case(reads, counts, 12, 12, want, {0: {"suspect": 14, "corrected": 14, "distinct": 6}})
    # 256 nt is the last eligible length
    a, b = rand_seq(rng, 256), rand_seq(rng, 257)
    out["len_256_257"] = case([a, mutate(a, 255), mutate(a, 128), mutate(a, 0), b, mutate(b, 100)], [BIG, 1, 1, 1, BIG, 1], 12, 12,
                              [a, a, a, a, b, mutate(b, 100)], {0: {"eligible": 4, "suspect": 3, "corrected": 3}})
    t = rand_seq(rng, 40)
    out["k_31"] = case([t, mutate(t, 20), mutate(t, 39), mutate(t, 0)], [BIG, 1, 1, 1], 31, 31, [t] * 4, {0: {"corrected": 3}})
    # sums beyond 2^32: two reads of 2^31 + 1 copies share their first 15 letters.  In 32 bits the shared windows would sum to 2: weak.
    x = rand_seq(rng, 15)
    a, b = x + rand_seq(rng, 10), x + rand_seq(rng, 10)
    out["beyond_2_32"] = case([a, b, mutate(a, 3)], [2 ** 31 + 1, 2 ** 31 + 1, 1], k, k, [a, b, a], {0: {"suspect": 1, "corrected": 1}})
    # a read corrected in two rounds: at k = 8 the windows over its second error are solid (a helper read q + r[18:] holds them), the first
    # error is corrected; at k = 9 the window that starts at 17 is weak and the second error goes
    while True:
        t, q = rand_seq(rng, 30), rand_seq(rng, 10)
        if q[-1] != t[17]:
            break
    r = mutate(mutate(t, 3), 25)
    helper = q + r[18:]
    out["two_rounds"] = case([t, r, helper], [BIG, 1, 10], 8, 9, [t, t, helper], {0: {"suspect": 1, "corrected": 1, "distinct": 3}, 1: {"suspect": 1, "corrected": 1, "distinct": 2}})
    out["empty"] = case([], [], k, 12, [])
    reads = [rand_seq(rng, L) for L in (9, 10, 18, 25, 40, 70)] + ["ACGTNACGTACGTAAA"]
    out["nothing_suspect"] = case(reads, [H + 1, 7, 20, 6, 1000, 6, 1], k, 11, reads, {0: {"suspect": 0, "distinct": 7}, 1: {"suspect": 0, "eligible": 4}})
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    return _cases()


@functools.lru_cache(maxsize=None)
def expected(name):
    c = all_cases()[name]
    return ec_restate.correct(c["reads"], c["counts"], c["ks"], c["ke"], c["H"])


def holds(name):
    """the restatement gives what the case was written for"""
    c, res = all_cases()[name], expected(name)
    assert res["final"] == c["want"], name
    for r, part in c["tally"].items():
        for key, v in part.items():
            assert res["tallies"][r][key] == v, (name, r, key, res["tallies"][r])
    if name == "beyond_2_32":
        S = ec_restate.spectrum(list(zip(c["reads"], c["counts"], range(3))), c["ks"])
        assert max(S.values()) > 2 ** 32 and max(S.values()) % 2 ** 32 <= c["H"]
    if name == "two_rounds":
        assert res["rounds"] == [[], [8, 9], []]
    if name == "single_window_merge":
        assert res["entries"] == [(c["reads"][1], BIG + 1, 0)]
    if name == "new_sequence":
        assert res["entries"][0][0] not in c["reads"] and res["entries"][0][1:] == (12, 0)


@functools.lru_cache(maxsize=None)
def random_set(seed, n_templates=6, letters="ACGT", lengths=(10, 16), ks=8, ke=9, h=2):
    """templates with planted errors: -> a case without ``want``"""
    rng = np.random.default_rng(seed)
    seen = {}
    for _ in range(n_templates):
        t = rand_seq(rng, int(rng.integers(lengths[0], lengths[1] + 1)), letters)
        seen.setdefault(t, int(rng.integers(1, 40)))
        for _ in range(int(rng.integers(0, 6))):
            e = t
            for _ in range(int(rng.integers(1, 3))):
                p = int(rng.integers(0, len(e)))
                e = e[:p] + letters[int(rng.integers(0, len(letters)))] + e[p + 1:]
            seen.setdefault(e, int(rng.integers(1, 4)))
    if seed % 7 == 0:
        seen.setdefault(rand_seq(rng, 9, letters) + "N" + rand_seq(rng, 5, letters), 2)
    reads = list(seen)
    return {"reads": reads, "counts": [seen[r] for r in reads], "ks": ks, "ke": ke, "H": h}


@functools.lru_cache(maxsize=None)
def big_set(n_distinct=20000, seed=77):
    """about n_distinct distinct reads of 18 to 30 nt: Zipf counts over templates, one or two substitutions planted"""
    rng = np.random.default_rng(seed)
    seen = {}
    n_templates = n_distinct // 8
    for ti in range(n_templates):
        t = rand_seq(rng, int(rng.integers(18, 31)))
        seen.setdefault(t, int(1 + 2000 // (1 + ti % 400)))
        for _ in range(7):
            e = mutate(t, int(rng.integers(0, len(t))), int(rng.integers(1, 4)))
            if rng.random() < 0.2:
                e = mutate(e, int(rng.integers(0, len(e))), int(rng.integers(1, 4)))
            seen.setdefault(e, int(rng.integers(1, 4)))
    reads = list(seen)
    return {"reads": reads, "counts": [seen[r] for r in reads], "ks": 15, "ke": 17, "H": 5}
