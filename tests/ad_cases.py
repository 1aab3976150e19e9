"""The cases of the ``-a auto`` kernels, shared by the CPU test (tests/test_adapter_auto.py), the host build
(tests/test_adapter_auto_hostsim.py) and the GPU test (tests/test_adapter_auto_gpu.py); no test in here.  A case is a dict: ``reads``
(distinct), ``counts`` and ``want``: some fields of the answer, written by hand for what the case is about.  ``expected(name)`` is the
restatement's answer (tests/ad_restate.py), computed once per case; ``holds(name)`` asserts that the case contains what it is for."""
import functools

import numpy as np

import ad_restate
from ad_restate import K

ILLUMINA = "TGGAATTCTCGGGTGCCAAGGAACTCCAG"  # the small-RNA 3' adapter (what `-a illumina` stands for)
TAIL = "TCACATCACGATCTCGTATGCCGTCTTCTGCTTGAAAAAAAAAA"  # what follows it in a read that runs on: index, flow-cell oligo, poly-A
QIA19 = "AACTGTAGGCACCATCAAT"


def rand_seq(rng, n, letters="ACGT"):
    return "".join(letters[x] for x in rng.integers(0, len(letters), n))


def case(reads, counts, **want):
    assert len(set(reads)) == len(reads) == len(counts)
    return {"reads": list(reads), "counts": [int(c) for c in counts], "want": want}


def planted(rng, adapter, cycles, n=200, behind=lambda rng: TAIL, counts=(1, 50)):
    """n distinct inserts of 18 .. 30 nt, each followed by the adapter and what comes behind it, cut at ``cycles``"""
    seen = {}
    while len(seen) < n:
        r = (rand_seq(rng, int(rng.integers(18, 31))) + adapter + behind(rng))[:cycles]
        seen.setdefault(r, int(rng.integers(counts[0], counts[1] + 1)))
    return list(seen), list(seen.values())


def at_offsets(rng, x, offsets, counts, behind=""):
    """one read per offset: random letters in front (the last one is G and T in turn: no letter in front of x reaches 90 %
    by chance), x at the offset, ``behind`` after it"""
    reads = []
    for i, o in enumerate(offsets):
        front = rand_seq(rng, o)
        if o:
            front = front[:-1] + "GT"[i % 2]
        reads.append(front + x + behind)
    return reads, list(counts)


X = "ACCAACACACAG"  # eleven letters of A and C, then G: three letters; A + X[:11] and C + X[:11] have two


def _cases():
    rng = np.random.default_rng(31)
    out = {}
    r, c = planted(rng, ILLUMINA, 50)
    out["planted_50"] = case(r, c, start=ILLUMINA[:K], prefix_of=ILLUMINA + TAIL)
    # x at five and at six offsets
    r, c = at_offsets(rng, X, range(1, 6), [10] * 5)
    out["spread_5"] = case(r, c, seq="", eligible=50, candidates=0)
    r, c = at_offsets(rng, X, range(1, 7), [10] * 6)
    out["spread_6"] = case(r, c, seq=X, eligible=60, candidates=1, support=60, spread=6, left_steps=0)
    # the floor ceil(T / 20) with T = 1990 (100; 99 is 99.5 rounded DOWN), and the floor 32
    for name, cx in (("floor_T_below", 99), ("floor_T_at", 100)):
        r, c = at_offsets(rng, X, range(1, 7), [cx - 5 * 16] + [16] * 5)
        fill = [rand_seq(rng, 30) for _ in range(30)]
        r, c = r + fill, c + [63] * 29 + [1990 - cx - 63 * 29]
        out[name] = case(r, c, eligible=1990, seq=X if cx == 100 else "", candidates=int(cx == 100))
    for name, cx in (("floor_32_below", 31), ("floor_32_at", 32)):
        r, c = at_offsets(rng, X, range(1, 7), [cx - 25] + [5] * 5)
        out[name] = case(r, c, eligible=cx, seq=X if cx == 32 else "", candidates=int(cx == 32))
    # the adapter's first 12 letters have two letters: the seed lies further right, the left walk (no complexity test) reaches the start
    two = "ACCACACAACAC" + "GTCAGTTGCATCGGATCCTAGA"
    r, c = planted(rng, two, 50)
    out["two_letter_start"] = case(r, c, start=two[:K], prefix_of=two + TAIL)
    # two seed candidates of equal C: the smaller string
    x2 = "CATTGGACTACG"
    r1, c1 = at_offsets(rng, X, range(1, 7), [10] * 6)
    r2, c2 = at_offsets(rng, x2, range(1, 7), [10] * 6)
    out["seed_tie"] = case(r2 + r1, c2 + c1, seq=min(X, x2), candidates=2, eligible=120)
    # equal C in a left step: reads that end in A + X[:11] and in C + X[:11] (two letters: no seed candidates), as heavy as X together
    ra, ca = at_offsets(rng, "A" + X[:11], range(1, 7), [10] * 6)
    rc, cc = at_offsets(rng, "C" + X[:11], range(1, 7), [10] * 6)
    rx, cx = at_offsets(rng, X, range(2, 8), [10] * 6)
    out["left_tie"] = case(rc + ra + rx, cc + ca + cx, seq="A" + X, left_steps=1, support=60, seed_sum=60)
    # equal C in a right step, which is also 2 C(z) = C(start) exactly: half of x's reads go on with A.., half with C..
    ra, ca = at_offsets(rng, X, (1, 3, 5), [10] * 3, behind="AGT")
    rc, cc = at_offsets(rng, X, (2, 4, 6), [10] * 3, behind="CTG")
    out["right_tie"] = case(rc + ra, cc + ca, seq=X + "AGT", support=60)
    # 10 C(y) = 9 C(first) exactly, and one count below
    for name, cy in (("left_90_exact", 90), ("left_90_below", 89)):
        r, c = at_offsets(rng, "G" + X, range(0, 6), [15] * 5 + [cy - 75])
        out[name] = case(r + [X], c + [100 - cy], seed_sum=100, left_steps=int(cy == 90), seq=("G" if cy == 90 else "") + X, support=cy if cy == 90 else 100)
    # 2 C(z) = C(start) exactly, and one count below
    for name, cz in (("right_half_exact", 50), ("right_half_below", 49)):
        ra, ca = at_offsets(rng, X, (1, 3, 5), [20, 20, cz - 40], behind="A")
        rx, cx = at_offsets(rng, X, (2, 4, 6), [20, 20, 60 - cz])
        out[name] = case(ra + rx, ca + cx, support=100, seq=X + ("A" if cz == 50 else ""))
    # the cap of 32 letters
    r, c = planted(rng, ILLUMINA, 75)
    out["cap_32"] = case(r, c, seq=(ILLUMINA + TAIL)[:32], len=32)
    # a period-3 sequence: every left step finds the same three 12-mers again, 64 times
    out["period_3"] = case(["ACG" * 30, "CGA" * 30], [40, 7], left_steps=64, len=32, eligible=47)
    # reads with N and of 257 nt that would bring x to seven offsets if they counted
    r, c = at_offsets(rng, X, range(1, 6), [10] * 5)
    withn = rand_seq(rng, 7) + "T" + X + "N"
    long257 = rand_seq(rng, 9) + "T" + X + rand_seq(rng, 257 - 10 - K)
    out["n_and_257"] = case(r + [withn, long257], c + [10, 10], seq="", eligible=50, candidates=0)
    # a window at p = 63 counts, one at p = 64 does not
    for name, o in (("p_63", 63), ("p_64", 64)):
        r, c = at_offsets(rng, X, [1, 2, 3, 4, 5, o], [10] * 6)
        out[name] = case(r, c, eligible=60, seq=X if o == 63 else "", spread=6 if o == 63 else 0)
    # every storage group, and x across the word boundaries at letters 32 and 64
    reads = []
    for i, (L, o) in enumerate(((12, 0), (13, 1), (31, 19), (32, 20), (33, 21), (63, 25), (64, 31), (65, 53), (128, 60), (129, 63), (255, 64), (256, 10))):
        front = rand_seq(rng, o)
        front = front[:-1] + "GT"[i % 2] if o else front
        reads.append(front + X + rand_seq(rng, L - o - K))
    out["lengths"] = case(reads, [3 + i for i in range(12)], eligible=sum(range(3, 15)), start=X)
    # sums beyond 2^32: in 32 bits C(x) would be 6
    r, c = at_offsets(rng, X, range(1, 7), [2 ** 31 + 1] * 6)
    out["beyond_2_32"] = case(r, c, seq=X, support=6 * (2 ** 31 + 1), eligible=6 * (2 ** 31 + 1))
    # 12 random letters (a UMI) behind a 19-nt adapter
    r, c = planted(rng, QIA19, 75, behind=lambda g: rand_seq(g, 12) + TAIL)
    out["umi_behind"] = case(r, c, seq=QIA19)
    out["empty"] = case([], [], seq="", eligible=0, candidates=0)
    out["nothing_eligible"] = case(["ACGTACGTACG", "ACGTNACGTACGTAAA", rand_seq(rng, 257), "NNNNNNNNNNNNNN"], [100, 100, 100, 100], seq="", eligible=0, candidates=0)
    reads = list(dict.fromkeys(rand_seq(rng, int(rng.integers(18, 51))) for _ in range(200)))
    out["no_adapter"] = case(reads, rng.integers(1, 51, len(reads)).tolist(), seq="", candidates=0)
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    return _cases()


@functools.lru_cache(maxsize=None)
def expected(name):
    c = all_cases()[name]
    return ad_restate.infer(c["reads"], c["counts"])


@functools.lru_cache(maxsize=None)
def probes(name):
    """every 12-mer of the case's reads, eight absent ones, a code past the table"""
    c = all_cases()[name]
    rng = np.random.default_rng(len(name))
    return ad_restate.probes_of(c["reads"], extra=[int(x) for x in rng.integers(0, 4 ** K, 8)] + [4 ** K + 5])


def probe_answers(res, codes):
    """(C, M) of the restatement for a list of codes"""
    strs = [ad_restate.decode(x) if x < 4 ** K else None for x in codes]
    return [res["C"](s) if s else 0 for s in strs], [res["M"](s) if s else 0 for s in strs]


def holds(name):
    """the restatement gives what the case was written for"""
    c, res = all_cases()[name], expected(name)
    for key, v in c["want"].items():
        if key == "prefix_of":
            assert res["len"] >= K and v.startswith(res["seq"]), (name, res["seq"])
        elif key == "start":
            assert ad_restate.decode(res["start"]) == v and res["seq"].startswith(v), (name, res["seq"])
        else:
            assert res[key] == v, (name, key, res[key])
    ties = res["ties"]
    if name == "seed_tie":
        assert ties["seed"] == 1
    if name == "left_tie":
        assert ties["left"] == 1 and res["C"]("C" + X[:11]) == res["C"]("A" + X[:11]) == 60
    if name == "right_tie":
        assert ties["right"] == 1 and 2 * res["C"](X[1:] + "C") == 2 * res["C"](X[1:] + "A") == res["support"]
    if name == "left_90_below":
        assert 10 * res["C"]("G" + X[:11]) == 9 * res["seed_sum"] - 10 and bin(res["M"]("G" + X[:11])).count("1") >= 6
    if name == "right_half_below":
        assert 2 * res["C"](X[1:] + "A") == res["support"] - 2
    if name == "two_letter_start":
        assert res["seed"] != res["start"] and res["left_steps"] >= 1 and len(set(ad_restate.decode(res["start"]))) == 2
    if name == "lengths":
        assert bin(res["M"](X)).count("1") == 11 and not (res["M"](X) >> 64) and (res["M"](X) >> 63) & 1
    if name == "n_and_257":
        T, C, M = ad_restate.spectrum([r.replace("N", "A")[:256] for r in c["reads"]], c["counts"])
        assert bin(M[X]).count("1") == 7  # (what counting them would give)
    if name == "beyond_2_32":
        assert res["support"] > 2 ** 32 and res["support"] % 2 ** 32 == 6
    if name == "planted_50":
        assert len(c["reads"]) == 200 and all(len(r) == 50 for r in c["reads"])


@functools.lru_cache(maxsize=None)
def random_set(seed):
    """a small tie-rich set over two letters (seed % 3 == 0; the 12-mer x then ends in G, so that it alone has three letters) or four: x
    behind six fronts of distinct lengths, with one of two extensions (in every fifth set also alone); six reads each that END in b + x[:11] for two
    letters b (what a left step looks up, without adding to x); in every fourth set a second motif, in every fourth x alone with three reads of 8 on either extension; counts of 8 and sometimes 16, so
    that equal sums are common"""
    rng = np.random.default_rng(1000 + seed)
    letters = "AC" if seed % 3 == 0 else "ACGT"
    x = rand_seq(rng, K - 1, letters) + ("G" if letters == "AC" else rand_seq(rng, 1))
    seen = {}

    def add(bodies, lo, even=False):
        for i, o in enumerate(rng.choice(np.arange(lo, 10), size=6, replace=False)):
            body = bodies[i % 2] if even else bodies[int(rng.integers(0, len(bodies)))]
            seen.setdefault(rand_seq(rng, int(o), letters) + body, 8 if even else int(rng.choice([8, 16], p=[0.85, 0.15])))

    ext = rand_seq(rng, int(rng.integers(1, 9)), letters)
    other = letters[(letters.index(ext[0]) + 1) % len(letters)] + rand_seq(rng, int(rng.integers(0, 8)), letters)  # (another first letter)
    add([x + ext, x + other] + ([x] if seed % 5 == 0 else []), 1, even=seed % 4 == 1)  # (even: three reads of 8 each way)
    for b in rng.choice(list(letters), 2, replace=False) if seed % 4 != 1 else ():
        add([str(b) + x[:K - 1]], 0)
    if seed % 4 == 3:  # a second motif of the same weight, or nearly
        add([rand_seq(rng, K - 1, letters) + ("T" if letters == "AC" else rand_seq(rng, 1))], 1)
    if seed % 7 == 0:
        seen.setdefault(rand_seq(rng, 3, letters) + x[:5] + "N" + x[6:] + ext, 16)
    reads = list(seen)
    return {"reads": reads, "counts": [seen[r] for r in reads]}


def synthetic_sample(seed, adapter, cycles, behind=None, n_reads=20000, n_templates=300, top_share=None, dimers=0.0, polyg=False, sub_rate=0.005):
    """reads as a sequencer would give them: Zipf counts over templates of 19 .. 34 nt, 3' and 5' isomiR variation, substitutions at
    ``sub_rate`` per letter; ``adapter`` None: none (the insert alone, at most ``cycles``).  -> (distinct reads, counts)"""
    rng = np.random.default_rng(seed)
    templates = [rand_seq(rng, int(rng.integers(19, 35))) for _ in range(n_templates)]
    w = 1.0 / np.arange(1, n_templates + 1)
    if top_share is not None:
        w[0] = top_share / (1 - top_share) * w[1:].sum()
    pick = rng.choice(n_templates, n_reads, p=w / w.sum())
    seen = {}
    for ti in pick:
        t = templates[ti]
        t = t[int(rng.integers(0, 3)) if rng.random() < 0.2 else 0:len(t) - (int(rng.integers(0, 4)) if rng.random() < 0.4 else 0)]
        if rng.random() < dimers:
            t = ""
        if adapter is None:
            r = t[:cycles]
        else:
            tail = behind(rng) if behind else TAIL
            r = t + adapter + tail
            r = (r + ("G" * cycles if polyg else rand_seq(rng, cycles)))[:cycles] if len(r) < cycles else r[:cycles]
        r = list(r)
        for p in np.flatnonzero(rng.random(len(r)) < sub_rate):
            r[p] = "ACGT"[("ACGT".index(r[p]) + int(rng.integers(1, 4))) % 4]
        r = "".join(r)
        if r:
            seen[r] = seen.get(r, 0) + 1
    return list(seen), list(seen.values())


NEB = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCAC"

SYNTHETIC = {  # name -> (keyword arguments of synthetic_sample, the planted sequence with what follows it, or None)
    "illumina_36": (dict(adapter=ILLUMINA, cycles=36), ILLUMINA + TAIL),
    "illumina_50": (dict(adapter=ILLUMINA, cycles=50), ILLUMINA + TAIL),
    "illumina_75": (dict(adapter=ILLUMINA, cycles=75), ILLUMINA + TAIL),
    "qia_umi": (dict(adapter=QIA19, cycles=75, behind=lambda g: rand_seq(g, 12)), QIA19),  # (random letters to the read's end)
    "neb_top_90": (dict(adapter=NEB, cycles=50, top_share=0.9), NEB + TAIL),
    "neb_top_99": (dict(adapter=NEB, cycles=50, top_share=0.99), NEB + TAIL),
    "dimers_30": (dict(adapter=ILLUMINA, cycles=50, dimers=0.3), ILLUMINA + TAIL),
    "poly_g": (dict(adapter=ILLUMINA, cycles=75, behind=lambda g: "", polyg=True), ILLUMINA + "G" * 75),
    "subs_2pc": (dict(adapter=ILLUMINA, cycles=50, sub_rate=0.02), ILLUMINA + TAIL),
    "no_adapter": (dict(adapter=None, cycles=50), None),
}
