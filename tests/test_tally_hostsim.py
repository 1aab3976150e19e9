"""The A-to-I tally kernel on the CPU: ``csrc/kernels_tally.hpp`` itself (k_tally<1>, k_tally<2>, the TallyMember predicate) compiled
for the host (tests/hostsim/tally_sim.cpp) against ``oracle.variant_tally``, the string restatement that the reference's own functions
pin (tests/test_a2i_gff_oracle.py, up to canonical sequences of 32 nt and reads of 35).  Every comparison is exact integer equality.
``directed_case`` below is shared with the GPU test (tests/test_tally_gpu.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostsim", "tally_sim.cpp")
SO = os.path.join(HERE, "hostsim", "_build", "libtallysim.so")
CSRC = os.path.join(HERE, "..", "mirge3.0_amd", "csrc")
KEYS = ("diag", "state", "n_seqs", "seq_true", "count_true", "canon", "kept_exact", "census")
EXACT_POL = dict(oracle.PASSES[0][3])  # -n 0, reads under 26 nt
ISO_POL = dict(oracle.PASSES[8][3])    # -5 1 -3 2 -v 2
FREQ = np.array([0.4, 1e300, 0.5])     # an isomiR read needs 3 copies in sample 0, 1 in sample 1 or 2 in sample 2


@pytest.fixture(scope="module")
def sim():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("kernels_tally.hpp", "mirge_core.hpp", "mirge_libbuild.hpp")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", SO, SRC])
    return C.CDLL(SO)


def _flat(strs):
    off = np.zeros(len(strs) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in strs], out=off[1:])
    return np.frombuffer(("".join(strs) or "\0").encode(), dtype=np.uint8).copy(), off


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def run_sim(sim, seqs, counts, pass_, ref, fam_of_ref, targets, retained, freq, exact_pass=0, iso_pass=8, chunk=256, block=64):
    """-> (error code, dict as ``_ffi.variant_tally`` returns it plus ``wide_members`` and ``n_chunks``)"""
    n, F = len(seqs), len(targets)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    assert counts.ndim == 2 and counts.shape[0] == n
    S = counts.shape[1]
    rd, roff = _flat(seqs)
    td, toff = _flat(targets)
    ps = np.ascontiguousarray(pass_, dtype=np.int8)
    rf = np.ascontiguousarray(ref, dtype=np.int32)
    fam = np.ascontiguousarray(np.r_[np.asarray(fam_of_ref, dtype=np.int32), np.int32(-1)])
    ret = None if retained is None else np.ascontiguousarray(retained, dtype=np.uint8)
    fq = np.ascontiguousarray(freq, dtype=np.float64)
    assert fq.shape[0] == S and ps.shape[0] == n and rf.shape[0] == n
    tabs = np.zeros((5, F, S), dtype=np.int64)
    cen = np.zeros((F, 32, 4, 4, 3, S), dtype=np.int64)
    diag, state = np.zeros(n + 1, dtype=np.int8), np.zeros(n + 1, dtype=np.int8)
    wide, n_chunks = np.zeros(1, dtype=np.int64), np.zeros(4, dtype=np.int32)
    rc = sim.sim_tally(_p(rd), _p(roff), C.c_int64(n), _p(ps), _p(rf), _p(counts), C.c_int32(S), C.c_int32(exact_pass), C.c_int32(iso_pass),
                       _p(fam), _p(td), _p(toff), C.c_int64(F), _p(ret), _p(fq), C.c_uint32(chunk), C.c_uint32(block),
                       _p(tabs), _p(cen), _p(diag), _p(state), _p(wide), _p(n_chunks))
    out = dict(zip(("n_seqs", "seq_true", "count_true", "canon", "kept_exact"), tabs))
    out.update(census=cen, diag=diag[:n], state=state[:n], wide_members=int(wide[0]), n_chunks=n_chunks.tolist())
    return rc, out


def assert_same(g, o, what=""):
    for k in KEYS:
        if not np.array_equal(g[k], o[k]):
            bad = np.argwhere(np.asarray(g[k]) != np.asarray(o[k]))
            raise AssertionError(f"{what}{k}: {len(bad)} cells differ, first at {bad[0].tolist()}: "
                                 f"{np.asarray(g[k])[tuple(bad[0])]} != {np.asarray(o[k])[tuple(bad[0])]}")


def rnd(rng, n):
    return "".join("ACGT"[int(c)] for c in rng.integers(0, 4, size=n))


# ---------------------------------------------------------------------------------------------------------------
# random unrelated pairs: every diagonal -63..31, the tie order, "no positive score", the pruning bound
# ---------------------------------------------------------------------------------------------------------------
PAIRS_PER_SEED = 10000


@pytest.mark.parametrize("seed", range(10))
def test_random_unrelated_pairs(sim, seed):
    """10 x 10 000 (target, read) pairs that have nothing to do with each other: targets of every length 1..32 (18, 25, 26, 31 and 32
    more often), reads of every length 1..64, one in four with N calls.  Random pairs score low, so that many diagonals tie and
    short ones reach no positive score at all: ``oracle.local_diagonal`` says which alignment the reference's aligner returns first.
    (pass, ref) are given, not computed: one read in two is an exact-miRNA row, the other an isomiR row."""
    rng = np.random.default_rng(1000 + seed)
    n_t = PAIRS_PER_SEED // 10
    lens = np.r_[np.arange(1, 33), np.repeat([18, 25, 26, 31, 32], 12)]
    targets = [rnd(rng, int(lens[(k + seed) % len(lens)])) for k in range(n_t)]
    seqs, ref = [], []
    for k in range(PAIRS_PER_SEED):
        L = 1 + (k * 7 + seed) % 64
        q = rnd(rng, L)
        if k % 4 == 3:
            for p in rng.integers(0, L, size=int(rng.integers(1, 4))):
                q = q[:p] + "N" + q[p + 1:]
        seqs.append(q); ref.append(k % n_t)
    assert {len(t) for t in targets} == set(range(1, 33)) and {len(q) for q in seqs} == set(range(1, 65))
    ps = np.where(np.arange(PAIRS_PER_SEED) % 2 == 0, 0, 8).astype(np.int8)
    counts = rng.integers(1, 50, size=(PAIRS_PER_SEED, 1))
    retained = rng.random(PAIRS_PER_SEED) < 0.7
    fam = np.arange(n_t)
    freq = np.array([1e300])
    rc, g = run_sim(sim, seqs, counts, ps, ref, fam, targets, retained, freq, chunk=64 + 64 * (seed % 3))
    assert rc == 0 and g["wide_members"] == 0 and min(g["n_chunks"]) > 1
    o = oracle.variant_tally(seqs, counts, ps, np.asarray(ref), fam, targets, retained, freq)
    assert_same(g, o)
    assert int(o["diag"].min()) <= -45 and int(o["diag"].max()) >= 20 and (o["state"] >= 0).all()  # (the ends: test_every_diagonal)


def test_every_diagonal(sim):
    """Every diagonal -63..31 as the answer, in both instances: the target is all G and the read all A but for one shared motif (C, CT or
    CTC) placed so that the only positive score lies on diagonal d -- at the first, a middle and the last place that d allows.  Then
    the same with the motif twice in the target, and twice in the read: two diagonals tie, and the alignment that ends first in the
    target, then first in the read, is returned."""
    targets, seqs, want = [], [], []
    for Lt, Lr in ((32, 64), (32, 33), (32, 32), (32, 31), (31, 64), (26, 47), (1, 64), (32, 1)):
        for d in range(-(Lr - 1), Lt):
            i_lo, i_hi = max(d, 0), min(Lt, d + Lr) - 1  # target bases on the diagonal
            for i in sorted({i_lo, (i_lo + i_hi) // 2, i_hi}):
                m = "CTC"[:min(3, i_hi - i + 1, 1 + (i + d) % 3)]
                t = "G" * i + m + "G" * (Lt - i - len(m))
                q = "A" * (i - d) + m + "A" * (Lr - (i - d) - len(m))
                targets.append(t); seqs.append(q); want.append(d)
                if i + 2 * len(m) + 1 <= Lt and len(m) < 3:  # the motif once more, further on in the target: a tie
                    t2 = t[:i + len(m) + 1] + m + t[i + 2 * len(m) + 1:]
                    targets.append(t2); seqs.append(q); want.append(d)
                j = i - d
                if j + 2 * len(m) + 1 <= Lr and len(m) < 3:  # ... or further on in the read: the same end in the target, first in the read
                    q2 = q[:j + len(m) + 1] + m + q[j + 2 * len(m) + 1:]
                    targets.append(t); seqs.append(q2); want.append(d)
    n = len(seqs)
    assert set(want) == set(range(-63, 32)) and all(len(t) <= 32 and len(q) <= 64 for t, q in zip(targets, seqs))
    ps = np.where(np.arange(n) % 2 == 0, 0, 8).astype(np.int8)
    counts = np.ones((n, 1), dtype=np.int64)
    freq = np.array([1.0])
    rc, g = run_sim(sim, seqs, counts, ps, np.arange(n), np.arange(n), targets, None, freq, chunk=64)
    assert rc == 0
    o = oracle.variant_tally(seqs, counts, ps, np.arange(n), np.arange(n), targets, None, freq)
    assert o["diag"].tolist() == want
    assert_same(g, o)


# ---------------------------------------------------------------------------------------------------------------
# the directed set: canonical sequences of 24..32 nt in precursors, every window around them, under the two miRNA policies
# ---------------------------------------------------------------------------------------------------------------
def directed_case(seed=2932):
    """-> dict: library (29 members), fam_of_ref, targets (27 families), raw reads with their sample ids (shuffled), and what the collapse
    of them must give (unique reads in order of first appearance, counts [U, 3]).

    Canonical sequences of 24..32 nt, three per length, each inside a precursor with 8 random flank bases per side.  One canonical each
    of 30 and 32 nt has a second library member, the canonical with its last two bases replaced, merged into the canonical's family;
    one member (a 27-nt one) has no family.  Reads: the windows precursor[8 + a : 8 + L + b], a in -3..3, b in -4..4 -- of the
    canonical's precursor and of the second members' -- each as it is, with a substitution (twice), with an N at base 5 and with
    one canonical A before Lt - 5 read as G; a few random reads of 70 and 300 nt.  Three samples, zero counts in some columns."""
    rng = np.random.default_rng(seed)
    canon, pre = [], []
    for L in range(24, 33):
        for _ in range(3):
            c = rnd(rng, L)
            canon.append(c); pre.append(rnd(rng, 8) + c + rnd(rng, 8))
    library, fam_of_ref, lib_pre = list(canon), list(range(len(canon))), list(pre)
    for L in (30, 32):
        f = next(k for k, c in enumerate(canon) if len(c) == L)
        tail = canon[f][-2:]
        new = "".join("ACGT"[("ACGT".index(b) + 1 + int(rng.integers(0, 3))) % 4] for b in tail)
        library.append(canon[f][:-2] + new); fam_of_ref.append(f)
        lib_pre.append(pre[f][:8] + library[-1] + pre[f][-8:])
    no_family = next(k for k, c in enumerate(canon) if len(c) == 27)
    fam_of_ref[no_family] = -1
    reads = []
    for r, (c, p) in enumerate(zip(library, lib_pre)):
        L = len(c)
        for a in range(-3, 4):
            for b in range(-4, 5):
                w = p[8 + a:8 + L + b]
                reads.append(w)
                for _ in range(2):
                    k = int(rng.integers(0, len(w)))
                    reads.append(w[:k] + "ACGT"[("ACGT".index(w[k]) + int(rng.integers(1, 4))) % 4] + w[k + 1:])
                reads.append(w[:5] + "N" + w[6:])
                apos = [q - a for q in range(L - 5) if c[q] == "A" and 0 <= q - a < len(w)]
                if apos:
                    k = apos[int(rng.integers(0, len(apos)))]
                    reads.append(w[:k] + "G" + w[k + 1:])
    reads += [rnd(rng, 70) for _ in range(6)] + [rnd(rng, 300) for _ in range(3)]
    uniq = list(dict.fromkeys(reads))
    cnt = rng.integers(1, 5, size=(len(uniq), 3)) * (rng.random((len(uniq), 3)) < 0.6)
    cnt[cnt.sum(axis=1) == 0, 1] = 1
    raw, sid = [], []
    for q, row in zip(uniq, cnt):
        for s in range(3):
            raw += [q] * int(row[s]); sid += [s] * int(row[s])
    order = rng.permutation(len(raw))
    raw, sid = [raw[k] for k in order], np.asarray(sid, dtype=np.int32)[order]
    first = {}
    for k, q in enumerate(raw):
        first.setdefault(q, k)
    useq = sorted(uniq, key=first.get)
    row_of = {q: k for k, q in enumerate(uniq)}
    counts = np.stack([cnt[row_of[q]] for q in useq]).astype(np.int64)
    retained = (rng.random(len(useq)) < 0.8).astype(np.uint8)
    return dict(library=library, canon=canon, fam_of_ref=np.asarray(fam_of_ref, dtype=np.int32), targets=canon, raw=raw, sid=sid,
                useq=useq, counts=counts, retained=retained, no_family=no_family)


def directed_annotation(case, useq=None):
    """(pass, ref) of ``oracle.cascade`` under the exact-miRNA and the isomiR policy, both on the one library"""
    data, off = _flat(case["useq"] if useq is None else useq)
    lib = _flat(case["library"])
    ps, ref, _, _ = oracle.cascade(data, off, [lib, lib], n_pass=2, policies=[EXACT_POL, ISO_POL])
    return ps, ref


def directed_coverage(case, useq, counts, ps, ref, o):
    """What the directed set is for, from the oracle's answers alone.  -> the figures, for the record."""
    fam = case["fam_of_ref"]
    lens = np.asarray([len(q) for q in useq])
    member = o["state"] >= 0
    long_m = member & (lens >= 32)
    fig = dict(reads=len(useq), members=int(member.sum()), long_accepted=int((long_m & (o["state"] == 1)).sum()),
               long_rejected=int((long_m & (o["state"] == 0)).sum()))
    assert fig["long_accepted"] >= 100 and fig["long_rejected"] >= 20, fig
    f_of = np.where(ps >= 0, fam[np.maximum(ref, 0)], -1)
    for L in (29, 30, 31, 32):
        fig[f"long_members_of_{L}"] = int(sum(long_m[i] and len(case["targets"][f_of[i]]) == L for i in np.nonzero(long_m)[0]))
        assert fig[f"long_members_of_{L}"] >= 5, fig
    cen = o["census"].reshape(len(case["targets"]), 32, -1)
    fig["census_col_26"] = int(cen[:, 26].sum())
    fig["census_cols_21_25"] = [int(cen[:, q].sum()) for q in range(21, 26)]
    assert fig["census_col_26"] > 0 and min(fig["census_cols_21_25"]) > 0, fig
    fig["through_merged_family"] = int((member & (ps >= 0) & (np.maximum(ref, 0) >= len(case["canon"]))).sum())
    fig["no_family"] = int(((ps >= 0) & (f_of < 0)).sum())
    gated = (ps == 1) & (f_of >= 0) & ~member
    fig["freq_gate"] = int(gated.sum())
    assert fig["through_merged_family"] >= 1 and fig["no_family"] >= 1 and fig["freq_gate"] >= 1, fig
    assert all(not any(float(counts[i, s]) * float(FREQ[s]) >= 1 for s in range(3)) for i in np.nonzero(gated)[0])
    fig["two_word_reads"] = int(((lens >= 32) & (lens <= 64)).sum())
    assert fig["two_word_reads"] > 2 * 256, fig  # (the runtime's chunks are multiples of 256 reads, one workgroup each)
    fig["kept_exact"] = int(o["kept_exact"].sum())
    fig["wide_unannotated"] = int(((lens > 64) & (ps < 0)).sum())
    assert fig["kept_exact"] > 0 and fig["wide_unannotated"] >= 9 and not ((lens > 64) & (ps >= 0)).any(), fig
    assert 8000 <= fig["reads"] <= 11000, fig
    return fig


@pytest.fixture(scope="module")
def directed():
    case = directed_case()
    ps, ref = directed_annotation(case)
    o = oracle.variant_tally(case["useq"], case["counts"], ps, ref, case["fam_of_ref"], case["targets"], case["retained"], FREQ,
                             exact_pass=0, iso_pass=1)
    return case, ps, ref, o


def test_directed_related_pairs(sim, directed):
    """The directed set under the annotation of ``oracle.cascade``: members of 32..35 nt in the two-word instance, merged families, a
    member without family, the frequency gate, census columns up to 26."""
    case, ps, ref, o = directed
    fig = directed_coverage(case, case["useq"], case["counts"], ps, ref, o)
    print("directed set:", fig)
    rc, g = run_sim(sim, case["useq"], case["counts"], ps, ref, case["fam_of_ref"], case["targets"], case["retained"], FREQ,
                    exact_pass=0, iso_pass=1)
    assert rc == 0 and g["wide_members"] == 0
    assert g["n_chunks"][1] > 1, g["n_chunks"]  # the two-word group: more than one member list
    assert_same(g, o)
    # the defaults: every reference its own family, every read retained
    o2 = oracle.variant_tally(case["useq"], case["counts"], ps, ref, np.arange(len(case["library"])), case["library"], None, FREQ,
                              exact_pass=0, iso_pass=1)
    rc, g2 = run_sim(sim, case["useq"], case["counts"], ps, ref, np.arange(len(case["library"])), case["library"], None, FREQ,
                     exact_pass=0, iso_pass=1, chunk=512, block=256)
    assert rc == 0
    assert_same(g2, o2, "defaults: ")


# ---------------------------------------------------------------------------------------------------------------
# table arithmetic
# ---------------------------------------------------------------------------------------------------------------
def _family_set(rng, n_reads=600):
    """a few families with close reads: (targets, library, fam_of_ref, reads, pass, ref)"""
    targets = [rnd(rng, L) for L in (19, 22, 22, 26, 30, 32)]
    library = list(targets) + [targets[4][:-3], targets[1][:-2] + "CA", rnd(rng, 21)]
    fam = [0, 1, 2, 3, 4, 5, 4, 1, -1]  # two references of different length in family 4; the last reference has no family
    reads, ps, ref = [], [], []
    for k in range(n_reads):
        r = int(rng.integers(0, len(library)))
        t = library[r]
        a, b = int(rng.integers(-2, 3)), int(rng.integers(-3, 4))
        q = rnd(rng, max(-a, 0)) + t[max(a, 0):len(t) + min(b, 0)] + rnd(rng, max(b, 0))
        for _ in range(int(rng.choice([0, 0, 1, 2]))):
            p = int(rng.integers(0, len(q)))
            q = q[:p] + "ACGTN"[int(rng.integers(0, 5))] + q[p + 1:]
        reads.append(q); ref.append(r); ps.append(0 if a == 0 and b == 0 and k % 3 else 8)
    return targets, library, np.asarray(fam), reads, np.asarray(ps, dtype=np.int8), np.asarray(ref)


@pytest.mark.parametrize("S", [1, 3, 5])
@pytest.mark.parametrize("masked", [False, True])
def test_tables(sim, S, masked):
    """Sample columns (zero counts, whole zero columns), the retained mask or none, the frequency gate at exactly 1.0 and just below it, references
    without family and two references of different length in one family."""
    rng = np.random.default_rng(77 + S)
    targets, library, fam, reads, ps, ref = _family_set(rng)
    n = len(reads)
    counts = rng.integers(1, 9, size=(n, S)) * (rng.random((n, S)) < 0.5)
    third, below = 1.0 / 3.0, np.nextafter(1.0 / 3.0, 0.0)
    assert 4 * 0.25 == 1.0 and 3 * third == 1.0 and 3 * below < 1.0 and 3 * 0.25 < 1.0
    # rows 0::5: count * freq == 1.0 exactly in column 0, nothing elsewhere: members.  rows 1::5: just below 1.0 in the last column: not.
    freq, at_one, zero_cols = {1: ([0.25], 4, []), 3: ([third, 0.25, below], 3, [1]),
                               5: ([0.25, third, 0.25, 0.25, below], 4, [2, 3])}[S]
    freq = np.asarray(freq)
    counts[0::5] = 0; counts[0::5, 0] = at_one; ps[0::5] = 8
    counts[1::5] = 0; counts[1::5, S - 1] = 3; ps[1::5] = 8
    if S == 5:
        counts[2::5] = 0; counts[2::5, 1] = 3; ps[2::5] = 8  # 3 * (1/3) == 1.0 in column 1
    counts[:, zero_cols] = 0                                  # samples in which nothing was counted
    retained = (rng.random(n) < 0.6) if masked else None
    rc, g = run_sim(sim, reads, counts, ps, ref, fam, targets, retained, freq, chunk=128)
    assert rc == 0
    o = oracle.variant_tally(reads, counts, ps, ref, fam, targets, retained, freq)
    assert_same(g, o)
    iso = ps == 8
    assert (g["state"][0::5][fam[ref[0::5]] >= 0] >= 0).all()          # count * freq == 1.0: members
    assert (g["state"][1::5] == -1).all()                                 # 3 * 0.25 and 3 * (just below 1/3) < 1: not members
    if S == 5:
        assert (g["state"][2::5][fam[ref[2::5]] >= 0] >= 0).all()        # 3 * (1/3) == 1.0: members
    for c in zero_cols:
        assert not g["n_seqs"][:, c].any() and not g["census"][..., c].any()
    assert all(g["n_seqs"][:, c].any() for c in range(S) if c not in zero_cols)
    assert (g["state"][iso & (fam[ref] < 0)] == -1).all() and (g["state"][fam[ref] < 0] == -1).all()
    assert g["n_seqs"][4].sum() > 0 and {len(library[r]) for r in ref[(fam[ref] == 4) & (g["state"] >= 0)]} == {30, 27}
    assert g["kept_exact"].sum() > 0 and g["canon"].sum() > 0 and (g["state"] == 0).any() and (g["state"] == 1).any()


def test_no_family_and_no_reads(sim):
    rng = np.random.default_rng(5)
    targets, library, fam, reads, ps, ref = _family_set(rng, 50)
    counts = rng.integers(1, 5, size=(50, 2))
    rc, g = run_sim(sim, reads, counts, ps, ref, np.full(len(library), -1), [], None, np.array([1e300, 1e300]))
    assert rc == 0 and (g["state"] == -1).all() and (g["diag"] == 0).all() and g["census"].size == 0
    o = oracle.variant_tally(reads, counts, ps, ref, np.full(len(library), -1), [], None, np.array([1e300, 1e300]))
    assert_same(g, o)
    rc, g = run_sim(sim, [], np.zeros((0, 2)), np.zeros(0), np.zeros(0), fam, targets, None, np.array([1.0, 1.0]))
    assert rc == 0 and g["diag"].size == 0 and not g["n_seqs"].any() and not g["census"].any()
    o = oracle.variant_tally([], np.zeros((0, 2), dtype=np.int64), np.zeros(0), np.zeros(0), fam, targets, None, np.array([1.0, 1.0]))
    assert_same(g, o)


def test_refusals_and_wide_members(sim):
    """What the runtime refuses, restated by the simulation: a canonical sequence of 33 nt, one with an N; and the member predicate over
    the reads that no instance of the kernel takes (more than 64 nt): a member among them is counted, never dropped in silence."""
    rng = np.random.default_rng(9)
    one = np.ones((1, 1))
    assert run_sim(sim, ["ACGTACGTACGTACGTACGT"], one, [0], [0], [0], [rnd(rng, 33)], None, [1.0])[0] == -6
    assert run_sim(sim, ["ACGTACGTACGTACGTACGT"], one, [0], [0], [0], ["ACGTNACGTACGTACGTACGT"], None, [1.0])[0] == -7
    t = rnd(rng, 30)
    reads = [rnd(rng, 20) + t + rnd(rng, 20), rnd(rng, 70), t, rnd(rng, 17) + t + rnd(rng, 17), rnd(rng, 18) + t + rnd(rng, 18)]
    ps, ref, fam = [8, -1, 0, 8, 8], [0, -1, 0, 0, 0], [0]
    counts = np.array([[1], [5], [2], [1], [0]])
    rc, g = run_sim(sim, reads, counts, ps, ref, fam, [t], None, [1.0])
    assert rc == 0 and g["wide_members"] == 1  # the 70-nt isomiR row; the 66-nt one has no count, the 64-nt one is tallied
    assert g["state"].tolist()[:3] == [-1, -1, 1] and g["state"][3] >= 0 and g["state"][4] == -1 and int(g["diag"][3]) == -17
    o = oracle.variant_tally(reads[1:4], counts[1:4], ps[1:4], np.asarray(ref[1:4]), fam, [t], None, [1.0])
    for k in ("diag", "state"):
        assert np.array_equal(g[k][1:4], o[k])
