"""``mirge_cluster_diagonals`` / ``mirge_cluster_pileup`` on random clusters against the brute-force restatement of
test_unmapped_features.py: diagonal, score, identity, flag, paddings and every tally, exactly; flagged rows through the host
twin to the text of the all-host route; one heavy cluster beside ten thousand small ones.  Seeds: MIRGE_FUZZ_SEEDS."""
import os

import numpy as np
import pytest

import mirge3_amd  # noqa: F401
from mirge3_amd import unmapped_features as uf
from test_unmapped_features import brute_arrays, brute_row

SEEDS = [int(x) for x in os.environ.get("MIRGE_FUZZ_SEEDS", "1,2,3").split(",") if x.strip()]
KEYS = ("diag", "score", "identity", "flag", "head", "tail", "col_off", "tally", "row_start")


@pytest.fixture(scope="module")
def gctx():
    from mirge3_amd import _ffi
    ctx = _ffi.Context(0)
    yield ctx
    ctx.close()


def rand(rng, n):
    return "".join("ACGT"[int(c)] for c in rng.integers(0, 4, n))


def window_read(rng, ext, flank, clen):
    """a window of w >= 16 columns of the cluster with up to 4 free bases past the window's ends in all and up to 2 substitutions
    (one of them may be an N).  On the window's own diagonal at least w - 2 bases match and at most 2 do not: the ungapped score
    is at least 2 * (w - 2) - 2 = 2 * w - 6.  The read has L <= w + 4 bases, so 2 * min(L, C) - 20 <= 2 * w - 12, which is less:
    no such row may be flagged"""
    free = int(rng.integers(0, 5))
    left = int(rng.integers(0, free + 1))
    a = int(rng.integers(0, max(1, clen - 16 + 1))) if rng.random() < 0.7 else 0
    b = int(rng.integers(min(clen, a + 16), clen + 1))
    lo, hi = (flank + a - left, flank + b + free - left) if rng.random() < 0.5 else (flank + a, flank + b)
    if rng.random() < 0.3:
        lo, hi = flank - left, flank + clen + (free - left)
    s = list(ext[lo:hi])
    for _ in range(int(rng.integers(0, 3))):
        k = int(rng.integers(0, len(s)))
        if s[k] == "N":
            continue
        s[k] = "N" if rng.random() < 0.2 else "ACGT"[("ACGT".index(s[k]) + 1 + int(rng.integers(0, 3))) % 4]
    return "".join(s)


def long_read(rng, ext, flank, clen):
    """45 to 64 nt (one in four exactly 64) over the whole of a 16-nt cluster: the overhang lies all in front, all behind or
    anywhere, so heads and tails of 40 and more occur; up to 2 substitutions inside the cluster's columns keep 2 * 16 - 6 > 12"""
    n = 64 if rng.random() < 0.25 else int(rng.integers(45, 65))
    side = rng.random()
    h = n - clen if side < 0.35 else 0 if side < 0.7 else int(rng.integers(0, n - clen + 1))
    s = list(ext[flank - h:flank - h + n])
    for _ in range(int(rng.integers(0, 3))):
        k = h + int(rng.integers(0, clen))
        if s[k] != "N":
            s[k] = "N" if rng.random() < 0.2 else "ACGT"[("ACGT".index(s[k]) + 1 + int(rng.integers(0, 3))) % 4]
    return "".join(s)


def fuzz_clusters(rng, n_clusters=60):
    out = []
    flank = 50
    for k in range(n_clusters):
        clen = 16 if k % 4 == 1 else int(rng.integers(16, 41))
        if k % 6 == 0:  # tandem: several diagonals reach the same score
            u = rand(rng, int(rng.integers(4, 9)))
            ext = (u * 40)[:clen + 2 * flank]
        else:
            ext = rand(rng, clen + 2 * flank)
        cseq = ext[flank:flank + clen]
        n = int(rng.integers(3, 401)) if k % 5 == 0 else int(rng.integers(3, 30))
        reads = [long_read(rng, ext, flank, clen) if k % 4 == 1 and rng.random() < 0.4 else window_read(rng, ext, flank, clen) for _ in range(n)]
        if k % 4 == 1:
            reads += [ext[flank - 48:flank + 16], ext[flank:flank + 64]]  # 64 nt with the whole overhang on one side
        if k % 6 == 0:
            reads += [(u * 12)[:int(rng.integers(16, 40))] for _ in range(3)]
        counts = [int(rng.integers(1, 1 << int(rng.integers(1, 41)))) for _ in reads]
        out.append((cseq, reads, counts))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_kernels_equal_brute_force(gctx, seed):
    rng = np.random.default_rng(seed)
    clusters = fuzz_clusters(rng)
    n_plain = sum(len(c[1]) for c in clusters)
    # rows built to fail the inequality: two segments of more than ten matches around an indel, and a read that shares nothing
    gapped = []
    while len(gapped) < 6:
        a = rand(rng, 40)
        if brute_row(a, a[1:14] + a[15:29])[1] >= 2 * 27 - 20:  # a repeat let the ungapped diagonal reach the gapped 34: not the case wanted
            continue
        gapped.append((a, [a[1:14] + a[15:29], a[0:30], a[4:40]], [5, 7, 9]))
    nothing = (a, [a[0:20], a[2:22], "N" * 18], [5, 7, 2])
    want = brute_arrays(None, clusters + gapped + [nothing])
    got = uf.device_arrays(gctx, clusters + gapped + [nothing])
    for k in KEYS:
        assert np.array_equal(np.asarray(want[k]), np.asarray(got[k])), k
    rs = want["row_start"]
    flagged_plain = int(np.count_nonzero(got["flag"][:n_plain]))
    ties = 0
    for cseq, reads, _ in clusters[::6]:
        for r in reads[-3:]:
            scores = {}
            for d in range(-(len(r) - 1), len(cseq)):
                h = top = 0
                for i in range(max(0, d), min(len(cseq), len(r) + d)):
                    h = max(0, h + (2 if cseq[i] == r[i - d] else -1))
                    top = max(top, h)
                scores[d] = top
            ties += sum(1 for v in scores.values() if v == max(scores.values())) > 1
    lens = [len(r) for c in clusters for r in c[1]]
    assert max(lens) == 64 and min(lens) == 16 and sum(1 for n in lens if n >= 45) >= 50
    assert int(got["head"].max()) >= 40 and int(got["tail"].max()) >= 40  # the paddings the LDS rows and columns are sized for
    print(f"\n[features fuzz {seed}] {n_plain} rows, {flagged_plain} flagged outside the built cases, {ties} rows with tied diagonals")
    assert ties >= 3
    assert flagged_plain <= n_plain // 100  # the cap: a kernel that flags everything cannot pass through the host route
    for k in range(len(clusters), len(clusters) + len(gapped)):
        f = got["flag"][rs[k]:rs[k + 1]]
        assert f.tolist() == [1, 0, 0]
    assert got["flag"][rs[-2]:rs[-1]].tolist() == [0, 0, 3]
    # the flagged clusters through the host twin: the same piles as the all-host route; the others: diagonal pile == string pile
    piles, flagged, fallback = uf.piles_from_arrays(clusters + gapped, {k: got[k] for k in KEYS})
    assert flagged == flagged_plain + 6 and fallback >= 18
    assert all("-" in p.rows[1].strip("-") for p in piles[-6:])  # the gap won: a gapped row
    for (cseq, reads, counts), p in list(zip(clusters + gapped, piles))[::7] + list(zip(gapped, piles[-6:])):
        q = uf.string_pile(cseq, reads, counts)
        assert (p.rows, p.exact, [tuple(t) for t in p.tally]) == (q.rows, q.exact, [tuple(t) for t in q.tally])
    with pytest.raises(ValueError):
        uf.string_pile(*nothing)  # the read that shares nothing with its cluster: the reference stops there as well


@pytest.mark.gpu
def test_one_heavy_cluster_beside_ten_thousand_small_ones(gctx):
    rng = np.random.default_rng(SEEDS[0])
    small, small_ext = [], []
    for _ in range(10000):
        ext = rand(rng, 24 + 16)
        small_ext.append((ext,))
        small.append((ext[8:32], [ext[8:32], ext[6:30], ext[10:34]], [int(x) for x in rng.integers(1, 1 << 40, 3)]))
    ext = rand(rng, 30 + 16)
    starts, lens = rng.integers(0, 12, 200000), rng.integers(16, 31, 200000)
    heavy = (ext[8:38], [ext[int(a):int(a) + int(n)] for a, n in zip(starts, lens)], [int(x) for x in rng.integers(1, 1 << 40, 200000)])
    clusters = small[:5000] + [heavy] + small[5000:]
    got = uf.device_arrays(gctx, clusters)
    assert not got["flag"].any()
    # the heavy cluster in numpy (its rows are exact windows: the diagonal is where the window was cut), the small ones by brute force
    k = 5000
    a, b = int(got["row_start"][k]), int(got["row_start"][k + 1])
    overlap = np.minimum(30, starts - 8 + lens) - np.maximum(0, starts - 8)  # identity counts the columns shared with the cluster
    assert np.array_equal(got["diag"][a:b], starts - 8) and np.array_equal(got["identity"][a:b], overlap)
    assert (int(got["head"][k]), int(got["tail"][k])) == (8, int((starts + lens).max()) - 38)
    tab = np.zeros((8 + 30 + int(got["tail"][k]), 5), dtype=np.int64)
    code = {c: i for i, c in enumerate("ATCG")}
    col = np.array([code[c] for c in ext], dtype=np.int64)
    cnt = np.array(heavy[2], dtype=np.int64)
    for j in range(30):
        m = lens > j
        np.add.at(tab, (starts[m] + j, col[starts[m] + j]), cnt[m])
    assert np.array_equal(got["tally"][int(got["col_off"][k]):int(got["col_off"][k + 1])], tab)
    # the small clusters are the cluster, the window 2 in front and the window 2 behind: diagonals 0, -2, 2, every score twice the
    # overlap, paddings 2 and 2, and the tallies in closed form over all ten thousand
    idx = np.array([i for i in range(len(clusters)) if i != k])
    rows = got["row_start"][idx][:, None] + np.arange(3)[None, :]
    assert np.array_equal(got["diag"][rows], np.tile(np.array([0, -2, 2], np.int32), (10000, 1)))
    assert np.array_equal(got["identity"][rows], np.tile(np.array([24, 22, 22], np.int32), (10000, 1)))
    assert np.array_equal(got["score"][rows], 2 * got["identity"][rows])
    assert np.array_equal(got["score"][a:b], 2 * overlap)
    assert (got["head"][idx] == 2).all() and (got["tail"][idx] == 2).all()
    assert np.array_equal(np.diff(got["col_off"])[idx], np.full(10000, 28))
    text = np.array([[code[c] for c in s[0][6:34]] for s in (s_ext for s_ext in small_ext)], dtype=np.int64)  # columns -2 .. 25
    cnts = np.array([c[2] for c in small], dtype=np.int64)
    want = np.zeros((10000, 28, 5), dtype=np.int64)
    cols = np.arange(28)
    for r, (lo, hi) in enumerate(((2, 26), (0, 24), (4, 28))):
        m = (cols >= lo) & (cols < hi)
        np.add.at(want, (np.arange(10000)[:, None], cols[m][None, :], text[:, m]), cnts[:, r][:, None])
    starts_col = got["col_off"][idx]
    gotten = got["tally"][(starts_col[:, None] + cols[None, :])]
    assert np.array_equal(gotten, want)
