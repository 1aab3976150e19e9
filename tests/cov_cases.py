"""The shared inputs of the ``--coverage`` tests (CPU restatement, host simulation of the kernels, GPU) and what they must give: the
runs of a per-base brute force written here -- every covered base of a (strand, chromosome) listed, its depth summed, the bases
run-length encoded.  A case: ``name -> (intervals, names)``; ``intervals`` = dict of the five arrays of ``mirge_coverage_runs``
(rank int32, start int64, len int32, weight uint32, minus uint8), ``names[rank]`` = the chromosome names for the text."""
import functools

import numpy as np

MAX_END = 2 ** 31 - 1


def make(rows):
    """rows: (rank, start, len, weight, minus)"""
    cols = list(zip(*rows)) if rows else [[], [], [], [], []]
    return dict(rank=np.asarray(cols[0], dtype=np.int32), start=np.asarray(cols[1], dtype=np.int64), len=np.asarray(cols[2], dtype=np.int32),
                weight=np.asarray(cols[3], dtype=np.uint32), minus=np.asarray(cols[4], dtype=np.uint8))


def brute(iv, stranded):
    """dict(strand, chrom, start, end, depth) in file order: plus strand first, then chromosome rank, then start"""
    out = dict(strand=[], chrom=[], start=[], end=[], depth=[])
    strand = iv["minus"].astype(np.int64) if stranded else np.zeros(iv["rank"].size, np.int64)
    group = strand * (1 << 32) + iv["rank"].astype(np.int64)
    for g in np.unique(group):
        pick = np.flatnonzero(group == g)
        start, ln, w = iv["start"][pick], iv["len"][pick].astype(np.int64), iv["weight"][pick].astype(np.int64)
        first = np.cumsum(ln) - ln
        bases = np.repeat(start, ln) + (np.arange(int(ln.sum()), dtype=np.int64) - np.repeat(first, ln))  # every base of every interval
        pos, inv = np.unique(bases, return_inverse=True)
        depth = np.zeros(pos.size, dtype=np.int64)
        np.add.at(depth, inv, np.repeat(w, ln))
        cut = np.flatnonzero((np.diff(pos) != 1) | (np.diff(depth) != 0)) + 1
        a, b = np.concatenate([[0], cut]), np.concatenate([cut, [pos.size]])
        out["strand"].append(np.full(a.size, g >> 32, dtype=np.uint8))
        out["chrom"].append(np.full(a.size, g & 0xFFFFFFFF, dtype=np.int32))
        out["start"].append(pos[a]); out["end"].append(pos[b - 1] + 1); out["depth"].append(depth[a])
    types = dict(strand=np.uint8, chrom=np.int32, start=np.int64, end=np.int64, depth=np.int64)
    return {k: (np.concatenate(v) if v else np.zeros(0)).astype(types[k]) for k, v in out.items()}


def text(runs, names, strand=None):
    rows = zip(runs["strand"].tolist(), runs["chrom"].tolist(), runs["start"].tolist(), runs["end"].tolist(), runs["depth"].tolist())
    return "".join("%s\t%d\t%d\t%d\n" % (names[c], s, e, d) for st, c, s, e, d in rows if strand is None or st == strand).encode()


def _random(seed, n, n_chrom, chrom_len, max_len, weights):
    rng = np.random.Generator(np.random.PCG64(seed))
    ln = rng.integers(1, max_len + 1, size=n)
    start = rng.integers(0, chrom_len, size=n)
    ln = np.minimum(ln, chrom_len - start)
    return dict(rank=rng.integers(0, n_chrom, size=n).astype(np.int32), start=start.astype(np.int64), len=ln.astype(np.int32),
                weight=rng.choice(np.asarray(weights, dtype=np.uint32), size=n), minus=rng.integers(0, 2, size=n).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def all_cases():
    W = 2 ** 32 - 1
    c = {}
    c["empty"] = make([])
    c["one"] = make([(0, 5, 7, 3, 0)])
    c["abut_equal"] = make([(0, 0, 10, 3, 0), (0, 10, 10, 3, 1)])
    c["abut_unequal"] = make([(0, 0, 10, 3, 0), (0, 10, 10, 4, 0)])
    c["nested_shared_ends"] = make([(0, 10, 40, 1, 0), (0, 20, 10, 2, 0), (0, 10, 10, 1, 1), (0, 40, 10, 5, 0), (0, 10, 40, 1, 0), (0, 25, 1, 1, 1)])
    # a ends where b and c start, w_a = w_b + w_c: the boundary at 10 cancels, then b ends where d starts with w_b = w_d: 20 cancels too
    c["cancel_chain"] = make([(1, 0, 10, 5, 0), (1, 10, 10, 2, 0), (1, 10, 25, 3, 0), (1, 20, 5, 2, 0), (1, 35, 5, 3, 1)])
    c["many_equal"] = make([(1, 100, 30, 1, 0)] * 10000)
    # [.., p) on chromosome k and [p, ..) on chromosome k + 1; ranks 0, 1, 4, 6 and the last one (9) stay empty
    c["chrom_boundary"] = (make([(2, 40, 10, 2, 0), (3, 50, 10, 2, 0), (5, 0, 3, 1, 1), (7, 60, 1, 1, 0), (8, 61, 1, 1, 0), (3, 60, 5, 3, 1)]),
                           ["chr%d" % k for k in range(10)])
    # plus and minus over the same bases; unstranded, [0, 10) + and [10, 20) - become one stretch, and 30..40 sums to the depth of 40..50
    c["strands"] = make([(0, 0, 10, 2, 0), (0, 10, 10, 2, 1), (0, 30, 10, 1, 0), (0, 30, 10, 2, 1), (0, 40, 10, 3, 0), (1, 5, 20, 4, 0), (1, 5, 20, 4, 1)])
    c["large_weights"] = make([(0, 7, 1, W, 0), (0, 7, 1, W, 1), (0, 7, 1, W, 0), (0, 6, 3, 1, 0)])
    c["extreme_positions"] = make([(0, 0, 5, 1, 0), (1, MAX_END - 4, 4, 2, 1), (1, MAX_END - 1, 1, 1, 0), (2, 0, 1, 1, 0)])
    for n in (255, 256, 257):
        c["count_%d" % n] = _random(1000 + n, n, 3, 2000, 40, [1, 1, 2, 3])
    c["count_65537"] = _random(65537, 65537, 4, 60000, 30, [1, 1, 1, 2, 7])
    c["fuzz"] = _random(20260, 2000, 3, 500, 64, [1, 1, 1, 2, 2, 3, 4, 5, 5, 1000])
    # digits: 9 -> 10 and 99 999 -> 100 000 in start, end and depth; names of 1 and 40 characters
    c["text"] = (make([(0, 8, 1, 9, 0), (0, 9, 1, 10, 0), (0, 99998, 1, 99999, 0), (0, 99999, 1, 100000, 1), (0, 100000, 1, 1, 0),
                       (1, 9, 1, 99999, 1), (1, 10, 99989, 100000, 0), (1, 99999, 2, 9, 1)]), ["c", "chromosome_with_a_name_of_forty_letters_"])
    out = {}
    for k, v in c.items():
        iv, names = v if isinstance(v, tuple) else (v, None)
        n_rank = int(iv["rank"].max()) + 1 if iv["rank"].size else 1
        out[k] = (iv, names if names is not None else ["chr%d" % r for r in range(n_rank)])
    assert len(out["text"][1][1]) == 40
    return out


@functools.lru_cache(maxsize=None)
def expected(name, stranded):
    return brute(all_cases()[name][0], stranded)
