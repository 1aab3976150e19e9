"""The cases of the ``--umi-cluster directional`` kernels, shared by the host build (tests/test_umi_cluster_hostsim.py) and the GPU test
(tests/test_umi_cluster_gpu.py); no test in here.  A case is ``(name, reads, counts, f, b)``: distinct UMI-tagged reads in the order they
first appeared (a read's first index is its position), their counts, and the UMI layout.  ``expected(case)`` is the restatement's founder
flags (tests/umi_restate.py, which also runs UMI-tools' sequential search both ways on the case), computed once per case."""
import functools

import numpy as np

import umi_restate

LAYOUTS = [(4, 4), (0, 12), (12, 0), (16, 16)]
LENGTHS = [31, 32, 33, 34, 63, 64, 65, 66, 127, 128, 129, 130]  # a `back` UMI straddles a packed word; the storage groups change at 32, 65, 129


def rand_seq(rng, n):
    return "".join("ACGT"[x] for x in rng.integers(0, 4, n))


def mutate(s, p, step=1):
    return s[:p] + "ACGT"[("ACGT".index(s[p]) + step) % 4] + s[p + 1:]


def threshold_case():
    """c(a) = 2 c(v) - 1 is an edge, 2 c(v) - 2 is none, for c(v) in 1, 2, 3, 1000 and 2^31 (2 c(v) - 1 = 2^32 - 1: a 32-bit product wraps).
    c(v) = 1 has no second half: 2 c(v) - 2 = 0 and no read has count 0.  Every pair has an insert of its own."""
    rng = np.random.default_rng(3)
    reads, counts = [], []
    for cv in (1, 2, 3, 1000, 2 ** 31):
        for ca in (2 * cv - 1, 2 * cv - 2):
            if ca < 1:
                continue
            v = rand_seq(rng, 28)
            reads += [v, mutate(v, 2)]
            counts += [cv, ca]
    return "threshold", reads, counts, 4, 4


def non_edge_case():
    rng = np.random.default_rng(4)
    f, b = 4, 4
    reads, counts = [], []

    def add(*pairs):
        for r, c in pairs:
            reads.append(r); counts.append(c)
    t = rand_seq(rng, 30)
    add((t, 9), (t[:4] + mutate(mutate(t[4:-4], 0), 7) + t[-4:], 1))   # the same UMI, another insert
    t = rand_seq(rng, 30)
    add((t, 9), (mutate(t, 4), 1), (mutate(t, 25), 1), (mutate(t, 12), 1))  # one difference inside the insert (its first, last, a middle letter)
    t = rand_seq(rng, 30)
    add((t, 9), (mutate(mutate(t, 0), 29), 1), (mutate(mutate(t, 1), 2), 1))  # two UMI differences
    t = rand_seq(rng, 30)
    add((t, 9), (t + "A", 1), (t[:-1], 1), (t[1:], 1))  # equal but for the length
    t = rand_seq(rng, 30)
    add((t, 9), (t[:1] + "N" + t[2:], 1), (t[:13] + "N" + t[14:], 1))  # a neighbour but for an N; an N in the insert
    t = rand_seq(rng, 30)
    add((t[:2] + "N" + t[3:], 9), (mutate(t[:2] + "N" + t[3:], 0), 1))  # two reads with an N, one UMI letter apart
    for L in (255, 256, 257, 300):  # 256 nt is the last eligible length (the long storage class holds it); 257 and beyond stand alone
        t = rand_seq(rng, L)
        add((t, 9), (mutate(t, 1), 1), (mutate(t, L - 1), 2))
    t = rand_seq(rng, 8)
    add((t, 9), (mutate(t, 3), 1), (mutate(t, 4), 3))  # len = f + b: an empty insert, every letter is UMI
    t = rand_seq(rng, 7)
    add((t, 9), (mutate(t, 0), 1))  # len < f + b: not eligible
    return "non_edges", reads, counts, f, b


def layout_case(f, b):
    """per tagged length: a centre, a one-letter variant at every end of the UMI region (edges), and variants of the insert's letters
    next to the UMI (no edges), counts on both sides of the threshold"""
    rng = np.random.default_rng(100 * f + b)
    reads, counts = [], []
    for L in LENGTHS:
        if L < f + b:
            continue
        t = rand_seq(rng, L)
        reads.append(t); counts.append(7)
        pos = sorted(set(p for p in ([0, f - 1] if f else []) + ([L - b, L - 1] if b else []) + [p for p in (31, 32, 63, 64, 95, 96, 127, 128) if p < f or L - b <= p < L]))
        for k, p in enumerate(pos):
            reads.append(mutate(t, p)); counts.append((1, 4, 13, 2)[k % 4])
            reads.append(mutate(t, p, 2)); counts.append((14, 1, 3, 1)[k % 4])
        for p in sorted({f, L - b - 1}):
            if f <= p < L - b:
                reads.append(mutate(t, p, 3)); counts.append(1)
    assert len(set(reads)) == len(reads)
    return f"layout_{f}_{b}", reads, counts, f, b


def hamming(a, b):
    return sum(x != y for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def induced_path(n=600, k=16, seed=11):
    """a self-avoiding walk in the Hamming graph of k-letter UMIs in which a step is rejected when it comes within distance 1 of any
    earlier node but the last: node i is a neighbour of i - 1 and i + 1 only"""
    rng = np.random.default_rng(seed)
    path = [rand_seq(rng, k)]
    arr = np.frombuffer(path[0].encode(), np.uint8)[None, :].copy()
    while len(path) < n:
        cand = mutate(path[-1], int(rng.integers(0, k)), int(rng.integers(1, 4)))
        c = np.frombuffer(cand.encode(), np.uint8)
        d = (arr != c).sum(axis=1)
        if (d[:-1] <= 1).any() or d[-1] != 1:
            continue
        path.append(cand)
        arr = np.vstack([arr, c])
    return tuple(path)


def chain_cases():
    f, b = 8, 8
    umis = list(induced_path())
    insert = "ACGTTGCAAGGCTTAACCGGAT"
    reads = [u[:f] + insert + u[f:] for u in umis]
    out = [("chain_alone", reads, [1] * len(reads), f, b)]
    # a count-2 read adjacent to the far end only: a letter of the last UMI changed so that no other path node is within distance 1
    last = umis[-1]
    big = None
    for p in range(16):
        for s in (1, 2, 3):
            c = mutate(last, p, s)
            if all(hamming(c, u) > 1 for u in umis[:-1]):
                big = c
                break
        if big:
            break
    assert big is not None
    out.append(("chain_big_end", reads + [big[:f] + insert + big[f:]], [1] * len(reads) + [2], f, b))
    perm = np.random.default_rng(5).permutation(len(reads))
    while not 100 < int(perm[0]) < 500:  # the earliest member is in the middle of the path
        perm = np.roll(perm, 1)
    out.append(("chain_shuffled", [reads[i] for i in perm], [1] * len(reads), f, b))
    return out


def heavy_case():
    """one insert with 5 000 UMIs within distance 2 of 40 centres (dense neighbourhoods, counts 1..50) beside 3 000 inserts of 1..3 UMIs"""
    rng = np.random.default_rng(21)
    f, b = 0, 12
    insert = rand_seq(rng, 22)
    centres = [rand_seq(rng, 12) for _ in range(40)]
    seen, reads, counts = set(), [], []
    while len(reads) < 5000:
        u = centres[int(rng.integers(0, 40))]
        for _ in range(int(rng.integers(0, 3))):
            u = mutate(u, int(rng.integers(0, 12)), int(rng.integers(1, 4)))
        if u in seen:
            continue
        seen.add(u)
        reads.append(insert + u); counts.append(int(rng.integers(1, 51)))
    small = set()
    while len(small) < 3000:
        small.add(rand_seq(rng, int(rng.integers(16, 30))))
    for ins in sorted(small):
        u = rand_seq(rng, 12)
        for k in range(int(rng.integers(1, 4))):
            r = ins + (u if k == 0 else mutate(u, int(rng.integers(0, 12)), k))
            if r not in seen:
                seen.add(r); reads.append(r); counts.append(int(rng.integers(1, 4)))
    order = rng.permutation(len(reads))
    return "heavy", [reads[i] for i in order], [counts[i] for i in order], f, b


def collisions_case():
    """2 000 tagged reads for MIRGE_TEST_UMI_HASH_BITS=6: 64 hash values, every probe walks through strangers"""
    rng = np.random.default_rng(33)
    f, b = 4, 4
    seen, reads, counts = set(), [], []
    while len(reads) < 2000:
        if reads and rng.integers(0, 3):
            t = reads[int(rng.integers(0, len(reads)))]
            p = int(rng.integers(0, len(t)))
            r = mutate(t, p, int(rng.integers(1, 4)))
        else:
            r = rand_seq(rng, int(rng.integers(24, 40)))
        if r in seen:
            continue
        seen.add(r); reads.append(r); counts.append(int(rng.choice([1, 1, 1, 2, 3, 5, 20])))
    return "collisions", reads, counts, f, b


def nothing_eligible_case():
    rng = np.random.default_rng(8)
    reads = [rand_seq(rng, 10) + "N" + rand_seq(rng, 12) for _ in range(5)] + [rand_seq(rng, 5), rand_seq(rng, 300)]
    reads.append(mutate(reads[-1], 0))
    return "nothing_eligible", reads, [1, 2, 3, 1, 1, 4, 2, 1], 4, 4


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = [threshold_case(), non_edge_case()] + [layout_case(f, b) for f, b in LAYOUTS] + chain_cases() + \
            [heavy_case(), collisions_case(), ("empty", [], [], 4, 4), nothing_eligible_case()]
    return {c[0]: c for c in cases}


@functools.lru_cache(maxsize=None)
def expected(name):
    _, reads, counts, f, b = all_cases()[name]
    return np.asarray(umi_restate.founders(reads, counts, list(range(len(reads))), f, b), dtype=np.uint8)


def path_length(reads, f, b):
    """the longest shortest path inside the count-1 graph of `reads`, from its first read, by breadth-first search"""
    _, adj = umi_restate.neighbours(reads, f, b)
    dist = {0: 0}
    q = [0]
    for a in q:
        for v in adj[a]:
            if v not in dist:
                dist[v] = dist[a] + 1
                q.append(v)
    return max(dist.values()), len(dist), max(len(a) for a in adj)
