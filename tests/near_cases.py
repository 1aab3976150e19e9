"""The named cases of ``--unmapped-nearest``: the smallest shapes at which the kernels can go wrong, shared by the CPU tests, the host
simulation and the GPU tests.  A case is ``dict(name, hairpins, queries, expect)``; ``expect`` maps a query's index to what the
specification gives by hand -- ``(D, hairpin, s, e)`` or a predicate on that tuple -- and tests/test_nearest.py holds the restatement to it.
``random_sets()`` is the random set: 300 queries over 30 libraries."""
import random

NO_HIT = (-1, -1, -1, -1)


def rnd_seq(rng: random.Random, n: int, letters: str = "ACGT") -> str:
    return "".join(rng.choice(letters) for _ in range(n))


def substitute(rng: random.Random, s: str, positions) -> str:
    out = list(s)
    for p in positions:
        out[p] = rng.choice([c for c in "ACGT" if c != out[p]])
    return "".join(out)


def _cases():
    rng = random.Random(20261021)
    out = []
    H = rnd_seq(rng, 150)
    # ---- the lengths around both instances' bounds; 11 and 65 are skipped
    lens = (11, 12, 31, 32, 33, 63, 64, 65)
    out.append(dict(name="lengths", hairpins=[H], queries=[H[40:40 + n] for n in lens],
                    expect={i: (NO_HIT if n in (11, 65) else (0, 0, 40, 40 + n)) for i, n in enumerate(lens)}))
    # ---- an exact hit, one substitution, one insertion, one deletion
    G = rnd_seq(rng, 80)
    q = G[20:44]
    ins = q[:11] + ("A" if q[11] != "A" and q[10] != "A" else ("C" if q[11] != "C" and q[10] != "C" else "G")) + q[11:]
    out.append(dict(name="edits", hairpins=[G], queries=[q, substitute(rng, q, [9]), ins, q[:13] + q[14:]],
                    expect={0: (0, 0, 20, 44), 1: (1, 0, 20, 44), 2: lambda r: r[0] == 1 and r[1] == 0 and r[3] == 44,
                            3: lambda r: r[0] == 1 and r[1] == 0 and r[3] == 44}))
    # ---- at a hairpin's first base and at its last
    out.append(dict(name="first_and_last_base", hairpins=[rnd_seq(rng, 30), G], queries=[G[:20], G[-20:], G[:33], G[-33:]],
                    expect={0: (0, 1, 0, 20), 1: (0, 1, 60, 80), 2: (0, 1, 0, 33), 3: (0, 1, 47, 80)}))
    # ---- a hairpin shorter than the query, a hairpin of one base, an empty hairpin
    short = "ACGTTGCATG"
    out.append(dict(name="short_hairpins", hairpins=["", short, "A", ""], queries=["GG" + short + "TTCC", "T" * 12, "C" * 40],
                    expect={0: (6, 1, 0, 10), 1: lambda r: r[0] == 9 and r[1] == 1, 2: lambda r: r[0] == 38 and r[1] == 1}))
    out.append(dict(name="one_base_library", hairpins=["", "A"], queries=["ACGTACGTACGT", "CCCCCCCCCCCCC"],
                    expect={0: (11, 1, 0, 1), 1: (13, 1, 0, 1)}))
    out.append(dict(name="library_without_a_base", hairpins=["", ""], queries=["ACGTACGTACGT"], expect={0: NO_HIT}))
    out.append(dict(name="no_hairpin", hairpins=[], queries=["ACGTACGTACGT"], expect={0: NO_HIT}))
    # ---- the tail of hairpin i followed by the head of hairpin i + 1: no state crosses the boundary
    A, B = rnd_seq(rng, 40), rnd_seq(rng, 40)
    out.append(dict(name="across_a_boundary", hairpins=[A, B], queries=[A[-10:] + B[:10], A[-17:] + B[:17]],
                    expect={0: lambda r: r[0] > 0, 1: lambda r: r[0] > 0}))
    # ---- two identical hairpins: the lower index
    out.append(dict(name="identical_hairpins", hairpins=[B, G, G, A], queries=[G[5:30], substitute(rng, G[30:70], [7, 22])],
                    expect={0: (0, 1, 5, 30), 1: (2, 1, 30, 70)}))
    # ---- a repeat inside one hairpin: the smallest end
    unit = rnd_seq(rng, 18)
    R = rnd_seq(rng, 9) + unit + rnd_seq(rng, 11) + unit + rnd_seq(rng, 7)
    out.append(dict(name="repeat_in_a_hairpin", hairpins=[R], queries=[unit], expect={0: (0, 0, 9, 27)}))
    # ---- a shorter and a longer substring tie (the first letter deleted, or substituted): the largest start
    core = G[30:50]
    wrong = next(c for c in "ACGT" if c != G[29])
    out.append(dict(name="largest_start", hairpins=[G], queries=[wrong + core], expect={0: (1, 0, 30, 50)}))
    # ---- N in the read, N in the hairpin: N matches nothing, not even N
    GN = G[:35] + "N" + G[36:]
    out.append(dict(name="n_letters", hairpins=[G, GN], queries=[G[20:25] + "N" + G[26:44], G[30:35] + "N" + G[36:48], "N" * 12],
                    expect={0: (1, 0, 20, 44), 1: (1, 0, 30, 48), 2: lambda r: r[0] == 12}))
    # ---- D = cap and D = cap + 1 at m = 16, 23, 24, 64 (K = 3: caps 2, 2, 3, 3; K = 8: 2, 2, 3, 8)
    C = rnd_seq(rng, 140)
    spread = lambda m, k: [int((i + 0.5) * m / k) for i in range(k)]
    qs, ex = [], {}
    for m, ks in ((16, (2, 3)), (23, (2, 3)), (24, (3, 4)), (64, (3, 4, 8, 9))):
        for k in ks:
            ex[len(qs)] = (lambda k: lambda r: r[0] == k and r[1] == 0)(k)
            qs.append(substitute(rng, C[50:50 + m], spread(m, k)))
    out.append(dict(name="caps", hairpins=[C], queries=qs, expect=ex))
    # ---- poly-A against poly-A
    out.append(dict(name="poly_a", hairpins=["A" * 50, "A" * 70], queries=["A" * 20, "A" * 64, "A" * 19 + "C"],
                    expect={0: (0, 0, 0, 20), 1: (0, 1, 0, 64), 2: (1, 0, 0, 19)}))
    # ---- 40 hairpins, with MIRGE_NEAR_CHUNK_BASES=64 some twenty chunks: the best hit in the last hairpin of the last chunk
    many = [rnd_seq(rng, rng.randint(20, 44)) for _ in range(39)] + [G[:41]]
    out.append(dict(name="forty_hairpins", hairpins=many, queries=[G[3:40], substitute(rng, G[1:41], [20]), many[17][2:18]],
                    expect={0: (0, 39, 3, 40), 1: (1, 39, 1, 41), 2: lambda r: r[0] == 0 and r[1] <= 17}))
    # ---- a hairpin longer than a workgroup's LDS stretch (4096 codes): read from global memory, a chunk of its own between two others
    long_h = rnd_seq(rng, 4500)
    out.append(dict(name="long_hairpin", hairpins=[A, long_h, B], queries=[long_h[4300:4340], B[3:30], A[:15], substitute(rng, long_h[10:70], [30])],
                    expect={0: (0, 1, 4300, 4340), 1: (0, 2, 3, 30), 2: (0, 0, 0, 15), 3: (1, 1, 10, 70)}))
    return out


CASES = _cases()


def edit(rng: random.Random, s: str, n: int) -> str:
    for _ in range(n):
        kind, p = rng.randrange(3), rng.randrange(len(s) + 1)
        if kind == 0 and p < len(s):
            s = s[:p] + rng.choice("ACGT") + s[p + 1:]
        elif kind == 1:
            s = s[:p] + rng.choice("ACGTN" if rng.random() < 0.1 else "ACGT") + s[p:]
        elif p < len(s) and len(s) > 1:
            s = s[:p] + s[p + 1:]
    return s


def random_sets(seed: int = 7, n_sets: int = 30, per_set: int = 10):
    """[(hairpins, queries)]: libraries of 1 to 6 hairpins of 1 to 120 nt; three quarters of the queries are library substrings with 0 to 5
    random edits, the rest random"""
    rng = random.Random(seed)
    out = []
    for _ in range(n_sets):
        hairpins = [rnd_seq(rng, rng.randint(1, 120), "ACGTN" if rng.random() < 0.15 else "ACGT") for _ in range(rng.randint(1, 6))]
        queries = []
        for _ in range(per_set):
            fit = [h for h in hairpins if len(h) >= 12]
            if fit and rng.random() < 0.75:
                h = rng.choice(fit)
                n = rng.randint(12, min(64, len(h)))
                at = rng.randrange(len(h) - n + 1)
                queries.append(edit(rng, h[at:at + n], rng.randint(0, 5)))
            else:
                queries.append(rnd_seq(rng, rng.randint(10, 66)))
        out.append((hairpins, queries))
    return out
