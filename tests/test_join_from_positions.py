"""The count join finds a miRNA read's reference from its POSITION (kernels_join.hpp, JoinGroups::from_pos) and the bulk
group's k_resolve runs behind the join's tables (native_ctx.hpp, PendingResolve); the tiny read groups' cascades are kept off
the stream of a k_cascade_fused group (native_collapse.hpp, small_group_slots).

Yardstick everywhere: numpy on what ``res.fetch()`` returns after the call -- pass, reference and count of every unique
read -- never the join's own output.  All comparisons are exact integer equality.
"""
import numpy as np
import pytest

import oracle
from helpers import oracle_libs_from
import mirge3_amd  # noqa: F401
from mirge3_amd import _ffi, synth
from mirge3_amd.cascade import Cascade, EXACT_PASS, ISO_PASS
from mirge3_amd.seqio import FlatSeqs, Library

pytestmark = pytest.mark.gpu

GRANULE = 16  # positions per entry of the resolve table (MIRGE_COARSE_SHIFT = 4)

# The first references of the miRNA library, by length.  A reference takes its length plus one separator position, so the
# starts are 0, 17, 40, 63, 104, 129, 136, 142, 143, 152, 160, 183: granule 1 (positions 16-31) holds ONE start at offset 1,
# granule 3 one at offset 15, granules 4, 5 and 7 none (code 16), granule 8 FOUR (code 17: references of 6, 5, 0 and 8 nt);
# reference 4 ends on position 127, the last of granule 7; reference 10 starts on a granule's first position.
CRAFTED_LENS = [16, 22, 22, 40, 24, 6, 5, 0, 8, 7, 22]


def _granule_codes(ref_start, n_refs, total):
    """The code of every granule as the library upload computes it: 1..15 = the offset of the only reference start
    strictly inside the granule, 16 = none, 17 = several."""
    starts = np.asarray(ref_start[:n_refs], dtype=np.int64)
    codes = []
    for x in range(0, int(total) + GRANULE, GRANULE):
        inside = starts[(starts > x) & (starts < x + GRANULE)]
        codes.append(16 if inside.size == 0 else (int(inside[0] - x) if inside.size == 1 else 17))
    return np.asarray(codes)


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world(ctx):
    """Tiny libraries whose miRNA library starts with the crafted references, the cascade over them, the crafted reads."""
    rng = np.random.default_rng(2024)
    base = synth.make_libraries(seed=41, scale="tiny")
    crafted = ["".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=L)) for L in CRAFTED_LENS]
    mir = base.libs["mirna"]
    seqs = crafted + mir.seqs.to_list()
    libs = dict(base.libs)
    libs["mirna"] = Library([f"crafted-{i}" for i in range(len(crafted))] + list(mir.names), FlatSeqs.from_list(seqs))
    lens = np.asarray([len(s) for s in seqs], dtype=np.int64)
    ref_start = np.concatenate([[0], np.cumsum(lens + 1)])
    assert list(ref_start[:12]) == [0, 17, 40, 63, 104, 129, 136, 142, 143, 152, 160, 183]
    codes = _granule_codes(ref_start, len(seqs), ref_start[-1])
    assert codes[1] == 1 and codes[3] == 15 and codes[4] == codes[5] == codes[7] == 16 and codes[8] == 17
    r = crafted
    exact = [
        r[0],            # position 0
        r[1],            # 17: the first base of a reference that starts inside a granule (code 1)
        r[1][3:],        # 20
        r[2],            # 40
        r[2][8:],        # 48: in front of reference 3's start in granule 3 (position 62 is a separator: no alignment starts there)
        r[2][6:],        # 46
        r[3][:24],       # 63: the start at offset 15 (code 15)
        r[3][1:25],      # 64: the first base of the next granule (code 16: the entry's own reference)
        r[3][17:40],     # 80
        r[3][20:40],     # 83 ... 102
        r[4],            # 104 ... 127: ends on the last position of granule 7
        r[4][8:],        # 112: the first base of granule 7
        r[4][10:],       # 114
        r[5], r[6], r[8], r[9],  # 129, 136, 143, 152: the references of granule 8 (code 17) and its neighbour
        r[10],           # 160: a reference that starts on a granule's first position
        r[10][2:],       # 162
        seqs[-1], seqs[-1][2:],  # the last reference of the library
        seqs[-2], seqs[len(crafted)], seqs[len(crafted) + 7][1:],
    ] + [seqs[len(crafted) + k] for k in range(1, 7)]
    iso = []  # one substitution inside the seed: not an exact-pass read; found by the isomiR pass one base further on
    for s in exact:
        if len(s) >= 18:
            x = list(s)
            x[5] = "ACGT"[("ACGT".index(x[5]) + 1) % 4]
            iso.append("".join(x))
    reads = list(dict.fromkeys(exact + iso))
    assert 40 <= len(reads) <= 200
    casc = Cascade(ctx, libs)
    yield dict(base=base, libs=libs, casc=casc, reads=reads, ref_start=ref_start, codes=codes, n_mirna=len(seqs))
    casc.close()


def _random_reads(rng, n, lo=18, hi=25):
    lens = rng.integers(lo, hi + 1, size=n)
    return ["".join(map(chr, row[:L])) for row, L in zip(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n, hi))], lens)]


def _sample(world, n_filler, general, seed):
    """Raw reads: the crafted reads with counts 1, 2 and 70 000 (> 2^16) in turn, synthetic reads of the tiny libraries and
    random filler; ``general``: reads with an N and reads of 40 nt besides, so that the result has several read groups."""
    rng = np.random.default_rng(seed)
    raw = []
    big_left = 2
    for i, s in enumerate(world["reads"]):
        c = (1, 2, 70000)[i % 3]
        if c == 70000:
            c = 70000 if big_left else 3
            big_left -= 1 if big_left else 0
        raw += [s] * c
    if n_filler:
        raw += [s for s in synth.make_reads(world["base"], min(n_filler, 3000), seed=seed).to_list() if len(s) <= 31 and "N" not in s]
        raw += _random_reads(rng, n_filler)
    if general:
        with_n = []
        for s in world["reads"][:30] + _random_reads(rng, 40):
            x = list(s)
            x[len(x) // 2] = "N"
            with_n.append("".join(x))
        raw += with_n * 2
        mr = world["libs"]["mrna"].seqs.to_list()
        raw += [mr[k % len(mr)][7 * k % 50:7 * k % 50 + 40] for k in range(60)] * 3
        raw += [s[:20] + "N" + s[21:] for s in raw[-5:]]
    order = rng.permutation(len(raw))
    return FlatSeqs.from_list([raw[k] for k in order])


def _numpy_tables(fetched, counts, n_pass, n_mirna):
    p, ref = fetched[0].astype(np.int64), fetched[1].astype(np.int64)
    c = counts.astype(np.int64)
    cls = np.zeros((n_pass, c.shape[1]), dtype=np.int64)
    ex = np.zeros((n_mirna, c.shape[1]), dtype=np.int64)
    iso = np.zeros((n_mirna, c.shape[1]), dtype=np.int64)
    ann = p >= 0
    np.add.at(cls, p[ann], c[ann])
    np.add.at(ex, ref[p == EXACT_PASS], c[p == EXACT_PASS])
    np.add.at(iso, ref[p == ISO_PASS], c[p == ISO_PASS])
    return cls, ex, iso


def _assert_tables(got, want):
    for g, w, nm in zip(got, want, ("class sums", "exact", "isomiR")):
        assert g.dtype == np.int64 and np.array_equal(g, w), (nm, np.argwhere(g != w)[:5])


@pytest.mark.parametrize("n_filler,general", [(0, False), (70000, False), (0, True), (70000, True)])
def test_tables_from_positions_equal_numpy_on_the_fetched_annotation(ctx, world, n_filler, general):
    """Both forms of the join (k_join_multi below 65 536 unique reads, k_join_rows from there on: its four-reads-per-thread path
    for a single read group, its general path for several) on the library of all three granule codes; and the deferred
    k_resolve writes what the immediate one of a cascade without a join writes."""
    casc, n_mirna = world["casc"], world["n_mirna"]
    raw = _ffi.DeviceReads.pack(ctx, _sample(world, n_filler, general, seed=7))
    uq, res = casc.collapse_and_run(raw)
    tabs = _ffi.count_join(ctx, uq, res, EXACT_PASS, ISO_PASS, n_mirna)
    f = res.fetch()
    counts, _ = uq.counts()
    U = len(uq)
    groups = (uq.group_counts() > 0).sum()
    print(f"unique reads {U}, read groups {groups}, annotated {(f[0] >= 0).sum()}, exact {(f[0] == EXACT_PASS).sum()}, "
          f"isomiR {(f[0] == ISO_PASS).sum()}, largest count {counts.max()}")
    assert (groups > 1) == general
    if n_filler:
        assert U >= 65536 and U % 4096 != 0  # k_join_rows; no multiple of 4 x workgroups x 1024 threads
    else:
        assert U < 1024
    assert counts.max() > 1 << 16 and (counts == 1).any() and (counts == 2).any()
    _assert_tables(tabs, _numpy_tables(f, counts, casc.n_pass, n_mirna))
    # the miRNA reads sit on granules of every code
    mi = (f[0] == EXACT_PASS) | (f[0] == ISO_PASS)
    pos = world["ref_start"][f[1][mi].astype(np.int64)] + f[2][mi]
    seen = set(world["codes"][pos // GRANULE].tolist())
    assert {1, 15, 16, 17} <= seen, seen
    assert (f[1][mi] == n_mirna - 1).any() and (f[0] == EXACT_PASS).sum() >= 20 and (f[0] == ISO_PASS).sum() >= 10
    # a second, identical cascade on which no join runs
    uq2, res2 = casc.collapse_and_run(raw)
    f2 = res2.fetch()
    o1, o2 = np.argsort(uq.counts()[1], kind="stable"), np.argsort(uq2.counts()[1], kind="stable")
    for a, b, nm in zip(f, f2, ("pass", "ref", "off", "mm")):
        assert np.array_equal(a[o1], b[o2]), nm
    for h in (res2, uq2, res, uq, raw):
        h.close()


def test_two_samples_through_the_merged_dictionary(ctx, world):
    casc, n_mirna = world["casc"], world["n_mirna"]
    raws = [_ffi.DeviceReads.pack(ctx, _sample(world, 40000, True, seed=s)) for s in (11, 12)]
    dicts = [r.collapse() for r in raws]
    merged = _ffi.DeviceReads.merge(ctx, dicts)
    assert merged.n_samples == 2 and len(merged) >= 65536
    res = casc.run(merged)
    tabs = _ffi.count_join(ctx, merged, res, EXACT_PASS, ISO_PASS, n_mirna)
    f = res.fetch()
    counts, _ = merged.counts()
    assert (counts > 0).all(axis=1).any() and (counts[:, 0] == 0).any() and (counts[:, 1] == 0).any()
    _assert_tables(tabs, _numpy_tables(f, counts, casc.n_pass, n_mirna))
    assert tabs[1].sum() > 2 * 70000 and tabs[2].sum() > 0
    for h in [res, merged] + dicts + raws:
        h.close()


def test_order_of_consumers(ctx, world):
    """fetch without a join, fetch behind a join, two joins on one result: the same references and offsets, the same tables;
    and a result closed directly behind its join."""
    casc, n_mirna = world["casc"], world["n_mirna"]
    raw = _ffi.DeviceReads.pack(ctx, _sample(world, 70000, True, seed=21))
    fetched, tables = [], []
    for n_joins in (0, 1, 2):
        uq, res = casc.collapse_and_run(raw)
        for _ in range(n_joins):
            tables.append(_ffi.count_join(ctx, uq, res, EXACT_PASS, ISO_PASS, n_mirna))
        f = res.fetch()
        order = np.argsort(uq.counts()[1], kind="stable")  # by first appearance in the raw reads: the same for every run
        fetched.append([a[order] for a in f])
        if n_joins == 2:
            _assert_tables(tables[-1], _numpy_tables(f, uq.counts()[0], casc.n_pass, n_mirna))
        res.close(); uq.close()
    for other in fetched[1:]:
        for a, b, nm in zip(fetched[0], other, ("pass", "ref", "off", "mm")):
            assert np.array_equal(a, b), nm
    assert (fetched[0][0] == EXACT_PASS).sum() >= 20
    for t in tables[1:]:
        _assert_tables(t, tables[0])
    uq, res = casc.collapse_and_run(raw)
    _ffi.count_join(ctx, uq, res, EXACT_PASS, ISO_PASS, n_mirna)
    res.close()  # no fetch in between: the deferred k_resolve still has its buffers
    uq.close()
    # the context is sound afterwards
    uq, res = casc.collapse_and_run(raw)
    t = _ffi.count_join(ctx, uq, res, EXACT_PASS, ISO_PASS, n_mirna)
    _assert_tables(t, tables[0])
    res.close(); uq.close(); raw.close()


# ---------------------------------------------------------------- small-group placement
@pytest.fixture(scope="module")
def placement(ctx):
    """One sample with a bulk group, a 2-word group of ~3 000 reads, a 1-word N group of 100 and a 2-word N group of 5; the
    oracle's annotation of every distinct read, computed once."""
    rng = np.random.default_rng(5)
    sl = synth.make_libraries(seed=52, scale="tiny")
    casc = Cascade(ctx, sl.libs)
    bulk = synth.make_reads(sl, 6000, seed=3).to_list()
    bulk = [s for s in bulk if len(s) <= 31 and "N" not in s] + _random_reads(rng, 3000)
    wide = []
    for key in ("mrna", "ncrna_others", "rrna"):
        lib = sl.libs[key].seqs.to_list()
        for k in range(1100):
            s = lib[int(rng.integers(0, len(lib)))]
            L = int(rng.integers(32, 65))
            if len(s) <= L:
                continue
            a = int(rng.integers(0, len(s) - L))
            x = list(s[a:a + L])
            if k % 3 == 0:
                q = int(rng.integers(0, L))
                x[q] = "ACGT"[("ACGT".index(x[q]) + 1) % 4] if x[q] in "ACGT" else "A"
            wide.append("".join(x))
    wide = [s for s in dict.fromkeys(wide) if "N" not in s]

    def with_n(s, q):
        return s[:q] + "N" + s[q + 1:]
    short_n = list(dict.fromkeys(with_n(s, 3 + k % 10) for k, s in enumerate(dict.fromkeys(bulk))))[:100]
    wide_n = [with_n(s, 9 + 4 * k) for k, s in enumerate(wide[:5])]
    # for the case with a k_cascade_fused group: a 2-word group beyond 32 768 unique reads, and a bulk group that stays the largest
    pad = dict(bulk_pad=_random_reads(rng, 40000), wide_pad=_random_reads(rng, 34000, 40, 40))
    groups = dict(bulk=bulk, wide=wide, short_n=short_n, wide_n=wide_n)
    assert len(set(bulk)) > len(wide) > 2500 and len(short_n) == 100 and len(wide_n) == 5, (len(set(bulk)), len(wide), len(short_n))
    distinct = FlatSeqs.from_list(list(dict.fromkeys(bulk + wide + short_n + wide_n + pad["bulk_pad"] + pad["wide_pad"])))
    o = oracle.cascade(distinct.data, distinct.offsets, oracle_libs_from(sl.libs), n_pass=9, indexed=True)
    want = {s: tuple(int(a[i]) for a in o) for i, s in enumerate(distinct.to_list())}
    yield dict(casc=casc, groups=groups, want=want, pad=pad)
    casc.close()


@pytest.mark.parametrize("left_out", [None, "bulk", "wide", "short_n", "wide_n", "fused"])
def test_small_group_placement_keeps_the_annotation(ctx, placement, left_out):
    """Every combination that leaves one of the two extra streams without a group (and the one that makes the 2-word group the
    bulk): the per-read annotation is the oracle's.  In these the 2-word group of ~3 000 reads takes the k_cascade_spec route like
    the two N groups; "fused" leaves nothing out and pads the 2-word group to ~37 000 unique reads (k_cascade_fused, extra stream 0,
    queued last) and the bulk group to ~46 000, so that both N groups are dealt to the other extra stream -- through the one-call
    route's hooks, scatter kernels included (more than 65 536 raw reads)."""
    reads = [s for name, g in placement["groups"].items() if name != left_out for s in g]
    if left_out == "fused":
        reads += placement["pad"]["bulk_pad"] + placement["pad"]["wide_pad"]
    raw = _ffi.DeviceReads.pack(ctx, FlatSeqs.from_list(reads))
    uq, res = placement["casc"].collapse_and_run(raw)
    f = res.fetch()
    useq = uq.unpack().to_list()
    present = (uq.group_counts() > 0).sum()
    assert present == (4 if left_out in (None, "fused") else 3), uq.group_counts()
    if left_out == "fused":
        gc = np.sort(uq.group_counts())
        assert gc[-1] > gc[-2] > 32768 and len(reads) > 65536, gc
    got = list(zip(*(a.tolist() for a in f)))
    bad = [(s, g, placement["want"][s]) for s, g in zip(useq, got) if g != placement["want"][s]]
    assert not bad, bad[:5]
    assert (f[0] >= 0).mean() > (0.25 if left_out != "fused" else 0.04)
    tabs = _ffi.count_join(ctx, uq, res, EXACT_PASS, ISO_PASS, len(placement["casc"].libs["mirna"]))
    _assert_tables(tabs, _numpy_tables(f, uq.counts()[0], 9, len(placement["casc"].libs["mirna"])))
    res.close(); uq.close(); raw.close()


def test_borrowed_libraries_closed_by_their_owner_before_the_fetch(ctx):
    """A cascade on a second context with libraries the first one owns (allowed: same device), then the owner closes its
    libraries, then the borrower fetches and joins: no k_resolve may be left waiting for granule tables that are gone.  The
    yardstick is the annotation fetched from an identical cascade BEFORE the libraries were closed."""
    sl = synth.make_libraries(seed=52, scale="tiny")
    casc = Cascade(ctx, sl.libs)
    reads = synth.make_reads(sl, 5000, seed=8, n_frac=0.02)
    ctx2 = _ffi.Context(0)
    try:
        dr = _ffi.DeviceReads.pack(ctx2, reads)
        uq = dr.collapse()
        first = _ffi.cascade_run(ctx2, uq, casc.dev_libs, casc.policies, casc._prepared)
        want = first.fetch()
        first.close()
        res = _ffi.cascade_run(ctx2, uq, casc.dev_libs, casc.policies, casc._prepared)
        casc.close()  # the owner's libraries go; nothing of ctx2 has been touched since its cascade
        got = res.fetch()
        for a, b, nm in zip(want, got, ("pass", "ref", "off", "mm")):
            assert np.array_equal(a, b), nm
        assert ((got[0] == EXACT_PASS) | (got[0] == ISO_PASS)).sum() > 100
        n_mirna = len(sl.libs["mirna"])
        tabs = _ffi.count_join(ctx2, uq, res, EXACT_PASS, ISO_PASS, n_mirna)  # joined from res_ref: the granule tables are gone
        _assert_tables(tabs, _numpy_tables(want, uq.counts()[0], 9, n_mirna))
        res.close(); uq.close(); dr.close()
    finally:
        ctx2.close()
