"""mirge_variant_tally (k_member_list + k_tally<1> / k_tally<2>) on the device where the kernel's packed words are full: canonical
sequences of 24..32 nt and their isomiR members of up to 35 nt, which sit in the two-word read group.  The directed set and the figures
it must reach are those of tests/test_tally_hostsim.py (``directed_case`` / ``directed_coverage``); the annotation comes from the device
cascade under the exact-miRNA and the isomiR policy on one library and must equal ``oracle.cascade``'s read by read, so that the tables
are compared on the members that were planned.  Every comparison with ``oracle.variant_tally`` is exact integer equality."""
import numpy as np
import pytest

import oracle
import mirge3_amd  # noqa: F401
from mirge3_amd import _ffi
from mirge3_amd.cascade import PASSES
from mirge3_amd.seqio import FlatSeqs
from test_tally_hostsim import FREQ, assert_same, directed_annotation, directed_case, directed_coverage, rnd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


def _policy(**kw):
    p = _ffi.MirgePolicy()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _pols():
    return [_policy(**PASSES[0][3]), _policy(**PASSES[8][3])]  # exact miRNA, isomiR miRNA


@pytest.fixture(scope="module")
def run(ctx):
    """the directed set collapsed and annotated on the device, and the oracle's answers for it (computed once)"""
    case = directed_case()
    lib = _ffi.DeviceLibrary(ctx, FlatSeqs.from_list(case["library"]))
    raw = _ffi.DeviceReads.pack(ctx, FlatSeqs.from_list(case["raw"]))
    uniq = raw.collapse(case["sid"], 3)
    res = _ffi.cascade_run(ctx, uniq, [lib, lib], _pols())
    ps, ref, _, _ = res.fetch()
    counts, _ = uniq.counts()
    useq = uniq.unpack().to_list()
    # the collapse gave the reads and the counts the case was made with (in an order of its own)
    want = {q: tuple(int(x) for x in row) for q, row in zip(case["useq"], case["counts"])}
    assert {q: tuple(int(x) for x in row) for q, row in zip(useq, counts)} == want
    ret_of = dict(zip(case["useq"], case["retained"]))
    retained = np.asarray([ret_of[q] for q in useq], dtype=np.uint8)
    o_ps, o_ref = directed_annotation(case, useq)
    c64 = counts.astype(np.int64)
    o = oracle.variant_tally(useq, c64, o_ps, o_ref, case["fam_of_ref"], case["targets"], retained, FREQ, exact_pass=0, iso_pass=1)
    yield dict(case=case, lib=lib, uniq=uniq, res=res, ps=ps, ref=ref, counts=c64, useq=useq, retained=retained, o_ps=o_ps, o_ref=o_ref, o=o)
    res.close(); uniq.close(); raw.close(); lib.close()


def test_annotation_equals_the_oracle_cascade(run):
    assert np.array_equal(run["ps"].astype(np.int64), run["o_ps"].astype(np.int64))
    assert np.array_equal(run["ref"].astype(np.int64), run["o_ref"].astype(np.int64))


def test_input_coverage(run):
    """what the directed set is made for, from the oracle alone (figures of the committed seed: 8981 reads, 4376 members; members of
    32 nt and more: 263 accepted, 62 rejected; 13 / 51 / 83 / 178 of them for canonical lengths 29 / 30 / 31 / 32)"""
    fig = directed_coverage(run["case"], run["useq"], run["counts"], run["o_ps"], run["o_ref"], run["o"])
    print("directed set:", fig)


def test_tables_equal_the_oracle(ctx, run):
    case = run["case"]
    g = _ffi.variant_tally(ctx, run["uniq"], run["res"], 0, 1, case["fam_of_ref"], FlatSeqs.from_list(case["targets"]), run["retained"], FREQ)
    o = run["o"]
    long_member = (o["state"] >= 0) & (np.asarray([len(q) for q in run["useq"]]) >= 32)
    print("members of 32 nt and more:", int(long_member.sum()), "state equal on", int((g["state"][long_member] == o["state"][long_member]).sum()),
          "| n_seqs", int(g["n_seqs"].sum()), "oracle", int(o["n_seqs"].sum()))
    assert_same(g, o)


def test_tables_with_the_defaults(ctx, run):
    """every reference its own family with its own sequence as the canonical one, every read retained, every isomiR read a member"""
    case = run["case"]
    fam = np.arange(len(case["library"]), dtype=np.int32)
    freq = np.full(3, 1e300)
    g = _ffi.variant_tally(ctx, run["uniq"], run["res"], 0, 1, fam, FlatSeqs.from_list(case["library"]), None, freq)
    o = oracle.variant_tally(run["useq"], run["counts"], run["o_ps"], run["o_ref"], fam, case["library"], None, freq, exact_pass=0, iso_pass=1)
    assert_same(g, o)
    assert ((o["state"] >= 0) == (run["o_ps"] >= 0)).all()


def _one_call(ctx, library, reads, targets, pols):
    lib = _ffi.DeviceLibrary(ctx, FlatSeqs.from_list(library))
    raw = _ffi.DeviceReads.pack(ctx, FlatSeqs.from_list(reads))
    uniq = raw.collapse()
    res = _ffi.cascade_run(ctx, uniq, [lib, lib], pols)
    ps = res.fetch()[0]
    useq = uniq.unpack().to_list()
    try:
        g = _ffi.variant_tally(ctx, uniq, res, 0, 1, np.zeros(len(library), dtype=np.int32), FlatSeqs.from_list(targets), None, np.array([1e300]))
    finally:
        res.close(); uniq.close(); raw.close(); lib.close()
    return useq, ps, g


def test_refusals_name_their_cause(ctx):
    rng = np.random.default_rng(33)
    t = rnd(rng, 30)
    reads = [t, t[1:] + "A", rnd(rng, 40)]
    with pytest.raises(RuntimeError, match="33 nt; the limit is 32"):
        _one_call(ctx, [t], reads, [rnd(rng, 33)], _pols())
    with pytest.raises(RuntimeError, match="other than A/C/G/T/U"):
        _one_call(ctx, [t], reads, [t[:7] + "N" + t[8:]], _pols())
    # the same call goes through with the canonical sequence itself
    useq, ps, g = _one_call(ctx, [t], reads, [t], _pols())
    assert sorted(g["state"].tolist()) == [-1, 1, 1]


def test_a_member_beyond_two_words_is_refused(ctx):
    """An isomiR policy that trims 20 bases at both ends annotates a 70-nt read whose middle 30 nt are the canonical sequence: a member
    in the four-word group, which no instance of k_tally takes.  The call fails and says why; it does not return state -1 for the read."""
    rng = np.random.default_rng(34)
    t = rnd(rng, 30)
    wide = rnd(rng, 20) + t + rnd(rng, 20)
    pols = [_policy(**PASSES[0][3]), _policy(**dict(PASSES[8][3], trim5=20, trim3=20))]
    lib = _ffi.DeviceLibrary(ctx, FlatSeqs.from_list([t]))
    raw = _ffi.DeviceReads.pack(ctx, FlatSeqs.from_list([wide, t[:24], rnd(rng, 90)]))
    uniq = raw.collapse()
    res = _ffi.cascade_run(ctx, uniq, [lib, lib], pols)
    ps = res.fetch()[0]
    useq = uniq.unpack().to_list()
    assert int(ps[useq.index(wide)]) == 1  # annotated by the isomiR pass: a member of the family's list
    with pytest.raises(RuntimeError, match="more than 64 nt"):
        _ffi.variant_tally(ctx, uniq, res, 0, 1, np.zeros(1, dtype=np.int32), FlatSeqs.from_list([t]), None, np.array([1e300]))
    res.close(); uniq.close(); raw.close(); lib.close()
