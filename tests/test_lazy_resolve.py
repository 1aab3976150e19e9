"""Reference resolution on first use (native_ctx.hpp, PendingResolve): the count join leaves the bulk group's k_resolve pending, a
result closed unread never runs it, and every reader of ``ref`` / ``off`` finds it launched in front of itself.

Yardstick: the annotation of a result fetched with NO join in between, and numpy on it.  All comparisons are exact integer (or
byte) equality.  Every case runs a step on ANOTHER sample first, so that the pool blocks a skipped k_resolve would leave unwritten
hold that sample's references, not a copy of the right answer."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import mirge3_amd  # noqa: F401
from mirge3_amd import _ffi
from mirge3_amd.cascade import EXACT_PASS, ISO_PASS
from mirge3_amd.fastpath import PASS_COLUMNS, names_by_pass
from test_join_from_positions import _assert_tables, _numpy_tables, _sample, ctx, world  # noqa: F401  (fixtures and sample maker)

pytestmark = pytest.mark.gpu


@contextmanager
def lazy_resolve(on):
    old = os.environ.get("MIRGE_LAZY_RESOLVE")
    os.environ["MIRGE_LAZY_RESOLVE"] = "1" if on else "0"
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("MIRGE_LAZY_RESOLVE")
        else:
            os.environ["MIRGE_LAZY_RESOLVE"] = old


@pytest.fixture(scope="module")
def sample(ctx, world):
    """The sample (about 70 000 unique one-word reads, a 2-word group, reads with an N), another one for the steps in between, and
    the yardstick: annotation and counts of the sample fetched without a join, in order of first appearance."""
    raw = _ffi.DeviceReads.pack(ctx, _sample(world, 70000, True, seed=31))
    other = _ffi.DeviceReads.pack(ctx, _sample(world, 50000, True, seed=32))
    uq, res = world["casc"].collapse_and_run(raw)
    f = res.fetch()
    counts, first = uq.counts()
    order = np.argsort(first, kind="stable")
    assert len(uq) >= 65536 and (uq.group_counts() > 0).sum() > 1
    assert (f[0] == EXACT_PASS).sum() >= 20 and (f[0] == ISO_PASS).sum() >= 10
    want = dict(f=[a[order] for a in f], counts=counts[order], tables=_numpy_tables(f, counts, world["casc"].n_pass, world["n_mirna"]))
    res.close(); uq.close()
    yield dict(raw=raw, other=other, want=want)
    other.close(); raw.close()


def _step(ctx, world, raw):
    """collapse + cascade + join, result closed unread -> the tables"""
    uq, res = world["casc"].collapse_and_run(raw)
    t = _ffi.count_join(ctx, uq, res, EXACT_PASS, ISO_PASS, world["n_mirna"])
    res.close(); uq.close()
    return t


def _in_first_appearance_order(uq, f):
    order = np.argsort(uq.counts()[1], kind="stable")
    return [a[order] for a in f]


def _assert_annotation(got, want):
    for a, b, nm in zip(got, want, ("pass", "ref", "off", "mm")):
        assert np.array_equal(a, b), (nm, np.argwhere(a != b)[:5])


def _launches(ctx, prefix):
    return sum(l for name, l, _, _ in ctx.profile_records() if name.startswith(prefix))


def test_result_closed_behind_its_join_never_resolves(ctx, world, sample):
    """case 1: join -> close: no k_resolve launch; with MIRGE_LAZY_RESOLVE=0 one; the next step's tables are right"""
    _step(ctx, world, sample["other"])
    ctx.profile(True)
    try:
        for lazy, n_resolve in ((True, 0), (False, 1)):
            with lazy_resolve(lazy):
                ctx.profile_reset()
                t = _step(ctx, world, sample["raw"])
                assert _launches(ctx, "k_cascade_bulk") == 1 and _launches(ctx, "k_join") >= 2  # the bulk route, k_join_rows
                assert _launches(ctx, "k_resolve") == n_resolve, ctx.profile_records()
                _assert_tables(t, sample["want"]["tables"])
                _assert_tables(_step(ctx, world, sample["raw"]), sample["want"]["tables"])  # the next step on the same context
    finally:
        ctx.profile(False)
        ctx.profile_reset()


def test_fetch_behind_a_join_resolves_first(ctx, world, sample):
    """case 2: join -> fetch: ref / off of a result fetched without a join"""
    _step(ctx, world, sample["other"])
    uq, res = world["casc"].collapse_and_run(sample["raw"])
    t = _ffi.count_join(ctx, uq, res, EXACT_PASS, ISO_PASS, world["n_mirna"])
    f = res.fetch()
    _assert_annotation(_in_first_appearance_order(uq, f), sample["want"]["f"])
    _assert_tables(t, sample["want"]["tables"])
    res.close(); uq.close()


def test_next_cascade_while_the_first_result_is_open(ctx, world, sample):
    """case 3: join -> the next collapse_and_run with the first result open -> fetch the first; and the second's own"""
    _step(ctx, world, sample["other"])
    uq, res = world["casc"].collapse_and_run(sample["raw"])
    _ffi.count_join(ctx, uq, res, EXACT_PASS, ISO_PASS, world["n_mirna"])
    uq2, res2 = world["casc"].collapse_and_run(sample["other"])
    t2 = _ffi.count_join(ctx, uq2, res2, EXACT_PASS, ISO_PASS, world["n_mirna"])
    f = res.fetch()
    _assert_annotation(_in_first_appearance_order(uq, f), sample["want"]["f"])
    f2 = res2.fetch()
    _assert_tables(t2, _numpy_tables(f2, uq2.counts()[0], world["casc"].n_pass, world["n_mirna"]))
    res2.close(); uq2.close(); res.close(); uq.close()


def test_device_csv_writer_behind_a_join(ctx, world, sample, tmp_path):
    """case 4: join -> mirge_annotation_csv_device without a fetch: the bytes of the same call behind a fetch, and of the host
    formatter on the fetched arrays"""
    _step(ctx, world, sample["other"])
    casc = world["casc"]
    uq, res = casc.collapse_and_run(sample["raw"])
    _ffi.count_join(ctx, uq, res, EXACT_PASS, ISO_PASS, world["n_mirna"])
    rows = np.arange(len(uq), dtype=np.int64)  # (an order computed on the device would be an entry point of its own)
    header = ",".join(["Sequence", "annotFlag"] + PASS_COLUMNS[:9] + ["S0"]) + "\n"
    nb = names_by_pass(casc)
    dirs = {k: tmp_path / k for k in ("unread", "fetched", "host")}
    for d in dirs.values():
        d.mkdir()
    cols = list(range(casc.n_pass))
    assert _ffi.annotation_csv_device(ctx, uq, res, dirs["unread"] / "mapped.csv", dirs["unread"] / "unmapped.csv", header, rows, cols, 9, nb)
    ps, ref, off, mm = res.fetch()
    assert _ffi.annotation_csv_device(ctx, uq, res, dirs["fetched"] / "mapped.csv", dirs["fetched"] / "unmapped.csv", header, rows, cols, 9, nb)
    _ffi.annotation_csv(dirs["host"] / "mapped.csv", dirs["host"] / "unmapped.csv", header, uq.unpack(), ps, ref, uq.counts()[0], rows, cols, 9, nb)
    for name in ("mapped.csv", "unmapped.csv"):
        unread = (dirs["unread"] / name).read_bytes()
        assert unread == (dirs["fetched"] / name).read_bytes() == (dirs["host"] / name).read_bytes(), name
        assert unread.count(b"\n") > 1000
    _assert_annotation(_in_first_appearance_order(uq, (ps, ref, off, mm)), sample["want"]["f"])
    res.close(); uq.close()


def test_second_join_from_references_after_a_library_is_destroyed(ctx, world, sample):
    """case 5: join -> a library destroyed -> a second join on the same result (from res_ref: ``from_pos == false``)"""
    _step(ctx, world, sample["other"])
    uq, res = world["casc"].collapse_and_run(sample["raw"])
    t1 = _ffi.count_join(ctx, uq, res, EXACT_PASS, ISO_PASS, world["n_mirna"])
    extra = _ffi.DeviceLibrary(ctx, world["libs"]["snorna"].seqs)
    # (created behind the join: the creation itself is an entry point that launches what is pending; the case below destroys a library
    #  with the kernel still pending)
    extra.close()
    t2 = _ffi.count_join(ctx, uq, res, EXACT_PASS, ISO_PASS, world["n_mirna"])
    _assert_tables(t1, sample["want"]["tables"])
    _assert_tables(t2, sample["want"]["tables"])
    res.close(); uq.close()
    # the same with the library made BEFORE the cascade: its destruction is the first entry point behind the join
    extra = _ffi.DeviceLibrary(ctx, world["libs"]["snorna"].seqs)
    _step(ctx, world, sample["other"])
    uq, res = world["casc"].collapse_and_run(sample["raw"])
    t1 = _ffi.count_join(ctx, uq, res, EXACT_PASS, ISO_PASS, world["n_mirna"])
    extra.close()
    t2 = _ffi.count_join(ctx, uq, res, EXACT_PASS, ISO_PASS, world["n_mirna"])
    _assert_tables(t1, sample["want"]["tables"])
    _assert_tables(t2, sample["want"]["tables"])
    _assert_annotation(_in_first_appearance_order(uq, res.fetch()), sample["want"]["f"])
    res.close(); uq.close()


def test_second_join_from_another_context(ctx, world, sample):
    """join on the result's own context (k_resolve stays pending) -> a join of the same result from ANOTHER context of the device,
    which reads res_ref: the pending kernel of the result's context goes first"""
    _step(ctx, world, sample["other"])
    uq, res = world["casc"].collapse_and_run(sample["raw"])
    t1 = _ffi.count_join(ctx, uq, res, EXACT_PASS, ISO_PASS, world["n_mirna"])
    ctx2 = _ffi.Context(0)
    try:
        t2 = _ffi.count_join(ctx2, uq, res, EXACT_PASS, ISO_PASS, world["n_mirna"])
    finally:
        ctx2.close()
    _assert_tables(t1, sample["want"]["tables"])
    _assert_tables(t2, sample["want"]["tables"])
    res.close(); uq.close()


def test_workgroup_clocks_of_a_closed_step(ctx, world, sample):
    """case 6: the profiled clock copy waits for no k_resolve: after a step closed unread, mirge_cascade_wg_times returns one clock
    per workgroup of THAT step's bulk launch (the two samples' launches differ in size), as it does with MIRGE_LAZY_RESOLVE=0"""
    grids = {}
    ctx.profile(True)
    try:
        for lazy in (False, True):
            with lazy_resolve(lazy):
                for key in ("raw", "other", "raw"):
                    _step(ctx, world, sample[key])
                    wg = _ffi.cascade_wg_times(ctx)
                    assert wg is not None and (wg > 0).all() and (wg < 1000.0).all()  # milliseconds per workgroup
                    grids.setdefault((lazy, key), []).append(len(wg))
    finally:
        ctx.profile(False)
        ctx.profile_reset()
    # one workgroup per 256 raw one-word reads of the sample (far below the chip's resident workgroups)
    for key in ("raw", "other"):
        n_bulk = int(sample[key].group_counts().max())
        want = (n_bulk + 255) // 256
        assert 64 < want <= 1024
        assert set(grids[(True, key)]) == set(grids[(False, key)]) == {want}, (key, grids)
    assert grids[(True, "raw")] != grids[(True, "other")]
