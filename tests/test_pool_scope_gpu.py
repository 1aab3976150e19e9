"""Every report and export call owns its pool blocks through one ``PoolScope`` (csrc/native_ctx.hpp): whatever way the call ends, all
of them are back in the context's pool.  ``Context.pool_stats()`` shows the pool's bookkeeping -- (bytes from the driver, blocks
handed out and not back, blocks in the free list) -- and this file holds every converted family to it:

* the same call three times in one context, the context synchronised before each reading: the blocks handed out after the second
  and the third call are those after the first (which may build tables that stay), the bytes after the third are those after the
  second (a steady state asks the driver for nothing), and the three outputs are equal;
* the same around a call that FAILS after it has allocated -- the contract failures the per-feature tests provoke, each a flag a
  kernel sets and the host reads, and the exporters' missing directory -- with a good call of the same kind between the failures
  that still gives the reference bytes.

What each call computes is checked by its own test file; the inputs are those files' small cases.  No test provokes a HIP error, a
device fault or an allocation failure."""
import numpy as np
import pytest

import mirge3_amd  # noqa: F401
from mirge3_amd import _ffi, bam_export, bigwig, coverage, gff, synth, unmapped_features
from mirge3_amd.cascade import Cascade, policies
from mirge3_amd.fastpath import names_by_pass
from mirge3_amd.seqio import FlatSeqs

import bw_cases
import cov_cases
import test_genome_filter as gf
import umi_cases
from helpers import write_gff_name_files
from test_coverage_gpu import _collapsed, _fuzz_libs
from test_sam_out import ORG
from test_staged_output_gpu import EXPORTERS, Case, run, sizes
from test_trf_clusters_hostsim import flat_groups, synth_groups
from test_trf_hostsim import MATURE_PASS, PRIMARY_PASS, infor_tables, synth_case, synth_infor
from test_unmapped_clusters import SKIP, random_records
from test_unmapped_features_fuzz import fuzz_clusters

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


def same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    if isinstance(a, FlatSeqs):
        return np.array_equal(a.data, b.data) and np.array_equal(a.offsets, b.offsets)
    return a == b


def readings(ctx, calls):
    """every call's result and the pool's bookkeeping behind it"""
    out = []
    for call in calls:
        got = call()
        ctx.sync()
        out.append((got, ctx.pool_stats()))
    return out


def assert_steady(stats, what):
    (_, out1, _), (bytes2, out2, _), (bytes3, out3, _) = stats
    print(f"{what}: pool_stats after the three calls: {stats}")
    assert out2 == out1 and out3 == out1, (what, "blocks handed out and not back", stats)
    assert bytes3 == bytes2, (what, "bytes from the driver", stats)


def three_calls(ctx, call, what):
    """-> the calls' common output"""
    got = readings(ctx, [call] * 3)
    assert_steady([s for _, s in got], what)
    assert same(got[0][0], got[1][0]) and same(got[0][0], got[2][0]), what
    return got[0][0]


def three_failures(ctx, bad, match, good, want, what):
    """bad, good, bad, good, bad: the failures leave the pool as the first of them did, the good calls give ``want``"""
    def failing():
        with pytest.raises(Exception, match=match):
            bad()
    got = readings(ctx, [failing, good, failing, good, failing])
    assert_steady([got[k][1] for k in (0, 2, 4)], what + " (failing)")
    assert same(got[1][0], want) and same(got[3][0], want), what


# ---------------------------------------------------------------------------------------------------------------------
# the four exporters (SAM, BAM with SamPrep; coverage with CovInput / CovDev; bigWig with BwJob), on test_staged_output_gpu's case
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case(ctx):
    c = Case(ctx)
    yield c
    c.close()


@pytest.fixture(scope="module")
def exported(case, tmp_path_factory):
    """{exporter: the files of sample 0} at the default sizes, one call each: the reference bytes (nothing is asserted here)"""
    with sizes():
        return {name: run(case, name, 0, tmp_path_factory.mktemp(name))[0] for name in EXPORTERS}


@pytest.mark.parametrize("name", EXPORTERS)
def test_exporters_hand_every_block_back(ctx, case, exported, name, tmp_path_factory):
    with sizes():
        assert three_calls(ctx, lambda: run(case, name, 0, tmp_path_factory.mktemp(name))[0], name) == exported[name]
    assert all(exported[name]) or name == "cov"  # (a strand's bedGraph may be empty)


@pytest.mark.parametrize("name", EXPORTERS)
def test_exporters_after_a_missing_directory(ctx, case, exported, name, tmp_path):
    good = tmp_path / "good"
    good.mkdir()
    with sizes():
        three_failures(ctx, lambda: getattr(case, name)(0, tmp_path / "missing"), "cannot write", lambda: run(case, name, 0, good)[0],
                       exported[name], name + ", missing directory")


def test_exporters_after_a_chromosome_no_sq_line_names(ctx, case, exported, tmp_path):
    good = tmp_path / "good"
    good.mkdir()
    header = b"@HD\tVN:1.6\n@SQ\tSN:chrNoReads\tLN:536870912\n"
    with sizes():
        three_failures(ctx, lambda: bam_export.write_sample(case.casc, case.uniq, case.res, case.order, 0, tmp_path / "x.bam", tmp_path / "x.bai", header, ORG),
                       "no @SQ line", lambda: run(case, "bam", 0, good)[0], exported["bam"], "bam, no @SQ line")
        paths = [tmp_path / "x.plus.bedgraph", tmp_path / "x.minus.bedgraph"]
        three_failures(ctx, lambda: coverage.write_sample(case.casc, case.uniq, case.res, case.order, 0, paths, True, ORG, ["chrNoReads"]),
                       "no @SQ line", lambda: run(case, "cov", 0, good)[0], exported["cov"], "coverage, no @SQ line")
    assert [p.name for p in tmp_path.iterdir()] == ["good"]


def test_bam_after_a_read_outside_the_index(ctx, tmp_path):
    """sample 0 holds a read whose START is 0 (built through the header's coordinates, as test_coverage_gpu.py does), sample 1 does not"""
    rng = np.random.Generator(np.random.PCG64(77003))
    libs = _fuzz_libs(rng, {"ENST0": "ENST0 chr1 segs:1-600 cds:+:0-599", "ENST2": "ENST2 chr1 segs:1-600 cds:+:1000-1599"})
    m = libs["mrna"].seqs.to_list()
    reads = sorted([m[0][0:30], m[2][570:600], m[2][100:140]])
    want = np.zeros((3, 2), dtype=np.int64)
    want[reads.index(m[0][0:30]), 0] = 2
    want[reads.index(m[2][570:600]), 1] = 3
    want[reads.index(m[2][100:140]), 1] = 1
    casc = Cascade(ctx, libs)
    uniq = _collapsed(ctx, reads, want)
    res = casc.run(uniq)
    order = np.arange(len(uniq), dtype=np.int64)
    header = b"@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:536870912\n"

    def write(s):
        n_rec, _, _ = bam_export.write_sample(casc, uniq, res, order, s, tmp_path / "x.bam", tmp_path / "x.bai", header, ORG)
        return n_rec, (tmp_path / "x.bam").read_bytes(), (tmp_path / "x.bai").read_bytes()
    try:
        ref = three_calls(ctx, lambda: write(1), "bam, two rows")
        assert ref[0] == 4
        for p in tmp_path.iterdir():
            p.unlink()
        three_failures(ctx, lambda: write(0), r"outside \[1, 2\^29\]", lambda: write(1), ref, "bam, outside [1, 2^29]")
    finally:
        res.close(); uniq.close(); casc.close()


# ---------------------------------------------------------------------------------------------------------------------
# coverage runs and bigWig from host intervals (CovUpload, CovDev, BwJob)
# ---------------------------------------------------------------------------------------------------------------------
def test_coverage_runs(ctx):
    iv, _ = cov_cases.all_cases()["fuzz"]
    ref = three_calls(ctx, lambda: coverage.runs_device(ctx, iv, True), "coverage runs")
    ok, bad = (0, 5, 7, 3, 0), (0, 5, 0, 3, 0)
    three_failures(ctx, lambda: coverage.runs_device(ctx, cov_cases.make([ok, bad, ok]), True), "outside the contract",
                   lambda: coverage.runs_device(ctx, iv, True), ref, "coverage runs")


def test_bigwig_from_intervals(ctx, tmp_path, monkeypatch):
    iv, names = cov_cases.all_cases()["fuzz"]
    lens = bw_cases.sizes_for(iv, len(names))
    for k, v in (("MIRGE_BW_SECTION_ITEMS", bw_cases.S_TEST), ("MIRGE_BW_ZOOM_BASE", bw_cases.BASE_TEST), ("MIRGE_BW_CHUNK_BYTES", 4096)):
        monkeypatch.setenv(k, str(v))  # (several sections per strand, several zoom levels, several groups per stretch)

    def call():
        paths = bigwig.sample_paths(tmp_path, "x", True)
        stats = bigwig.from_intervals(ctx, iv, names, lens, True, paths)
        return stats, [p.read_bytes() for p in paths]
    stats, _ = three_calls(ctx, call, "bigWig from intervals")
    assert all(st["sections"] > 2 and st["levels"] > 1 for st in stats)


# ---------------------------------------------------------------------------------------------------------------------
# the CSV tail, the isomiR records and the GFF on smoke()'s sample
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def annotated(ctx):
    sl = synth.make_libraries(seed=5, scale="ci")
    casc = Cascade(ctx, sl.libs)
    reads = synth.make_reads(sl, 6000, seed=9, n_frac=0.01)
    sid = (np.arange(len(reads)) % 2).astype(np.int32)
    raw = _ffi.DeviceReads.pack(ctx, reads)
    uniq = raw.collapse(sid, 2)
    raw.close()
    res = casc.run(uniq)
    yield dict(sl=sl, casc=casc, uniq=uniq, res=res)
    res.close(); uniq.close(); casc.close()


def test_csv_order_and_range_calls(ctx, annotated, tmp_path):
    casc, uniq, res = annotated["casc"], annotated["uniq"], annotated["res"]
    order = three_calls(ctx, uniq.sorted_order, "sorted order")
    assert sorted(order.tolist()) == list(range(len(uniq)))
    splitters = three_calls(ctx, lambda: uniq.range_sample(3), "range sample")
    three_calls(ctx, lambda: uniq.range_split(np.sort(splitters)), "range split")
    assert three_calls(ctx, uniq.nonzero_per_sample, "nonzero per sample").sum() >= len(uniq)
    nb, cols = names_by_pass(casc), list(range(casc.n_pass))

    def write():
        assert _ffi.annotation_csv_device(ctx, uniq, res, tmp_path / "mapped.csv", tmp_path / "unmapped.csv", "h\n", order, cols, casc.n_pass, nb)
        return (tmp_path / "mapped.csv").read_bytes(), (tmp_path / "unmapped.csv").read_bytes()
    mapped, unmapped = three_calls(ctx, write, "annotation csv")
    assert mapped.count(b"\n") + unmapped.count(b"\n") == len(uniq) + 2
    assert three_calls(ctx, lambda: _ffi.annotation_csv_device_sizes(ctx, uniq, res, order, cols, casc.n_pass, nb), "annotation csv sizes") == \
        (len(mapped) - 2, len(unmapped) - 2)


def test_isomir_records_and_gff(ctx, annotated, tmp_path):
    sl, casc, uniq, res = annotated["sl"], annotated["casc"], annotated["uniq"], annotated["res"]
    mir, hp = sl.libs["mirna"], sl.libs["hairpin"]
    mirDict = dict(zip(mir.names, mir.seqs.to_list()))
    pre_of = {nm: hp.names[int(sl.mir_hairpin[k])] for k, nm in enumerate(mir.names)}
    args = write_gff_name_files(tmp_path / "libs", mirDict, pre_of)
    tables = gff.name_tables(args, "miRBase", casc)
    ps = res.fetch()[0]
    rows = np.nonzero((ps == 0) | (ps == 8))[0].astype(np.int64)
    recs = three_calls(ctx, lambda: gff.isomir_records(casc, uniq, res, tables, rows), "isomiR records")
    assert len(recs) == len(rows) > 500
    order = uniq.sorted_order()

    def write():
        out = gff.write_gff_device_with(tables, tmp_path / "x.gff", "miRBase", ["S1", "S2"], casc, uniq, res, order)
        return out["lines"], (tmp_path / "x.gff").read_bytes()
    lines, _ = three_calls(ctx, write, "gff")
    assert lines > 500


# ---------------------------------------------------------------------------------------------------------------------
# genome counts, loci (one batch and several), windows; loci clusters; the pile-up pair
# ---------------------------------------------------------------------------------------------------------------------
def test_genome_loci_and_clusters(ctx, monkeypatch):
    rng = np.random.default_rng(32)
    refs = gf.random_genome(rng, [4000, 2500, 1500])
    qs = gf.query_set(rng, refs, 120)
    genome, flat = gf._genome(ctx, refs), gf._flat(qs)
    try:
        three_calls(ctx, lambda: genome.align_counts(flat, 1, 28, 2, 0, 2), "genome counts")
        whole = three_calls(ctx, lambda: genome.align_loci(flat, 1, 28, 2, 0, 2, 2), "genome loci")
        monkeypatch.setenv("MIRGE_LOCI_BATCH", "7")  # (every batch builds and hands back tables of its own, in both passes)
        assert same(three_calls(ctx, lambda: genome.align_loci(flat, 1, 28, 2, 0, 2, 2), "genome loci in batches"), whole)
        assert len(whole["query"]) > 0  # (records to report: the fill pass and the sorts ran)
        n = 5
        windows = three_calls(ctx, lambda: genome.fetch(np.zeros(n, np.uint32), np.arange(n) * 100, np.full(n, 60), np.arange(n) % 2, np.ones(n)), "genome windows")
        assert [len(w) for w in windows] == [60] * n
    finally:
        genome.close()
    ref, off, strand, length = random_records(rng, 2500, span=5000)
    qcount = np.arange(1, len(ref) + 1, dtype=np.int64)
    tab = three_calls(ctx, lambda: _ffi.loci_cluster(ctx, ref, off, strand, np.arange(len(ref)), length, qcount, SKIP, 14, True), "loci clusters")
    assert len(tab["ref"]) > 10


def test_pileup(ctx):
    clusters = fuzz_clusters(np.random.default_rng(5), n_clusters=12)
    got = three_calls(ctx, lambda: unmapped_features.device_arrays(ctx, clusters), "cluster diagonals + pileup")
    assert int(got["head"].max()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# tRF hits, assignment, row counts and clusters; UMI clusters
# ---------------------------------------------------------------------------------------------------------------------
def test_trf_calls(ctx):
    mature, primary, anticodon, reads = synth_case(seed=11, n_random=300)
    mlib, plib = _ffi.DeviceLibrary(ctx, FlatSeqs.from_list(mature)), _ffi.DeviceLibrary(ctx, FlatSeqs.from_list(primary))
    pol = policies(4)
    raw = _ffi.DeviceReads.pack(ctx, FlatSeqs.from_list(reads))
    uniq = raw.collapse()
    raw.close()
    res = _ffi.cascade_run(ctx, uniq, [None, None, mlib, plib], pol)
    try:
        ps = res.fetch()[0]
        rows = np.nonzero(ps >= 0)[0].astype(np.int64)
        other = np.nonzero(ps < 0)[0][:1].astype(np.int64)
        assert len(rows) > 200 and len(other) == 1

        def hits(r):
            return _ffi.trf_hits(ctx, uniq, res, MATURE_PASS, mlib, pol[MATURE_PASS], PRIMARY_PASS, plib, pol[PRIMARY_PASS], r, anticodon)
        ref = three_calls(ctx, lambda: hits(rows), "tRF hits")
        assert ref["row"].shape[0] >= len(rows)
        three_failures(ctx, lambda: hits(other), "neither a mature-tRNA nor a primary-tRNA read", lambda: hits(rows), ref, "tRF hits")
        tref, ref_ptr, strings, _, cs, ce, rank = infor_tables(synth_infor(mature[:15]), len(mature))
        pick = np.nonzero((ref["cls"] == 0) & (tref[ref["ref"]] >= 0))[0][:300]  # records on mature tRNAs with predefined tRFs: (read, reference, 1-based start)
        assert len(pick) > 50
        three_calls(ctx, lambda: _ffi.trf_assign(ctx, uniq, res, ref["row"][pick], tref[ref["ref"][pick]], ref["off"][pick] + 1, ref_ptr, strings, cs, ce,
                                                 rank), "tRF assign")
        counts = three_calls(ctx, lambda: _ffi.trf_row_counts(ctx, uniq, rows), "tRF row counts")
        assert counts.shape == (len(rows), 1)
    finally:
        for h in (res, uniq, mlib, plib):
            h.close()


def test_trf_cluster(ctx):
    reads, groups = synth_groups()
    raw = _ffi.DeviceReads.pack(ctx, FlatSeqs.from_list(reads))
    uniq = raw.collapse()
    raw.close()
    try:
        handle = {rd: k for k, rd in enumerate(uniq.unpack().to_list())}
        ptr, read, off, rp, tlen = flat_groups(groups)

        def good():
            return _ffi.trf_cluster(ctx, uniq, ptr, [handle[reads[i]] for i in read], off, rp, tlen)
        ref = three_calls(ctx, good, "tRF cluster")
        three_failures(ctx, lambda: _ffi.trf_cluster(ctx, uniq, [0, 1], [0], [250], [1.0], [256]), "does not fit its template", good, ref, "tRF cluster")
    finally:
        uniq.close()


def test_umi_cluster(ctx):
    _, reads, counts, f, b = umi_cases.all_cases()["chain_alone"]  # (several rounds of the label propagation)
    raw = _ffi.DeviceReads.pack(ctx, FlatSeqs.from_list(list(reads)))
    tagged = raw.collapse(weights=np.asarray(counts, dtype=np.uint32))
    try:
        flags = three_calls(ctx, lambda: tagged.umi_cluster(f, b), "UMI cluster")
        assert len(flags) == len(reads) and _ffi.umi_cluster_stats()["rounds"] >= 2
    finally:
        tagged.close(); raw.close()
