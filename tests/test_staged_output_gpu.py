"""The four exporters that write a file straight from the resident run -- ``--sam-out``, ``--sorted-bam``, ``--coverage`` and
``--coverage-bigwig`` -- share one staged writer (StagePipe, csrc/native_stage.hpp) and one output-file owner (OutFile,
csrc/native_host.hpp).  What each writes is checked against host formatters and simulations by its own test file; this one is
about the shared part, on one case of a few hundred unique reads from the fuzz libraries of test_sorted_bam_gpu.py (positions a
BAM index holds, reads a BAM QNAME holds), two samples, the second without a kept row:

* the chunk variable of each exporter set so that the output takes exactly one, two and three chunks (the second device half is
  allocated from two on, the third chunk is the first to reuse a half): the bytes of the run at the default sizes;
* in one fresh context SAM in small chunks, then BAM, coverage and bigWig at the default sizes, then SAM in small chunks again --
  the page-locked staging grows, stays and is cut into other halves: the bytes of single calls, each in a context of its own;
* an output directory that does not exist: "cannot write", nothing created, nothing left of the group's other file, and the same
  call to a good path in the same context then writes the same bytes as before.

The references come from one call per exporter and sample, each exporter in a fresh context; SAM and bedGraph are also compared
with the host formatters there.  No test provokes a device fault: the failures are host I/O errors."""
import contextlib
import gzip
import os

import numpy as np
import pytest

import mirge3_amd  # noqa: F401
from mirge3_amd import _ffi, bam_export, bigwig, coverage, sam_export
from mirge3_amd.cascade import Cascade
from mirge3_amd.seqio import FlatSeqs

import bigwig_reader
import cov_cases
from test_sam_out import ORG
from test_sam_out_gpu import _fuzz_reads
from test_sorted_bam_gpu import _bam_libs

pytestmark = pytest.mark.gpu

CHROMS = ["chr3", "chrNoReads", "chr1", "chr5", "chr2", "chr4"]
SQ = [(nm, 1 << 29) for nm in CHROMS]
SAM_HEADER = b"@HD\tVN:1.0\tSO:unsorted\n@CO\tstaged\n"
BAM_HEADER = ("@HD\tVN:1.6\n" + "".join(f"@SQ\tSN:{nm}\tLN:{ln}\n" for nm, ln in SQ)).encode()
BGZF_EOF = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
SIZE_VARS = ("MIRGE_SAM_CHUNK_BYTES", "MIRGE_SAM_TILE_BYTES", "MIRGE_BAM_CHUNK_BLOCKS", "MIRGE_BAM_BLOCK_BYTES", "MIRGE_BAM_DEFLATE",
             "MIRGE_COV_CHUNK_BYTES", "MIRGE_COV_TILE_BYTES", "MIRGE_BW_CHUNK_BYTES", "MIRGE_BW_SECTION_ITEMS", "MIRGE_BW_ZOOM_BASE", "MIRGE_BW_DEFLATE")
SAM_TILE, COV_TILE = 256, 64
BAM_BLOCK = 65280                                    # MIRGE_BAM_BLOCK_BYTES' default: uncompressed bytes per BGZF block
BW_STRIDE = (24 + 1024 * 12 + 11 + 15) & ~15         # a section's slot at MIRGE_BW_SECTION_ITEMS' default (native_bw.hpp, BwJob::stream)


@contextlib.contextmanager
def sizes(**env):
    """the exporters' size variables as given, every other one of them unset (the defaults); restored afterwards"""
    old = {k: os.environ.pop(k, None) for k in SIZE_VARS}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        yield
    finally:
        for k in SIZE_VARS:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in old.items() if v is not None})


class Case:
    """the reads, annotated and collapsed in ``ctx``; sample 0 keeps rows (one of them 8000 times), sample 1 none"""
    def __init__(self, ctx):
        rng = np.random.Generator(np.random.PCG64(99001))
        libs = _bam_libs(rng)
        reads = sorted(r for r in _fuzz_reads(rng, libs) if len(r) <= 64)
        self.casc = Cascade(ctx, libs)
        dr = _ffi.DeviceReads.pack(ctx, FlatSeqs.from_list(reads))
        r0 = self.casc.run(dr)
        ps, ref, _, _ = r0.fetch()
        r0.close(); dr.close()
        self.hp = sam_export.host_passes(self.casc)
        writes = np.zeros(len(reads), dtype=bool)
        for i in range(len(reads)):
            p = int(ps[i])
            if p in self.hp:
                writes[i] = sam_export.lift_of(sam_export.header_dictionary(self.hp[p]["headers"]), self.hp[p]["names"][int(ref[i])], ORG) is not None
        want = rng.integers(1, 6, size=(len(reads), 2))
        want[writes, 1] = 0
        want[[i for i in range(len(reads)) if writes[i] and len(reads[i]) == 16][0], 0] = 8000  # (the outputs span several default BGZF blocks)
        ent = [(i, s) for i in range(len(reads)) for s in range(2) if want[i, s] > 0]
        raw = _ffi.DeviceReads.pack(ctx, FlatSeqs.from_list([reads[i] for i, _ in ent]))
        self.uniq = raw.collapse(np.asarray([s for _, s in ent], dtype=np.int32), 2, weights=np.asarray([want[i, s] for i, s in ent], dtype=np.uint32))
        raw.close()
        self.res = self.casc.run(self.uniq)
        self.order = rng.permutation(len(self.uniq)).astype(np.int64)
        assert 200 < len(reads) == len(self.uniq) < 1000 and writes.sum() > 100

    def close(self):
        self.res.close(); self.uniq.close(); self.casc.close()

    # every exporter: (case, sample, directory) -> (the files' paths, the units its chunk variable cuts)
    def sam(self, s, d):
        _, n_bytes = sam_export.write_sample(self.casc, self.uniq, self.res, self.order, s, d / "x.sam", SAM_HEADER, ORG)
        return [d / "x.sam"], -(-n_bytes // SAM_TILE)

    def bam(self, s, d, bai_dir=None):
        paths = [d / "x_sorted.bam", (bai_dir or d) / "x_sorted.bai"]
        _, n_stream, _ = bam_export.write_sample(self.casc, self.uniq, self.res, self.order, s, paths[0], paths[1], BAM_HEADER, ORG, threads=4)
        return paths, -(-n_stream // BAM_BLOCK)

    def cov(self, s, d, minus_dir=None):
        paths = [d / "x.plus.bedgraph", (minus_dir or d) / "x.minus.bedgraph"]
        st = coverage.write_sample(self.casc, self.uniq, self.res, self.order, s, paths, True, ORG, CHROMS)
        return paths, -(-st["bytes"] // COV_TILE)

    def bw(self, s, d, minus_dir=None):
        paths = [d / "x.plus.bw", (minus_dir or d) / "x.minus.bw"]
        st = bigwig.write_sample(self.casc, self.uniq, self.res, self.order, s, paths, True, ORG, SQ)
        return paths, st[0]["sections"]


EXPORTERS = ["sam", "bam", "cov", "bw"]


def chunked(name, units, k):
    """the size variables under which ``units`` (tiles, blocks, sections) take exactly ``k`` chunks"""
    per = next(p for p in range(1, units + 1) if -(-units // p) == k)
    return {"sam": dict(MIRGE_SAM_TILE_BYTES=SAM_TILE, MIRGE_SAM_CHUNK_BYTES=per * SAM_TILE), "bam": dict(MIRGE_BAM_CHUNK_BLOCKS=per),
            "cov": dict(MIRGE_COV_TILE_BYTES=COV_TILE, MIRGE_COV_CHUNK_BYTES=per * COV_TILE), "bw": dict(MIRGE_BW_CHUNK_BYTES=per * BW_STRIDE)}[name]


def run(case, name, s, d):
    paths, units = getattr(case, name)(s, d)
    assert sorted(os.listdir(d)) == sorted(p.name for p in paths)  # (no temporary file stays)
    out = [p.read_bytes() for p in paths]
    for p in paths:
        p.unlink()
    return out, units


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    """{exporter: ([files of sample 0, files of sample 1], units of sample 0)} at the default sizes, each exporter in a context of its own"""
    out = {}
    for name in EXPORTERS:
        ctx = _ffi.Context(0)
        case = Case(ctx)
        try:
            with sizes():
                d = tmp_path_factory.mktemp(name)
                (f0, units), (f1, _) = run(case, name, 0, d), run(case, name, 1, d)
            out[name] = ([f0, f1], units)
            if name == "sam":
                useq, (counts, _) = case.uniq.unpack().to_list(), case.uniq.counts()
                assert f0[0] == SAM_HEADER + sam_export.format_sam_host(useq, *case.res.fetch(), counts, case.order, 0, case.hp, ORG)
            if name == "cov":
                useq, (counts, _) = case.uniq.unpack().to_list(), case.uniq.counts()
                ps, rf, off, _ = case.res.fetch()
                rank = {nm: k for k, nm in enumerate(CHROMS)}
                rows = coverage.intervals_host(useq, ps, rf, off, counts, case.order, 0, case.hp, ORG)
                runs = coverage.coverage_host(cov_cases.make([(rank[c], a, n, w, mi) for c, a, n, w, mi in rows]), True)
                assert f0 == [coverage.format_bedgraph(runs, CHROMS, 0), coverage.format_bedgraph(runs, CHROMS, 1)] and all(f0)
        finally:
            case.close(); ctx.close()
    assert all(units >= 5 for _, units in out.values()), {k: v[1] for k, v in out.items()}  # (three chunks of at least one unit each, and then some)
    return out


@pytest.fixture(scope="module")
def case():
    ctx = _ffi.Context(0)
    c = Case(ctx)
    yield c
    c.close(); ctx.close()


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("name", EXPORTERS)
def test_exactly_k_chunks_write_the_default_runs_bytes(case, ref, name, k, tmp_path):
    files, units = ref[name]
    with sizes(**chunked(name, units, k)):
        assert run(case, name, 0, tmp_path)[0] == files[0]
        assert run(case, name, 1, tmp_path)[0] == files[1]


def test_a_sample_without_a_kept_row_gets_its_empty_files(ref):
    assert ref["sam"][0][1] == [SAM_HEADER]
    assert ref["cov"][0][1] == [b"", b""]
    bam, bai = ref["bam"][0][1]
    assert bam.endswith(BGZF_EOF) and gzip.decompress(bam) == bam_export.header_blob(BAM_HEADER)[0]  # the header's block and the EOF block
    assert bai == bam_export.format_bam_host(b"", BAM_HEADER)[1]
    for blob in ref["bw"][0][1]:
        got = bigwig_reader.read(blob)
        assert got["items"] == [] and [c[0].decode() for c in got["chroms"]] == sorted(CHROMS, key=lambda s: s.encode())


def test_the_shared_staging_grows_and_is_cut_anew_across_exporters(ref, tmp_path):
    ctx = _ffi.Context(0)
    c = Case(ctx)
    try:
        small = chunked("sam", ref["sam"][1], 3)
        for name, env in [("sam", small), ("bam", {}), ("cov", {}), ("bw", {}), ("sam", small)]:
            with sizes(**env):
                assert run(c, name, 0, tmp_path)[0] == ref[name][0][0], name
    finally:
        c.close(); ctx.close()


@pytest.mark.parametrize("name", EXPORTERS)
def test_a_failed_call_leaves_no_file_and_a_usable_context(case, ref, name, tmp_path):
    good, missing = tmp_path / "good", tmp_path / "missing"
    good.mkdir()
    with sizes():
        attempts = [lambda: getattr(case, name)(0, missing)]
        if name != "sam":  # the second file of a group cannot be opened: the first does not stay
            attempts.append(lambda: getattr(case, name)(0, good, missing))
        for attempt in attempts:
            with pytest.raises(RuntimeError, match="cannot write"):
                attempt()
            assert not missing.exists() and os.listdir(good) == []
            assert run(case, name, 0, good)[0] == ref[name][0][0]
