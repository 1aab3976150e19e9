"""The deflate of ``k_bam_blocks`` on the GPU on payloads that BAM records cannot produce (tests/deflate_probe.py; the same payloads and
assertions as tests/test_bam_deflate_hostsim.py): a sample whose counts are all zero selects no rows, so ``mirge_bam_write_device``
deflates the header alone and an ``@CO`` line of the ``--sam-header`` file is the payload -- the stored fallback (BTYPE 00) and the edge
of its decision, 9-bit literals, every length and distance code the parse can reach, last members of 1 to 257 bytes."""
import os

import numpy as np
import pytest

import mirge3_amd  # noqa: F401
from mirge3_amd import _ffi, bam_export
from mirge3_amd.cascade import Cascade
from mirge3_amd.seqio import FlatSeqs, Library

import bam_reader
import deflate_probe as dp
from test_sam_out import ORG
from test_sam_out_gpu import _rnd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gctx():
    ctx = _ffi.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def empty_sample(gctx):
    """a few reads of one mRNA, all in sample 0 of two: sample 1 writes the header alone"""
    rng = np.random.Generator(np.random.PCG64(98))
    seq = _rnd(rng, 600)
    mrna = Library(["ENST0"], FlatSeqs.from_list([seq]), ["ENST0 chr1 segs:1-600 cds:+:1000-1599"])
    tiny = lambda p: Library([p + "0"], FlatSeqs.from_list([_rnd(rng, 80)]), [p + "0"])
    libs = {"mirna": tiny("miR-"), "hairpin": tiny("mir-"), "mature_trna": tiny("tRNA-"), "pre_trna": tiny("pre-"), "snorna": tiny("SNO"),
            "rrna": tiny("RR"), "ncrna_others": tiny("NC"), "mrna": mrna}
    reads = sorted({seq[o:o + 25] for o in range(0, 500, 37)})
    casc = Cascade(gctx, libs)
    raw = _ffi.DeviceReads.pack(gctx, FlatSeqs.from_list(reads))
    uniq = raw.collapse(np.zeros(len(reads), dtype=np.int32), 2)
    raw.close()
    res = casc.run(uniq)
    try:
        counts, _ = uniq.counts()
        assert counts.shape[1] == 2 and int(counts[:, 0].min()) == 1 and int(counts[:, 1].max()) == 0
        yield dict(casc=casc, uniq=uniq, res=res, order=np.arange(len(uniq), dtype=np.int64))
    finally:
        res.close(); uniq.close(); casc.close()


def deflated(g, header, block, tmp_path, monkeypatch):
    """-> (the file, bam_reader.decode_bam of it): sample 1 through mirge_bam_write_device at this block size"""
    for var in ("MIRGE_BAM_BLOCK_BYTES", "MIRGE_BAM_CHUNK_BLOCKS", "MIRGE_BAM_DEFLATE"):
        monkeypatch.delenv(var, raising=False)
    if block != dp.DEFAULT_BLOCK:
        monkeypatch.setenv("MIRGE_BAM_BLOCK_BYTES", str(block))
    bam_path, bai_path = tmp_path / "h_sorted.bam", tmp_path / "h_sorted.bai"
    got = bam_export.write_sample(g["casc"], g["uniq"], g["res"], g["order"], 1, bam_path, bai_path, header, ORG)
    bam = bam_path.read_bytes()
    assert got == (0, len(bam_export.header_blob(header)[0]), os.path.getsize(bam_path))
    assert bai_path.read_bytes() == dp.EMPTY_BAI
    return bam, bam_reader.decode_bam(bam)  # (every member's BSIZE, CRC-32 and ISIZE are checked there)


@pytest.mark.parametrize("block", [64, 4096, dp.DEFAULT_BLOCK])
def test_high_bytes_are_stored(empty_sample, block, tmp_path, monkeypatch):
    header, span = dp.high_distinct() if block == dp.DEFAULT_BLOCK else dp.high_random()
    bam, d = deflated(empty_sample, header, block, tmp_path, monkeypatch)
    free, inside = dp.check_high(d, bam, header, span, block)
    print(f"block {block}: {free} of {inside} blocks inside the payload are match-free and stored")


@pytest.mark.parametrize("h", dp.EDGE_H)
def test_stored_exactly_when_the_fixed_form_is_no_shorter(empty_sample, h, tmp_path, monkeypatch):
    header, span = dp.edge_payload(h)
    bam, d = deflated(empty_sample, header, dp.EDGE_BLOCK, tmp_path, monkeypatch)
    dp.check_edge(d, bam, header, span, h)


@pytest.fixture(scope="module")
def codes():
    return dp.codes_payload()


@pytest.mark.parametrize("block", [dp.DEFAULT_BLOCK, 4096])
def test_every_length_and_distance_code(empty_sample, codes, block, tmp_path, monkeypatch):
    header, _span, plants = codes
    bam, d = deflated(empty_sample, header, block, tmp_path, monkeypatch)
    len_codes, dist_codes = dp.check_codes(d, bam, header, plants, block)
    print(f"block {block}: length codes {sorted(len_codes)}, distance codes {sorted(dist_codes)}")


@pytest.mark.parametrize("rem", dp.SHORT_REMAINDERS)
def test_short_last_member(empty_sample, rem, tmp_path, monkeypatch):
    header, _span = dp.short_payload(rem)
    bam, d = deflated(empty_sample, header, dp.SHORT_BLOCK, tmp_path, monkeypatch)
    dp.check_short(d, bam, header, rem)
