"""``MIRGE_BAM_DEFLATE=tight`` on the GPU, through ``bam_export.write_sample``: the device's file is, byte for byte, the file the same
kernel source compiled for the host makes of the same stream (tests/hostsim/bam_sim.cpp through ``test_sorted_bam_hostsim.run`` with
``deflate == 3``; what that file must satisfy is asserted in tests/test_bam_tight_hostsim.py and, once more, here).  The ``.bai`` goes
through ``test_sorted_bam_gpu.check_file``; the variable, the refusal of an unknown route and the CLI's ``--bam-deflate tight`` run
once each."""
import os

import numpy as np
import pytest

import mirge3_amd  # noqa: F401
from mirge3_amd import _ffi, bam_export, sam_export
from mirge3_amd.cascade import Cascade
from mirge3_amd.seqio import FlatSeqs

import bam_reader
import deflate_probe as dp
import deflate_tight_probe as tp
from test_bam_deflate_gpu import empty_sample, gctx  # noqa: F401  (fixtures)
from test_bam_dynamic_gpu import ENV, write
from test_sam_out import GOLDEN, ORG, golden_inputs
from test_sam_out_gpu import OTHER_OUTPUTS, _cli
from test_sam_out_hostsim import _oracle_annotation
from test_sorted_bam import expected_lines, golden_bodies, golden_header
from test_sorted_bam_gpu import check_file
from test_sorted_bam_hostsim import run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden_case(gctx):
    """the golden reads, one row raised to 1234 copies (as tests/test_bam_dynamic_gpu.py's), with what the host build needs of the device's run"""
    libs, samples, seqs, counts = golden_inputs()
    counts = counts.copy()
    S = len(samples)
    casc = Cascade(gctx, libs)

    def annotate(cnt):
        ent = [(i, s) for i in range(len(seqs)) for s in range(S) if cnt[i, s] > 0]
        raw = _ffi.DeviceReads.pack(gctx, FlatSeqs.from_list([seqs[i] for i, _ in ent]))
        uniq = raw.collapse(np.asarray([s for _, s in ent], dtype=np.int32), S, weights=np.asarray([cnt[i, s] for i, s in ent], dtype=np.uint32))
        raw.close()
        return uniq, casc.run(uniq)

    def frame(uniq, res):
        useq = uniq.unpack().to_list()
        dev_counts, _ = uniq.counts()
        order = np.argsort(np.asarray(useq, dtype=object), kind="stable").astype(np.int64)  # the sorted union
        ann = res.fetch()
        return useq, dev_counts, order, ann, sam_export.format_sam_host(useq, *ann, dev_counts, order, 0, sam_export.host_passes(casc), ORG)

    uniq, res = annotate(counts)
    body = frame(uniq, res)[4]
    heavy = seqs.index(body.decode().split("\n")[3].split("\t")[0].rsplit("_", 1)[0])  # a read that writes lines in sample 0
    res.close(); uniq.close()
    counts[heavy, 0] = 1234
    uniq, res = annotate(counts)
    try:
        useq, dev_counts, order, ann, body = frame(uniq, res)
        assert body.count(b"_1233\t") == 1
        header, names = golden_header()
        yield dict(casc=casc, uniq=uniq, res=res, order=order, body=body, header=header, names=names,
                   host=dict(libs=libs, seqs=useq, ann=ann, counts=dev_counts, order=order))
    finally:
        res.close(); uniq.close(); casc.close()


@pytest.fixture(scope="module")
def host_empty():
    """the host build's sample without rows: its stream is the header alone, as the device's"""
    libs, _samples, seqs, counts = golden_inputs()
    return dict(libs=libs, seqs=seqs, ann=_oracle_annotation(libs, seqs), counts=np.zeros_like(counts), order=np.arange(len(seqs)))


def host_file(h, header, block, sample=0):
    members, _n_rec = run(h["libs"], h["seqs"], *h["ann"], h["counts"], h["order"], sample, header, block, 3)
    return members + bam_reader.EOF_BLOCK


@pytest.mark.parametrize("block", [256, 4096, 65280])
def test_records_are_the_host_builds_bytes(golden_case, block, tmp_path, monkeypatch):
    g = golden_case
    bam, bai, got = write(g, 0, g["header"], block, "tight", tmp_path, monkeypatch, chunk=7)
    want = expected_lines(g["body"], g["names"])
    d = bam_reader.decode_bam(bam)  # (every member's BSIZE, CRC-32 and ISIZE are checked there)
    assert d["lines"] == want
    assert got == (len(want), sum(len(m["payload"]) for m in d["members"]), len(bam))
    fbam, _fbai, _ = write(g, 0, g["header"], block, None, tmp_path, monkeypatch, chunk=7)
    members = tp.check_tight(d, bam, bam_reader.decode_bam(fbam))
    print(f"block {block}: members stored / fixed / dynamic {tp.btypes(members)}; {len(bam)} bytes against {len(fbam)} of the default route")
    host = host_file(g["host"], g["header"], block)
    assert [m["payload"] for m in bam_reader.decode_bam(host)["members"]] == [m["payload"] for m in d["members"]], "the host build saw another stream"
    assert bam == host, "the device and the host build disagree"
    check_file(bam, bai, len(g["names"]), want, bam_export.format_bam_host(g["body"], g["header"], block_bytes=block)[0], np.random.Generator(np.random.PCG64(6)))


def test_equal_bytes_are_the_host_builds_bytes(empty_sample, host_empty, tmp_path, monkeypatch):
    header, _span = tp.equal_bytes(dp.DEFAULT_BLOCK, dp.DEFAULT_BLOCK)
    bam, bai, _got = write(empty_sample, 1, header, dp.DEFAULT_BLOCK, "tight", tmp_path, monkeypatch)
    assert bai == dp.EMPTY_BAI and bam == host_file(host_empty, header, dp.DEFAULT_BLOCK)
    fbam, _, _ = write(empty_sample, 1, header, dp.DEFAULT_BLOCK, None, tmp_path, monkeypatch)
    tp.check_tight(bam_reader.decode_bam(bam), bam, bam_reader.decode_bam(fbam))


def test_short_last_member_is_the_host_builds_bytes(empty_sample, host_empty, tmp_path, monkeypatch):
    header, _span = dp.short_payload(257)
    bam, _bai, _got = write(empty_sample, 1, header, dp.SHORT_BLOCK, "tight", tmp_path, monkeypatch)
    assert bam == host_file(host_empty, header, dp.SHORT_BLOCK)
    d = bam_reader.decode_bam(bam)
    assert [len(m["payload"]) for m in d["members"][:-1]] == [dp.SHORT_BLOCK] * 2 + [257]
    assert b"".join(m["payload"] for m in d["members"]) == bam_export.header_blob(header)[0]


def test_unknown_route_is_refused_with_all_four_names(empty_sample, tmp_path, monkeypatch):
    header, _span = dp.short_payload(0)
    with pytest.raises(RuntimeError, match="MIRGE_BAM_DEFLATE is 'device', 'dynamic', 'tight' or 'host'"):
        write(empty_sample, 1, header, dp.DEFAULT_BLOCK, "fast", tmp_path, monkeypatch)
    assert not os.listdir(tmp_path)


def test_cli_flag_wins_over_the_variable(tmp_path):
    """(the CLI is what this test is about: one run with the flag under MIRGE_BAM_DEFLATE=host, one plain run)"""
    _, samples, seqs, counts = golden_inputs()
    files = []
    for s, nm in enumerate(samples):
        p = tmp_path / f"{nm}.fastq"
        with open(p, "w") as fh:
            for k, (seq, row) in enumerate(zip(seqs, counts)):
                for c in range(int(row[s])):
                    fh.write(f"@r{k}_{c}\n{seq}\n+\n{'I' * len(seq)}\n")
        files.append(str(p))
    header, names = golden_header()
    hfile = tmp_path / "header.sam"
    hfile.write_bytes(header)
    base = ["-s", ",".join(files), "-lib", os.path.join(GOLDEN, "libs"), "-on", ORG, "-db", "miRBase", "-o", str(tmp_path), "-shh", "--sorted-bam", "--sam-header", str(hfile)]
    old = {v: os.environ.pop(v, None) for v in ENV}
    try:
        _cli(base + ["-dn", "plain"])
        os.environ["MIRGE_BAM_DEFLATE"] = "host"
        _cli(base + ["-dn", "flag", "--bam-deflate", "tight"])
        _cli(base + ["-dn", "host"])
    finally:
        os.environ.pop("MIRGE_BAM_DEFLATE", None)
        os.environ.update({v: x for v, x in old.items() if x is not None})
    bodies = golden_bodies()
    for nm in samples:
        got, plain, host = ((tmp_path / dn / f"{nm}_sorted.bam").read_bytes() for dn in ("flag", "plain", "host"))
        d, pd = bam_reader.decode_bam(got), bam_reader.decode_bam(plain)
        assert d["lines"] == pd["lines"] == expected_lines(bodies[nm], names)
        tp.check_tight(d, got, pd)
        assert got != host and got != plain  # (neither zlib's members nor the default route's)
        check_file(got, (tmp_path / "flag" / f"{nm}_sorted.bai").read_bytes(), len(names), d["lines"], bam_export.format_bam_host(bodies[nm], header)[0])
    for f in OTHER_OUTPUTS:
        assert (tmp_path / "flag" / f).read_bytes() == (tmp_path / "plain" / f).read_bytes(), f
