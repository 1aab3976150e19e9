"""``--sorted-bam`` on the GPU: the golden run through the CLI (tests/golden/sam_out: the reference's own files) with the device deflate
and with ``MIRGE_BAM_DEFLATE=host``, and without the switch; ``mirge_bam_write_device`` against ``bam_export.format_bam_host`` on a few
hundred unique reads with a row of 1500 copies, ties, positions around the bin boundaries and an N, at block sizes 256, 4096 and the
default, and at header lengths of every residue modulo the probe distance; a sample of all-distinct reads, which needs no stored
block (the stored fallback itself: tests/test_bam_deflate_gpu.py).  Files are read back through tests/bam_reader.py."""
import os

import numpy as np
import pytest

import mirge3_amd  # noqa: F401
from mirge3_amd import _ffi, bam_export, sam_export
from mirge3_amd.cascade import Cascade
from mirge3_amd.seqio import FlatSeqs, Library

import bam_reader
from test_sam_out import GOLDEN, ORG, golden_inputs
from test_sam_out_gpu import OTHER_OUTPUTS, _cli, _fuzz_reads, _rnd
from test_sorted_bam import HEADER_CASES, expected_lines, golden_bodies, golden_header, header_of_length

pytestmark = pytest.mark.gpu


def check_file(bam: bytes, bai: bytes, n_ref: int, want_lines, host_bam: bytes, rng=None):
    """every member well-formed (read_bgzf), the records and the uncompressed stream those of format_bam_host, the .bai the tests'
    builder's for the file's actual member offsets, region queries through it like a brute-force scan"""
    d = bam_reader.decode_bam(bam)
    assert d["lines"] == want_lines
    h = bam_reader.decode_bam(host_bam)
    assert b"".join(m["payload"] for m in d["members"]) == b"".join(m["payload"] for m in h["members"])
    assert [r[:3] for r in d["recs"]] == [r[:3] for r in h["recs"]]
    assert bai == bam_reader.build_bai(n_ref, d["recs"])
    if rng is not None and d["recs"]:
        idx = bam_reader.parse_bai(bai)
        for q in range(60):
            r = d["recs"][int(rng.integers(0, len(d["recs"])))]
            beg = max(0, r[1] + int(rng.integers(-40, 40)))
            end = beg + int(rng.choice([1, 30, 20000, 1 << 20]))
            assert bam_reader.query(idx, d["recs"], r[0], beg, end) == bam_reader.brute(d["recs"], r[0], beg, end)
    return d


# ---------------------------------------------------------------------------------------------------------------------
# 1. the golden case through the CLI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sorted_bam")
    _, samples, seqs, counts = golden_inputs()
    files = []
    for s, nm in enumerate(samples):
        p = tmp / f"{nm}.fastq"
        with open(p, "w") as fh:
            k = 0
            for seq, row in zip(seqs, counts):
                for _ in range(int(row[s])):
                    fh.write(f"@r{k}\n{seq}\n+\n{'I' * len(seq)}\n")
                    k += 1
        files.append(str(p))
    header, names = golden_header()
    hfile = tmp / "header.sam"
    hfile.write_bytes(header)
    base = ["-s", ",".join(files), "-lib", os.path.join(GOLDEN, "libs"), "-on", ORG, "-db", "miRBase", "-o", str(tmp), "-shh"]
    old = os.environ.pop("MIRGE_BAM_DEFLATE", None)
    try:
        _cli(base + ["-dn", "device", "--sorted-bam", "--sam-header", str(hfile)])
        os.environ["MIRGE_BAM_DEFLATE"] = "host"
        _cli(base + ["-dn", "host", "--sorted-bam", "--sam-header", str(hfile)])
        del os.environ["MIRGE_BAM_DEFLATE"]
        _cli(base + ["-dn", "plain"])
    finally:
        os.environ.pop("MIRGE_BAM_DEFLATE", None)
        if old is not None:
            os.environ["MIRGE_BAM_DEFLATE"] = old
    return tmp, samples, header, names


@pytest.mark.parametrize("route", ["device", "host"])
def test_cli_golden_files(golden_runs, route):
    tmp, samples, header, names = golden_runs
    bodies = golden_bodies()
    for nm in samples:
        bam, bai = (tmp / route / f"{nm}_sorted.bam").read_bytes(), (tmp / route / f"{nm}_sorted.bai").read_bytes()
        host_bam, _ = bam_export.format_bam_host(bodies[nm], header)
        d = check_file(bam, bai, len(names), expected_lines(bodies[nm], names), host_bam)
        assert d["text"] == bam_export.header_text(header) and [r[0] for r in d["refs"]] == names
        if route == "device":
            assert all(m["single"] and m["btype"] == 1 for m in d["members"][:-1])


def test_cli_without_the_switch_writes_no_bam_and_the_same_other_files(golden_runs):
    tmp = golden_runs[0]
    assert not [f for f in os.listdir(tmp / "plain") if f.endswith((".bam", ".bai", ".sam"))]
    assert not [f for f in os.listdir(tmp / "device") if f.endswith(".sam")]  # independent of --sam-out
    assert sorted(f for f in os.listdir(tmp / "device") if not f.endswith((".bam", ".bai"))) == sorted(os.listdir(tmp / "plain"))
    for f in OTHER_OUTPUTS:
        assert (tmp / "device" / f).read_bytes() == (tmp / "plain" / f).read_bytes(), f


# ---------------------------------------------------------------------------------------------------------------------
# 2. fuzzer: the device call against format_bam_host
# ---------------------------------------------------------------------------------------------------------------------
EDGES = [1 << 14, 1 << 17, 1 << 20, 1 << 23, 1 << 26]


def _bam_libs(rng):
    """one segment per reference, either strand, coordinates below 2^29 and often around a bin boundary; the first three snoRNAs
    share one stretch of chr1 (plus, minus, plus) so that reads of them tie"""
    def head(name, length, i, g=None, minus=None):
        fixed_g = g is not None
        if int(rng.integers(0, 12)) == 0 and not fixed_g:
            return name  # no lift: no record
        if not fixed_g:
            g = EDGES[i % 5] * int(rng.integers(1, 3)) - int(rng.integers(0, length)) if rng.random() < 0.6 else int(rng.integers(1000, 1 << 28))
            minus = bool(rng.integers(0, 2))
        return f"{name} chr{1 if fixed_g else 1 + i % 5} segs:1-{length} cds:{'-' if minus else '+'}:{g}-{g + length - 1}"

    def lib(prefix, n, length, fixed=()):
        seqs = [_rnd(rng, length) for _ in range(n)]
        names = [f"{prefix}{i}" for i in range(n)]
        return Library(names, FlatSeqs.from_list(seqs), [head(nm, length, i, *(fixed[i] if i < len(fixed) else ())) for i, nm in enumerate(names)])
    g0 = (1 << 14) - 40
    mir = lib("miR-", 24, 22)
    hseq = [_rnd(rng, 15) + m + _rnd(rng, 50) for m in mir.seqs.to_list()[:12]]
    hp = Library([f"mir-{i}" for i in range(12)], FlatSeqs.from_list(hseq), [head(f"mir-{i}", len(hseq[i]), i) for i in range(12)])
    return {"mirna": mir, "hairpin": hp, "mature_trna": lib("tRNA-", 4, 74), "pre_trna": lib("pre-tRNA-", 4, 92),
            "snorna": lib("SNO", 12, 140, fixed=[(g0, False), (g0, True), (g0, False)]), "rrna": lib("RR", 6, 400),
            "ncrna_others": lib("NC", 12, 420), "mrna": lib("ENST", 16, 600)}


@pytest.fixture(scope="module")
def fuzz_case():
    rng = np.random.Generator(np.random.PCG64(88002))
    libs = _bam_libs(rng)
    sno = libs["snorna"].seqs.to_list()
    tie = [sno[0][10:30], sno[2][10:30], sno[1][140 - 30:140 - 10]]  # all three start at g0 + 10: plus, plus, minus
    reads = sorted({r for r in _fuzz_reads(rng, libs) if len(r) <= 64} | set(tie))  # (a 300-nt read's QNAME is an error: no BAM)
    ctx = _ffi.Context(0)
    casc = Cascade(ctx, libs)
    S = 2
    want = rng.integers(0, 6, size=(len(reads), S))
    want[:, 0] = np.maximum(want[:, 0], 1)
    for r in tie:
        want[reads.index(r), :] = (3, 2)
    want[reads.index(tie[0]), 0] = 1500  # digit bands 1 to 4; one row spans many blocks
    ent = [(i, s) for i in range(len(reads)) for s in range(S) if want[i, s] > 0]
    raw = _ffi.DeviceReads.pack(ctx, FlatSeqs.from_list([reads[i] for i, _ in ent]))
    uniq = raw.collapse(np.asarray([s for _, s in ent], dtype=np.int32), S, weights=np.asarray([want[i, s] for i, s in ent], dtype=np.uint32))
    raw.close()
    res = casc.run(uniq)
    try:
        useq = uniq.unpack().to_list()
        counts, _ = uniq.counts()
        order = rng.permutation(len(useq)).astype(np.int64)
        hp = sam_export.host_passes(casc)
        bodies = [sam_export.format_sam_host(useq, *res.fetch(), counts, order, s, hp, ORG) for s in range(S)]
        names = ["chr3", "chrNoReads", "chr1", "chr5", "chr2", "chr4"]
        header = ("@HD\tVN:1.6\n" + "".join(f"@SQ\tSN:{nm}\tLN:{1 << 29}\n" for nm in names)).encode()
        lines = expected_lines(bodies[0], names)
        keys = [(ln.split("\t")[2], ln.split("\t")[3]) for ln in lines if ln.split("\t")[0].endswith("_0")]
        tied = [ln for ln in lines if ln.split("\t")[0].endswith("_0") and keys.count((ln.split("\t")[2], ln.split("\t")[3])) > 1]
        flags = [ln.split("\t")[1] for ln in tied if ln.split("\t")[3] == str((1 << 14) - 40 + 10)]
        assert flags.count("0") >= 2 and flags.count("16") >= 1, flags          # two on one strand, one on the other, one position
        assert any("N" in ln.split("\t")[9] for ln in lines) and bodies[0].count(b"_1499\t") == 1
        ends = {int(ln.split("\t")[3]) - 1 + len(ln.split("\t")[9]) for ln in lines}
        starts = {int(ln.split("\t")[3]) - 1 for ln in lines}
        edges = [m * e for e in EDGES for m in (1, 2)]
        assert any(e - 40 < x <= e for e in edges for x in ends) and any(e - 40 < x < e for e in edges for x in starts)  # just under a boundary
        yield dict(casc=casc, uniq=uniq, res=res, order=order, bodies=bodies, header=header, names=names, S=S)
    finally:
        res.close(); uniq.close(); casc.close()


@pytest.mark.parametrize("route", ["device", "host"])
@pytest.mark.parametrize("block", [256, 4096, None], ids=["block256_chunk7", "block4096", "default_block"])
def test_device_equals_format_bam_host(fuzz_case, block, route, tmp_path, monkeypatch):
    for var in ("MIRGE_BAM_BLOCK_BYTES", "MIRGE_BAM_CHUNK_BLOCKS", "MIRGE_BAM_DEFLATE"):
        monkeypatch.delenv(var, raising=False)
    if block:
        monkeypatch.setenv("MIRGE_BAM_BLOCK_BYTES", str(block))
    if block == 256:
        monkeypatch.setenv("MIRGE_BAM_CHUNK_BLOCKS", "7")
    if route == "host":
        monkeypatch.setenv("MIRGE_BAM_DEFLATE", "host")
    f = fuzz_case
    rng = np.random.Generator(np.random.PCG64(5))
    for s in range(f["S"]):
        bam_path, bai_path = tmp_path / f"S{s}_sorted.bam", tmp_path / f"S{s}_sorted.bai"
        n_rec, n_stream, n_file = bam_export.write_sample(f["casc"], f["uniq"], f["res"], f["order"], s, bam_path, bai_path, f["header"], ORG, threads=4)
        host_bam, _ = bam_export.format_bam_host(f["bodies"][s], f["header"], block_bytes=block or bam_export.BLOCK_BYTES)
        want = expected_lines(f["bodies"][s], f["names"])
        d = check_file(bam_path.read_bytes(), bai_path.read_bytes(), len(f["names"]), want, host_bam, rng)
        assert n_rec == len(want) and n_file == os.path.getsize(bam_path) and n_stream == sum(len(m["payload"]) for m in d["members"])
        if block:
            assert d["block"] == block
        if route == "device" and block != 256 and s == 0:  # 1500 copies of one record: matches, not literals
            assert n_file < n_stream // 2, (n_file, n_stream)


@pytest.mark.parametrize("block,want", HEADER_CASES, ids=[f"block{b}_H{w}" for b, w in HEADER_CASES])
def test_header_length_against_the_records(fuzz_case, block, want, tmp_path, monkeypatch):
    """where the header ends inside a block and inside a probe's 32 bytes decides which probe writes the first records"""
    for var in ("MIRGE_BAM_BLOCK_BYTES", "MIRGE_BAM_CHUNK_BLOCKS", "MIRGE_BAM_DEFLATE"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("MIRGE_BAM_BLOCK_BYTES", str(block))
    f = fuzz_case
    header = header_of_length(f["header"], block, want)
    H = len(bam_export.header_blob(header)[0])
    assert H % block == want and (block != 256 or H % 32 == want % 32)
    for s in range(f["S"]):
        bam_path, bai_path = tmp_path / f"S{s}_sorted.bam", tmp_path / f"S{s}_sorted.bai"
        n_rec, n_stream, n_file = bam_export.write_sample(f["casc"], f["uniq"], f["res"], f["order"], s, bam_path, bai_path, header, ORG, threads=4)
        host_bam, _ = bam_export.format_bam_host(f["bodies"][s], header, block_bytes=block)
        want_lines = expected_lines(f["bodies"][s], f["names"])
        d = check_file(bam_path.read_bytes(), bai_path.read_bytes(), len(f["names"]), want_lines, host_bam)
        assert d["block"] == block and n_rec == len(want_lines) and n_file == os.path.getsize(bam_path)
        assert n_stream == sum(len(m["payload"]) for m in d["members"]) > H


def test_device_errors_name_the_chromosome_and_write_nothing(fuzz_case, tmp_path):
    f = fuzz_case
    header = b"@SQ\tSN:chr3\tLN:536870912\n@SQ\tSN:chr2\tLN:536870912\n@SQ\tSN:chr4\tLN:536870912\n@SQ\tSN:chr5\tLN:536870912\n"
    with pytest.raises(Exception, match="chr1"):
        bam_export.write_sample(f["casc"], f["uniq"], f["res"], f["order"], 0, tmp_path / "x.bam", tmp_path / "x.bai", header, ORG)
    assert not os.listdir(tmp_path)


# ---------------------------------------------------------------------------------------------------------------------
# 3. all-distinct reads with count 1
# ---------------------------------------------------------------------------------------------------------------------
def test_all_distinct_reads_need_no_stored_block(tmp_path, monkeypatch):
    """Even when no record repeats, every record holds a run of QUAL bytes and the same fixed fields, so the fixed-Huffman block is
    shorter than the stored one: the fallback is provably not needed here, and BTYPE says so (01 in every member).  The fallback's
    arithmetic is what keeps BSIZE below 65536 whatever the data; read_bgzf checks BSIZE, CRC-32 and ISIZE of every member."""
    for var in ("MIRGE_BAM_BLOCK_BYTES", "MIRGE_BAM_CHUNK_BLOCKS", "MIRGE_BAM_DEFLATE"):
        monkeypatch.delenv(var, raising=False)
    rng = np.random.Generator(np.random.PCG64(99))
    seqs = [_rnd(rng, 600) for _ in range(64)]
    names = [f"ENST{i}" for i in range(64)]
    mrna = Library(names, FlatSeqs.from_list(seqs), [f"{nm} chr1 segs:1-600 cds:+:{1000 + 700 * i}-{1599 + 700 * i}" for i, nm in enumerate(names)])
    tiny = lambda p: Library([p + "0"], FlatSeqs.from_list([_rnd(rng, 80)]), [p + "0"])
    libs = {"mirna": tiny("miR-"), "hairpin": tiny("mir-"), "mature_trna": tiny("tRNA-"), "pre_trna": tiny("pre-"), "snorna": tiny("SNO"),
            "rrna": tiny("RR"), "ncrna_others": tiny("NC"), "mrna": mrna}
    reads = sorted({seqs[int(rng.integers(0, 64))][o:o + 25] for o in rng.integers(0, 575, size=2600).tolist()})
    ctx = _ffi.Context(0)
    casc = Cascade(ctx, libs)
    raw = _ffi.DeviceReads.pack(ctx, FlatSeqs.from_list(reads))
    uniq = raw.collapse(np.zeros(len(reads), dtype=np.int32), 1)
    raw.close()
    res = casc.run(uniq)
    try:
        useq = uniq.unpack().to_list()
        counts, _ = uniq.counts()
        order = np.arange(len(useq), dtype=np.int64)
        header = b"@SQ\tSN:chr1\tLN:536870912\n"
        body = sam_export.format_sam_host(useq, *res.fetch(), counts, order, 0, sam_export.host_passes(casc), ORG)
        bam_export.write_sample(casc, uniq, res, order, 0, tmp_path / "d.bam", tmp_path / "d.bai", header, ORG)
    finally:
        res.close(); uniq.close(); casc.close()
    assert int(counts.max()) == 1 and body.count(b"\n") > 400
    host_bam, _ = bam_export.format_bam_host(body, header)
    d = check_file((tmp_path / "d.bam").read_bytes(), (tmp_path / "d.bai").read_bytes(), 1, expected_lines(body, ["chr1"]), host_bam)
    assert len(d["members"]) >= 3
    for m in d["members"][:-1]:
        assert m["bsize"] < 65536 and m["single"] and m["btype"] == 1 and m["bsize"] < len(m["payload"])
