"""``MIRGE_BAM_DEFLATE=dynamic`` on the GPU: the assertions of tests/test_bam_dynamic_hostsim.py through ``bam_export.write_sample``
(every file against the file of the default route on the same stream: tests/deflate_dyn_probe.py), the ``.bai`` through
``test_sorted_bam_gpu.check_file``, the code-length builder through ``mirge_bam_huffman_probe`` against the host harness, the CLI's
``--bam-deflate dynamic`` once, and the refusal of an unknown route."""
import os

import numpy as np
import pytest

import mirge3_amd  # noqa: F401
from mirge3_amd import _ffi, bam_export, sam_export
from mirge3_amd.cascade import Cascade
from mirge3_amd.seqio import FlatSeqs

import bam_reader
import deflate_dyn_probe as dy
import deflate_probe as dp
from test_bam_deflate_gpu import empty_sample, gctx  # noqa: F401  (fixtures)
from test_bam_dynamic_hostsim import sim_lengths
from test_sam_out import GOLDEN, ORG, golden_inputs
from test_sam_out_gpu import OTHER_OUTPUTS, _cli
from test_sorted_bam import HEADER_CASES, expected_lines, golden_bodies, golden_header, header_of_length
from test_sorted_bam_gpu import check_file

pytestmark = pytest.mark.gpu
ENV = ("MIRGE_BAM_BLOCK_BYTES", "MIRGE_BAM_CHUNK_BLOCKS", "MIRGE_BAM_DEFLATE")


def write(g, sample, header, block, route, tmp_path, monkeypatch, chunk=None):
    """-> (the .bam, the .bai, write_sample's triple) of one sample at this block size on this route"""
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    if block != dp.DEFAULT_BLOCK:
        monkeypatch.setenv("MIRGE_BAM_BLOCK_BYTES", str(block))
    if chunk:
        monkeypatch.setenv("MIRGE_BAM_CHUNK_BLOCKS", str(chunk))
    if route:
        monkeypatch.setenv("MIRGE_BAM_DEFLATE", route)
    bam_path, bai_path = tmp_path / f"{route}_sorted.bam", tmp_path / f"{route}_sorted.bai"
    got = bam_export.write_sample(g["casc"], g["uniq"], g["res"], g["order"], sample, bam_path, bai_path, header, ORG)
    return bam_path.read_bytes(), bai_path.read_bytes(), got


def both(g, sample, header, block, tmp_path, monkeypatch, chunk=None):
    """-> ((file, decode_bam, .bai) of the dynamic route, the same of the default route)"""
    out = []
    for route in ("dynamic", None):
        bam, bai, got = write(g, sample, header, block, route, tmp_path, monkeypatch, chunk)
        d = bam_reader.decode_bam(bam)  # (every member's BSIZE, CRC-32 and ISIZE are checked there)
        assert got == (len(d["lines"]), sum(len(m["payload"]) for m in d["members"]), len(bam))
        out.append((bam, d, bai))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# records: the golden reads, one row raised to 1234 copies
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_case(gctx):
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

    def bodies_of(uniq, res):
        useq = uniq.unpack().to_list()
        dev_counts, _ = uniq.counts()
        order = np.argsort(np.asarray(useq, dtype=object), kind="stable").astype(np.int64)  # the frame: the sorted union
        hp = sam_export.host_passes(casc)
        return useq, order, [sam_export.format_sam_host(useq, *res.fetch(), dev_counts, order, s, hp, ORG) for s in range(S)]

    uniq, res = annotate(counts)
    _useq, _order, bodies = bodies_of(uniq, res)
    heavy = seqs.index(bodies[0].decode().split("\n")[3].split("\t")[0].rsplit("_", 1)[0])  # a read that writes lines in sample 0
    res.close(); uniq.close()
    counts[heavy, 0] = 1234
    uniq, res = annotate(counts)
    try:
        _useq, order, bodies = bodies_of(uniq, res)
        assert bodies[0].count(b"_1233\t") == 1
        header, names = golden_header()
        yield dict(casc=casc, uniq=uniq, res=res, order=order, bodies=bodies, header=header, names=names)
    finally:
        res.close(); uniq.close(); casc.close()


@pytest.mark.parametrize("block", [256, 4096, 65280], ids=["block256_chunk7", "block4096", "default_block"])
def test_records(golden_case, block, tmp_path, monkeypatch):
    g = golden_case
    (bam, d, bai), (fbam, fd, fbai) = both(g, 0, g["header"], block, tmp_path, monkeypatch, chunk=7 if block == 256 else None)
    want = expected_lines(g["bodies"][0], g["names"])
    assert d["lines"] == fd["lines"] == want
    res = dy.check_dynamic(d, bam, fd, fbam)
    print(f"block {block}: members stored / fixed / dynamic {res['btypes']}, left out {res['left_out']}; {len(bam)} bytes against {len(fbam)} fixed")
    if block >= 4096:
        assert res["btypes"][2] >= 1
    host_bam, _ = bam_export.format_bam_host(g["bodies"][0], g["header"], block_bytes=block)
    check_file(bam, bai, len(g["names"]), want, host_bam, np.random.Generator(np.random.PCG64(6)))
    assert d["block"] == block or block == 65280


@pytest.mark.parametrize("block,want", [HEADER_CASES[5], HEADER_CASES[-1]], ids=lambda v: str(v))
def test_header_length_against_the_records(golden_case, block, want, tmp_path, monkeypatch):
    g = golden_case
    header = header_of_length(g["header"], block, want)
    assert len(bam_export.header_blob(header)[0]) % block == want
    (bam, d, bai), (fbam, fd, _) = both(g, 1, header, block, tmp_path, monkeypatch)
    lines = expected_lines(g["bodies"][1], g["names"])
    assert d["lines"] == fd["lines"] == lines and len(lines) > 20
    dy.check_dynamic(d, bam, fd, fbam)
    check_file(bam, bai, len(g["names"]), lines, bam_export.format_bam_host(g["bodies"][1], header, block_bytes=block)[0])


def test_cli_flag_writes_the_same_records_in_a_file_no_larger(tmp_path):
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
        os.environ["MIRGE_BAM_DEFLATE"] = "host"  # the flag wins over the environment
        _cli(base + ["-dn", "flag", "--bam-deflate", "dynamic"])
    finally:
        os.environ.pop("MIRGE_BAM_DEFLATE", None)
        os.environ.update({v: x for v, x in old.items() if x is not None})
    bodies = golden_bodies()
    for nm in samples:
        got, plain = (tmp_path / "flag" / f"{nm}_sorted.bam").read_bytes(), (tmp_path / "plain" / f"{nm}_sorted.bam").read_bytes()
        d, pd = bam_reader.decode_bam(got), bam_reader.decode_bam(plain)
        assert d["lines"] == pd["lines"] == expected_lines(bodies[nm], names) and len(got) <= len(plain)
        res = dy.check_dynamic(d, got, pd, plain)
        assert res["btypes"][2] >= 1  # (zlib on the host would write members the device's parse does not: check_dynamic holds them against it)
        check_file(got, (tmp_path / "flag" / f"{nm}_sorted.bai").read_bytes(), len(names), d["lines"], bam_export.format_bam_host(bodies[nm], header)[0])
    for f in OTHER_OUTPUTS:
        assert (tmp_path / "flag" / f).read_bytes() == (tmp_path / "plain" / f).read_bytes(), f


# ---------------------------------------------------------------------------------------------------------------------
# payloads that records cannot produce
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [64, 4096, dp.DEFAULT_BLOCK])
def test_high_bytes(empty_sample, block, tmp_path, monkeypatch):
    header, span = dp.high_distinct() if block == dp.DEFAULT_BLOCK else dp.high_random()
    (bam, d, bai), (fbam, fd, _) = both(empty_sample, 1, header, block, tmp_path, monkeypatch)
    assert bai == dp.EMPTY_BAI
    res = dy.check_dynamic(d, bam, fd, fbam)
    free = dy.check_high_dynamic(res, d, header, span, block)
    sizes = sorted(m["bsize"] - 26 for _u, m, *_ in res["dynamic"])
    print(f"block {block}: {free} match-free blocks inside the payload; members stored / fixed / dynamic {res['btypes']}; dynamic cdata {sizes[:1]} .. {sizes[-1:]} bytes")


@pytest.fixture(scope="module")
def codes():
    return dp.codes_payload()


@pytest.mark.parametrize("block", [dp.DEFAULT_BLOCK, 4096])
def test_every_length_and_distance_code(empty_sample, codes, block, tmp_path, monkeypatch):
    header, _span, plants = codes
    (bam, d, _), (fbam, fd, _) = both(empty_sample, 1, header, block, tmp_path, monkeypatch)
    res = dy.check_dynamic(d, bam, fd, fbam)
    len_codes, dist_codes = dy.check_plants(res, d, bam, plants) if block == dp.DEFAULT_BLOCK else dy.codes_seen(res)
    print(f"block {block}: members stored / fixed / dynamic {res['btypes']}; over the dynamic ones length codes {sorted(len_codes)}, distance codes {sorted(dist_codes)}")


@pytest.mark.parametrize("rem", dp.SHORT_REMAINDERS)
def test_short_last_member(empty_sample, rem, tmp_path, monkeypatch):
    header, _span = dp.short_payload(rem)
    (bam, d, _), (fbam, fd, _) = both(empty_sample, 1, header, dp.SHORT_BLOCK, tmp_path, monkeypatch)
    res = dy.check_dynamic(d, bam, fd, fbam)
    blob = bam_export.header_blob(header)[0]
    assert [len(m["payload"]) for m in d["members"][:-1]] == [dp.SHORT_BLOCK] * 2 + ([rem] if rem else [])
    assert b"".join(m["payload"] for m in d["members"]) == blob and res["btypes"][2] >= 2


# ---------------------------------------------------------------------------------------------------------------------
# the builder alone, and the refusal
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,max_bits,counts", dy.builder_cases(), ids=[c[0] for c in dy.builder_cases()])
def test_builder(gctx, name, max_bits, counts):
    lengths = np.stack([_ffi.bam_huffman_probe(gctx, c, max_bits) for c in counts])
    excess = [dy.check_lengths(c, x, max_bits) for c, x in zip(counts, lengths)]
    acted = [e for e in excess if e is not None]
    print(f"{name}: {len(counts)} vectors, the limit acted on {len(acted)}; excess over package-merge: {sorted(acted)[-5:]} at most")
    assert np.array_equal(lengths, sim_lengths(counts, max_bits)), "the device and the host harness disagree"


def test_builder_refuses_what_cannot_be_coded(gctx):
    for counts, max_bits in ((np.ones(289, np.uint32), 15), (np.ones(19, np.uint32), 4), (np.ones(19, np.uint32), 16), (np.ones(0, np.uint32), 7)):
        with pytest.raises(RuntimeError, match="mirge_bam_huffman_probe"):
            _ffi.bam_huffman_probe(gctx, counts, max_bits)


def test_unknown_route_is_refused_with_all_three_names(empty_sample, tmp_path, monkeypatch):
    header, _span = dp.short_payload(0)
    with pytest.raises(RuntimeError, match="MIRGE_BAM_DEFLATE is 'device', 'dynamic' or 'host'"):
        write(empty_sample, 1, header, dp.DEFAULT_BLOCK, "fast", tmp_path, monkeypatch)
    assert not os.listdir(tmp_path)
