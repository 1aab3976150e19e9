"""``--bgzf-out`` on the GPU.  ``mirge_bgzf_write`` on every stream of tests/bgzf_cases.py: the device's file is byte for byte the file of
the same kernel compiled for the host (tests/test_bgzf_hostsim.py) -- the file is a function of the stream and the block size -- and the
``host`` route's file inflates to the same stream under the same ``.gzi`` uncompressed offsets.  Then the exporters on the small samples
of test_sam_out_gpu.py and test_coverage_gpu.py: the decompressed files are the plain route's files, the ``.gz`` does not depend on the
chunk, an empty sample is the EOF block alone, a failed call leaves nothing, and the command line end to end."""
import gzip
import os

import pytest

import mirge3_amd  # noqa: F401
from mirge3_amd import _ffi, bgzf, coverage, sam_export

import bgzf_cases
from test_bgzf_hostsim import run as hostsim
from test_coverage import golden_bedgraph
from test_coverage_gpu import ctx, fuzz_case as cov_case  # noqa: F401  (fixtures)
from test_sam_out import GOLDEN, ORG, golden_inputs
from test_sam_out_gpu import _cli, fuzz_case as sam_case  # noqa: F401  (sam_case: a fixture)

pytestmark = pytest.mark.gpu
ENV = ("MIRGE_BGZF_BLOCK_BYTES", "MIRGE_BGZF_DEFLATE", "MIRGE_BGZF_CHUNK_BYTES", "MIRGE_SAM_CHUNK_BYTES", "MIRGE_SAM_TILE_BYTES",
       "MIRGE_COV_CHUNK_BYTES", "MIRGE_COV_TILE_BYTES")


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def _pair(path):
    with open(path, "rb") as a, open(bgzf.gzi_path(path), "rb") as b:
        return a.read(), b.read()


def _no_leftovers(folder):
    assert not [f for f in os.listdir(folder) if f.endswith(".tmp")], os.listdir(folder)


@pytest.mark.parametrize("name", sorted(bgzf_cases.all_cases()))
def test_device_file_is_the_hostsim_file(ctx, name, tmp_path, monkeypatch):
    s, block = bgzf_cases.all_cases()[name]
    want_gz, want_gzi, _ = hostsim(s, block)
    st = bgzf.write_device(ctx, s, tmp_path / "d.gz", block)
    gz, gzi = _pair(tmp_path / "d.gz")
    assert gz == want_gz and gzi == want_gzi
    btypes = bgzf_cases.check_device_file(s, block, gz, gzi, st)
    # more chunks than staging halves: the same file
    monkeypatch.setenv("MIRGE_BGZF_CHUNK_BYTES", str(3 * block))
    bgzf.write_device(ctx, s, tmp_path / "c.gz", block)
    assert _pair(tmp_path / "c.gz") == (gz, gzi)
    # the host route: zlib's members over the same blocks
    monkeypatch.setenv("MIRGE_BGZF_DEFLATE", "host")
    sth = bgzf.write_device(ctx, s, tmp_path / "h.gz", block)
    hgz, hgzi = _pair(tmp_path / "h.gz")
    assert gzip.decompress(hgz) == s
    hm = bgzf.check_index(hgz, hgzi)
    assert [u for _, u in bgzf.read_gzi(hgzi)] == [u for _, u in bgzf.read_gzi(gzi)] and len(hm) == sum(btypes)
    assert sth["file_bytes"] == len(hgz) and sth["members"] == len(hm) and sth["stream_bytes"] == len(s)
    _no_leftovers(tmp_path)
    print(f"{name}: {len(s)} -> {len(gz)} bytes on the device {btypes}, {len(hgz)} through zlib")


def test_a_wrong_route_or_block_size_fails_before_a_file_is_opened(ctx, tmp_path, monkeypatch):
    monkeypatch.setenv("MIRGE_BGZF_DEFLATE", "zlib")
    with pytest.raises(RuntimeError, match="MIRGE_BGZF_DEFLATE"):
        bgzf.write_device(ctx, b"text", tmp_path / "x.gz")
    monkeypatch.delenv("MIRGE_BGZF_DEFLATE")
    for block in (63, 65281):
        with pytest.raises(RuntimeError, match="64 .. 65280"):
            bgzf.write_device(ctx, b"text", tmp_path / "x.gz", block)
    assert not os.listdir(tmp_path)


# ---------------------------------------------------------------------------------------------------------------------
# the exporters
# ---------------------------------------------------------------------------------------------------------------------
HEADER = b"@HD\tVN:1.0\tSO:unsorted\n@CO\tfuzz"


def test_sam_gz_inflates_to_the_plain_file_whatever_the_chunk(sam_case, tmp_path, monkeypatch):
    f = sam_case
    args = (f["casc"], f["uniq"], f["res"], f["order"])
    for s in range(f["S"]):
        plain = tmp_path / f"S{s}.sam"
        n_lines, n_bytes = sam_export.write_sample(*args, s, plain, HEADER, ORG)
        want = plain.read_bytes()
        assert want == HEADER + f["expected"][s]
        monkeypatch.setenv("MIRGE_BGZF_BLOCK_BYTES", "256")
        monkeypatch.setenv("MIRGE_SAM_CHUNK_BYTES", "4096")   # more chunks than halves; the header ends inside the first block
        monkeypatch.setenv("MIRGE_SAM_TILE_BYTES", "256")
        small = tmp_path / f"S{s}.small.sam.gz"
        got = sam_export.write_sample(*args, s, small, HEADER, ORG, bgzf_out=True)
        monkeypatch.delenv("MIRGE_SAM_CHUNK_BYTES")
        monkeypatch.delenv("MIRGE_SAM_TILE_BYTES")
        whole = tmp_path / f"S{s}.sam.gz"
        assert sam_export.write_sample(*args, s, whole, HEADER, ORG, bgzf_out=True) == got
        assert got[:2] == (n_lines, n_bytes)
        gz, gzi = _pair(whole)
        assert _pair(small) == (gz, gzi)
        assert gzip.decompress(gz) == want
        ms = bgzf.check_index(gz, gzi)
        st = got[2]
        assert all(m["single"] and m["bsize"] <= m["isize"] + 31 for m in ms) and len(ms) == (len(want) + 255) // 256
        assert [st["stored"], st["fixed"], st["dynamic"]] == [sum(m["btype"] == t for m in ms) for t in range(3)]
        assert st["file_bytes"] == len(gz) and st["stream_bytes"] == len(want) and st["members"] == len(ms)
        # the host route: the same stream under the same uncompressed offsets
        monkeypatch.setenv("MIRGE_BGZF_DEFLATE", "host")
        hpath = tmp_path / f"S{s}.host.sam.gz"
        sam_export.write_sample(*args, s, hpath, HEADER, ORG, bgzf_out=True)
        hgz, hgzi = _pair(hpath)
        assert gzip.decompress(hgz) == want and [u for _, u in bgzf.read_gzi(hgzi)] == [u for _, u in bgzf.read_gzi(gzi)]
        bgzf.check_index(hgz, hgzi)
        monkeypatch.delenv("MIRGE_BGZF_DEFLATE")
        monkeypatch.delenv("MIRGE_BGZF_BLOCK_BYTES")
        if s == 1:  # the default block: 65280 bytes
            big = tmp_path / "S1.big.sam.gz"
            sam_export.write_sample(*args, s, big, HEADER, ORG, bgzf_out=True)
            bgz, bgzi = _pair(big)
            assert gzip.decompress(bgz) == want and len(bgzf.check_index(bgz, bgzi)) == (len(want) + 65279) // 65280 > 6
    # the sample without a kept row, and no header: the EOF block alone
    empty = tmp_path / "empty.sam.gz"
    assert sam_export.write_sample(*args, 3, empty, b"", ORG, bgzf_out=True)[:2] == (0, 0)
    assert _pair(empty) == (bgzf.EOF_BLOCK, bytes(8))
    _no_leftovers(tmp_path)


@pytest.mark.parametrize("stranded", [False, True], ids=["unstranded", "stranded"])
def test_bedgraph_gz_inflates_to_the_plain_files_whatever_the_chunk(cov_case, stranded, tmp_path, monkeypatch):
    f = cov_case
    args = (f["casc"], f["uniq"], f["res"], f["order"])
    for s in range(f["S"]):
        plain = coverage.sample_paths(tmp_path, f"S{s}", stranded)
        st0 = coverage.write_sample(*args, s, plain, stranded, ORG)
        want = [p.read_bytes() for p in plain]
        monkeypatch.setenv("MIRGE_BGZF_BLOCK_BYTES", "256")
        monkeypatch.setenv("MIRGE_COV_CHUNK_BYTES", "4096")   # more chunks than halves; `split` inside a block-sized stretch
        monkeypatch.setenv("MIRGE_COV_TILE_BYTES", "64")
        small = coverage.sample_paths(tmp_path, f"S{s}.small", stranded, True)
        st1 = coverage.write_sample(*args, s, small, stranded, ORG, bgzf_out=True)
        monkeypatch.delenv("MIRGE_COV_CHUNK_BYTES")
        monkeypatch.delenv("MIRGE_COV_TILE_BYTES")
        whole = coverage.sample_paths(tmp_path, f"S{s}", stranded, True)
        assert str(whole[0]).endswith(".bedgraph.gz")
        st2 = coverage.write_sample(*args, s, whole, stranded, ORG, bgzf_out=True)
        assert st1 == st2 and {k: st2[k] for k in st0} == st0
        monkeypatch.setenv("MIRGE_BGZF_DEFLATE", "host")
        host = coverage.sample_paths(tmp_path, f"S{s}.host", stranded, True)
        coverage.write_sample(*args, s, host, stranded, ORG, bgzf_out=True)
        monkeypatch.delenv("MIRGE_BGZF_DEFLATE")
        monkeypatch.delenv("MIRGE_BGZF_BLOCK_BYTES")
        for k, text in enumerate(want):
            gz, gzi = _pair(whole[k])
            assert _pair(small[k]) == (gz, gzi)
            assert gzip.decompress(gz) == text
            ms = bgzf.check_index(gz, gzi)
            # each strand's file is a stream of its own: block 0 starts at its text's byte 0
            assert [m["payload"] for m in ms] == [text[a:a + 256] for a in range(0, len(text), 256)] and all(m["single"] for m in ms)
            fs = st2["bgzf"][k]
            assert fs["file_bytes"] == len(gz) and fs["stream_bytes"] == len(text) and fs["members"] == len(ms)
            assert [fs["stored"], fs["fixed"], fs["dynamic"]] == [sum(m["btype"] == t for m in ms) for t in range(3)]
            hgz, hgzi = _pair(host[k])
            assert gzip.decompress(hgz) == text and [u for _, u in bgzf.read_gzi(hgzi)] == [u for _, u in bgzf.read_gzi(gzi)]
            if s == 3:  # no kept row
                assert text == b"" and (gz, gzi) == (bgzf.EOF_BLOCK, bytes(8))
        if s == 0:  # (more chunks than staging halves)
            assert sum(len(x) for x in want) > 4096 * 3
    _no_leftovers(tmp_path)


def test_a_failing_call_leaves_no_gz_gzi_or_tmp(cov_case, tmp_path, monkeypatch):
    f = cov_case
    monkeypatch.setenv("MIRGE_BGZF_BLOCK_BYTES", "256")
    used = sorted({c for c, *_ in f["rows"][0]})
    for stranded in (False, True):
        paths = coverage.sample_paths(tmp_path, "S0", stranded, True)
        with pytest.raises(ValueError, match="'" + used[-1] + "'.*no @SQ line"):
            coverage.write_sample(f["casc"], f["uniq"], f["res"], f["order"], 0, paths, stranded, ORG, used[:-1], bgzf_out=True)
        assert not os.listdir(tmp_path)
    monkeypatch.setenv("MIRGE_BGZF_DEFLATE", "zlib")
    with pytest.raises(ValueError, match="MIRGE_BGZF_DEFLATE"):
        coverage.write_sample(f["casc"], f["uniq"], f["res"], f["order"], 0, coverage.sample_paths(tmp_path, "S0", True, True), True, ORG, bgzf_out=True)
    assert not os.listdir(tmp_path)


def test_command_line_end_to_end(tmp_path):
    _, samples, seqs, counts = golden_inputs()
    files = []
    for s, nm in enumerate(samples):
        p = tmp_path / f"{nm}.fastq"
        with open(p, "w") as fh:
            k = 0
            for seq, row in zip(seqs, counts):
                for _ in range(int(row[s])):
                    fh.write(f"@r{k}\n{seq}\n+\n{'I' * len(seq)}\n")
                    k += 1
        files.append(str(p))
    _cli(["-s", ",".join(files), "-lib", os.path.join(GOLDEN, "libs"), "-on", ORG, "-db", "miRBase", "-o", str(tmp_path), "-shh", "-dn", "bgzf",
          "--sam-out", "--coverage", "stranded", "--bgzf-out"])
    out = tmp_path / "bgzf"
    for nm in samples:
        gz, gzi = _pair(out / f"{nm}.sam.gz")
        with open(os.path.join(GOLDEN, nm + ".sam"), "rb") as fh:
            assert gzip.decompress(gz) == fh.read(), nm
        bgzf.check_index(gz, gzi)
        for strand, want in zip(("plus", "minus"), golden_bedgraph(nm, True)):
            gz, gzi = _pair(out / f"{nm}.{strand}.bedgraph.gz")
            assert gzip.decompress(gz) == want, (nm, strand)
            bgzf.check_index(gz, gzi)
    assert not [f for f in os.listdir(out) if f.endswith((".sam", ".bedgraph", ".tmp"))]
    assert len([f for f in os.listdir(out) if f.endswith(".gz")]) == len([f for f in os.listdir(out) if f.endswith(".gzi")]) == 3 * len(samples)
    log = (out / "run.log").read_text()
    assert log.count(" compressed bytes, ") == 2 * len(samples) and " stored, " in log and " dynamic" in log
