"""CPU tests of ``--bgzf-out``'s host side (mirge3_amd/bgzf.py): the layout reference ``write_host``, the structural reader ``members``
and ``read_gzi`` against ``gzip.decompress`` and against each other on every stream of tests/bgzf_cases.py; the ``.gzi`` invariant; the
command line's refusals."""
import gzip
import os
import struct

import pytest

import mirge3_amd  # noqa: F401
from mirge3_amd import bgzf
from mirge3_amd.cli import parse_args

import bgzf_cases


@pytest.mark.parametrize("name", sorted(bgzf_cases.all_cases()))
def test_write_host_members_and_gzi(name):
    s, block = bgzf_cases.all_cases()[name]
    gz, gzi = bgzf.write_host(s, block)
    assert gzip.decompress(gz) == s
    ms = bgzf.check_index(gz, gzi)
    assert [m["payload"] for m in ms] == [s[a:a + block] for a in range(0, len(s), block)]
    assert all(m["bsize"] <= m["isize"] + 31 for m in ms)
    # the pairs, restated: one per member after the first; the compressed offset lands on a member's magic, the uncompressed offset is
    # the summed ISIZE in front of it
    pairs = bgzf.read_gzi(gzi)
    assert len(pairs) == max(len(ms) - 1, 0) and struct.unpack_from("<Q", gzi)[0] == len(pairs)
    for k, (c, u) in enumerate(pairs):
        assert gz[c:c + 4] == b"\x1f\x8b\x08\x04" and gz[c + 12:c + 14] == b"BC"
        assert u == sum(m["isize"] for m in ms[:k + 1]) == (k + 1) * block
    assert gz.endswith(bgzf.EOF_BLOCK) and gzip.decompress(bgzf.EOF_BLOCK) == b""
    if not s:
        assert gz == bgzf.EOF_BLOCK and gzi == bytes(8)


def test_the_reader_refuses_what_is_not_a_bgzf_file():
    s, block = bgzf_cases.all_cases()["sam_S2_b4096"]
    gz, gzi = bgzf.write_host(s, block)
    ms = bgzf.members(gz)
    first = ms[0]["bsize"]
    for bad in (gz[:-28],                                        # no EOF block
                gz[:-1],                                         # a cut file
                gz + bgzf.EOF_BLOCK,                             # an empty member in front of the EOF block
                gzip.compress(s),                                # a gzip file without the BC field
                gz[:first - 8] + bytes(4) + gz[first - 4:],      # a wrong CRC-32
                gz[:first - 4] + bytes(4) + gz[first:],          # a wrong ISIZE
                gz[:16] + struct.pack("<H", first) + gz[18:]):   # a BSIZE one too large
        with pytest.raises(ValueError):
            bgzf.members(bad)
    for bad in (gzi[:-1], gzi + bytes(16), b""):
        with pytest.raises(ValueError):
            bgzf.read_gzi(bad)
    pairs = bgzf.read_gzi(gzi)
    moved = struct.pack("<Q", len(pairs)) + b"".join(struct.pack("<QQ", c + (k == 0), u) for k, (c, u) in enumerate(pairs))
    with pytest.raises(ValueError):
        bgzf.check_index(gz, moved)
    with pytest.raises(ValueError):
        bgzf.check_index(gz, struct.pack("<Q", len(pairs) - 1) + gzi[8:-16])


def test_block_size_and_route(monkeypatch):
    monkeypatch.delenv("MIRGE_BGZF_BLOCK_BYTES", raising=False)
    monkeypatch.delenv("MIRGE_BGZF_DEFLATE", raising=False)
    assert bgzf.block_bytes() == 65280 == bgzf.BLOCK_BYTES and bgzf.route() == "device"
    for v in ("64", "256", "65280"):
        monkeypatch.setenv("MIRGE_BGZF_BLOCK_BYTES", v)
        assert bgzf.block_bytes() == int(v)
    for v in ("63", "65281", "many", "-1"):
        monkeypatch.setenv("MIRGE_BGZF_BLOCK_BYTES", v)
        with pytest.raises(ValueError):
            bgzf.block_bytes()
    monkeypatch.setenv("MIRGE_BGZF_DEFLATE", "host")
    assert bgzf.route() == "host"
    monkeypatch.setenv("MIRGE_BGZF_DEFLATE", "zlib")
    with pytest.raises(ValueError):
        bgzf.route()
    for b in (63, 65281):
        with pytest.raises(ValueError):
            bgzf.write_host(b"x", b)


def test_command_line(tmp_path, monkeypatch, capsys):
    monkeypatch.delenv("MIRGE_BGZF_BLOCK_BYTES", raising=False)
    monkeypatch.delenv("MIRGE_BGZF_DEFLATE", raising=False)
    base = ["-s", "x.fastq", "-lib", "L", "-on", "human"]
    hdr = tmp_path / "h.txt"
    hdr.write_text("@HD\tVN:1.0\n@SQ\tSN:chr1\tLN:1000\n")
    assert parse_args(base).bgzf_out is False and parse_args(base + ["--sam-out"]).bgzf_out is False
    assert parse_args(base + ["--sam-out", "--bgzf-out"]).bgzf_out is True
    assert parse_args(base + ["--coverage", "--bgzf-out"]).coverage == "unstranded"
    a = parse_args(base + ["--bgzf-out", "--coverage", "stranded", "--sam-out"])
    assert a.bgzf_out and a.coverage == "stranded" and a.sam_out
    # --sam-header, --coverage-bigwig and --sorted-bam beside it behave as before
    b = parse_args(base + ["--bgzf-out", "--coverage", "--coverage-bigwig", "--sorted-bam", "--sam-header", str(hdr)])
    assert b.bgzf_out and b.coverage_bigwig and b.sorted_bam and not b.sam_out
    # the flag alone, or beside outputs it does not touch
    for bad in (["--bgzf-out"], ["--bgzf-out", "--sorted-bam", "--sam-header", str(hdr)], ["--bgzf-out", "--gff"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        parse_args(base + ["--bgzf-out"])
    assert "--bgzf-out requires --sam-out or --coverage" in capsys.readouterr().err
    # together with what the two switches refuse
    for sw in (["--sam-out"], ["--coverage"]):
        for extra in (["-spl"], ["-rr"], ["--backend", "bowtie"]):
            with pytest.raises(SystemExit):
                parse_args(base + ["--bgzf-out"] + sw + extra)
            assert "runs on the device-resident route" in capsys.readouterr().err
    # a route or a block size the native call would refuse is refused here, before anything is written
    monkeypatch.setenv("MIRGE_BGZF_DEFLATE", "zlib")
    with pytest.raises(SystemExit):
        parse_args(base + ["--sam-out", "--bgzf-out"])
    assert "MIRGE_BGZF_DEFLATE" in capsys.readouterr().err
    assert parse_args(base + ["--sam-out"]).sam_out  # (without the flag the variable is nobody's business)
    monkeypatch.setenv("MIRGE_BGZF_DEFLATE", "host")
    monkeypatch.setenv("MIRGE_BGZF_BLOCK_BYTES", "32")
    with pytest.raises(SystemExit):
        parse_args(base + ["--coverage", "--bgzf-out"])
    assert "MIRGE_BGZF_BLOCK_BYTES" in capsys.readouterr().err


def test_sharded_run_refuses_the_flag_with_its_switch(tmp_path, monkeypatch):
    from mirge3_amd import cli, multigpu
    import torch.distributed
    (tmp_path / "L" / "human" / "index.Libs").mkdir(parents=True)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.delenv("MIRGE_BGZF_DEFLATE", raising=False)
    monkeypatch.delenv("MIRGE_BGZF_BLOCK_BYTES", raising=False)
    monkeypatch.setattr(torch.distributed, "init_process_group", lambda *a, **k: None)
    monkeypatch.setattr(multigpu, "agree_on_run_directory", lambda *a, **k: "out")
    with pytest.raises(SystemExit) as e:
        cli.main(["-s", "x.fastq", "-lib", str(tmp_path / "L"), "-on", "human", "-o", str(tmp_path), "--coverage", "--bgzf-out", "-shh"])
    assert "--coverage is a single-process option" in str(e.value)
    assert not [f for f in os.listdir(tmp_path) if f.endswith((".gz", ".gzi", ".tmp"))]


def test_the_abi_names_the_three_exports():
    from mirge3_amd import _ffi
    for name in ("mirge_bgzf_write", "mirge_sam_write_device_bgzf", "mirge_coverage_write_device_bgzf"):
        assert name in _ffi.EXPORTS
