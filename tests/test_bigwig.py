"""``--coverage-bigwig`` on the host (no GPU): ``bigwig.write_host`` -- the slow writer the device is compared with -- read back by
tests/bigwig_reader.py against the per-base restatement of tests/bw_cases.py on the cases of tests/cov_cases.py and the directed cases;
the chromosome B+ tree at 1, 255, 256, 257 and 70 000 names; the empty file; the command line's refusals; the C ABI's names."""
import os
import struct

import numpy as np
import pytest

import bigwig_reader
import bw_cases
import cov_cases
from mirge3_amd import bigwig


def files_of(iv, names, sizes, S, base, stranded, compress=False):
    runs = cov_cases.brute(iv, stranded)
    out = []
    for strand in ((0, 1) if stranded else (None,)):
        out.append((bigwig.write_host(runs, names, sizes, strand, S, base, compress), bw_cases.strand_runs(runs, strand)))
    return out


@pytest.mark.parametrize("stranded", [False, True], ids=["unstranded", "stranded"])
@pytest.mark.parametrize("name", sorted(cov_cases.all_cases()))
def test_write_host_reads_back_as_the_brute_force(name, stranded):
    iv, names = cov_cases.all_cases()[name]
    sizes = bw_cases.sizes_for(iv, len(names))
    big = name == "count_65537"
    S, base = (1024, 64) if big else (bw_cases.S_TEST, bw_cases.BASE_TEST)
    for compress in ((False,) if big else (False, True)):
        for blob, rows in files_of(iv, names, sizes, S, base, stranded, compress):
            got = bigwig_reader.read(blob, strict=False)
            bw_cases.check(got, bw_cases.restate(rows, names, sizes, S, base))
            assert (got["uncompress_buf"] != 0) == (compress and len(rows) > 0)
            assert sorted(c[0] for c in got["chroms"]) == sorted(n.encode() for n in names)


@pytest.mark.parametrize("name", sorted(bw_cases.directed()))
def test_directed_cases_hold_what_they_are_for(name):
    iv, names, sizes, S, base = bw_cases.directed()[name]
    for stranded in (False, True):
        for blob, rows in files_of(iv, names, sizes, S, base, stranded):
            got = bigwig_reader.read(blob)
            bw_cases.check(got, bw_cases.restate(rows, names, sizes, S, base))
    got = bigwig_reader.read(files_of(iv, names, sizes, S, base, False)[0][0])
    if name == "layout":
        assert [c[0] for c in got["chroms"]] == [b"a", b"b", b"c", b"d"] and {i[0] for i in got["items"]} == {0, 2, 3}
        per = {c: [s[3] for s in got["sections"] if s[0] == c] for c in (0, 2, 3)}
        assert per[3] == [3] and per[2] == [3, 1] and per[0][-1] < 3 and set(per[0][:-1]) == {3}
        levels = [z[0] for z in got["zoom"]]
        assert 1 <= len(levels) < 8 and levels == [4 * 4 ** k for k in range(len(levels))]  # (kept levels, and one that fails)
        r0 = got["zoom"][0][1]
        assert sum(1 for r in r0 if r[0] == 2 and 300 <= r[1] < 460) == 40               # a run over 40 bins
        assert [r for r in r0 if r[0] == 3 and r[1] == 100][0][3] == 2                    # two abutting runs in one bin
        assert [r for r in r0 if r[0] == 3 and r[1] == 8][0][2:4] == (12, 4)              # a run that ends on a bin edge
        assert [r for r in r0 if r[0] == 2 and r[1] == 996][0][2:4] == (999, 3)           # the last bin, clipped by LN
    if name == "depths":
        vals = [i[3] for i in got["items"]]
        b24 = bw_cases.f32_bits(2 ** 24)
        assert got["items"][:3] == [(0, 0, 4, b24), (0, 10, 12, b24), (0, 12, 14, b24)]  # 2^24 + 1 on [10, 12) rounds to even, and stays an item of its own
        assert bw_cases.f32_bits(3 * (2 ** 32 - 1) + 1) in vals and bw_cases.f32_bits(2 ** 24 + 1) == bw_cases.f32_bits(2 ** 24)
    if name == "extreme":
        assert got["items"][-1][2] == 2 ** 31 - 1 and dict((c[0], c[2]) for c in got["chroms"])[b"y"] == 2 ** 31 - 1
        with pytest.raises(ValueError, match="beyond its LN 2147483646"):
            bigwig.write_host(cov_cases.brute(iv, False), names, [5, 2 ** 31 - 2])
    if name == "empty":
        assert got["items"] == [] and got["zoom"] == [] and got["summary"] == (0, 0.0, 0.0, 0.0, 0.0) and len(got["chroms"]) == 3


@pytest.mark.parametrize("n", [1, 255, 256, 257, 70000])
def test_the_chromosome_tree_finds_every_name(n):
    names = ["c%x" % ((k * 2654435761) % (1 << 32)) + "_" * (k % 3) for k in range(n)]
    sizes = [1000 + k for k in range(n)]
    iv = cov_cases.make([(n // 2, 5, 7, 3, 0)])
    blob = bigwig.write_host(cov_cases.brute(iv, False), names, sizes, None, 3, 4)
    got = bigwig_reader.read(blob)
    assert len(got["chroms"]) == n
    cid = {nm: k for k, nm in enumerate(sorted(x.encode() for x in names))}
    step = 1 if n < 1000 else 97
    for k in list(range(0, n, step)) + [n - 1]:
        assert bigwig_reader.find_chrom(blob, got["tree_at"], names[k].encode()) == (cid[names[k].encode()], sizes[k])
    assert bigwig_reader.find_chrom(blob, got["tree_at"], b"absent") is None
    assert got["items"] == [(cid[names[n // 2].encode()], 5, 12, bw_cases.f32_bits(3))]


def test_settings_and_chromosomes_are_checked(monkeypatch):
    for var, bad in (("MIRGE_BW_SECTION_ITEMS", "0"), ("MIRGE_BW_SECTION_ITEMS", "1025"), ("MIRGE_BW_ZOOM_BASE", "0"), ("MIRGE_BW_DEFLATE", "host")):
        monkeypatch.setenv(var, bad)
        with pytest.raises(ValueError, match=var):
            bigwig.env_settings()
        monkeypatch.delenv(var)
    assert bigwig.env_settings() == (1024, 64, "device")
    with pytest.raises(ValueError, match="twice"):
        bigwig.chrom_ids(["a", "a"], [1, 2])
    with pytest.raises(ValueError, match="2\\^32 - 1"):
        bigwig.chrom_ids(["a"], [2 ** 32])
    assert bigwig.chrom_ids(["chr2", "chr10", "chr1"], [1, 2, 2 ** 32 - 1]).tolist() == [2, 1, 0]
    assert bigwig.parse_sizes(b"@HD\tVN:1.0\n@SQ\tSN:chr2\tLN:9\n@SQ\tSN:chr1\tLN:4294967295\n") == [("chr2", 9), ("chr1", 2 ** 32 - 1)]


def test_command_line(tmp_path, capsys):
    from mirge3_amd.cli import parse_args
    hdr, nosq, big, twice = (tmp_path / n for n in ("hdr.sam", "nosq.sam", "big.sam", "twice.sam"))
    hdr.write_bytes(b"@HD\tVN:1.0\n@SQ\tSN:chr2\tLN:900\n@SQ\tSN:chr1\tLN:700\n")
    nosq.write_bytes(b"@HD\tVN:1.0\n")
    big.write_bytes(b"@SQ\tSN:chr1\tLN:4294967296\n")
    twice.write_bytes(b"@SQ\tSN:chr1\tLN:5\n@SQ\tSN:chr1\tLN:6\n")
    (tmp_path / "L").mkdir()
    base = ["-s", "x.fastq", "-lib", str(tmp_path / "L"), "-on", "human", "-o", str(tmp_path)]
    assert parse_args(base).coverage_bigwig is False and parse_args(base + ["--coverage"]).coverage_bigwig is False
    a = parse_args(base + ["--coverage", "stranded", "--coverage-bigwig", "--sam-header", str(hdr)])
    assert a.coverage_bigwig is True and a.coverage == "stranded"
    for extra, msg in ((["--coverage-bigwig", "--sam-header", str(hdr)], "--coverage-bigwig requires --coverage"),
                       (["--coverage", "--coverage-bigwig"], "--coverage-bigwig needs --sam-header"),
                       (["--coverage", "--coverage-bigwig", "--sam-header", str(nosq)], "--coverage-bigwig needs --sam-header"),
                       (["--coverage", "--coverage-bigwig", "--sam-header", str(big)], "above 2^32 - 1"),
                       (["--coverage", "--coverage-bigwig", "--sam-header", str(twice)], "twice"),
                       (["--coverage", "--coverage-bigwig", "--sam-header", str(hdr), "-spl"], "--coverage runs on the device-resident route"),
                       (["--coverage", "--coverage-bigwig", "--sam-header", str(hdr), "--backend", "bowtie"], "--coverage runs on the device-resident route")):
        with pytest.raises(SystemExit):
            parse_args(base + extra)
        assert msg in capsys.readouterr().err, extra
    assert not any(p.suffix == ".bw" for p in tmp_path.iterdir())


def test_c_abi_names_the_two_calls():
    from mirge3_amd import _ffi
    assert "mirge_bigwig_from_intervals" in _ffi.EXPORTS and "mirge_bigwig_write_device" in _ffi.EXPORTS
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "mirge_native.h")).read()
    assert "int mirge_bigwig_from_intervals(" in text and "int mirge_bigwig_write_device(" in text


def test_log_line_notes_the_rounding():
    st = dict(sections=2, items=5, levels=1, bytes=999, max_depth=2 ** 24, zoom_records=[2])
    assert "rounded to float32" in bigwig.log_line("S1", "S1.bw", st) and "2 sections, 5 items, 1 zoom levels (records: 2), 999 bytes" in bigwig.log_line("S1", "S1.bw", st)
    assert "rounded" not in bigwig.log_line("S1", "S1.bw", dict(st, max_depth=2 ** 24 - 1))


def test_pybigwig_reads_the_same_intervals(tmp_path):
    pyBigWig = pytest.importorskip("pyBigWig")
    iv, names, sizes, S, base = bw_cases.directed()["layout"]
    blob, rows = files_of(iv, names, sizes, S, base, False, compress=True)[0]
    path = tmp_path / "layout.bw"
    path.write_bytes(blob)
    bw = pyBigWig.open(str(path))
    assert bw.chroms() == dict(zip(names, sizes))
    for r, nm in enumerate(names):
        want = [(s, e, float(d)) for rr, s, e, d in rows if rr == r]
        assert list(bw.intervals(nm) or []) == want
