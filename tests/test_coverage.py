"""``--coverage`` on the host (no GPU): ``coverage.coverage_host`` -- the slow restatement the device is compared with -- against the
per-base brute force of tests/cov_cases.py on every case; both against each other on the intervals of the reference's own
``<sample>.sam`` files (tests/golden/sam_out: both strands, seven chromosomes), in both modes and under both chromosome orders; the
command line's implications and refusals."""
import os

import numpy as np
import pytest

import mirge3_amd  # noqa: F401
from mirge3_amd import coverage
from mirge3_amd.cli import parse_args

import cov_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sam_out")
KEYS = ("strand", "chrom", "start", "end", "depth")


def sam_intervals(name, sq_names=None):
    """(intervals, ranked chromosome names) of the lines of tests/golden/sam_out/<name>.sam: one interval of weight 1 per line"""
    with open(os.path.join(GOLDEN, name + ".sam")) as fh:
        rows = [ln.split("\t") for ln in fh if not ln.startswith("@")]
    names = list(sq_names) if sq_names is not None else sorted({r[2] for r in rows}, key=lambda s: s.encode())
    rank = {nm: k for k, nm in enumerate(names)}
    assert all(r[1] in ("0", "16") and r[5] == "%dM" % len(r[9]) for r in rows)
    return cov_cases.make([(rank[r[2]], int(r[3]) - 1, len(r[9]), 1, 1 if r[1] == "16" else 0) for r in rows]), names


def golden_bedgraph(name, stranded, sq_names=None):
    """the brute force's file(s) for a golden sample: [whole] or [plus, minus]"""
    iv, names = sam_intervals(name, sq_names)
    runs = cov_cases.brute(iv, stranded)
    return [cov_cases.text(runs, names, 0), cov_cases.text(runs, names, 1)] if stranded else [cov_cases.text(runs, names)]


@pytest.mark.parametrize("stranded", [False, True], ids=["unstranded", "stranded"])
@pytest.mark.parametrize("name", sorted(cov_cases.all_cases()))
def test_coverage_host_equals_the_brute_force(name, stranded):
    iv, names = cov_cases.all_cases()[name]
    got, want = coverage.coverage_host(iv, stranded), cov_cases.expected(name, stranded)
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (name, k)
    assert coverage.format_bedgraph(got, names) == cov_cases.text(want, names)
    assert coverage.format_bedgraph(got, names, 1) == cov_cases.text(want, names, 1)


@pytest.mark.parametrize("sample", ["S1", "S2"])
def test_golden_sam_lines(sample):
    iv, names = sam_intervals(sample)
    assert len(names) >= 6 and 0 < int(iv["minus"].sum()) < iv["minus"].size
    other = [names[1], names[0]] + names[:1:-1]  # an @SQ order that is not the byte order
    for order in (None, other):
        iv, nm = sam_intervals(sample, order)
        for stranded in (False, True):
            runs = coverage.coverage_host(iv, stranded)
            files = [coverage.format_bedgraph(runs, nm, 0), coverage.format_bedgraph(runs, nm, 1)] if stranded else [coverage.format_bedgraph(runs, nm)]
            assert files == golden_bedgraph(sample, stranded, order)
            assert all(f and not f.startswith(b"@") and f.endswith(b"\n") for f in files)
            chrom_seq = [ln.split(b"\t")[0].decode() for ln in files[0].splitlines()]
            assert [c for k, c in enumerate(chrom_seq) if k == 0 or chrom_seq[k - 1] != c] == [c for c in nm if c in chrom_seq]


def test_coverage_host_refuses_what_the_device_refuses():
    ok = (0, 5, 7, 3, 0)
    for bad in ((-1, 5, 7, 3, 0), (0, -1, 7, 3, 0), (0, 5, 0, 3, 0), (0, 5, 7, 0, 0), (0, 2 ** 31 - 7, 7, 1, 0)):
        with pytest.raises(ValueError):
            coverage.coverage_host(cov_cases.make([ok, bad]), False)


def test_sq_order():
    assert coverage.sq_order(None) is None and coverage.sq_order(b"@HD\tVN:1.0\n@CO\tnothing") is None
    assert coverage.sq_order(b"@HD\tVN:1.0\n@SQ\tSN:chr2\tLN:9\n@SQ\tSN:chr1\tLN:7\n") == ["chr2", "chr1"]
    with pytest.raises(ValueError):
        coverage.sq_order(b"@SQ\tSN:chr2\n")


def test_command_line(tmp_path):
    base = ["-s", "x.fastq", "-lib", "L", "-on", "human"]
    hdr = tmp_path / "h.txt"
    hdr.write_text("@HD\tVN:1.0\n@SQ\tSN:chr1\tLN:1000\n")
    nosq = tmp_path / "nosq.txt"
    nosq.write_text("@HD\tVN:1.0\n")
    broken = tmp_path / "broken.txt"
    broken.write_text("@SQ\tSN:chr1\n")
    assert parse_args(base).coverage is None
    a = parse_args(base + ["--coverage"])
    assert a.coverage == "unstranded" and a.sam_out is False and a.sorted_bam is False and a.sam_header is None
    assert parse_args(["--coverage"] + base).coverage == "unstranded"  # (bare, in front of another switch)
    assert parse_args(base + ["--coverage", "unstranded"]).coverage == "unstranded"
    assert parse_args(base + ["--coverage", "stranded"]).coverage == "stranded"
    # --sam-header is legal with --coverage alone, with or without @SQ lines
    assert parse_args(base + ["--coverage", "--sam-header", str(hdr)]).sam_header == str(hdr)
    assert parse_args(base + ["--coverage", "stranded", "--sam-header", str(nosq)]).coverage == "stranded"
    b = parse_args(base + ["--coverage", "--sam-out", "--sorted-bam", "--sam-header", str(hdr)])
    assert b.coverage == "unstranded" and b.sam_out and b.sorted_bam
    for bad in (["--coverage", "both"], ["--coverage", "-spl"], ["--coverage", "-rr"], ["--coverage", "stranded", "--backend", "bowtie"],
                ["--coverage", "--sam-header", str(tmp_path / "missing")], ["--coverage", "--sam-header", str(broken)], ["--sam-header", str(hdr)]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)


def test_refusals_are_worded_like_the_neighbours(tmp_path, capsys):
    base = ["-s", "x.fastq", "-lib", "L", "-on", "human"]
    for extra in (["-spl"], ["-rr"], ["--backend", "bowtie"]):
        with pytest.raises(SystemExit):
            parse_args(base + ["--coverage"] + extra)
        assert "--coverage runs on the device-resident route: not together with -spl / -rr / --backend bowtie" in capsys.readouterr().err


def test_sharded_run_refuses_coverage(tmp_path, monkeypatch):
    from mirge3_amd import cli, multigpu
    import torch.distributed
    (tmp_path / "L" / "human" / "index.Libs").mkdir(parents=True)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(torch.distributed, "init_process_group", lambda *a, **k: None)
    monkeypatch.setattr(multigpu, "agree_on_run_directory", lambda *a, **k: "out")
    with pytest.raises(SystemExit) as e:
        cli.main(["-s", "x.fastq", "-lib", str(tmp_path / "L"), "-on", "human", "-o", str(tmp_path), "--coverage", "stranded", "-shh"])
    assert "--coverage is a single-process option" in str(e.value)


def test_the_abi_names_both_exports():
    from mirge3_amd import _ffi
    assert "mirge_coverage_runs" in _ffi.EXPORTS and "mirge_coverage_write_device" in _ffi.EXPORTS
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "..", "include", "mirge_native.h")) as fh:
        text = fh.read()
    assert "int mirge_coverage_runs(" in text and "int mirge_coverage_write_device(" in text
