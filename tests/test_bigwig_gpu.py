"""``--coverage-bigwig`` on the GPU.  The files of ``mirge_bigwig_from_intervals`` (host intervals) and of ``mirge_bigwig_write_device``
(the resident run of test_coverage_gpu.py's fuzzer) equal the host simulation's (tests/hostsim/bw_sim.cpp: the same kernel source on
the CPU) byte for byte on both deflate routes, at S = 3, zoom base 4 and groups of 4096 or 512 bytes; the raw route also equals ``write_host``, and
every file reads back through tests/bigwig_reader.py (Python's zlib inflates the device's streams) as the per-base restatement.  The
directed cases are tests/bw_cases.py's; what each is for is asserted on the CPU in test_bigwig.py.  One run through the command line."""
import os

import numpy as np
import pytest

import mirge3_amd  # noqa: F401
from mirge3_amd import bigwig, coverage

import bigwig_reader
import bw_cases
import cov_cases
from test_bigwig_hostsim import run_sim, sim  # noqa: F401  (sim: the module-scoped fixture that builds the simulation)
from test_coverage_gpu import ORG, SQ_ORDER, _cli, ctx, fuzz_case  # noqa: F401  (ctx, fuzz_case: fixtures)
from test_sam_out import GOLDEN, golden_inputs
from test_coverage import golden_bedgraph

pytestmark = pytest.mark.gpu
ROUTES = {"none": 0, "device": 1}


def settings(monkeypatch, S, base, route, chunk=4096):
    monkeypatch.setenv("MIRGE_BW_SECTION_ITEMS", str(S))
    monkeypatch.setenv("MIRGE_BW_ZOOM_BASE", str(base))
    monkeypatch.setenv("MIRGE_BW_DEFLATE", route)
    monkeypatch.setenv("MIRGE_BW_CHUNK_BYTES", str(chunk))


def compare(sim, blobs, stats, runs, names, sizes, stranded, S, base, route):
    for f, strand in enumerate((0, 1) if stranded else (None,)):
        want, sim_stats, _ = run_sim(sim, runs, names, sizes, stranded, f, S, base, ROUTES[route])
        assert blobs[f] == want, (route, f)
        if route == "none":
            assert blobs[f] == bigwig.write_host(runs, names, sizes, strand, S, base)
        got = bigwig_reader.read(blobs[f])
        bw_cases.check(got, bw_cases.restate(bw_cases.strand_runs(runs, strand), names, sizes, S, base))
        st = stats[f]
        assert [st["sections"], st["items"], st["levels"], st["bytes"]] == sim_stats[:4] and st["bytes"] == len(blobs[f])
        assert st["zoom_records"] == [len(z[1]) for z in got["zoom"]] and st["max_depth"] == sim_stats[4]
    return got


@pytest.mark.parametrize("route", ["none", "device"])
@pytest.mark.parametrize("stranded", [False, True], ids=["unstranded", "stranded"])
@pytest.mark.parametrize("name", sorted(bw_cases.directed()))
def test_from_intervals_equals_the_simulation(ctx, sim, name, stranded, route, tmp_path, monkeypatch):
    iv, names, sizes, S, base = bw_cases.directed()[name]
    settings(monkeypatch, S, base, route)
    paths = bigwig.sample_paths(tmp_path, name, stranded)
    stats = bigwig.from_intervals(ctx, iv, names, sizes, stranded, paths)
    assert sorted(os.listdir(tmp_path)) == sorted(p.name for p in paths)  # (no temporary file stays)
    got = compare(sim, [p.read_bytes() for p in paths], stats, cov_cases.brute(iv, stranded), names, sizes, stranded, S, base, route)
    if route == "device" and not stranded:
        want_forms = {"incompressible": ["stored"], "ladder_1024": ["fixed"], "single_items": ["fixed", "fixed"]}  # (test_bigwig_hostsim.py's docstring)
        if name in want_forms:
            assert got["forms"] == want_forms[name]
    if name == "depths":
        assert stats[0]["max_depth"] == (3 * (2 ** 32 - 1) + 1 if not stranded else 2 * (2 ** 32 - 1) + 1)


@pytest.mark.parametrize("name", ["fuzz", "count_257", "chrom_boundary", "extreme_positions"])
def test_from_intervals_on_the_coverage_cases(ctx, sim, name, tmp_path, monkeypatch):
    iv, names = cov_cases.all_cases()[name]
    sizes = bw_cases.sizes_for(iv, len(names))
    for route in ("none", "device"):
        settings(monkeypatch, bw_cases.S_TEST, bw_cases.BASE_TEST, route)
        paths = bigwig.sample_paths(tmp_path, name + route, True)
        stats = bigwig.from_intervals(ctx, iv, names, sizes, True, paths)
        compare(sim, [p.read_bytes() for p in paths], stats, cov_cases.brute(iv, True), names, sizes, True, bw_cases.S_TEST, bw_cases.BASE_TEST, route)


def test_a_run_beyond_its_chromosome_fails_and_leaves_no_file(ctx, tmp_path, monkeypatch):
    iv, names, sizes, S, base = bw_cases.directed()["extreme"]
    settings(monkeypatch, S, base, "device")
    for stranded in (False, True):
        with pytest.raises(ValueError, match="'y' ends at 2147483647, beyond its LN 2147483646"):
            bigwig.from_intervals(ctx, iv, names, [5, 2 ** 31 - 2], stranded, bigwig.sample_paths(tmp_path, "bad", stranded))
        assert not os.listdir(tmp_path)
    monkeypatch.setenv("MIRGE_BW_DEFLATE", "host")
    with pytest.raises(RuntimeError, match="MIRGE_BW_DEFLATE"):
        bigwig.from_intervals(ctx, iv, names, sizes, False, bigwig.sample_paths(tmp_path, "bad", False))
    assert not os.listdir(tmp_path)


@pytest.mark.parametrize("route", ["none", "device"])
@pytest.mark.parametrize("stranded", [False, True], ids=["unstranded", "stranded"])
def test_the_resident_route_equals_the_simulation(fuzz_case, sim, stranded, route, tmp_path, monkeypatch):
    f = fuzz_case
    used = sorted({c for r in f["rows"] for c, *_ in r}, key=lambda s: s.encode())
    names = ["chrUn_not_used"] + used[::-1] + ["chrM"]  # the @SQ order: opposite to the byte order, with names no row uses
    sq = [(nm, 2 ** 31 - 1 - 3 * k) for k, nm in enumerate(names)]
    sizes = [s for _, s in sq]
    rank = {nm: k for k, nm in enumerate(names)}
    settings(monkeypatch, bw_cases.S_TEST, bw_cases.BASE_TEST, route, chunk=512)  # (groups of 6 sections: a slot is 80 bytes at S = 3)
    for s in range(f["S"]):
        paths = bigwig.sample_paths(tmp_path, f"S{s}", stranded)
        stats = bigwig.write_sample(f["casc"], f["uniq"], f["res"], f["order"], s, paths, stranded, ORG, sq)
        runs = coverage.coverage_host(cov_cases.make([(rank[c], a, n, w, mi) for c, a, n, w, mi in f["rows"][s]]), stranded)
        compare(sim, [p.read_bytes() for p in paths], stats, runs, names, sizes, stranded, bw_cases.S_TEST, bw_cases.BASE_TEST, route)
        if s == 0:  # (more groups than staging halves, in every file)
            assert all(st["sections"] > 2 * (512 // 80) for st in stats)
        if s == 3:
            assert [st["items"] for st in stats] == [0] * len(paths)
    # a chromosome shorter than a row that lies on it: named, and no file
    worst = max(f["rows"][0], key=lambda r: r[1] + r[2])
    short = [(nm, worst[1] + worst[2] - 1 if nm == worst[0] else ln) for nm, ln in sq]
    paths = bigwig.sample_paths(tmp_path, "short", stranded)
    with pytest.raises(ValueError, match=f"'{worst[0]}' ends at {worst[1] + worst[2]}, beyond its LN {worst[1] + worst[2] - 1}"):
        bigwig.write_sample(f["casc"], f["uniq"], f["res"], f["order"], 0, paths, stranded, ORG, short)
    assert not [p for p in paths if p.exists()] and not [x for x in os.listdir(tmp_path) if x.endswith(".tmp")]


def test_cli_writes_bigwig_beside_an_unchanged_bedgraph(tmp_path):
    _, samples, seqs, counts = golden_inputs()
    files = []
    for s, nm in enumerate(samples):
        files.append(str(tmp_path / f"{nm}.fastq"))
        with open(files[-1], "w") as fh:
            k = 0
            for seq, row in zip(seqs, counts):
                for _ in range(int(row[s])):
                    fh.write(f"@r{k}\n{seq}\n+\n{'I' * len(seq)}\n")
                    k += 1
    header = tmp_path / "header.sam"
    header.write_text("@HD\tVN:1.0\tSO:unsorted\n" + "".join(f"@SQ\tSN:{c}\tLN:248956422\n" for c in SQ_ORDER))
    _cli(["-s", ",".join(files), "-lib", os.path.join(GOLDEN, "libs"), "-on", ORG, "-db", "miRBase", "-o", str(tmp_path), "-shh", "-dn", "bigwig",
          "--coverage", "stranded", "--coverage-bigwig", "--sam-header", str(header)])
    tmp = tmp_path
    log = (tmp / "bigwig" / "run.log").read_text()
    ids = {nm: k for k, nm in enumerate(sorted(SQ_ORDER, key=lambda s: s.encode()))}
    for nm in samples:
        beds = [(tmp / "bigwig" / f"{nm}.{s}.bedgraph").read_bytes() for s in ("plus", "minus")]
        assert beds == golden_bedgraph(nm, True, SQ_ORDER)
        for s, bed in zip(("plus", "minus"), beds):
            got = bigwig_reader.read((tmp / "bigwig" / f"{nm}.{s}.bw").read_bytes())
            want = sorted((ids[c.decode()], int(a), int(b), bw_cases.f32_bits(int(d))) for c, a, b, d in (ln.split(b"\t") for ln in bed.splitlines()))
            assert got["items"] == want and [c[0].decode() for c in got["chroms"]] == sorted(SQ_ORDER, key=lambda s: s.encode())
            assert f"coverage-bigwig {nm} {nm}.{s}.bw: {len(got['sections'])} sections, {len(want)} items, {len(got['zoom'])} zoom levels" in log
