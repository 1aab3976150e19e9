"""``--coverage`` on the GPU.  ``mirge_coverage_runs`` on every case of tests/cov_cases.py against the per-base brute force;
``mirge_coverage_write_device`` against ``coverage.coverage_host`` on a few hundred unique reads built like test_sam_out_gpu.py's
fuzzer (references on both strands, some without coordinates, a row of 100 001 copies) at the default sizes and at a 64-byte tile in
4096-byte chunks, where boundaries fall inside numbers and names; the golden inputs through the CLI in both modes, under an ``@SQ`` order
and without the switch; the two data errors.  Whole files and whole arrays, exactly."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mirge3_amd  # noqa: F401
from mirge3_amd import _ffi, coverage, sam_export
from mirge3_amd.cascade import Cascade
from mirge3_amd.seqio import FlatSeqs, Library

import cov_cases
from test_coverage import KEYS, golden_bedgraph
from test_sam_out import GOLDEN, ORG, golden_inputs
from test_sam_out_gpu import _fuzz_reads, _rnd

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
OTHER_OUTPUTS = ("mapped.csv", "unmapped.csv", "miR.Counts.csv", "miR.RPM.csv", "annotation.report.csv")
SQ_ORDER = ["chr2", "chr1", "chr9", "chr3", "chr4", "chr5", "chr6"]


@pytest.fixture(scope="module")
def ctx():
    return _ffi.Context(0)


@pytest.mark.parametrize("stranded", [False, True], ids=["unstranded", "stranded"])
@pytest.mark.parametrize("name", sorted(cov_cases.all_cases()))
def test_runs_equal_the_brute_force(ctx, name, stranded):
    iv, _ = cov_cases.all_cases()[name]
    got, want = coverage.runs_device(ctx, iv, stranded), cov_cases.expected(name, stranded)
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (name, k)


def test_an_interval_outside_the_contract_fails_the_call(ctx):
    ok = (0, 5, 7, 3, 0)
    for bad in ((-1, 5, 7, 3, 0), (0, -1, 7, 3, 0), (0, 5, 0, 3, 0), (0, 5, 7, 0, 0), (0, 2 ** 31 - 7, 7, 1, 0)):
        with pytest.raises(RuntimeError, match="outside the contract"):
            coverage.runs_device(ctx, cov_cases.make([ok, bad, ok]), True)
    assert coverage.runs_device(ctx, cov_cases.make([ok, (1, 2 ** 31 - 8, 7, 1, 1)]), True)["end"].tolist() == [12, 2 ** 31 - 1]


# ---------------------------------------------------------------------------------------------------------------------
# the device call from the resident run against coverage_host
# ---------------------------------------------------------------------------------------------------------------------
def _coordinates(rng, name, length, chrom):
    """test_sam_out_gpu._coordinates with genome coordinates a bedGraph of this project holds (below 2^31)"""
    kind = int(rng.integers(0, 10))
    if kind == 0:
        return name
    if kind == 1:
        return f"{name} {chrom}_PATCH segs:1-{length} cds:+:100-{99 + length}"
    n_seg = int(rng.integers(1, 5))
    cuts = sorted(set(int(x) for x in rng.integers(2, max(3, length), size=n_seg - 1)))
    bounds = [1] + cuts + [length + 1]
    # (a few references close together, so that rows of different references overlap and abut)
    segs, cds, g = [], [], int(rng.integers(10_000_000, 10_003_000)) if rng.random() < 0.5 else int(rng.integers(10_000_000, 2_000_000_000))
    minus = bool(rng.integers(0, 2))
    for a, b in zip(bounds[:-1], bounds[1:]):
        s = a + (3 if (rng.random() < 0.2 and b - a > 8) else 0)
        segs.append(f"{s}-{b - 1}")
        cds.append(f"{g}-{g + (b - 1 - s)}")
        g = g - int(rng.integers(500, 5000)) - (b - a) if minus else g + (b - a) + int(rng.integers(500, 5000))
    return f"{name} {chrom} segs:{','.join(segs)} cds:{'-' if minus else '+'}:{','.join(cds)}"


def _fuzz_libs(rng, mrna_headers=None):
    def lib(prefix, n, length):
        seqs = [_rnd(rng, length) for _ in range(n)]
        names = [f"{prefix}{i}" for i in range(n)]
        return Library(names, FlatSeqs.from_list(seqs), [_coordinates(rng, nm, length, f"chr{1 + i % 5}") for i, nm in enumerate(names)])
    mir = lib("miR-", 24, 22)
    mseq = mir.seqs.to_list()
    hseq = [_rnd(rng, 15) + m + _rnd(rng, 50) for m in mseq[:12]]
    hp = Library([f"mir-{i}" for i in range(12)], FlatSeqs.from_list(hseq),
                 [_coordinates(rng, f"mir-{i}", len(hseq[i]), f"chr{1 + i % 3}") for i in range(12)])
    libs = {"mirna": mir, "hairpin": hp, "mature_trna": lib("tRNA-", 4, 74), "pre_trna": lib("pre-tRNA-", 4, 92), "snorna": lib("SNO", 12, 140),
            "rrna": lib("RR", 6, 400), "ncrna_others": lib("NC", 12, 420), "mrna": lib("ENST", 16, 600)}
    if mrna_headers:
        m = libs["mrna"]
        libs["mrna"] = Library(m.names, m.seqs, [mrna_headers.get(nm, h) for nm, h in zip(m.names, m.headers)])
    return libs


def _collapsed(ctx, reads, want):
    """unique reads with the count matrix ``want`` [reads][S] (test_sam_out_gpu.fuzz_case)"""
    S = want.shape[1]
    ent = [(i, s) for i in range(len(reads)) for s in range(S) if want[i, s] > 0]
    raw = _ffi.DeviceReads.pack(ctx, FlatSeqs.from_list([reads[i] for i, _ in ent]))
    uniq = raw.collapse(np.asarray([s for _, s in ent], dtype=np.int32), S, weights=np.asarray([want[i, s] for i, s in ent], dtype=np.uint32))
    raw.close()
    return uniq


def _expected_files(rows, names, stranded):
    rank = {nm: k for k, nm in enumerate(names)}
    runs = coverage.coverage_host(cov_cases.make([(rank[c], s, n, w, mi) for c, s, n, w, mi in rows]), stranded)
    return [coverage.format_bedgraph(runs, names, 0), coverage.format_bedgraph(runs, names, 1)] if stranded else [coverage.format_bedgraph(runs, names)]


@pytest.fixture(scope="module")
def fuzz_case(ctx):
    rng = np.random.Generator(np.random.PCG64(77002))
    libs = _fuzz_libs(rng)
    reads = _fuzz_reads(rng, libs)
    casc = Cascade(ctx, libs)
    S = 4
    want = rng.integers(1, 40, size=(len(reads), S))
    want[rng.random(size=want.shape) < 0.35] = 0
    want[:, 0] = np.maximum(want[:, 0], 1)
    dr = _ffi.DeviceReads.pack(ctx, FlatSeqs.from_list(reads))
    r0 = casc.run(dr)
    ps, ref, _, _ = r0.fetch()
    r0.close(); dr.close()
    hp = sam_export.host_passes(casc)
    writes = np.zeros(len(reads), dtype=bool)
    for i in range(len(reads)):
        p = int(ps[i])
        if p in hp:
            writes[i] = sam_export.lift_of(sam_export.header_dictionary(hp[p]["headers"]), hp[p]["names"][int(ref[i])], ORG) is not None
    want[writes, 3] = 0                                        # sample 3: a count only where NO row is kept -> empty files
    want[~writes, 3] = np.maximum(want[~writes, 3], 1)
    short = [i for i in range(len(reads)) if writes[i] and len(reads[i]) == 16]
    want[short[0], 1] = 100001                                 # one heavy row beside rows of count 1
    want[short[1:4], 1] = 1
    uniq = _collapsed(ctx, reads, want)
    res = casc.run(uniq)
    useq = uniq.unpack().to_list()
    counts, _ = uniq.counts()
    assert sorted(useq) == reads and int(counts.max()) == 100001
    order = rng.permutation(len(useq)).astype(np.int64)
    ps, ref, off, _mm = res.fetch()
    rows = [coverage.intervals_host(useq, ps, ref, off, counts, order, s, hp, ORG) for s in range(S)]
    assert rows[3] == [] and all(len(r) > 100 for r in rows[:3]) and {mi for r in rows for *_, mi in r} == {0, 1}
    yield dict(casc=casc, uniq=uniq, res=res, order=order, rows=rows, S=S)
    res.close(); uniq.close(); casc.close()


@pytest.mark.parametrize("stranded", [False, True], ids=["unstranded", "stranded"])
@pytest.mark.parametrize("sizes", [None, (4096, 64)], ids=["default_sizes", "chunk4096_tile64"])
def test_device_equals_coverage_host(fuzz_case, sizes, stranded, tmp_path, monkeypatch):
    if sizes:
        monkeypatch.setenv("MIRGE_COV_CHUNK_BYTES", str(sizes[0]))
        monkeypatch.setenv("MIRGE_COV_TILE_BYTES", str(sizes[1]))
    else:
        monkeypatch.delenv("MIRGE_COV_CHUNK_BYTES", raising=False)
        monkeypatch.delenv("MIRGE_COV_TILE_BYTES", raising=False)
    f = fuzz_case
    byte_order = sorted({c for r in f["rows"] for c, *_ in r}, key=lambda s: s.encode())
    # the default sizes under the byte order, the small ones under an @SQ order with names no row uses
    names = byte_order if sizes is None else ["chrUn_not_used"] + byte_order[::-1] + ["chrM"]
    for s in range(f["S"]):
        paths = coverage.sample_paths(tmp_path, f"S{s}", stranded)
        st = coverage.write_sample(f["casc"], f["uniq"], f["res"], f["order"], s, paths, stranded, ORG, None if sizes is None else names)
        want = _expected_files(f["rows"][s], names, stranded)
        got = [p.read_bytes() for p in paths]
        assert got == want, f"sample {s}"
        assert st["bytes"] == sum(len(x) for x in got) and st["lines"] == sum(x.count(b"\n") for x in got)
        assert st["intervals"] == len(f["rows"][s]) and st["weight"] == sum(r[3] for r in f["rows"][s])
        if s == 0:  # (more chunks than staging halves, and the split between the two files inside a chunk)
            assert sum(len(x) for x in got) > 4096 * 3
        if s == 1:
            assert any(int(ln.split(b"\t")[3]) >= 100001 for x in got for ln in x.splitlines())


def test_a_chromosome_no_sq_line_names_fails_and_leaves_no_file(fuzz_case, tmp_path):
    f = fuzz_case
    used = sorted({c for c, *_ in f["rows"][0]})
    for stranded in (False, True):
        paths = coverage.sample_paths(tmp_path, "S0", stranded)
        with pytest.raises(ValueError, match="'" + used[-1] + "'.*no @SQ line"):
            coverage.write_sample(f["casc"], f["uniq"], f["res"], f["order"], 0, paths, stranded, ORG, used[:-1])
        assert not os.listdir(tmp_path)
    # the sample without a kept row does not mind
    paths = coverage.sample_paths(tmp_path, "S3", True)
    assert coverage.write_sample(f["casc"], f["uniq"], f["res"], f["order"], 3, paths, True, ORG, [])["lines"] == 0
    assert [p.read_bytes() for p in paths] == [b"", b""]


def test_a_row_outside_the_positions_fails_naming_the_read(ctx, tmp_path):
    """START < 1 and an end beyond 2^31 - 1, built through header coordinates"""
    rng = np.random.Generator(np.random.PCG64(77003))
    libs = _fuzz_libs(rng, {"ENST0": "ENST0 chr1 segs:1-600 cds:+:0-599", "ENST1": "ENST1 chr1 segs:1-600 cds:+:2147483600-2147484199",
                            "ENST2": "ENST2 chr1 segs:1-600 cds:+:2147483000-2147483599"})
    m = libs["mrna"].seqs.to_list()
    reads = sorted([m[0][0:30], m[1][30:60], m[2][570:600], m[2][100:140]])
    want = np.zeros((4, 3), dtype=np.int64)
    want[reads.index(m[0][0:30]), 0] = 2       # START 0
    want[reads.index(m[1][30:60]), 1] = 1      # the end lies beyond 2^31 - 1
    want[reads.index(m[2][570:600]), 2] = 3    # both inside: the third sample succeeds
    want[reads.index(m[2][100:140]), 2] = 1
    casc = Cascade(ctx, libs)
    uniq = _collapsed(ctx, reads, want)
    res = casc.run(uniq)
    order = np.arange(len(uniq), dtype=np.int64)
    try:
        for s, (read, refname) in enumerate([(m[0][0:30], "ENST0"), (m[1][30:60], "ENST1")]):
            for stranded in (False, True):
                with pytest.raises(ValueError, match=read + ".*" + refname):
                    coverage.write_sample(casc, uniq, res, order, s, coverage.sample_paths(tmp_path, "bad", stranded), stranded, ORG)
            assert not os.listdir(tmp_path)
        path = coverage.sample_paths(tmp_path, "good", False)
        coverage.write_sample(casc, uniq, res, order, 2, path, False, ORG)
        assert path[0].read_bytes() == b"chr1\t2147483099\t2147483139\t1\nchr1\t2147483569\t2147483599\t3\n"
    finally:
        res.close(); uniq.close(); casc.close()


# ---------------------------------------------------------------------------------------------------------------------
# the golden inputs through the CLI
# ---------------------------------------------------------------------------------------------------------------------
def _cli(argv):
    cmd = [sys.executable, "-c", "import sys; sys.path.insert(0, %r); import mirge3_amd; from mirge3_amd.cli import main; main()" % ROOT]
    r = subprocess.run(cmd + list(argv), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.fixture(scope="module")
def golden_runs(tmp_path_factory):
    """the golden inputs through the CLI: --coverage, --coverage stranded, --coverage --sam-header FILE (chr2 before chr1), no switch"""
    tmp = tmp_path_factory.mktemp("coverage")
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
    header = tmp / "header.sam"
    header.write_text("@HD\tVN:1.0\tSO:unsorted\n" + "".join(f"@SQ\tSN:{c}\tLN:248956422\n" for c in SQ_ORDER))
    base = ["-s", ",".join(files), "-lib", os.path.join(GOLDEN, "libs"), "-on", ORG, "-db", "miRBase", "-o", str(tmp), "-shh"]
    _cli(base + ["-dn", "unstranded", "--coverage"])
    _cli(base + ["-dn", "stranded", "--coverage", "stranded"])
    _cli(base + ["-dn", "sq_order", "--coverage", "--sam-header", str(header)])
    _cli(base + ["-dn", "plain"])
    return tmp, samples


def test_cli_golden_files(golden_runs):
    tmp, samples = golden_runs
    for nm in samples:
        assert [(tmp / "unstranded" / f"{nm}.bedgraph").read_bytes()] == golden_bedgraph(nm, False)
        assert [(tmp / "stranded" / f"{nm}.plus.bedgraph").read_bytes(), (tmp / "stranded" / f"{nm}.minus.bedgraph").read_bytes()] == golden_bedgraph(nm, True)
        got = (tmp / "sq_order" / f"{nm}.bedgraph").read_bytes()
        assert [got] == golden_bedgraph(nm, False, SQ_ORDER) and got.startswith(b"chr2\t") and got != golden_bedgraph(nm, False)[0]
        log = (tmp / "unstranded" / "run.log").read_text()
        assert f"{nm}: " in log and " intervals, summed weight " in log
    assert sorted(f for f in os.listdir(tmp / "stranded") if f.endswith(".bedgraph")) == sorted(f"{nm}.{s}.bedgraph" for nm in samples for s in ("plus", "minus"))
    assert not [f for f in os.listdir(tmp / "unstranded") if f.endswith((".sam", ".bam"))]


def test_cli_sq_list_lacking_chr6_fails_naming_it_and_leaves_no_bedgraph(golden_runs):
    tmp, samples = golden_runs
    header = tmp / "header_without_chr6.sam"
    header.write_text("".join(f"@SQ\tSN:{c}\tLN:248956422\n" for c in SQ_ORDER if c != "chr6"))
    files = ",".join(str(tmp / f"{nm}.fastq") for nm in samples)
    cmd = [sys.executable, "-c", "import sys; sys.path.insert(0, %r); import mirge3_amd; from mirge3_amd.cli import main; main()" % ROOT]
    r = subprocess.run(cmd + ["-s", files, "-lib", os.path.join(GOLDEN, "libs"), "-on", ORG, "-db", "miRBase", "-o", str(tmp), "-shh", "-dn", "no_chr6",
                              "--coverage", "stranded", "--sam-header", str(header)], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "'chr6'" in r.stderr and "no @SQ line" in r.stderr
    assert not [f for f in os.listdir(tmp / "no_chr6") if f.endswith(".bedgraph")]


def test_cli_without_the_switch_writes_no_bedgraph_and_the_same_other_files(golden_runs):
    tmp, samples = golden_runs
    assert not [f for f in os.listdir(tmp / "plain") if f.endswith(".bedgraph")]
    assert sorted(f for f in os.listdir(tmp / "unstranded") if not f.endswith(".bedgraph")) == sorted(os.listdir(tmp / "plain"))
    for f in OTHER_OUTPUTS:
        assert (tmp / "unstranded" / f).read_bytes() == (tmp / "plain" / f).read_bytes(), f
