"""``--sam-out`` on the GPU: the golden run through the CLI (tests/golden/sam_out: the reference's own files), with and without
``--sam-header`` and without the switch; ``mirge_sam_write_device`` against ``sam_export.format_sam_host`` on a few hundred unique
reads of every length class at the default chunk / tile sizes and at sizes that put their boundaries inside lines, inside a QNAME's
digits and inside a row of 100 001 copies.  Whole files, byte for byte."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mirge3_amd  # noqa: F401
from mirge3_amd import _ffi, sam_export
from mirge3_amd.cascade import Cascade
from mirge3_amd.seqio import FlatSeqs, Library

from test_sam_out import GOLDEN, ORG, golden_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
OTHER_OUTPUTS = ("mapped.csv", "unmapped.csv", "miR.Counts.csv", "miR.RPM.csv", "annotation.report.csv")


def _cli(argv):
    cmd = [sys.executable, "-c", "import sys; sys.path.insert(0, %r); import mirge3_amd; from mirge3_amd.cli import main; main()" % ROOT]
    r = subprocess.run(cmd + list(argv), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.fixture(scope="module")
def golden_runs(tmp_path_factory):
    """the golden inputs through the CLI three times: --sam-out, --sam-out --sam-header FILE, neither"""
    tmp = tmp_path_factory.mktemp("sam_out")
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
    header.write_bytes(b"@HD\tVN:1.0\tSO:unsorted\n@SQ\tSN:chr1\tLN:248956422\n@SQ\tSN:chr2\tLN:242193529\n@CO\tno newline at the end")
    base = ["-s", ",".join(files), "-lib", os.path.join(GOLDEN, "libs"), "-on", ORG, "-db", "miRBase", "-o", str(tmp), "-shh"]
    _cli(base + ["-dn", "sam", "--sam-out"])
    _cli(base + ["-dn", "sam_header", "--sam-out", "--sam-header", str(header)])
    _cli(base + ["-dn", "plain"])
    return tmp, samples, header.read_bytes()


def test_cli_golden_files(golden_runs):
    tmp, samples, _ = golden_runs
    for nm in samples:
        with open(os.path.join(GOLDEN, nm + ".sam"), "rb") as fh:
            assert (tmp / "sam" / (nm + ".sam")).read_bytes() == fh.read(), nm
    assert "--sam-out without --sam-header" in (tmp / "sam" / "run.log").read_text()


def test_cli_golden_files_with_header_file(golden_runs):
    tmp, samples, header = golden_runs
    for nm in samples:
        with open(os.path.join(GOLDEN, nm + ".sam"), "rb") as fh:
            body = fh.read()[len(sam_export.DEFAULT_HEADER):]
        assert (tmp / "sam_header" / (nm + ".sam")).read_bytes() == header + body, nm
    assert "--sam-out without --sam-header" not in (tmp / "sam_header" / "run.log").read_text()


def test_cli_without_the_switch_writes_no_sam_and_the_same_other_files(golden_runs):
    tmp, samples, _ = golden_runs
    assert not [f for f in os.listdir(tmp / "plain") if f.endswith(".sam")]
    assert sorted(f for f in os.listdir(tmp / "sam") if not f.endswith(".sam")) == sorted(os.listdir(tmp / "plain"))
    for f in OTHER_OUTPUTS:
        assert (tmp / "sam" / f).read_bytes() == (tmp / "plain" / f).read_bytes(), f


# ---------------------------------------------------------------------------------------------------------------------
# fuzzer: the device call against format_sam_host
# ---------------------------------------------------------------------------------------------------------------------
def _rnd(rng, n):
    return "".join("ACGT"[int(c)] for c in rng.integers(0, 4, size=n))


def _coordinates(rng, name, length, chrom):
    """a header line: one to four segments that tile 1..length (sometimes with a gap), either strand; some references get none"""
    kind = int(rng.integers(0, 10))
    if kind == 0:
        return name
    if kind == 1:
        return f"{name} {chrom}_PATCH segs:1-{length} cds:+:100-{99 + length}"
    n_seg = int(rng.integers(1, 5))
    cuts = sorted(set(int(x) for x in rng.integers(2, max(3, length), size=n_seg - 1)))
    bounds = [1] + cuts + [length + 1]
    segs, cds, g = [], [], int(rng.integers(10_000_000, 5_000_000_000))
    minus = bool(rng.integers(0, 2))
    for a, b in zip(bounds[:-1], bounds[1:]):
        s = a + (3 if (rng.random() < 0.2 and b - a > 8) else 0)  # a gap in front of the segment: some POS lie in no segment
        segs.append(f"{s}-{b - 1}")
        cds.append(f"{g}-{g + (b - 1 - s)}")
        g = g - int(rng.integers(500, 5000)) - (b - a) if minus else g + (b - a) + int(rng.integers(500, 5000))
    return f"{name} {chrom} segs:{','.join(segs)} cds:{'-' if minus else '+'}:{','.join(cds)}"


def _fuzz_libs(rng):
    def lib(prefix, n, length):
        seqs = [_rnd(rng, length) for _ in range(n)]
        names = [f"{prefix}{i}" for i in range(n)]
        return Library(names, FlatSeqs.from_list(seqs), [_coordinates(rng, nm, length, f"chr{1 + i % 5}") for i, nm in enumerate(names)])
    mir = lib("miR-", 24, 22)
    mseq = mir.seqs.to_list()
    hseq = [_rnd(rng, 15) + m + _rnd(rng, 50) for m in mseq[:12]]
    hp = Library([f"mir-{i}" for i in range(12)], FlatSeqs.from_list(hseq),
                 [_coordinates(rng, f"mir-{i}", len(hseq[i]), f"chr{1 + i % 3}") for i in range(12)])
    return {"mirna": mir, "hairpin": hp, "mature_trna": lib("tRNA-", 4, 74), "pre_trna": lib("pre-tRNA-", 4, 92), "snorna": lib("SNO", 12, 140),
            "rrna": lib("RR", 6, 400), "ncrna_others": lib("NC", 12, 420), "mrna": lib("ENST", 16, 600)}


def _fuzz_reads(rng, libs):
    reads = set()
    for key in ("snorna", "rrna", "ncrna_others", "mrna", "hairpin"):
        seqs = libs[key].seqs.to_list()
        for L in (16, 25, 26, 64, 300):
            for _ in range(14):
                q = seqs[int(rng.integers(0, len(seqs)))]
                if len(q) < L:
                    continue
                o = int(rng.integers(0, len(q) - L + 1))
                r = list(q[o:o + L])
                u = rng.random()
                if u < 0.25 and key != "mrna":  # one mismatch, or an N, where the pass allows one
                    r[int(rng.integers(0, min(L, 28)))] = "N" if u < 0.1 else "ACGT"[int(rng.integers(0, 4))]
                reads.add("".join(r))
    mseq = libs["mirna"].seqs.to_list()
    for m in mseq:
        reads.add(m)                                           # exact miRNA
        reads.add(_rnd(rng, 1) + m[:20] + _rnd(rng, 2))        # isomiR pass: 1 and 2 bases cut
        r = list(m[1:21]); r[int(rng.integers(0, 20))] = "ACGT"[int(rng.integers(0, 4))]
        reads.add(_rnd(rng, 1) + "".join(r) + _rnd(rng, 2))
    for L in (16, 25, 26, 64, 300):
        for _ in range(6):
            reads.add(_rnd(rng, L))                            # unmapped
    return sorted(reads)


@pytest.fixture(scope="module")
def fuzz_case():
    rng = np.random.Generator(np.random.PCG64(77001))
    libs = _fuzz_libs(rng)
    reads = _fuzz_reads(rng, libs)
    ctx = _ffi.Context(0)
    casc = Cascade(ctx, libs)
    S = 4
    want = rng.integers(1, 40, size=(len(reads), S))
    want[rng.random(size=want.shape) < 0.35] = 0               # zero counts sprinkled in
    want[:, 0] = np.maximum(want[:, 0], 1)                     # (every read exists somewhere)
    # annotate once to learn which rows write lines: sample 3 keeps a count only where NO line is written
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
    want[writes, 3] = 0
    want[~writes, 3] = np.maximum(want[~writes, 3], 1)
    short = [i for i in range(len(reads)) if writes[i] and len(reads[i]) == 16]
    want[short[0], 1] = 100001                                 # one heavy row beside rows of count 1
    want[short[1:4], 1] = 1
    ent = [(i, s) for i in range(len(reads)) for s in range(S) if want[i, s] > 0]
    raw = _ffi.DeviceReads.pack(ctx, FlatSeqs.from_list([reads[i] for i, _ in ent]))
    uniq = raw.collapse(np.asarray([s for _, s in ent], dtype=np.int32), S, weights=np.asarray([want[i, s] for i, s in ent], dtype=np.uint32))
    raw.close()
    res = casc.run(uniq)
    useq = uniq.unpack().to_list()
    counts, _ = uniq.counts()
    assert sorted(useq) == reads and int(counts.max()) == 100001
    order = rng.permutation(len(useq)).astype(np.int64)
    ann = res.fetch()
    lengths = {len(useq[i]) for i in range(len(useq)) if int(ann[0][i]) in hp}
    assert {16, 25, 26, 64, 300} <= lengths and set(sam_export.CLASS_PASSES) <= set(int(p) for p in ann[0])
    expected = [sam_export.format_sam_host(useq, *ann, counts, order, s, hp, ORG) for s in range(S)]
    assert expected[3] == b"" and all(len(e) > 0 for e in expected[:3])
    assert any(b"\t16\t" in e for e in expected) and len(expected[1]) > 4096 * 100
    yield dict(casc=casc, uniq=uniq, res=res, order=order, expected=expected, counts=counts, S=S)
    res.close(); uniq.close(); casc.close()


@pytest.mark.parametrize("sizes", [None, (4096, 256)], ids=["default_sizes", "chunk4096_tile256"])
def test_device_equals_format_sam_host(fuzz_case, sizes, tmp_path, monkeypatch):
    if sizes:
        monkeypatch.setenv("MIRGE_SAM_CHUNK_BYTES", str(sizes[0]))
        monkeypatch.setenv("MIRGE_SAM_TILE_BYTES", str(sizes[1]))
    else:
        monkeypatch.delenv("MIRGE_SAM_CHUNK_BYTES", raising=False)
        monkeypatch.delenv("MIRGE_SAM_TILE_BYTES", raising=False)
    f = fuzz_case
    header = b"@HD\tVN:1.0\tSO:unsorted\n@CO\tfuzz"
    for s in range(f["S"]):
        path = tmp_path / f"S{s}.sam"
        n_lines, n_bytes = sam_export.write_sample(f["casc"], f["uniq"], f["res"], f["order"], s, path, header, ORG)
        got = path.read_bytes()
        assert got == header + f["expected"][s], f"sample {s}"
        assert n_bytes == len(got) - len(header) == os.path.getsize(path) - len(header)
        assert n_lines == f["expected"][s].count(b"\n")
