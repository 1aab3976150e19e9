"""``--trf-report`` on the MI355X.  The CLI on tests/golden/case8_trf: the six files equal what the reference wrote.  The device
calls (``mirge_trf_hits_run``, ``mirge_trf_assign``, ``mirge_trf_row_counts``: csrc/native_trf.hpp) through the C ABI: the real
cascade classifies the reads of a synthetic tRNA library, the hit records are held against a brute-force enumeration of every
window and the assignment against ``assign_cluster`` restated (tests/test_trf_hostsim.py).  Two library sizes: one whose probe
tables are bitmap + CSR bounds, one padded with random references beyond 4^10 / 4 positions so that its tables are self-contained
entries (``MirgeKTable``)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import mirge3_amd  # noqa: F401
from mirge3_amd import _ffi
from mirge3_amd.cascade import policies
from mirge3_amd.seqio import FlatSeqs

from test_trf import DB, GOLDEN, ORG, SAMPLES, SIX
from test_trf_hostsim import (MATURE_PASS, PRIMARY_PASS, Text, assign_rows, classify, expected_assign, expected_records, infor_tables,
                              synth_case, synth_infor)

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _cli(argv):
    cmd = [sys.executable, "-c", "import sys; sys.path.insert(0, %r); import mirge3_amd; from mirge3_amd.cli import main; main()" % ROOT]
    r = subprocess.run(cmd + list(argv), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def test_cli_writes_the_reference_files(tmp_path):
    """(the CLI is what this test is about: one run with the switch, one with an annotation file missing)"""
    files = ",".join(os.path.join(GOLDEN, s + ".fastq") for s in SAMPLES)
    base = ["-s", files, "-lib", os.path.join(GOLDEN, "libs"), "-on", ORG, "-db", DB, "-o", str(tmp_path), "-shh"]
    _cli(base + ["-dn", "trf", "--trf-report"])
    for f in SIX:
        with open(os.path.join(GOLDEN, f), "rb") as fh:
            assert (tmp_path / "trf" / f).read_bytes() == fh.read(), f
    assert sorted(os.listdir(tmp_path / "trf" / "tRFs.samples.tmp")) == sorted(os.path.basename(f) for f in SIX[4:])
    libs = tmp_path / "libs"
    shutil.copytree(os.path.join(GOLDEN, "libs"), libs)
    gone = libs / ORG / "annotation.Libs" / f"{ORG}_tRF_merges.csv"
    os.remove(gone)
    _cli(["-s", files, "-lib", str(libs), "-on", ORG, "-db", DB, "-o", str(tmp_path), "-shh", "-dn", "missing", "--trf-report"])
    assert f"File {gone} does not exist!!\nProceeding the annotation with out -trf\n" in (tmp_path / "missing" / "run.log").read_text()
    assert not [f for f in os.listdir(tmp_path / "missing") if "tRF" in f] and (tmp_path / "missing" / "mapped.csv").exists()


def _filler(n_bases, seed):
    rng = np.random.default_rng(seed)
    return ["".join("ACGT"[x] for x in rng.integers(0, 4, 900)) for _ in range(n_bases // 900 + 1)]


class Run:
    """libraries on the device, the reads collapsed and classified by the real cascade, and the brute force's answer for the same
    reads in the handle's order"""

    def __init__(self, filler_bases):
        mature, primary, self.anticodon, reads = synth_case(seed=11, n_random=1500)
        self.mature = mature + (_filler(filler_bases, 21) if filler_bases else [])
        self.primary = primary + (_filler(filler_bases, 22) if filler_bases else [])
        self.anticodon = self.anticodon + [30] * (len(self.mature) - len(mature))
        self.ctx = _ffi.Context(0)
        self.mlib = _ffi.DeviceLibrary(self.ctx, FlatSeqs.from_list(self.mature))
        self.plib = _ffi.DeviceLibrary(self.ctx, FlatSeqs.from_list(self.primary))
        self.pol = policies(4)
        raw = _ffi.DeviceReads.pack(self.ctx, FlatSeqs.from_list(reads))
        self.uniq = raw.collapse()
        raw.close()
        self.reads = self.uniq.unpack().to_list()
        assert sorted(self.reads) == sorted(reads)
        self.res = _ffi.cascade_run(self.ctx, self.uniq, [None, None, self.mlib, self.plib], self.pol)
        self.tm, self.tp = Text(self.mature), Text(self.primary)
        self.tm.prefilter(); self.tp.prefilter()
        self.ps, self.mm, self.hits = classify(self.reads, self.tm, self.tp, fast=True)

    def close(self):
        for h in (self.res, self.uniq, self.mlib, self.plib, self.ctx):
            h.close()


@pytest.fixture(scope="module", params=[0, 270000], ids=["bitmap-csr", "entries"])
def run(request):
    r = Run(request.param)
    yield r
    r.close()


def test_cascade_classes_are_the_brute_force_classes(run):
    ps, _, _, mm = run.res.fetch()
    assert np.array_equal(ps, run.ps)
    sel = run.ps >= 0
    assert np.array_equal(mm[sel], run.mm[sel])
    lens = np.asarray([len(r) for r in run.reads])
    for lo, hi in ((16, 31), (32, 64), (65, 95)):  # W = 1, 2, 4
        assert (sel & (lens >= lo) & (lens <= hi)).sum() > 20


def test_hit_records_equal_brute_force(run):
    rows = np.asarray(sorted(run.hits), dtype=np.int64)
    np.random.default_rng(2).shuffle(rows)
    got = _ffi.trf_hits(run.ctx, run.uniq, run.res, MATURE_PASS, run.mlib, run.pol[MATURE_PASS], PRIMARY_PASS, run.plib,
                        run.pol[PRIMARY_PASS], rows, run.anticodon)
    got = [tuple(int(got[k][i]) for k in ("row", "ref", "off", "mm", "cls", "type")) for i in range(got["row"].shape[0])]
    want = expected_records(run.reads, rows.tolist(), run.ps, run.mm, run.hits, run.tm, run.anticodon)
    assert len(want) > len(rows)  # (reads with several windows)
    assert got == want  # as sorted lists: a duplicate or a miss shows


def test_hits_of_no_rows_and_of_a_foreign_row(run):
    empty = _ffi.trf_hits(run.ctx, run.uniq, run.res, MATURE_PASS, run.mlib, run.pol[MATURE_PASS], PRIMARY_PASS, run.plib,
                          run.pol[PRIMARY_PASS], np.zeros(0, np.int64), run.anticodon)
    assert empty["row"].shape[0] == 0
    other = np.nonzero(run.ps < 0)[0][:1]
    with pytest.raises(RuntimeError, match="neither a mature-tRNA nor a primary-tRNA read"):
        _ffi.trf_hits(run.ctx, run.uniq, run.res, MATURE_PASS, run.mlib, run.pol[MATURE_PASS], PRIMARY_PASS, run.plib,
                      run.pol[PRIMARY_PASS], other, run.anticodon)


def test_assignment_equals_the_restatement(run):
    case = dict(reads=run.reads, mature=run.mature, hits=run.hits, ps=run.ps)
    infor = synth_infor(run.mature[:15])
    tref, ref_ptr, strings, names, cs, ce, rank = infor_tables(infor, len(run.mature))
    rows = assign_rows(case, infor, n=500)
    want = expected_assign(case, infor, rows)
    assert any(d == 8 for d, _ in want) and any(d == 9 for d, _ in want) and any(n is None for _, n in want)
    dist, trf = _ffi.trf_assign(run.ctx, run.uniq, run.res, [r[0] for r in rows], tref[[r[1] for r in rows]], [r[2] for r in rows],
                                ref_ptr, strings, cs, ce, rank)
    got = [(int(d), names[t] if t >= 0 else None) for d, t in zip(dist, trf)]
    assert got == want
