"""``--trf-clusters`` on the MI355X.  ``mirge_trf_cluster`` (csrc/native_trf.hpp) through the C ABI on the groups of
tests/test_trf_clusters_hostsim.py: every returned array equals the NumPy restatement of the reference's clustering exactly, ``rho``
as float32 bits.  The CLI on tests/golden/case9_trf_clusters: every file equals what the reference wrote, the two clustering files per
sample included; ``--trf-report`` alone leaves them out."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mirge3_amd  # noqa: F401
from mirge3_amd import _ffi
from mirge3_amd.cli import parse_args
from mirge3_amd.seqio import FlatSeqs

from test_trf_clusters import DB, GOLDEN, NEW, OLD, ORG, SAMPLE_FILES, TOP
from test_trf_clusters_hostsim import assert_equal, check_case, flat_groups, want  # noqa: F401  (want: the shared fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_device_arrays_equal_the_restatement(want):  # noqa: F811
    reads, groups, w = want
    check_case(want)
    ctx = _ffi.Context(0)
    raw = _ffi.DeviceReads.pack(ctx, FlatSeqs.from_list(reads))
    uniq = raw.collapse()
    raw.close()
    try:
        handle = {rd: k for k, rd in enumerate(uniq.unpack().to_list())}
        assert len(handle) == len(reads)
        ptr, read, off, rp, tlen = flat_groups(groups)
        got = _ffi.trf_cluster(ctx, uniq, ptr, [handle[reads[i]] for i in read], off, rp, tlen)
        assert_equal(got, w)
        with pytest.raises(RuntimeError, match="a template of 257 columns is longer than 256"):
            _ffi.trf_cluster(ctx, uniq, [0, 1], [0], [0], [1.0], [257], gauss=_ffi.trf_gauss(257))
        with pytest.raises(RuntimeError, match="does not fit its template"):
            _ffi.trf_cluster(ctx, uniq, [0, 1], [0], [250], [1.0], [256])
        empty = _ffi.trf_cluster(ctx, uniq, [0, 0], [], [], [], [80])
        assert empty["rho"].shape[0] == 0 and empty["nclust"].tolist() == [0]
    finally:
        uniq.close()
        ctx.close()


def _cli(argv):
    cmd = [sys.executable, "-c", "import sys; sys.path.insert(0, %r); import mirge3_amd; from mirge3_amd.cli import main; main()" % ROOT]
    r = subprocess.run(cmd + list(argv), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def test_cli_writes_the_reference_files(tmp_path):
    """(the CLI is what this test is about: one run with the switch, one with --trf-report alone)"""
    files = ",".join(os.path.join(GOLDEN, f) for f in SAMPLE_FILES)
    base = ["-s", files, "-lib", os.path.join(GOLDEN, "libs"), "-on", ORG, "-db", DB, "-o", str(tmp_path), "-shh"]
    _cli(base + ["-dn", "clusters", "--trf-clusters"])
    for f in TOP + OLD + NEW:
        with open(os.path.join(GOLDEN, f), "rb") as fh:
            assert (tmp_path / "clusters" / f).read_bytes() == fh.read(), f
    assert sorted(os.listdir(tmp_path / "clusters" / "tRFs.samples.tmp")) == sorted(os.path.basename(f) for f in OLD + NEW)
    _cli(base + ["-dn", "report", "--trf-report"])
    for f in TOP + OLD:
        with open(os.path.join(GOLDEN, f), "rb") as fh:
            assert (tmp_path / "report" / f).read_bytes() == fh.read(), f
    assert sorted(os.listdir(tmp_path / "report" / "tRFs.samples.tmp")) == sorted(os.path.basename(f) for f in OLD)


def test_switch_with_spl_is_an_argparse_error(capsys):
    with pytest.raises(SystemExit) as e:
        parse_args(["-s", "x.fastq", "-lib", "L", "-on", "human", "--trf-clusters", "-spl"])
    assert e.value.code == 2 and "--trf-clusters" in capsys.readouterr().err
