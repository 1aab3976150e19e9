"""``-a auto`` on the MI355X: ``mirge_adapter_infer`` (csrc/native_adapter.hpp, csrc/kernels_adapter.hpp) through the C ABI on the cases of
tests/ad_cases.py and on 300 random tie-rich sets -- inputs built with ``DeviceReads.pack`` + ``collapse(weights=counts)`` so that counts
are free to choose --, on a dictionary that ``mirge_collapse`` made of a FASTQ text of 72 000 raw records (its partitioned route), then
the command line on synthetic samples.  Every field of ``mirge_adapter`` and C and M of every probed 12-mer (all of the case's and
absent ones) are compared exactly with the restatement (tests/ad_restate.py), with the table filled by the store-and-sum form and by the atomic one."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import ad_cases
import ad_restate
from helpers import GoldenCase, ORG
import mirge3_amd  # noqa: F401
from mirge3_amd import _ffi, adapter_auto
from mirge3_amd.seqio import FlatSeqs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(params=["sort", "atomic"])
def form(request, monkeypatch):
    """how the table is filled (MIRGE_ADAPTER_COUNT, read per call): store-and-sum, or an atomic add and or per window"""
    monkeypatch.setenv("MIRGE_ADAPTER_COUNT", request.param)
    return request.param


def infer(ctx, reads, counts, codes):
    raw = _ffi.DeviceReads.pack(ctx, FlatSeqs.from_list(list(reads)))
    d0 = raw.collapse(weights=np.asarray(counts, dtype=np.uint32))
    try:
        assert len(d0) == len(reads)
        got, sums, masks = d0.adapter_infer(codes)
        return got, sums.tolist(), masks.tolist()
    finally:
        d0.close(); raw.close()


def same(ctx, reads, counts, want, codes, name):
    got, sums, masks = infer(ctx, reads, counts, codes)
    assert got == ad_restate.fields(want), name
    wsum, wmask = ad_cases.probe_answers(want, codes)
    assert sums == wsum and masks == wmask, name


@pytest.mark.parametrize("name", sorted(ad_cases.all_cases()))
def test_cases_equal_the_restatement(ctx, name, form):
    c = ad_cases.all_cases()[name]
    same(ctx, c["reads"], c["counts"], ad_cases.expected(name), ad_cases.probes(name), name)


def test_random_sets_equal_the_restatement(ctx, form):
    ties = {"seed": 0, "left": 0, "right": 0}
    for seed in range(300):
        c = ad_cases.random_set(seed)
        want = ad_restate.infer(c["reads"], c["counts"])
        same(ctx, c["reads"], c["counts"], want, ad_restate.probes_of(c["reads"], extra=[seed, 4 ** 12 - 1 - seed, 4 ** 12]), seed)
        for k in ties:
            ties[k] += want["ties"][k]
    assert min(ties.values()) > 0, ties


def test_without_probes_and_twice_over(ctx):
    """the call without a probe list, and again on the same dictionary: the table is cleared per call"""
    c = ad_cases.all_cases()["planted_50"]
    raw = _ffi.DeviceReads.pack(ctx, FlatSeqs.from_list(c["reads"]))
    d0 = raw.collapse(weights=np.asarray(c["counts"], dtype=np.uint32))
    try:
        want = ad_restate.fields(ad_cases.expected("planted_50"))
        assert d0.adapter_infer() == want and d0.adapter_infer() == want
        assert d0.adapter_infer(np.zeros(0, np.uint32))[0] == want
    finally:
        d0.close(); raw.close()


def _fastq(reads):
    return "".join(f"@r{i}\n{r}\n+\n{'I' * len(r)}\n" for i, r in enumerate(reads)).encode()


def _dictionary(reads):
    d = {}
    for r in reads:
        d[r] = d.get(r, 0) + 1
    return list(d), list(d.values())


def test_a_dictionary_of_72000_raw_records_equals_the_restatement(ctx, form):
    """a FASTQ text of 72 000 records (a synthetic sample at 50 cycles, some reads with an N) parsed without trimming and collapsed by
    ``mirge_collapse``: 65 536 reads and more take its partitioned route, whose handle order is unspecified"""
    dreads, dcounts = ad_cases.synthetic_sample(3, adapter=ad_cases.ILLUMINA, cycles=50, n_reads=72000)
    rng = np.random.default_rng(4)
    reads = np.repeat(np.arange(len(dreads)), dcounts)
    reads = [dreads[i] for i in rng.permutation(reads)]
    for i in range(0, len(reads), 97):
        reads[i] = reads[i][:30] + "N" + reads[i][31:]
    assert len(reads) == 72000
    dreads, dcounts = _dictionary(reads)
    want = ad_restate.infer(dreads, dcounts)
    assert want["seq"].startswith(ad_cases.ILLUMINA[:20]) and want["eligible"] == 72000 - len(range(0, 72000, 97))
    codes = ad_restate.probes_of(dreads[:300], extra=[0, 4 ** 12 - 1])
    raw, n_rec = _ffi.DeviceReads.parse(ctx, _fastq(reads), 1, 0, None)
    d0 = raw.collapse()
    try:
        assert n_rec == 72000 and len(d0) == len(dreads)
        got, sums, masks = d0.adapter_infer(codes)
    finally:
        d0.close(); raw.close()
    assert got == ad_restate.fields(want)
    wsum, wmask = ad_cases.probe_answers(want, codes)
    assert sums.tolist() == wsum and masks.tolist() == wmask


def test_a_two_column_dictionary_and_raw_reads_are_refused(ctx, monkeypatch):
    reads = ["ACGTACGTACGTACGTACGTAC", "ACGTACGTACGTACGTACGTAA", "TTGTACGTACGTACGTACGTAA"]
    raw = _ffi.DeviceReads.pack(ctx, FlatSeqs.from_list(reads))
    two = raw.collapse(np.asarray([0, 1, 1], dtype=np.int32), 2)
    try:
        with pytest.raises(RuntimeError, match="one count column"):
            two.adapter_infer()
        with pytest.raises(RuntimeError):
            raw.adapter_infer()  # no collapse result
        one = raw.collapse()
        try:
            monkeypatch.setenv("MIRGE_ADAPTER_COUNT", "fastest")
            with pytest.raises(RuntimeError, match="MIRGE_ADAPTER_COUNT"):
                one.adapter_infer()
        finally:
            one.close()
    finally:
        two.close(); raw.close()


# ---- the command line ----------------------------------------------------------------------------------------------------------
OFF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmer_correct_off")
TABLES = ("miR.Counts.csv", "miR.RPM.csv", "annotation.report.csv", "mapped.csv", "unmapped.csv")


def _inserts(sample):
    """the committed synthetic inserts of tests/golden/kmer_correct_off (19 .. 25 nt, about 940 per sample)"""
    with open(os.path.join(OFF, f"{sample}.fastq")) as fh:
        return fh.read().split("\n")[1::4]


def _with_adapter(inserts, adapter, cycles=50):
    return [(r + adapter + ad_cases.TAIL)[:cycles] for r in inserts]


def _cli(argv):
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    cmd = [sys.executable, "-c", "import sys; sys.path.insert(0, %r); import mirge3_amd; from mirge3_amd.cli import main; main()" % root]
    return subprocess.run(cmd + list(argv), capture_output=True, text=True, timeout=600)


def _files(out):
    return sorted(f for f in os.listdir(out) if os.path.isfile(os.path.join(out, f)))


@pytest.mark.parametrize("gz", [False, True], ids=["plain", "gz"])
def test_command_line_equals_the_explicit_adapter(tmp_path, gz):
    """two samples that carry one adapter: the run with ``-a auto`` writes, byte for byte, the files of the run with ``-a <the restatement's
    sequence>`` but for run.log and adapter.auto.csv, which are the restatement's"""
    case = GoldenCase("case2_two_samples")
    files, wants = [], []
    for s in ("S1", "S2"):
        reads = _with_adapter(_inserts(s), ad_cases.ILLUMINA, cycles=75)  # (75: both samples' walks reach the cap of 32 letters)
        wants.append((ad_restate.infer(*_dictionary(reads)), len(reads), len(set(reads))))
        p = tmp_path / (f"{s}.fastq.gz" if gz else f"{s}.fastq")
        p.write_bytes(gzip.compress(_fastq(reads)) if gz else _fastq(reads))
        files.append(str(p))
    seq = wants[0][0]["seq"]
    assert wants[1][0]["seq"] == seq == (ad_cases.ILLUMINA + ad_cases.TAIL)[:32]
    common = ["-s", ",".join(files), "-lib", case.libdir, "-on", ORG, "-db", "miRBase", "-o", str(tmp_path), "-shh", "-tcf"]
    for name, a in (("auto", "auto"), ("explicit", seq)):
        r = _cli(common + ["-dn", name, "-a", a])
        assert r.returncode == 0, r.stderr[-3000:]
    names = _files(tmp_path / "explicit")
    assert _files(tmp_path / "auto") == sorted(names + ["adapter.auto.csv"]) and set(TABLES) <= set(names)
    for name in names:
        if name != "run.log":
            assert (tmp_path / "auto" / name).read_bytes() == (tmp_path / "explicit" / name).read_bytes(), name
    assert (tmp_path / "auto" / "adapter.auto.csv").read_text() == ad_restate.csv_text([(s, *w) for s, w in zip(("S1", "S2"), wants)])
    log = (tmp_path / "auto" / "run.log").read_text()
    for s, (want, n, _) in zip(("S1", "S2"), wants):
        assert ad_restate.log_line(s, want, n) + "\n" in log
    assert log.index("adapter auto S2") < log.index("Cutadapt finished for file S1")  # all samples inferred before any is parsed
    assert "adapter auto" not in (tmp_path / "explicit" / "run.log").read_text()
    with open(tmp_path / "auto" / "miR.Counts.csv") as fh:
        assert sum(float(x) for line in fh.read().splitlines()[1:] for x in line.split(",")[1:]) > 1500  # (the reads were trimmed: they map)


def test_two_samples_with_different_adapters_and_one_without(tmp_path):
    """each sample is trimmed with its own sequence: its column of miR.Counts.csv is that of its one-sample run with its own explicit
    adapter; a third sample without an adapter stops the run, named, before any count table exists"""
    case = GoldenCase("case2_two_samples")
    adapters = {"S1": ad_cases.ILLUMINA, "S2": ad_cases.NEB}
    files, seqs = {}, {}
    for s, a in adapters.items():
        reads = _with_adapter(_inserts(s), a)
        seqs[s] = ad_restate.infer(*_dictionary(reads))["seq"]
        assert seqs[s].startswith(a[:15])
        files[s] = tmp_path / f"{s}.fastq"
        files[s].write_bytes(_fastq(reads))
    files["S3"] = tmp_path / "S3.fastq"
    files["S3"].write_bytes(_fastq(_inserts("S1")[:600]))
    none = ad_restate.infer(*_dictionary(_inserts("S1")[:600]))
    assert none["seq"] == "" and none["eligible"] == 600
    common = ["-lib", case.libdir, "-on", ORG, "-db", "miRBase", "-o", str(tmp_path), "-shh"]
    r = _cli(common + ["-s", f"{files['S1']},{files['S2']}", "-dn", "both", "-a", "auto"])
    assert r.returncode == 0, r.stderr[-3000:]

    def columns(path):
        with open(path) as fh:
            rows = [line.split(",") for line in fh.read().splitlines()]
        return {name: {row[0]: row[1 + k] for row in rows[1:]} for k, name in enumerate(rows[0][1:])}

    both = columns(tmp_path / "both" / "miR.Counts.csv")
    for s in ("S1", "S2"):
        r = _cli(common + ["-s", str(files[s]), "-dn", "only" + s, "-a", seqs[s]])
        assert r.returncode == 0, r.stderr[-3000:]
        alone = columns(tmp_path / ("only" + s) / "miR.Counts.csv")[s]
        assert both[s] == alone and sum(float(v) for v in alone.values()) > 700, s
    r = _cli(common + ["-s", f"{files['S1']},{files['S3']},{files['S2']}", "-dn", "third", "-a", "auto"])
    assert r.returncode != 0 and "S3" in r.stderr and "T = 600" in r.stderr and "no adapter" in r.stderr
    assert _files(tmp_path / "third") == ["adapter.auto.csv", "run.log"]
    lines = (tmp_path / "third" / "adapter.auto.csv").read_text().splitlines()
    assert lines[1].startswith(f"S1,{seqs['S1']},") and lines[2].startswith("S3,,0,0,600,600,") and lines[3].startswith(f"S2,{seqs['S2']},")
    assert "no adapter in sample S3" in (tmp_path / "third" / "run.log").read_text()
