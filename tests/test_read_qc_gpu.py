"""``--read-qc`` on the MI355X: ``mirge_reads_parse_trim_qc`` / ``mirge_qc_fetch`` / ``mirge_qc_class_profile`` (csrc/native_qc.hpp,
csrc/kernels_qc.hpp) through the C ABI on the cases of tests/qc_cases.py and on random small texts, exactly, in either form of the text
histogram (MIRGE_QC_FORM) -- here the trimmed bounds are k_trim's own --, a sample fed in pieces, two samples side by side, the reads the
call returns, the class profile against NumPy, then the command line on a committed sample with and without the flag."""
import os
import subprocess
import sys

import numpy as np
import pytest

import qc_cases
import qc_restate
from helpers import GoldenCase, ORG
import mirge3_amd  # noqa: F401
from mirge3_amd import _ffi, readqc
from mirge3_amd.seqio import FlatSeqs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(params=["pos", "read"])
def form(request, monkeypatch):
    """the form of the text histogram (MIRGE_QC_FORM, read per call): a lane per position, or a lane per read"""
    monkeypatch.setenv("MIRGE_QC_FORM", request.param)
    return request.param


def pieces_of(case, n: int):
    """the case's text cut into ``n`` pieces at record boundaries (one piece when it has fewer records)"""
    period = {1: 4, 2: 2, 3: 1}[case["fmt"]]
    lines = case["text"].split(b"\n")
    n_rec = len(qc_restate.records(case["text"], case["fmt"]))
    if n <= 1 or n_rec < n:
        return [case["text"]]
    cuts = [n_rec * k // n * period for k in range(n)] + [len(lines)]
    return [b"\n".join(lines[a:b]) + (b"\n" if b < len(lines) else b"") for a, b in zip(cuts, cuts[1:])]


def trim_of(case):
    kw = qc_cases.trim_kwargs(case)
    return None if kw is None else _ffi.MirgeTrim.make(**kw)


def feed(ctx, qc, case, text):
    r, n = _ffi.DeviceReads.parse_qc(ctx, text, case["fmt"], case["min_len"], trim_of(case), qc)
    r.close()
    return n


def run(ctx, case, pieces=1):
    qc = _ffi.ReadQc(ctx)
    try:
        n = sum(feed(ctx, qc, case, t) for t in pieces_of(case, pieces))
        tables, has_q = qc.fetch()
    finally:
        qc.close()
    assert has_q == (case["fmt"] == 1 and n > 0)
    return readqc.sample_entries(tables, case["fmt"] == 1)


@pytest.mark.parametrize("name", sorted(qc_cases.all_cases()))
def test_cases_equal_the_restatement(ctx, name, form):
    case = qc_cases.all_cases()[name]
    want = qc_cases.expected(name)
    assert run(ctx, case) == want
    assert run(ctx, case, pieces=3) == want  # a sample streamed in three pieces: the same tables


def test_random_texts_equal_the_restatement(ctx, form):
    for seed in range(120):
        case = qc_cases.random_text(seed)
        assert run(ctx, case, pieces=1 + seed % 3) == qc_cases.restated(case), seed


def test_two_samples_do_not_leak_into_each_other(ctx, form):
    a, b = qc_cases.all_cases()["a_thousand_records"], qc_cases.all_cases()["chain_counted_per_modifier"]
    qa, qb = _ffi.ReadQc(ctx), _ffi.ReadQc(ctx)
    try:
        pa = pieces_of(a, 4)
        feed(ctx, qa, a, pa[0])
        feed(ctx, qb, b, b["text"])
        for t in pa[1:]:
            feed(ctx, qa, a, t)
        assert readqc.sample_entries(*qa.fetch()) == qc_cases.expected("a_thousand_records")
        assert readqc.sample_entries(*qb.fetch()) == qc_cases.expected("chain_counted_per_modifier")
        qa.reset()
        assert readqc.sample_entries(qa.fetch()[0], True)[("reads", "raw", None, None, None)] == 0
    finally:
        qa.close(); qb.close()


@pytest.mark.parametrize("name", ["a_thousand_records", "chain_counted_per_modifier", "fasta", "quality_line_of_the_wrong_length", "crlf"])
def test_the_reads_are_those_of_parse_trim(ctx, name, form):
    case = qc_cases.all_cases()[name]
    qc = _ffi.ReadQc(ctx)
    r1, n1 = _ffi.DeviceReads.parse_qc(ctx, case["text"], case["fmt"], case["min_len"], trim_of(case), qc)
    r0, n0 = _ffi.DeviceReads.parse(ctx, case["text"], case["fmt"], case["min_len"], trim_of(case))
    r2, n2 = _ffi.DeviceReads.parse_qc(ctx, case["text"], case["fmt"], case["min_len"], trim_of(case), None)
    try:
        assert n1 == n0 == n2 and len(r1) == len(r0) == len(r2) and len(r0) > 0
        assert r1.unpack().to_list() == r0.unpack().to_list() == r2.unpack().to_list()
        assert r1.group_counts().tolist() == r0.group_counts().tolist()
    finally:
        r0.close(); r1.close(); r2.close(); qc.close()


def test_a_bad_form_and_a_foreign_handle_are_refused(ctx, monkeypatch):
    case = qc_cases.all_cases()["one_record"]
    qc = _ffi.ReadQc(ctx)
    try:
        monkeypatch.setenv("MIRGE_QC_FORM", "fastest")
        with pytest.raises(RuntimeError, match="MIRGE_QC_FORM"):
            _ffi.DeviceReads.parse_qc(ctx, case["text"], 1, 16, None, qc)
        monkeypatch.delenv("MIRGE_QC_FORM")
        assert feed(ctx, qc, case, case["text"]) == 1
    finally:
        qc.close()


@pytest.mark.parametrize("S", [1, 3])
def test_class_profile_equals_numpy(ctx, S):
    """a dictionary with reads of every width class, some with a leading N, some empty-handed in a sample; passes set by hand"""
    rng = np.random.default_rng(5 + S)
    lens = [0, 1, 17, 22, 22, 22, 31, 32, 63, 64, 65, 128, 129, 255, 256, 257, 300, 1000] + [int(x) for x in rng.integers(16, 40, 3000)]
    seqs = set()
    for n in lens:
        s = "".join("ACGT"[i] for i in rng.integers(0, 4, n))
        if n and rng.integers(0, 6) == 0:
            s = "N" + s[1:]
        if n > 3 and rng.integers(0, 6) == 0:
            s = s[:2] + "N" + s[3:]
        seqs.add(s)
    seqs = sorted(seqs)
    raw = _ffi.DeviceReads.pack(ctx, FlatSeqs.from_list(seqs))
    sid = rng.integers(0, S, len(seqs)).astype(np.int32)
    w = rng.integers(1, 5000, len(seqs)).astype(np.uint32)
    uniq = raw.collapse(sid, S, weights=w)
    from mirge3_amd.cascade import Cascade
    from mirge3_amd import synth
    casc = Cascade(ctx, synth.make_libraries(seed=5, scale="ci").libs)
    res = casc.run(uniq)
    try:
        got = _ffi.qc_class_profile(ctx, uniq, res)
        ps = res.fetch()[0].astype(np.int64)
        useq = uniq.unpack().to_list()
        counts = uniq.counts()[0]
        first = np.array([4 if not s or s[0] == "N" else "ACGT".index(s[0]) for s in useq])
        want = qc_restate.class_profile(ps, np.array([len(s) for s in useq]), first, counts, res.n_pass)
        assert got.shape == want.shape == (S, res.n_pass + 1, 257, 5, 2) and np.array_equal(got, want)
        assert got[..., 0].sum() == int(w.sum()) and got[:, :, 256].sum() > 0 and got[:, :, :, 4].sum() > 0
    finally:
        res.close(); uniq.close(); raw.close()


# ---- the command line ----------------------------------------------------------------------------------------------------------
OFF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmer_correct_off")
REPORT_CLASSES = {"Hairpin miRNAs": ["hairpin miRNA"], "mature tRNA Reads": ["mature tRNA"], "primary tRNA Reads": ["primary tRNA"], "snoRNA Reads": ["snoRNA"],
                  "rRNA Reads": ["rRNA"], "ncRNA others": ["ncrna others"], "mRNA Reads": ["mRNA"], "All miRNA Reads": ["exact miRNA", "isomiR miRNA"],
                  "Remaining Reads": ["unmapped"]}


def _cli(argv):
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    cmd = [sys.executable, "-c", "import sys; sys.path.insert(0, %r); import mirge3_amd; from mirge3_amd.cli import main; main()" % root]
    return subprocess.run(cmd + list(argv), capture_output=True, text=True, timeout=600)


def _files(out):
    return sorted(f for f in os.listdir(out) if os.path.isfile(os.path.join(out, f)))


def _tsv(path):
    rows = [line.split("\t") for line in open(path).read().splitlines()]
    assert rows[0] == ["#mirge3amd-readqc", "1"]
    return {tuple(r[:5]): int(r[5]) for r in rows[1:]}


@pytest.mark.parametrize("count", ["once", "per-modifier"])
def test_command_line_with_and_without_the_flag(tmp_path, count):
    """the two committed samples of tests/golden/kmer_correct_off, each read followed by an adapter and trimmed by -a / -q / --trim-n: every
    other output file is byte-identical, and the new ones agree with annotation.report.csv and with the restatement"""
    case = GoldenCase("case2_two_samples")
    adapter = "TGGAATTCTCGGGTGCCAAGG"
    files = []
    for s in ("S1", "S2"):
        lines = open(os.path.join(OFF, f"{s}.fastq")).read().split("\n")
        recs = [(r + adapter)[:50] for r in lines[1::4] if r]
        recs[3] = "NN" + recs[3][2:]
        text = "".join(f"@r{i}\n{r}\n+\n{'I' * (len(r) - 3)}5#!\n" for i, r in enumerate(recs))
        p = tmp_path / f"{s}.fastq"
        p.write_text(text)
        files.append(str(p))
    common = ["-s", ",".join(files), "-lib", case.libdir, "-on", ORG, "-db", "miRBase", "-o", str(tmp_path), "-shh", "-tcf", "-a", adapter, "-q", "10",
              "--trim-n", "--trim-count", count]
    for name, extra in (("with", ["--read-qc"]), ("without", [])):
        r = _cli(common + ["-dn", name] + extra)
        assert r.returncode == 0, r.stderr[-3000:]
    names = _files(tmp_path / "without")
    assert _files(tmp_path / "with") == sorted(names + ["S1.readqc.tsv", "S2.readqc.tsv", "readqc.summary.csv"])
    for name in names:
        if name != "run.log":
            assert (tmp_path / "with" / name).read_bytes() == (tmp_path / "without" / name).read_bytes(), name
    log = (tmp_path / "with" / "run.log").read_text()
    assert "read qc" not in (tmp_path / "without" / "run.log").read_text()
    header, *rows = [line.split(",") for line in (tmp_path / "with" / "annotation.report.csv").read_text().splitlines()]
    report = {row[0]: dict(zip(header[1:], row[1:])) for row in rows}
    opts = dict(q_back=10, adapter=adapter, trim_n=True)
    for s, f in zip(("S1", "S2"), files):
        got = _tsv(tmp_path / "with" / f"{s}.readqc.tsv")
        want = qc_restate.entries(open(f, "rb").read(), 1, 16, opts)
        show = lambda x: "." if x is None else str(x)
        assert {k: v for k, v in got.items() if k[1] != "annotated"} == {tuple(show(x) for x in k): v for k, v in want.items()}
        assert (tmp_path / "with" / f"{s}.readqc.tsv").read_text() == readqc.file_text(
            {**want, **{(k[0], k[1], k[2], int(k[3]), k[4]): v for k, v in got.items() if k[1] == "annotated"}}, readqc.class_names(9))
        assert got[("reads", "raw", ".", ".", ".")] == int(report[s]["Total Input Reads"])
        if count == "once":
            assert got[("reads", "trimmed", ".", ".", ".")] == int(report[s]["Trimmed Reads (all)"])
        by_class = {}
        for k, v in got.items():
            if k[0] == "class_length":
                by_class[k[2]] = by_class.get(k[2], 0) + v
        for column, classes in REPORT_CLASSES.items():
            assert sum(by_class.get(c, 0) for c in classes) == int(float(report[s][column])), (s, column)
        assert sum(by_class.values()) == int(report[s]["Trimmed Reads (all)"])
        assert sum(v for k, v in got.items() if k[0] == "class_length_unique") == int(report[s]["Trimmed Reads (unique)"])
        assert readqc.log_line(s, want) + "\n" in log
    e = [qc_restate.entries(open(f, "rb").read(), 1, 16, opts) for f in files]
    assert (tmp_path / "with" / "readqc.summary.csv").read_text() == readqc.summary_text(["S1", "S2"], e)
