"""``--trimmed-out`` on the MI355X: ``mirge_fqout_*`` / ``mirge_reads_parse_trim_out`` (csrc/native_fq.hpp, csrc/kernels_fq.hpp) through the C ABI
on the cases of tests/fq_cases.py and on random small texts -- here the bounds are k_trim's own --, exact bytes against the restatement
(tests/fq_restate.py): the plain file, the BGZF file with blocks of 64 and 65280 bytes on both routes, a sample fed in one piece and in three,
small tiles and chunks, the reads the call returns, the numbers of ``finish``, the error case, a writer that is dropped, two writers side by
side; then the command line on a committed sample, with and without the flag, and the round trip through the written file."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import fq_cases
import fq_restate
import qc_restate
from helpers import GoldenCase, ORG
import mirge3_amd  # noqa: F401
from mirge3_amd import _ffi, bgzf, trimmed_out

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("MIRGE_FQ_TILE_BYTES", "MIRGE_FQ_CHUNK_BYTES", "MIRGE_BGZF_DEFLATE", "MIRGE_BGZF_BLOCK_BYTES"):
        monkeypatch.delenv(k, raising=False)


def pieces_of(case, n: int):
    """the case's text cut into ``n`` pieces at record boundaries (one piece when it has fewer records)"""
    period = {1: 4, 2: 2, 3: 1}[case["fmt"]]
    lines = case["text"].split(b"\n")
    n_rec = len(qc_restate.records(case["text"], case["fmt"]))
    if n <= 1 or n_rec < n:
        return [case["text"]]
    cuts = [n_rec * k // n * period for k in range(n)] + [len(lines)]
    if case["fmt"] == 3:  # (empty lines at the end of a text are no records of format 3: a piece ends with a letter)
        for k in range(1, n):
            while cuts[k] > 0 and not lines[cuts[k] - 1]:
                cuts[k] -= 1
        cuts = sorted(set(cuts))
    return [b"\n".join(lines[a:b]) + (b"\n" if b < len(lines) else b"") for a, b in zip(cuts, cuts[1:])]


def trim_of(case):
    kw = fq_cases.trim_kwargs(case)
    return None if kw is None else _ffi.MirgeTrim.make(**kw)


def small(monkeypatch, tile=256, chunk=4096):
    monkeypatch.setenv("MIRGE_FQ_TILE_BYTES", str(tile))
    monkeypatch.setenv("MIRGE_FQ_CHUNK_BYTES", str(chunk))


def write(ctx, case, directory, mode="plain", pieces=1, block=0, sample="S"):
    """the case's text through a writer in ``directory`` -> (the bytes of the file, of its .gzi or None, finish's numbers, the reads)"""
    os.makedirs(directory, exist_ok=True)
    w = _ffi.TrimmedOut(ctx, directory, sample, mode, block)
    reads = []
    try:
        for t in pieces_of(case, pieces):
            r, _ = _ffi.DeviceReads.parse_out(ctx, t, case["fmt"], case["min_len"], trim_of(case), None, w)
            reads += r.unpack().to_list()
            r.close()
        st = w.finish()
    finally:
        w.close()
    assert sorted(os.listdir(directory)) == sorted([os.path.basename(st["path"])] + ([os.path.basename(st["path"]) + ".gzi"] if mode == "gz" else []))
    data = open(st["path"], "rb").read()
    gzi = open(st["path"] + ".gzi", "rb").read() if mode == "gz" else None
    return data, gzi, st, reads


def check_stats(st, case, want, mode="plain"):
    rs = fq_restate.stats(case["text"], case["fmt"], case["min_len"], case["opts"])
    assert {k: st[k] for k in rs} == rs and st["stream_bytes"] == len(want)
    if mode == "plain":
        assert [st[k] for k in ("file_bytes", "members", "stored", "fixed", "dynamic")] == [len(want), 0, 0, 0, 0]


@pytest.mark.parametrize("name", sorted(fq_cases.all_cases()))
def test_the_plain_file_is_the_restatement(ctx, name, tmp_path, monkeypatch):
    case, want = fq_cases.all_cases()[name], fq_cases.expected(name)
    data, _, st, _ = write(ctx, case, tmp_path / "a")
    assert data == want
    check_stats(st, case, want)
    assert os.path.basename(st["path"]) == trimmed_out.file_name("S", case["fmt"])
    small(monkeypatch)
    assert write(ctx, case, tmp_path / "b", pieces=3)[0] == want  # three pieces, tiles of 256 bytes, chunks of 4096
    small(monkeypatch, tile=64)
    assert write(ctx, case, tmp_path / "c")[0] == want


@pytest.mark.parametrize("block", [64, 65280])
@pytest.mark.parametrize("name", sorted(fq_cases.all_cases()))
def test_the_bgzf_file_inflates_to_the_restatement(ctx, name, block, tmp_path, monkeypatch):
    case, want = fq_cases.all_cases()[name], fq_cases.expected(name)
    gz, gzi, st, _ = write(ctx, case, tmp_path / "a", "gz", block=block)
    ms = bgzf.check_index(gz, gzi)
    assert gzip.decompress(gz) == want
    assert [m["payload"] for m in ms] == [want[at:at + block] for at in range(0, len(want), block)]
    assert all(m["single"] for m in ms)
    check_stats(st, case, want, "gz")
    assert (st["file_bytes"], st["members"]) == (len(gz), len(ms)) and st["stored"] + st["fixed"] + st["dynamic"] == len(ms)
    if not want:
        assert gz == bgzf.EOF_BLOCK and gzi == bytes(8)
    # the file is a function of S and B alone: the bytes mirge_bgzf_write makes of S
    bgzf.write_device(ctx, want, tmp_path / "ref.gz", block)
    assert gz == (tmp_path / "ref.gz").read_bytes() and gzi == (tmp_path / "ref.gz.gzi").read_bytes()
    # ... not of pieces, chunks or tiles
    small(monkeypatch)
    gz3, gzi3, st3, _ = write(ctx, case, tmp_path / "b", "gz", pieces=3, block=block)
    assert (gz3, gzi3) == (gz, gzi) and {**st3, "path": None} == {**st, "path": None}
    # the host route: the same stream under the same uncompressed offsets
    monkeypatch.setenv("MIRGE_BGZF_DEFLATE", "host")
    gzh, gzih, sth, _ = write(ctx, case, tmp_path / "c", "gz", pieces=3, block=block)
    assert [m["payload"] for m in bgzf.check_index(gzh, gzih)] == [m["payload"] for m in ms]
    assert [u for _, u in bgzf.read_gzi(gzih)] == [u for _, u in bgzf.read_gzi(gzi)] and sth["stream_bytes"] == st["stream_bytes"]


def test_random_texts(ctx, tmp_path, monkeypatch):
    for seed in range(120):
        case = fq_cases.random_text(seed)
        want = fq_cases.restated(case)
        if seed % 2:
            small(monkeypatch, tile=(64, 256)[seed % 4 // 2])
        data, _, st, _ = write(ctx, case, tmp_path / f"p{seed}", pieces=1 + seed % 3)
        assert data == want, seed
        check_stats(st, case, want)
        gz, gzi, _, _ = write(ctx, case, tmp_path / f"g{seed}", "gz", pieces=1 + (seed + 1) % 3, block=(64, 65280)[seed % 2])
        assert gzip.decompress(gz) == want and b"".join(m["payload"] for m in bgzf.check_index(gz, gzi)) == want, seed
        monkeypatch.delenv("MIRGE_FQ_TILE_BYTES", raising=False)
        monkeypatch.delenv("MIRGE_FQ_CHUNK_BYTES", raising=False)


@pytest.mark.parametrize("name", ["a_thousand_records", "chain_counted_per_modifier", "fasta", "crlf", "tiny_records_and_empty_reads"])
def test_the_reads_are_those_of_parse_trim(ctx, name, tmp_path):
    case = fq_cases.all_cases()[name]
    _, _, _, got = write(ctx, case, tmp_path / "a")
    r0, n0 = _ffi.DeviceReads.parse(ctx, case["text"], case["fmt"], case["min_len"], trim_of(case))
    r2, n2 = _ffi.DeviceReads.parse_out(ctx, case["text"], case["fmt"], case["min_len"], trim_of(case), None, None)  # no writer: parse_qc
    try:
        assert n0 == n2 and len(r0) > 0 and got == r0.unpack().to_list() == r2.unpack().to_list()
        assert r0.group_counts().tolist() == r2.group_counts().tolist()
    finally:
        r0.close(); r2.close()


def test_a_quality_line_of_the_wrong_length_fails_and_leaves_nothing(ctx, tmp_path):
    case = fq_cases.error_case()
    good = fq_cases.all_cases()["one_record"]
    for mode in ("plain", "gz"):
        d = tmp_path / mode
        os.makedirs(d)
        w = _ffi.TrimmedOut(ctx, d, "S", mode)
        r, _ = _ffi.DeviceReads.parse_out(ctx, good["text"], 1, good["min_len"], None, None, w)  # a good piece first: something is in the file
        r.close()
        assert len(os.listdir(d)) == (2 if mode == "gz" else 1) and all(f.endswith(".tmp") for f in os.listdir(d))
        with pytest.raises(RuntimeError, match="--trimmed-out: mirge_reads_parse: a record's quality line is not as long as its sequence line"):
            _ffi.DeviceReads.parse_out(ctx, case["text"], 1, case["min_len"], trim_of(case), None, w)
        assert os.listdir(d) == []  # no file, nor a .tmp
        with pytest.raises(RuntimeError, match="failed"):
            w.finish()
        w.close()
        assert os.listdir(d) == []


def test_a_piece_whose_reads_cannot_be_packed_writes_nothing(ctx, tmp_path):
    w = _ffi.TrimmedOut(ctx, tmp_path, "S", "plain")
    with pytest.raises(RuntimeError, match="no nucleotide code"):
        _ffi.DeviceReads.parse_out(ctx, b"@a\nACGTACGTACGTACGT!ACGT\n+\nIIIIIIIIIIIIIIIIIIIII\n", 1, 16, None, None, w)
    assert os.listdir(tmp_path) == []
    w.close()


def test_a_writer_dropped_without_finish_leaves_nothing(ctx, tmp_path):
    case = fq_cases.all_cases()["a_thousand_records"]
    for mode in ("plain", "gz"):
        w = _ffi.TrimmedOut(ctx, tmp_path, "S", mode, 64)
        r, _ = _ffi.DeviceReads.parse_out(ctx, case["text"], 1, case["min_len"], trim_of(case), None, w)
        r.close()
        assert os.listdir(tmp_path) != []
        w.close()
        assert os.listdir(tmp_path) == []
    # reset: the pieces written so far are written again, from offset 0
    w = _ffi.TrimmedOut(ctx, tmp_path, "S", "gz", 64)
    for rounds in range(2):
        for t in pieces_of(case, 2 if rounds == 0 else 3)[:None if rounds else 1]:
            _ffi.DeviceReads.parse_out(ctx, t, 1, case["min_len"], trim_of(case), None, w)[0].close()
        if rounds == 0:
            w.reset()
    st = w.finish()
    assert gzip.decompress(open(st["path"], "rb").read()) == fq_cases.expected("a_thousand_records")


def test_two_writers_fed_alternately_do_not_mix(ctx, tmp_path):
    a, b = fq_cases.all_cases()["a_thousand_records"], fq_cases.all_cases()["fasta"]
    wa, wb = _ffi.TrimmedOut(ctx, tmp_path, "A", "gz", 64), _ffi.TrimmedOut(ctx, tmp_path, "B", "plain")
    try:
        pa = pieces_of(a, 4)
        feed = lambda w, case, t: _ffi.DeviceReads.parse_out(ctx, t, case["fmt"], case["min_len"], trim_of(case), None, w)[0].close()
        feed(wa, a, pa[0])
        feed(wb, b, b["text"])
        for t in pa[1:]:
            feed(wa, a, t)
        sa, sb = wa.finish(), wb.finish()
    finally:
        wa.close(); wb.close()
    assert gzip.decompress(open(sa["path"], "rb").read()) == fq_cases.expected("a_thousand_records")
    assert open(sb["path"], "rb").read() == fq_cases.expected("fasta") and sb["path"].endswith("B.trimmed.fasta")
    assert sorted(os.listdir(tmp_path)) == ["A.trimmed.fastq.gz", "A.trimmed.fastq.gz.gzi", "B.trimmed.fasta"]


def test_bad_sizes_are_refused(ctx, tmp_path, monkeypatch):
    monkeypatch.setenv("MIRGE_BGZF_BLOCK_BYTES", "63")
    with pytest.raises(RuntimeError, match="MIRGE_BGZF_BLOCK_BYTES"):
        _ffi.TrimmedOut(ctx, tmp_path, "S", "gz").handle_for(1)
    monkeypatch.delenv("MIRGE_BGZF_BLOCK_BYTES")
    monkeypatch.setenv("MIRGE_BGZF_DEFLATE", "fastest")
    with pytest.raises(RuntimeError, match="MIRGE_BGZF_DEFLATE"):
        _ffi.TrimmedOut(ctx, tmp_path, "S", "gz").handle_for(1)
    monkeypatch.delenv("MIRGE_BGZF_DEFLATE")
    monkeypatch.setenv("MIRGE_FQ_TILE_BYTES", "100")
    case = fq_cases.all_cases()["one_record"]
    w = _ffi.TrimmedOut(ctx, tmp_path, "S", "plain")
    with pytest.raises(RuntimeError, match="MIRGE_FQ_TILE_BYTES"):
        _ffi.DeviceReads.parse_out(ctx, case["text"], 1, 16, None, None, w)
    w.close()
    assert os.listdir(tmp_path) == []


# ---- the command line ----------------------------------------------------------------------------------------------------------
OFF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmer_correct_off")
ADAPTER = "TGGAATTCTCGGGTGCCAAGG"
ROUND_TRIP = ("miR.Counts.csv", "miR.RPM.csv", "mapped.csv", "unmapped.csv", "S1.trim.collapse.fa", "S2.trim.collapse.fa")


def _cli(argv):
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    cmd = [sys.executable, "-c", "import sys; sys.path.insert(0, %r); import mirge3_amd; from mirge3_amd.cli import main; main()" % root]
    return subprocess.run(cmd + list(argv), capture_output=True, text=True, timeout=600)


def _files(out):
    return sorted(f for f in os.listdir(out) if os.path.isfile(os.path.join(out, f)))


def test_command_line_with_and_without_the_flag_and_the_round_trip(tmp_path):
    """the sample construction of test_read_qc_gpu.py: the two committed samples of tests/golden/kmer_correct_off, each read followed by an adapter
    and trimmed by -a / -q / --trim-n"""
    case = GoldenCase("case2_two_samples")
    files = []
    for s in ("S1", "S2"):
        lines = open(os.path.join(OFF, f"{s}.fastq")).read().split("\n")
        recs = [(r + ADAPTER)[:50] for r in lines[1::4] if r]
        recs[3] = "NN" + recs[3][2:]
        text = "".join(f"@r{i}\n{r}\n+\n{'I' * (len(r) - 3)}5#!\n" for i, r in enumerate(recs))
        p = tmp_path / f"{s}.fastq"
        p.write_text(text)
        files.append(str(p))
    opts = dict(q_back=10, adapter=ADAPTER, trim_n=True)
    want = {s: fq_restate.stream(open(f, "rb").read(), 1, 16, opts) for s, f in zip(("S1", "S2"), files)}
    # the chain is not idempotent in general (a quality trim of an adapter-cut prefix can cut again): on this sample it is
    again = dict(q_back=10, trim_n=True)
    for s in want:
        assert fq_restate.stream(want[s], 1, 16, again) == want[s]
        buf, recs = qc_restate.views(want[s], 1, 16, again)
        assert all(r["trimmed"] == r["line"] for r in recs) and len(recs) > 100

    def common(sources, name):
        return ["-s", ",".join(sources), "-lib", case.libdir, "-on", ORG, "-db", "miRBase", "-o", str(tmp_path), "-shh", "-tcf", "-q", "10", "--trim-n",
                "--trim-count", "once", "-dn", name]

    for name, extra in (("plain", ["--trimmed-out"]), ("gz", ["--trimmed-out", "gz"]), ("without", [])):
        r = _cli(common(files, name) + ["-a", ADAPTER] + extra)
        assert r.returncode == 0, r.stderr[-3000:]
    names = _files(tmp_path / "without")
    assert _files(tmp_path / "plain") == sorted(names + ["S1.trimmed.fastq", "S2.trimmed.fastq"])
    assert _files(tmp_path / "gz") == sorted(names + [f"{s}.trimmed.fastq.gz{x}" for s in ("S1", "S2") for x in ("", ".gzi")])
    for name in names:
        if name != "run.log":
            for d in ("plain", "gz"):
                assert (tmp_path / d / name).read_bytes() == (tmp_path / "without" / name).read_bytes(), (d, name)
    assert "trimmed out" not in (tmp_path / "without" / "run.log").read_text()
    header, *rows = [line.split(",") for line in (tmp_path / "plain" / "annotation.report.csv").read_text().splitlines()]
    report = {row[0]: dict(zip(header[1:], row[1:])) for row in rows}
    log = {d: (tmp_path / d / "run.log").read_text() for d in ("plain", "gz")}
    for s, f in zip(("S1", "S2"), files):
        plain = (tmp_path / "plain" / f"{s}.trimmed.fastq").read_bytes()
        assert plain == want[s]
        gz, gzi = (tmp_path / "gz" / f"{s}.trimmed.fastq.gz").read_bytes(), (tmp_path / "gz" / f"{s}.trimmed.fastq.gz.gzi").read_bytes()
        ms = bgzf.check_index(gz, gzi)
        assert gzip.decompress(gz) == plain
        st = fq_restate.stats(open(f, "rb").read(), 1, 16, opts)
        assert st["written"] == int(report[s]["Trimmed Reads (all)"]) and st["records"] == int(report[s]["Total Input Reads"])
        forms = [sum(1 for m in ms if m["btype"] == b) for b in range(3)]
        full = dict(st, file_bytes=len(gz), members=len(ms), stored=forms[0], fixed=forms[1], dynamic=forms[2])
        assert trimmed_out.log_line(s, full) + "\n" in log["plain"] and trimmed_out.log_line(s, full, "gz") + "\n" in log["gz"]
    # the round trip: the written files, under the samples' names, through the same chain without -a
    os.makedirs(tmp_path / "rt")
    for s in ("S1", "S2"):
        (tmp_path / "rt" / f"{s}.fastq").write_bytes((tmp_path / "plain" / f"{s}.trimmed.fastq").read_bytes())
    r = _cli(common([str(tmp_path / "rt" / f"{s}.fastq") for s in ("S1", "S2")], "again"))
    assert r.returncode == 0, r.stderr[-3000:]
    for name in ROUND_TRIP:
        assert (tmp_path / "again" / name).read_bytes() == (tmp_path / "plain" / name).read_bytes(), name
