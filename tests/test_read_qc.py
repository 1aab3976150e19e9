"""``--read-qc`` without a GPU: the writers of ``<sample>.readqc.tsv`` and ``readqc.summary.csv`` byte for byte on a hand-written expected
file, the entries read off the device's table layout, the command line's refusals, and the flag's absence from a run without it."""
import os

import numpy as np
import pytest

import qc_cases
import qc_restate
import mirge3_amd  # noqa: F401
from mirge3_amd import _ffi, cli, collapse, readqc

TEXT = b"@a\nACG\n+\nI5!\n@b\nNT\n+\nII\n"  # qualities 40 20 0 / 40 40; with --minimum-length 3 the second read is in no trimmed section
ROWS = [
    ("reads", "raw", ".", ".", ".", 2), ("reads", "trimmed", ".", ".", ".", 1), ("bases", "raw", ".", ".", ".", 5), ("bases", "trimmed", ".", ".", ".", 3),
    ("reads_with_N", "raw", ".", ".", ".", 1), ("reads_with_N", "trimmed", ".", ".", ".", 0), ("empty_reads", "raw", ".", ".", ".", 0),
    ("empty_reads", "trimmed", ".", ".", ".", 0), ("qual_clamped", "raw", ".", ".", ".", 0), ("qual_clamped", "trimmed", ".", ".", ".", 0),
    ("qual_length_mismatch", "raw", ".", ".", ".", 0), ("qual_length_mismatch", "trimmed", ".", ".", ".", 0),
    ("length", "raw", 2, ".", ".", 1), ("length", "raw", 3, ".", ".", 1), ("length", "trimmed", 3, ".", ".", 1),
    ("base", "raw", 0, "A", ".", 1), ("base", "raw", 0, "N", ".", 1), ("base", "raw", 1, "C", ".", 1), ("base", "raw", 1, "T", ".", 1),
    ("base", "raw", 2, "G", ".", 1), ("base", "trimmed", 0, "A", ".", 1), ("base", "trimmed", 1, "C", ".", 1), ("base", "trimmed", 2, "G", ".", 1),
    ("qual", "raw", 0, 40, ".", 2), ("qual", "raw", 1, 20, ".", 1), ("qual", "raw", 1, 40, ".", 1), ("qual", "raw", 2, 0, ".", 1),
    ("qual", "trimmed", 0, 40, ".", 1), ("qual", "trimmed", 1, 20, ".", 1), ("qual", "trimmed", 2, 0, ".", 1),
    ("meanq", "raw", 20, ".", ".", 1), ("meanq", "raw", 40, ".", ".", 1), ("meanq", "trimmed", 20, ".", ".", 1),
    ("gc", "raw", 0, ".", ".", 1), ("gc", "raw", 66, ".", ".", 1), ("gc", "trimmed", 66, ".", ".", 1),
    ("first", "raw", 2, "N", ".", 1), ("first", "raw", 3, "A", ".", 1), ("first", "trimmed", 3, "A", ".", 1),
    ("class_length", "annotated", "exact miRNA", 3, "A", 5), ("class_length", "annotated", "isomiR miRNA", 22, "T", 7),
    ("class_length", "annotated", "isomiR miRNA", 256, "C", 1), ("class_length", "annotated", "unmapped", 2, "N", 1),
    ("class_length_unique", "annotated", "exact miRNA", 3, "A", 2), ("class_length_unique", "annotated", "isomiR miRNA", 22, "T", 3),
    ("class_length_unique", "annotated", "isomiR miRNA", 256, "C", 1), ("class_length_unique", "annotated", "unmapped", 2, "N", 1),
]
EXPECT = "#mirge3amd-readqc\t1\n" + "".join("\t".join(str(x) for x in row) + "\n" for row in ROWS)


def _entries():
    e = qc_restate.entries(TEXT, 1, 3, None)
    profile = np.zeros((10, 257, 5, 2), np.int64)
    profile[0, 3, 0] = (5, 2)
    profile[8, 22, 3] = (7, 3)
    profile[8, 256, 1] = (1, 1)
    profile[9, 2, 4] = (1, 1)
    classes = readqc.class_names(9)
    assert classes[0] == "exact miRNA" and classes[8] == "isomiR miRNA" and classes[9] == "unmapped" and len(classes) == 10
    e.update(readqc.class_entries(profile, classes))
    return e, classes


def test_the_file_byte_for_byte(tmp_path):
    e, classes = _entries()
    assert readqc.file_text(e, classes) == EXPECT
    path = readqc.write_sample(tmp_path, "S1", e, classes)
    assert path.name == "S1.readqc.tsv" and path.read_bytes() == EXPECT.encode() and os.listdir(tmp_path) == ["S1.readqc.tsv"]  # (no .tmp left)
    # the order does not depend on the order of insertion, and a table cell of 0 is no line
    e2 = dict(reversed(list(e.items())))
    e2[("length", "raw", 7, None, None)] = 0
    assert readqc.file_text(e2, classes) == EXPECT
    # numbers sort as numbers, letters A C G T N
    e3 = {("base", "raw", p, l, None): 1 for p in (10, 9, 256, 100) for l in "NTGCA"}
    keys = [tuple(line.split("\t")[2:4]) for line in readqc.file_text(e3).splitlines()[1:]]
    assert keys == [(str(p), l) for p in (9, 10, 100, 256) for l in "ACGTN"]


def test_the_summary_and_the_log_line(tmp_path):
    e, _ = _entries()
    f = qc_restate.entries(b">x\nACGT\n", 2, 0, None)
    text = readqc.summary_text(["S1", "S2"], [e, f])
    assert text == "sample,view,reads,bases,gc_bases,n_bases,q20_bases,q30_bases\nS1,raw,2,5,2,1,4,3\nS1,trimmed,1,3,2,0,2,1\nS2,raw,1,4,2,0,,\nS2,trimmed,1,4,2,0,,\n"
    assert readqc.write_summary(tmp_path, ["S1", "S2"], [e, f]).read_text() == text and os.listdir(tmp_path) == ["readqc.summary.csv"]
    assert readqc.log_line("S1", e) == "read qc S1: raw 2 reads, 5 bases; trimmed 1 reads, 3 bases; modal trimmed length 3"
    assert readqc.modal_trimmed_length({("length", "trimmed", 30, None, None): 4, ("length", "trimmed", 22, None, None): 4, ("length", "raw", 5, None, None): 9}) == 22
    assert readqc.modal_trimmed_length({}) == 0


def test_entries_from_the_device_layout():
    """a table block filled by hand at the documented offsets (include/mirge_native.h) reads back as the restatement's entries"""
    t = np.zeros((2, readqc.VIEW_WORDS), np.int64)
    t[0, 0:6] = (2, 5, 1, 0, 0, 0)
    t[1, 0:6] = (1, 3, 0, 0, 0, 0)
    t[0, 8 + 2] = t[0, 8 + 3] = t[1, 8 + 3] = 1
    base, qual = 8 + 65536, 8 + 65536 + 257 * 5
    meanq = qual + 257 * 94
    gc, first = meanq + 94, meanq + 94 + 101
    for v, cells in ((0, [(0, 0), (0, 4), (1, 1), (1, 3), (2, 2)]), (1, [(0, 0), (1, 1), (2, 2)])):
        for p, l in cells:
            t[v, base + p * 5 + l] = 1
    t[0, qual + 0 * 94 + 40] = 2
    t[0, qual + 1 * 94 + 20] = t[0, qual + 1 * 94 + 40] = t[0, qual + 2 * 94 + 0] = 1
    t[1, qual + 0 * 94 + 40] = t[1, qual + 1 * 94 + 20] = t[1, qual + 2 * 94 + 0] = 1
    t[0, meanq + 20] = t[0, meanq + 40] = t[1, meanq + 20] = 1
    t[0, gc + 0] = t[0, gc + 66] = t[1, gc + 66] = 1
    t[0, first + 2 * 5 + 4] = t[0, first + 3 * 5 + 0] = t[1, first + 3 * 5 + 0] = 1
    assert readqc.sample_entries(t, True) == qc_restate.entries(TEXT, 1, 3, None)
    no_q = readqc.sample_entries(t, False)
    assert not any(k[0] in ("qual", "meanq", "qual_clamped", "qual_length_mismatch") for k in no_q) and ("base", "raw", 0, "A", None) in no_q


@pytest.mark.parametrize("name", sorted(qc_cases.all_cases()))
def test_the_identities_hold_on_every_expected_result(name):
    qc_restate.identities(qc_cases.expected(name))
    text = readqc.file_text(qc_cases.expected(name))
    assert text.startswith(readqc.HEADER) and all(len(line.split("\t")) == 6 and int(line.split("\t")[5]) >= 0 for line in text.splitlines()[1:])


BASE = ["-s", "a.fastq", "-lib", "libs", "-on", "human"]


@pytest.mark.parametrize("argv,word", [(["-umi", "4,4"], "-umi"), (["-umi", "4,4", "-udd"], "-umi"), (["-spl"], "-spl"), (["-rr"], "-rr"),
                                        (["--backend", "bowtie"], "bowtie")])
def test_the_command_line_refuses(argv, word, capsys):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(BASE + ["--read-qc"] + argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--read-qc" in err and word in err
    assert cli.parse_args(BASE + argv).read_qc is False  # (the same line without the flag is accepted)


def test_a_sharded_run_and_a_bad_form_are_refused(capsys, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cli.parse_args(BASE + ["--read-qc"])
    assert "single-process" in capsys.readouterr().err
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.setenv("MIRGE_QC_FORM", "fastest")
    with pytest.raises(SystemExit):
        cli.parse_args(BASE + ["--read-qc"])
    assert "MIRGE_QC_FORM" in capsys.readouterr().err
    assert cli.parse_args(BASE).read_qc is False  # (read with the flag only)
    for ok in ("pos", "read", ""):
        monkeypatch.setenv("MIRGE_QC_FORM", ok)
        assert cli.parse_args(BASE + ["--read-qc"]).read_qc is True


@pytest.mark.parametrize("argv", [[], ["-a", "auto"], ["--kmer-correct"], ["-a", "TGGAATTCTCGG", "-q", "20", "--trim-n", "-u", "2"], ["-tcf"], ["-gff"]])
def test_the_command_line_accepts(argv):
    assert cli.parse_args(BASE + ["--read-qc"] + argv).read_qc is True
    assert readqc.refusal(cli.parse_args(BASE + argv)) == ""


def test_a_run_without_the_flag_makes_the_calls_it_made(monkeypatch):
    """without an accumulator ``parse_sample`` and the streamed route call ``DeviceReads.parse`` exactly as before; with one, ``parse_qc`` with
    the same arguments and the one handle for every piece"""
    calls = []
    monkeypatch.setattr(_ffi.DeviceReads, "parse", staticmethod(lambda ctx, text, fmt=0, min_len=0, trim=None: (calls.append(("parse", bytes(text), fmt, min_len, trim)) or ["r"], 1)))
    monkeypatch.setattr(_ffi.DeviceReads, "parse_qc",
                        staticmethod(lambda ctx, text, fmt, min_len, trim, qc: (calls.append(("parse_qc", bytes(text), fmt, min_len, trim, qc)) or ["r"], 1)))
    monkeypatch.setattr(_ffi.DeviceReads, "concat", staticmethod(lambda ctx, parts: ["joined"]))
    assert cli.parse_args(BASE).read_qc is False
    assert collapse.parse_sample(None, TEXT, 16, "trim", None) == (["r"], 1)
    assert calls == [("parse", TEXT, 0, 16, "trim")]
    del calls[:]
    assert collapse.parse_sample(None, TEXT, 16, "trim", None, qc="handle") == (["r"], 1)
    assert calls == [("parse_qc", TEXT, 0, 16, "trim", "handle")]
    with pytest.raises(RuntimeError, match="-umi"):
        collapse.parse_sample(None, TEXT, 16, "trim", _ffi.MirgeUmi.make(4, 4), qc="handle")

    class Pieces:
        inflate_s, text_bytes, pieces, path = 0.0, 0, 3, "x"

        def __iter__(self):
            return iter([TEXT, TEXT[:13], ("whole", b">x\nACGT\n")])

        def close(self):
            pass

    class Part(list):
        def close(self):
            pass

    monkeypatch.setattr(_ffi.DeviceReads, "parse", staticmethod(lambda ctx, text, fmt=0, min_len=0, trim=None: (calls.append(("parse", bytes(text), fmt)) or Part(), 1)))
    monkeypatch.setattr(_ffi.DeviceReads, "parse_qc", staticmethod(lambda ctx, text, fmt, min_len, trim, qc: (calls.append(("parse_qc", bytes(text), fmt, qc)) or Part(), 1)))
    del calls[:]
    assert collapse._parse_stream_once(None, Pieces(), 16, None)[1] == 3
    assert calls == [("parse", TEXT, 1), ("parse", TEXT[:13], 1), ("parse", b">x\nACGT\n", 0)]
    del calls[:]
    assert collapse._parse_stream_once(None, Pieces(), 16, None, None, "handle")[1] == 3
    assert calls == [("parse_qc", TEXT, 1, "handle"), ("parse_qc", TEXT[:13], 1, "handle"), ("parse_qc", b">x\nACGT\n", 0, "handle")]
