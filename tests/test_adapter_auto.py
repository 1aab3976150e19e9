"""``-a auto`` without a GPU: the restatement (tests/ad_restate.py) on the named cases and on ten synthetic samples, ``head_text`` on the
forms a FASTQ file comes in, the command line's refusals, and the writer of ``adapter.auto.csv``."""
import gzip
import os

import pytest

import ad_cases
import ad_restate
import mirge3_amd  # noqa: F401
from mirge3_amd import adapter_auto, cli


@pytest.mark.parametrize("name", sorted(ad_cases.all_cases()))
def test_a_case_holds_what_it_is_for(name):
    ad_cases.holds(name)


@pytest.mark.parametrize("name", sorted(ad_cases.SYNTHETIC))
def test_the_restatement_finds_the_planted_adapter(name):
    """20 000 reads over 300 Zipf templates of 19 .. 34 nt with isomiR variation and substitutions: a prefix of at least 12 letters, from
    letter 0, of the planted sequence and what follows it; "no adapter" where none was planted"""
    kw, planted = ad_cases.SYNTHETIC[name]
    reads, counts = ad_cases.synthetic_sample(7, **kw)
    res = ad_restate.infer(reads, counts)
    assert res["eligible"] == 20000
    if planted is None:
        assert res["seq"] == "" and res["len"] == 0
    else:
        assert res["len"] >= 12 and planted.startswith(res["seq"]), res["seq"]
        assert 12 <= res["len"] <= 32 and res["support"] >= res["eligible"] // 20


def _fastq(n, eol="\n"):
    return "".join(f"@r{i}{eol}ACGTACGTACGTAC{'ACGT'[i % 4]}{eol}+{eol}IIIIIIIIIIIIIII{eol}" for i in range(n)).encode()


def test_head_text_plain_and_crlf(tmp_path):
    for eol in ("\n", "\r\n"):
        text = _fastq(1000, eol)
        p = tmp_path / "s.fastq"
        p.write_bytes(text)
        one = _fastq(1, eol)
        assert adapter_auto.head_text(p, 1) == one
        assert adapter_auto.head_text(p, 10, chunk=64) == _fastq(10, eol)  # (many small reads of the file)
        assert adapter_auto.head_text(p, 1000) == text and adapter_auto.head_text(p, 5000) == text
        p.write_bytes(text[:-1])  # no newline behind the last record
        assert adapter_auto.head_text(p, 5000) == text[:-1] and adapter_auto.head_text(p, 999) == _fastq(999, eol)
    (tmp_path / "empty.fastq").write_bytes(b"")
    assert adapter_auto.head_text(tmp_path / "empty.fastq", 4) == b""


def test_head_text_gz_members_and_truncation(tmp_path):
    text = _fastq(3000)
    one = tmp_path / "one.fastq.gz"
    one.write_bytes(gzip.compress(text))
    cut = text.index(b"@r1700\n")
    many = tmp_path / "many.fq.gz"  # three members, the first of them empty, the cuts inside a record
    many.write_bytes(gzip.compress(b"") + gzip.compress(text[:777]) + gzip.compress(text[777:cut + 9]) + gzip.compress(text[cut + 9:]))
    blocks = tmp_path / "blocks.fastq.gz"  # many small members with an extra field, as BGZF has them
    blocks.write_bytes(b"".join(gzip.compress(text[o:o + 500]) for o in range(0, len(text), 500)) + gzip.compress(b""))
    for p in (one, many, blocks):
        for chunk in (1 << 20, 301):
            assert adapter_auto.head_text(p, 1, chunk) == _fastq(1)
            assert adapter_auto.head_text(p, 1701, chunk) == _fastq(1701)
            assert adapter_auto.head_text(p, 3000, chunk) == text and adapter_auto.head_text(p, 1 << 18, chunk) == text
    whole = one.read_bytes()
    trunc = tmp_path / "trunc.fastq.gz"
    trunc.write_bytes(whole[:len(whole) // 2])  # ends inside its member
    got = adapter_auto.head_text(trunc, 3000)
    assert 0 < len(got) < len(text) and text.startswith(got)
    assert adapter_auto.head_text(trunc, 5) == _fastq(5)
    trunc.write_bytes(whole + b"not a gzip member")  # rubbish behind the last member
    assert adapter_auto.head_text(trunc, 5000) == text


BASE = ["-s", "a.fastq", "-lib", "libs", "-on", "human"]


def _refused(argv, capsys, monkeypatch=None):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(BASE + argv)
    assert e.value.code == 2
    return capsys.readouterr().err


@pytest.mark.parametrize("argv", [
    ["-g", "auto"], ["-a", "auto", "-a", "ACGTACGTAC"], ["-a", "ACGTACGTAC", "-a", "auto"], ["-a", "auto", "-a", "auto"],
    ["-g", "ACGTACGT", "-a", "auto"], ["-a", "auto$"], ["-a", "^auto"], ["-g", "^auto"], ["-a", "ACGT...auto"], ["-a", "auto...ACGT"],
    ["-g", "auto...ACGT"], ["-a", "auto", "-g", "ACGT", "-g", "TTTT"], ["-a", "auto", "-spl"], ["-a", "auto", "-rr"],
    ["-a", "auto", "--backend", "bowtie"]])
def test_the_command_line_refuses(argv, capsys):
    assert "auto" in _refused(argv, capsys)


def test_a_sharded_run_and_a_bad_head_size_are_refused(capsys, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert "single-process" in _refused(["-a", "auto"], capsys)
    monkeypatch.delenv("WORLD_SIZE")
    for bad in ("0", "x", str(2 ** 24 + 1), "-4"):
        monkeypatch.setenv("MIRGE_ADAPTER_HEAD_READS", bad)
        assert "MIRGE_ADAPTER_HEAD_READS" in _refused(["-a", "auto"], capsys)
        assert cli.parse_args(BASE + ["-a", "ACGTACGT"]).adapter_auto is False  # (read with -a auto only)
    monkeypatch.setenv("MIRGE_ADAPTER_HEAD_READS", str(2 ** 24))
    assert cli.parse_args(BASE + ["-a", "auto"]).adapter_auto and adapter_auto.head_reads() == 2 ** 24
    monkeypatch.delenv("MIRGE_ADAPTER_HEAD_READS")
    assert adapter_auto.head_reads() == 2 ** 18


@pytest.mark.parametrize("argv", [
    ["-a", "auto"], ["-a", "auto", "-g", "GTTCAGAGTTC"], ["-a", "auto", "-g", "illumina"], ["-a", "auto", "-umi", "4,4", "-udd"],
    ["-a", "auto", "-umi", "0,12", "--qiagenumi"], ["-a", "auto", "-n", "2"], ["-a", "auto", "--kmer-correct"]])
def test_the_command_line_accepts(argv):
    args = cli.parse_args(BASE + argv)
    assert args.adapter_auto is True and args.adapters[0] == ("back", "auto")


def test_auto_is_the_lower_case_literal_and_nothing_else_changes():
    from mirge3_amd.collapse import adapters_from_args
    for argv in (["-a", "AUTO"], ["-a", "illumina"], ["-a", "TGGAATTC", "-g", "illumina"], []):
        args = cli.parse_args(BASE + argv)
        assert args.adapter_auto is False
        assert adapters_from_args(args) == adapters_from_args(args, auto="TTTT")
    args = cli.parse_args(BASE + ["-a", "auto", "-g", "illumina"])
    assert adapters_from_args(args, auto="TGGAATTCTCGG") == [("back", "TGGAATTCTCGG"), ("front", "GTTCAGAGTTCTACAGTCCGACGATC")]
    assert adapters_from_args(args) == [("back", "auto"), ("front", "GTTCAGAGTTCTACAGTCCGACGATC")]


def test_the_csv_and_the_log_line():
    r1 = ad_restate.infer(*(ad_cases.all_cases()["planted_50"][k] for k in ("reads", "counts")))
    r0 = ad_restate.infer(*(ad_cases.all_cases()["no_adapter"][k] for k in ("reads", "counts")))
    rows = [dict(ad_restate.fields(r1), records=5000, distinct=200), dict(ad_restate.fields(r0), records=4986, distinct=200)]
    text = adapter_auto.csv_text(["S1", "S2"], rows)
    assert text == ad_restate.csv_text([("S1", r1, 5000, 200), ("S2", r0, 4986, 200)])
    lines = text.split("\n")
    assert lines[0] == "Sample,Adapter,Length,Support,Eligible,Records,Distinct" and lines[3] == ""
    assert lines[1] == f"S1,{r1['seq']},{r1['len']},{r1['support']},{r1['eligible']},5000,200" and lines[2] == f"S2,,0,0,{r0['eligible']},4986,200"
    assert adapter_auto.log_line("S1", rows[0]) == ad_restate.log_line("S1", r1, 5000)
    assert adapter_auto.log_line("S1", rows[0]).startswith(f"adapter auto S1: {r1['seq']} (support {r1['support']} of {r1['eligible']} eligible reads in the first 5000 records)")
