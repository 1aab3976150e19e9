"""CPU tests of ``--trimmed-out``: the restatement (tests/fq_restate.py) against one hand-written input / output pair, the refusals through
``cli.parse_args``, the file names and the run.log line, and the restatement's record count against the ``trimmed`` view of
``qc_restate.entries`` on every case."""
import pytest

import fq_cases
import fq_restate
import qc_restate
import mirge3_amd  # noqa: F401
from mirge3_amd import cli, trimmed_out

ADAPTER = "TGGAATTCTCGGGTGCC"
HAND_IN = (b"@first read\r\nTGAGGTAGTAGGTTGTATAGTTTGGAATTCTCGGGTGCCAAGG\r\n+first read\r\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\r\n"
           b"@\nACGTTGGAATTCTCGGGTGCC\n+\nIIIIIIIIIIIIIIIIIIIII\n"                      # four letters in front of the adapter: too short
           b"@third\nNNacgtuACGTRYACGTTTTN\n+\nIIIIIIIIIIIIIIIIIII##\n"                  # lower case, U and IUPAC codes stay; N ends and a bad tail go
           b"@fourth\nGGGGCCCCAAAATTTTGGGG\n+\n5555555555555555555I\n\n")
HAND_OUT = (b"@first read\nTGAGGTAGTAGGTTGTATAGTT\n+\nIIIIIIIIIIIIIIIIIIIIII\n"
            b"@third\nacgtuACGTRYACGTTT\n+\nIIIIIIIIIIIIIIIII\n"
            b"@fourth\nGGGGCCCCAAAATTTTGGGG\n+\n5555555555555555555I\n")


def test_the_restatement_on_a_hand_written_pair():
    opts = dict(q_back=10, adapter=ADAPTER, trim_n=True)
    assert fq_restate.stream(HAND_IN, 1, 16, opts) == HAND_OUT
    assert fq_restate.stats(HAND_IN, 1, 16, opts) == dict(records=4, written=3, stream_bytes=len(HAND_OUT))
    # -m 0 keeps the second record, cut to its four letters
    assert fq_restate.stream(HAND_IN, 1, 0, opts).split(b"\n")[4:8] == [b"@", b"ACGT", b"+", b"IIII"]
    # the other formats
    assert fq_restate.stream(b">a b\r\nACGTACGTAC\r\n>c\nAC\n", 2, 5, None) == b">a b\nACGTACGTAC\n"
    assert fq_restate.stream(b"ACGTAC\n\nacgu\n", 3, 0, dict(cut=[1])) == b"CGTAC\n\ncgu\n"
    with pytest.raises(fq_restate.QualityLengthMismatch):
        fq_restate.stream(b"@a\nACGT\n+\nIII\n", 1, 0, None)


def _args(*extra):
    return cli.parse_args(["-s", "a.fastq", "-lib", "L", "-on", "human", "-db", "miRBase", "-o", "out"] + list(extra))


def test_the_flag_and_its_refusals(monkeypatch, capsys):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("MIRGE_BGZF_DEFLATE", raising=False)
    monkeypatch.delenv("MIRGE_BGZF_BLOCK_BYTES", raising=False)
    assert _args().trimmed_out is None
    assert _args("--trimmed-out").trimmed_out == "plain" and _args("--trimmed-out", "plain").trimmed_out == "plain"
    assert _args("--trimmed-out", "gz").trimmed_out == "gz"
    # legal beside it
    ok = _args("--trimmed-out", "gz", "-a", "auto", "--read-qc", "--kmer-correct", "-tcf")
    assert ok.trimmed_out == "gz" and ok.read_qc and trimmed_out.refusal(ok) == ""

    def refused(argv, text):
        with pytest.raises(SystemExit):
            _args(*argv)
        assert text in capsys.readouterr().err

    refused(["--trimmed-out", "bz2"], "invalid choice")
    refused(["--trimmed-out", "-umi", "4,0"], "--trimmed-out: not together with -umi")
    refused(["--trimmed-out", "-spl"], "--trimmed-out runs on the device-resident route")
    refused(["--trimmed-out", "-rr"], "--trimmed-out runs on the device-resident route")
    refused(["--trimmed-out", "--backend", "bowtie"], "--trimmed-out runs on the device-resident route")
    monkeypatch.setenv("WORLD_SIZE", "2")
    refused(["--trimmed-out"], "--trimmed-out is a single-process option")
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.setenv("MIRGE_BGZF_DEFLATE", "fastest")
    refused(["--trimmed-out", "gz"], "MIRGE_BGZF_DEFLATE")
    assert _args("--trimmed-out").trimmed_out == "plain"  # (the plain file asks nothing of BGZF)
    monkeypatch.setenv("MIRGE_BGZF_DEFLATE", "host")
    monkeypatch.setenv("MIRGE_BGZF_BLOCK_BYTES", "63")
    refused(["--trimmed-out", "gz"], "MIRGE_BGZF_BLOCK_BYTES")
    monkeypatch.setenv("MIRGE_BGZF_BLOCK_BYTES", "64")
    assert _args("--trimmed-out", "gz").trimmed_out == "gz"


def test_file_names_and_the_log_line():
    assert trimmed_out.file_name("S1", 1) == "S1.trimmed.fastq" and trimmed_out.file_name("S1", 2) == "S1.trimmed.fasta"
    assert trimmed_out.file_name("S1", 3, "plain") == "S1.trimmed.txt" and trimmed_out.file_name("a.b", 1, "gz") == "a.b.trimmed.fastq.gz"
    with pytest.raises(ValueError):
        trimmed_out.file_name("S1", 1, "bz2")
    st = dict(records=10, written=7, stream_bytes=700, file_bytes=228, members=2, stored=0, fixed=1, dynamic=1)
    assert trimmed_out.log_line("S1", st) == "trimmed out S1: 10 records, 7 written, 3 too short, 700 bytes"
    assert trimmed_out.log_line("S1", st, "gz") == ("trimmed out S1: 10 records, 7 written, 3 too short, 700 bytes; 228 file bytes, 2 members "
                                                   "(stored 0, fixed 1, dynamic 1)")
    for phrase in ("--minimum-length", "``+``", "MIRGE_BGZF_BLOCK_BYTES", "BEFORE correction", "--trimmed-out:"):
        assert phrase in trimmed_out.__doc__


@pytest.mark.parametrize("name", sorted(fq_cases.all_cases()))
def test_written_records_are_the_trimmed_view_of_read_qc(name):
    case = fq_cases.all_cases()[name]
    st = fq_restate.stats(case["text"], case["fmt"], case["min_len"], case["opts"])
    e = qc_restate.entries(case["text"], case["fmt"], case["min_len"], case["opts"])
    assert st["written"] == e[("reads", "trimmed", None, None, None)] and st["records"] == e[("reads", "raw", None, None, None)]
    want = fq_cases.expected(name)
    assert st["stream_bytes"] == len(want) and want.count(b"\n") == st["written"] * {1: 4, 2: 2, 3: 1}[case["fmt"]]
