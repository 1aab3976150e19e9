"""``--sam-out`` on the host (no GPU): the header-line parser and the lift tables rule by rule, ``format_sam_host`` -- the plain
Python restatement the device is compared with -- against the files the reference wrote (tests/golden/sam_out, made by
tests/golden/make_golden_sam_out.py), the digit-band byte count, the command line."""
import csv
import os

import numpy as np
import pytest

import oracle
import mirge3_amd  # noqa: F401
from mirge3_amd import sam_export
from mirge3_amd.cascade import PASSES
from mirge3_amd.cli import parse_args
from mirge3_amd.seqio import FlatSeqs, load_library_dir

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sam_out")
ORG, DB = "synthorg", "miRBase"


def golden_inputs():
    libs = load_library_dir(os.path.join(GOLDEN, "libs"), ORG, DB)
    with open(os.path.join(GOLDEN, "collapsed_input.csv")) as fh:
        rows = list(csv.reader(fh))
    seqs = [r[0] for r in rows[1:]]
    counts = np.array([[int(x) for x in r[1:]] for r in rows[1:]], dtype=np.int64)
    return libs, rows[0][1:], seqs, counts


def host_passes_of(libs):
    return {p: dict(names=libs[PASSES[p][1]].names, headers=libs[PASSES[p][1]].headers, seqs=libs[PASSES[p][1]].seqs.to_list(),
                    trim5=int(PASSES[p][3].get("trim5", 0)), trim3=int(PASSES[p][3].get("trim3", 0))) for p in sam_export.CLASS_PASSES}


def test_header_lines_accepted_and_rejected():
    H = sam_export.header_dictionary
    ok = "ENST1.2 chr1 segs:1-9,10-981 cds:+:65565-65573,69037-70008"
    d = H([ok])
    assert sam_export.lift_of(d, "ENST1.2", "human") == ("chr1", False, [(1, 9), (10, 981)], [(65565, 65573), (69037, 70008)])
    # PATCH anywhere in the line; fewer than 4 tokens; token 2 / token 3 without their ':' pieces; wrong prefixes
    for bad in ("E chr1_PATCH segs:1-9 cds:+:5-13", "E chr1 segs:1-9", "E chr1 segs cds:+:5-13", "E chr1 segs:1-9 cds:+", "E",
                "E chr1 exons:1-9 cds:+:5-13", "E chr1 segs:1-9 utr:+:5-13", "E  chr1 segs:1-9 cds:+:5-13", ""):
        assert sam_export.lift_of(H([bad]), "E", "human") is None, bad
    # a line that parses only in part leaves its segs entry behind but no chromosome
    assert "E#segs" in H(["E chr1 segs:1-9 cds:+"]) and "E" not in H(["E chr1 segs:1-9 cds:+"])
    # the strand is '+' only when the field is exactly '+'
    assert sam_export.lift_of(H(["E chr1 segs:1-9 cds:-:5-13"]), "E", "human")[1] is True
    assert sam_export.lift_of(H(["E chr1 segs:1-9 cds:1:5-13"]), "E", "human")[1] is True
    assert sam_export.lift_of(H(["E chr1 segs:1-9 cds:+:5-13"]), "E", "human")[1] is False
    # the chromosome is token 1 verbatim -- for hamster its third ':' piece, and no line without one
    assert sam_export.lift_of(H(["E chromosome:GRCh38:12 segs:1-9 cds:+:5-13"]), "E", "human")[0] == "chromosome:GRCh38:12"
    assert sam_export.lift_of(H(["E chromosome:CriGri:7:1:9 segs:1-9 cds:+:5-13"]), "E", "hamster")[0] == "7"
    assert sam_export.lift_of(H(["E chr7 segs:1-9 cds:+:5-13"]), "E", "hamster") is None
    # a name the library does not know; a later line of the same name wins
    assert sam_export.lift_of(d, "ENST9", "human") is None
    assert sam_export.lift_of(H([ok, "ENST1.2 chr2 segs:1-5 cds:-:7-11"]), "ENST1.2", "human") == ("chr2", True, [(1, 5)], [(7, 11)])
    # lists that are no numbers, or fewer cds entries than segments: dropped
    assert sam_export.lift_of(H(["E chr1 segs:1-x cds:+:5-13"]), "E", "human") is None
    assert sam_export.lift_of(H(["E chr1 segs:1-9,10-20 cds:+:5-13"]), "E", "human") is None


def test_lift_tables_are_the_parsed_headers():
    libs, _, _, _ = golden_inputs()
    for key in ("snorna", "rrna", "ncrna_others", "mrna", "mirna", "hairpin"):
        lib = libs[key]
        t = sam_export.lift_tables(lib.names, lib.headers, ORG)
        d = sam_export.header_dictionary(lib.headers)
        chroms = FlatSeqs(t["chrom_data"], t["chrom_off"]).to_list() if t["n_chrom"] else []
        for r, nm in enumerate(lib.names):
            lf = sam_export.lift_of(d, nm, ORG)
            a, b = int(t["seg_ptr"][r]), int(t["seg_ptr"][r + 1])
            if lf is None:
                assert t["chrom_of_ref"][r] == -1 and a == b
                continue
            assert chroms[t["chrom_of_ref"][r]] == lf[0] and bool(t["minus"][r]) == lf[1]
            assert list(zip(t["seg_s"][a:b].tolist(), t["seg_e"][a:b].tolist())) == lf[2]
            assert list(zip(t["cds_lo"][a:b].tolist(), t["cds_hi"][a:b].tolist())) == lf[3]
    t = sam_export.lift_tables(libs["snorna"].names, libs["snorna"].headers, ORG)
    assert t["chrom_of_ref"].tolist()[2:] == [-1, -1] and t["minus"].tolist()[:2] == [0, 1]  # SNO3: no coordinates, SNO4: only segs
    assert sam_export.lift_tables(libs["rrna"].names, libs["rrna"].headers, ORG)["chrom_of_ref"][1] == -1  # the PATCH header


def test_format_sam_host_equals_the_reference_files():
    libs, samples, seqs, counts = golden_inputs()
    reads = FlatSeqs.from_list(seqs)
    olibs = [(libs[PASSES[p][1]].seqs.data, libs[PASSES[p][1]].seqs.offsets) for p in range(9)]
    ps, ref, off, mm = oracle.cascade(reads.data, reads.offsets, olibs, n_pass=9, indexed=True)
    assert set(sam_export.CLASS_PASSES) <= set(int(p) for p in ps)  # every one of the seven source passes
    order = np.arange(len(seqs))  # two samples: the frame is the sorted union, which is the fixture's row order
    assert seqs == sorted(seqs)
    for s, name in enumerate(samples):
        body = sam_export.format_sam_host(seqs, ps, ref, off, mm, counts, order, s, host_passes_of(libs), ORG)
        with open(os.path.join(GOLDEN, name + ".sam"), "rb") as fh:
            assert sam_export.DEFAULT_HEADER + body == fh.read(), name


@pytest.mark.parametrize("c", [1, 9, 10, 11, 99, 100, 101, 1000, 100001])
def test_digit_band_bytes(c):
    tail = sam_export.line_suffix("ACGTACGTACGTACGTAC", 0, 0, ("chr1", False, [(1, 50)], [(100, 149)]), "TT" + "ACGTACGTACGTACGTAC" + "GG", 2, 0)
    lines = ["ACGTACGTACGTACGTAC_" + str(k) + tail for k in range(c)]
    fixed = len(lines[0]) - 1
    assert sam_export.digit_band_bytes(fixed, c) == sum(len(x) for x in lines)


def test_command_line(tmp_path):
    base = ["-s", "x.fastq", "-lib", "L", "-on", "human"]
    hdr = tmp_path / "h.txt"
    hdr.write_text("@HD\tVN:1.0\n")
    a = parse_args(base + ["--sam-out"])
    assert a.sam_out is True and a.sam_header is None
    assert parse_args(base).sam_out is False
    assert parse_args(base + ["--sam-out", "--sam-header", str(hdr)]).sam_header == str(hdr)
    for bad in (["--sam-header", str(hdr)], ["--sam-out", "-spl"], ["--sam-out", "-rr"], ["--sam-out", "--backend", "bowtie"],
                ["--sam-out", "--sam-header", str(tmp_path / "missing")], ["-bam"], ["--bam-out"], ["-bam", "--sam-out"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)


def test_sharded_run_refuses_sam_out(tmp_path, monkeypatch):
    from mirge3_amd import cli
    (tmp_path / "L" / "human" / "index.Libs").mkdir(parents=True)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    called = {}

    class _Dist:
        @staticmethod
        def init_process_group(*a, **k):
            called["init"] = True
    import torch.distributed
    monkeypatch.setattr(torch.distributed, "init_process_group", _Dist.init_process_group)
    from mirge3_amd import multigpu
    monkeypatch.setattr(multigpu, "agree_on_run_directory", lambda *a, **k: "out")
    with pytest.raises(SystemExit) as e:
        cli.main(["-s", "x.fastq", "-lib", str(tmp_path / "L"), "-on", "human", "-o", str(tmp_path), "--sam-out", "-shh"])
    assert "--sam-out is a single-process option" in str(e.value)
