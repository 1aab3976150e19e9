"""``--sorted-bam`` on the host (no GPU): ``bam_export.format_bam_host`` -- the plain Python restatement the device is compared with --
against the reference's own ``<sample>.sam`` files (tests/golden/sam_out) read back through tests/bam_reader.py, the ``@HD`` rules,
the errors, reg2bin at the bin boundaries, the index against a brute-force scan, the command line."""
import os
import struct

import numpy as np
import pytest

import mirge3_amd  # noqa: F401
from mirge3_amd import bam_export, sam_export
from mirge3_amd.cli import parse_args

import bam_reader
from test_sam_out import GOLDEN


def golden_bodies():
    """{sample: the lines of the reference's <sample>.sam below its header}"""
    out = {}
    for nm in ("S1", "S2"):
        with open(os.path.join(GOLDEN, nm + ".sam"), "rb") as fh:
            data = fh.read()
        assert data.startswith(sam_export.DEFAULT_HEADER)
        out[nm] = data[len(sam_export.DEFAULT_HEADER):]
    return out


def golden_header():
    """written here from the RNAMEs of the golden files: first appearance order with the first two swapped, plus one @SQ no read
    lies on, behind an @HD line that says 'unsorted'"""
    seen = []
    for body in golden_bodies().values():
        for line in body.decode().split("\n"):
            if line and line.split("\t")[2] not in seen:
                seen.append(line.split("\t")[2])
    assert len(seen) >= 2
    names = [seen[1], seen[0]] + seen[2:]
    names.insert(1, "chrNoReads")
    return ("@HD\tVN:1.0\tSO:unsorted\n" + "".join(f"@SQ\tSN:{nm}\tLN:{(1 << 29) - k}\n" for k, nm in enumerate(names)) + "@CO\tgolden\n").encode(), names


# (block size, what the stream's header bytes H leave modulo it).  k_bam_blocks hands a record to the first 32-byte probe point at or
# behind its start, and the header's end is where that rule begins: at block 256 H takes every residue modulo the probe distance 32, and
# modulo 256 the residues 0, 1 and 255 with them; at block 64 the header is longer than two blocks and ends inside a probe's stretch
HEADER_CASES = [(256, {0: 0, 1: 1, 31: 255}.get(r, r + 32 * (r % 8))) for r in range(32)] + [(64, 37)]


def header_of_length(header: bytes, block: int, want: int) -> bytes:
    """header with one more @CO line, padded so that the stream's header bytes (header_blob) leave `want` modulo block"""
    base = len(bam_export.header_blob(header + b"@CO\t\n")[0])
    out = header + b"@CO\t" + b"p" * ((want - base) % block + (2 * block if block == 64 else 0)) + b"\n"
    assert len(bam_export.header_blob(out)[0]) % block == want and (block != 64 or len(bam_export.header_blob(out)[0]) > 2 * block)
    return out


def expected_lines(body: bytes, names):
    refid_of = {nm: k for k, nm in enumerate(names)}
    lines = [ln for ln in body.decode().split("\n") if ln]
    return sorted(lines, key=lambda ln: bam_reader.sort_key(ln, refid_of))  # (stable)


def sam_line(qname, flag, rname, start, seq):
    return "\t".join([qname, str(flag), rname, str(start), "255", f"{len(seq)}M", "*", "0", "0", seq, "I" * len(seq), "XA:i:0", f"MD:Z:{len(seq)}", "NM:i:0"])


@pytest.mark.parametrize("block", [bam_export.BLOCK_BYTES, 300])
def test_format_bam_host_decodes_to_the_reference_files_sorted(block):
    header, names = golden_header()
    for nm, body in golden_bodies().items():
        bam, bai = bam_export.format_bam_host(body, header, block_bytes=block)
        d = bam_reader.decode_bam(bam)
        want = expected_lines(body, names)
        assert d["lines"] == want and len(want) > 20, nm
        assert sorted(want) == sorted(ln for ln in body.decode().split("\n") if ln)
        assert d["text"] == bam_export.header_text(header) and [r[0] for r in d["refs"]] == names
        assert d["refs"][1] == ("chrNoReads", (1 << 29) - 1)
        assert bai == bam_reader.build_bai(len(names), d["recs"]), nm
        idx = bam_reader.parse_bai(bai)
        assert idx[1] == dict(bins={}, meta=None, lin=[])  # the @SQ without reads: an empty entry
        assert sum(r["meta"][1][0] for r in idx if r["meta"]) == len(want)
        if block == 300:
            assert len(d["members"]) > 20


def test_header_text_rules():
    T = bam_export.header_text
    assert T(b"@HD\tVN:1.0\tSO:unsorted\n@SQ\tSN:a\tLN:5\n") == b"@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:a\tLN:5\n"
    assert T(b"@HD\tVN:1.6\n@SQ\tSN:a\tLN:5\n") == b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:a\tLN:5\n"
    assert T(b"@HD\tVN:1.6\tSO:queryname\tGO:none\n") == b"@HD\tVN:1.6\tSO:coordinate\tGO:none\n"
    assert T(b"@SQ\tSN:a\tLN:5\n@CO\tx") == b"@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:a\tLN:5\n@CO\tx"
    assert T(b"@HD\tVN:1.0") == b"@HD\tVN:1.0\tSO:coordinate"
    blob, refs = bam_export.header_blob(b"@SQ\tSN:b\tLN:7\n@SQ\tSN:a\tLN:5\n")
    assert refs == [("b", 7), ("a", 5)]  # refID is the @SQ order
    text = b"@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:b\tLN:7\n@SQ\tSN:a\tLN:5\n"
    assert blob == b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", 2) + struct.pack("<i", 2) + b"b\0" + struct.pack("<i", 7) + \
        struct.pack("<i", 2) + b"a\0" + struct.pack("<i", 5)


def test_errors():
    header = b"@HD\tVN:1.0\n@SQ\tSN:chr1\tLN:1000\n"
    for bad in (b"@HD\tVN:1.0\n", b"", b"@SQ\tSN:chr1\n", b"@SQ\tLN:5\n", b"@SQ\tSN:a\tLN:5\n@SQ\tSN:a\tLN:6\n"):
        with pytest.raises(ValueError):
            bam_export.parse_sq(bad)
    with pytest.raises(ValueError, match="chr9"):
        bam_export.format_bam_host((sam_line("ACGTACGTACGTACGT_0", 0, "chr9", 5, "ACGTACGTACGTACGT") + "\n").encode(), header)
    read = "ACGT" * 63  # 252 nt: READ_0 has 254 characters
    bam, _ = bam_export.format_bam_host((sam_line(read + "_0", 0, "chr1", 5, read) + "\n").encode(), header)
    assert bam_reader.decode_bam(bam)["lines"] == [sam_line(read + "_0", 0, "chr1", 5, read)]
    with pytest.raises(ValueError, match="253 nt"):
        bam_export.format_bam_host((sam_line(read + "A_0", 0, "chr1", 5, read + "A") + "\n").encode(), header)
    with pytest.raises(ValueError, match="2\\^29"):
        bam_export.format_bam_host((sam_line("ACGTACGTACGTACGT_0", 0, "chr1", (1 << 29) - 14, "ACGTACGTACGTACGT") + "\n").encode(), header)


def test_command_line(tmp_path):
    base = ["-s", "x.fastq", "-lib", "L", "-on", "human"]
    hdr = tmp_path / "h.txt"
    hdr.write_text("@HD\tVN:1.0\n@SQ\tSN:chr1\tLN:1000\n")
    nosq = tmp_path / "nosq.txt"
    nosq.write_text("@HD\tVN:1.0\n")
    a = parse_args(base + ["--sorted-bam", "--sam-header", str(hdr)])
    assert a.sorted_bam is True and a.sam_out is False and a.sam_header == str(hdr)
    assert parse_args(base).sorted_bam is False
    b = parse_args(base + ["--sorted-bam", "--sam-out", "--sam-header", str(hdr)])
    assert b.sorted_bam and b.sam_out
    sh = ["--sam-header", str(hdr)]
    for bad in (["--sam-header", str(hdr)], ["--sorted-bam"], ["--sorted-bam", "--sam-header", str(nosq)], ["--sorted-bam", "-spl"] + sh,
                ["--sorted-bam", "-rr"] + sh, ["--sorted-bam", "--backend", "bowtie"] + sh, ["--sorted-bam", "--sam-header", str(tmp_path / "missing")],
                ["-bam"], ["--bam-out"], ["-bam", "--sorted-bam"] + sh):
        with pytest.raises(SystemExit):
            parse_args(base + bad)


def test_sharded_run_refuses_sorted_bam(tmp_path, monkeypatch):
    from mirge3_amd import cli, multigpu
    import torch.distributed
    (tmp_path / "L" / "human" / "index.Libs").mkdir(parents=True)
    hdr = tmp_path / "h.txt"
    hdr.write_text("@SQ\tSN:chr1\tLN:1000\n")
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(torch.distributed, "init_process_group", lambda *a, **k: None)
    monkeypatch.setattr(multigpu, "agree_on_run_directory", lambda *a, **k: "out")
    with pytest.raises(SystemExit) as e:
        cli.main(["-s", "x.fastq", "-lib", str(tmp_path / "L"), "-on", "human", "-o", str(tmp_path), "--sorted-bam", "--sam-header", str(hdr), "-shh"])
    assert "--sorted-bam is a single-process option" in str(e.value)


# bins from the SAM specification 5.3 worked by hand: level offsets 4681 (16 kb), 585, 73, 9, 1, 0
BOUNDARY_BINS = [(14, 4681 + 0, 585), (17, 4681 + 7, 73), (20, 4681 + 63, 9), (23, 4681 + 511, 1), (26, 4681 + 4095, 0)]


def test_reg2bin_at_the_bin_boundaries():
    header = b"@SQ\tSN:chr1\tLN:536870912\n"
    lines = []
    for shift, inside, crossing in BOUNDARY_BINS:
        pos = (1 << shift) - 1
        for f in (bam_export.reg2bin, bam_reader.reg2bin):
            assert f(pos, pos + 1) == inside and f(pos, pos + 2) == crossing and f(pos - 15, pos + 1) == inside and f(pos - 15, pos + 2) == crossing
        lines.append(sam_line(f"ACGTACGTACGTACGT_{shift}", 0, "chr1", pos + 1 - 15, "ACGTACGTACGTACGT"))      # ends at the boundary
        lines.append(sam_line(f"ACGTACGTACGTACGTA_{shift}", 16, "chr1", pos + 1 - 15, "ACGTACGTACGTACGTA"))   # crosses it
    bam, bai = bam_export.format_bam_host(("\n".join(lines) + "\n").encode(), header, block_bytes=200)
    d = bam_reader.decode_bam(bam)  # (the reader checks every record's bin against its own reg2bin)
    assert d["lines"] == lines and bai == bam_reader.build_bai(1, d["recs"])
    idx = bam_reader.parse_bai(bai)
    assert set(idx[0]["bins"]) == {b for _, a, c in BOUNDARY_BINS for b in (a, c)}
    for shift, _, _ in BOUNDARY_BINS:
        edge = 1 << shift
        assert len(bam_reader.query(idx, d["recs"], 0, edge, edge + 1)) == 1 and len(bam_reader.query(idx, d["recs"], 0, edge - 1, edge)) == 2


def test_index_answers_region_queries_like_a_brute_force_scan():
    rng = np.random.Generator(np.random.PCG64(20260))
    names = ["chrA", "chrEmpty", "chrB", "chrC"]
    header = "".join(f"@SQ\tSN:{nm}\tLN:{1 << 29}\n" for nm in names).encode()
    lines = []
    for k in range(600):
        ref = names[int(rng.choice([0, 2, 3], p=[0.6, 0.3, 0.1]))]
        L = int(rng.integers(16, 60))
        u = rng.random()
        if u < 0.3:  # around a bin boundary of some level
            pos = (1 << int(rng.choice([14, 17, 20, 23, 26]))) * int(rng.integers(1, 4)) - int(rng.integers(0, 2 * L))
        elif u < 0.6:  # a dense stretch
            pos = 50000 + int(rng.integers(0, 40000))
        else:
            pos = int(rng.integers(0, (1 << 28)))
        seq = "".join("ACGT"[int(c)] for c in rng.integers(0, 4, size=L))
        for c in range(int(rng.choice([1, 1, 1, 3, 12]))):
            lines.append(sam_line(f"{seq}_{c}", int(rng.choice([0, 16])) if c == 0 else int(lines[-1].split("\t")[1]), ref, max(1, pos + 1), seq))
    bam, bai = bam_export.format_bam_host(("\n".join(lines) + "\n").encode(), header, block_bytes=1000)
    d = bam_reader.decode_bam(bam)
    assert d["lines"] == expected_lines(("\n".join(lines) + "\n").encode(), names)
    assert bai == bam_reader.build_bai(len(names), d["recs"])
    idx = bam_reader.parse_bai(bai)
    hits = 0
    for q in range(200):
        ref = int(rng.integers(0, len(names)))
        if q % 2:
            r = d["recs"][int(rng.integers(0, len(d["recs"])))]
            ref, beg = r[0], max(0, r[1] + int(rng.integers(-40, 40)))
        else:
            beg = int(rng.integers(0, 1 << 28))
        end = beg + int(rng.choice([1, 30, 5000, 20000, 1 << 20, 1 << 27]))
        got, want = bam_reader.query(idx, d["recs"], ref, beg, end), bam_reader.brute(d["recs"], ref, beg, end)
        assert got == want, (ref, beg, end)
        hits += bool(want)
    assert hits > 80
