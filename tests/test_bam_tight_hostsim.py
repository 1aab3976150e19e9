"""``MIRGE_BAM_DEFLATE=tight`` on the CPU: ``k_bam_blocks`` with ``deflate == 3`` of ``csrc/kernels_bam.hpp`` compiled for the host
(tests/hostsim/bam_sim.cpp through ``test_sorted_bam_hostsim.run``).  The route parses the blocks of the other routes anew, so every
file is held against the stream (tests/deflate_tight_probe.py): the same payloads as under ``deflate == 1``, every member a valid one
no larger than its stored form, its symbols -- read with the decoders of tests/deflate_probe.py and tests/deflate_dyn_probe.py --
expanding to its payload.  What the new parse is for is asserted where it is structural: a row of 1234 copies is matched one record
back and its file is smaller than the dynamic route's; matches run across the threads' segments.  tests/test_bam_tight_gpu.py holds
the device's files against the files made here."""
import os
import statistics

import pytest

import mirge3_amd  # noqa: F401
from mirge3_amd import bam_export

import bam_reader
import deflate_probe as dp
import deflate_tight_probe as tp
from test_bam_deflate_hostsim import empty_sample  # noqa: F401  (a fixture)
from test_sorted_bam import HEADER_CASES, expected_lines, header_of_length
from test_sorted_bam_hostsim import case, run  # noqa: F401  (case: a fixture)


def sim_file(g, header, block, deflate, sample=0):
    """-> (the members with the EOF block behind them, decode_bam of that file)"""
    members, n_rec = run(g["libs"], g["seqs"], *g["ann"], g["counts"], g["order"], sample, header, block, deflate)
    bam = members + bam_reader.EOF_BLOCK
    d = bam_reader.decode_bam(bam)  # (every member's BSIZE, CRC-32 and ISIZE are checked there)
    assert n_rec == len(d["lines"])
    return bam, d


def tight_and_fixed(g, header, block, sample=0):
    """-> (the tight file, decode_bam of it, check_tight's members)"""
    bam, d = sim_file(g, header, block, 3, sample)
    _fbam, fd = sim_file(g, header, block, 1, sample)
    return bam, d, tp.check_tight(d, bam, fd)


@pytest.fixture(scope="module")
def record_files(case):
    """the 1234-copy sample per block size: the tight file, what check_tight read off it, the dynamic route's file"""
    out = {}
    for block in (256, 4096, 65280):
        bam, d, members = tight_and_fixed(case, case["header"], block)
        out[block] = dict(bam=bam, d=d, members=members, dynamic=sim_file(case, case["header"], block, 2)[0] if block >= 4096 else None)
    return out


@pytest.mark.parametrize("block", [256, 4096, 65280])
def test_records(case, record_files, block):
    """(at 256 a thread owns one byte: every match crosses segments)"""
    f = record_files[block]
    assert f["d"]["lines"] == expected_lines(case["bodies"][0], case["names"])
    crossing = sum(len(tp.crossing_matches(s, len(m["payload"]))) for _u, m, s in f["members"])
    print(f"block {block}: members stored / fixed / dynamic {tp.btypes(f['members'])}, {len(f['bam'])} bytes, {crossing} matches across a segment's end")
    assert crossing >= 1


def heavy_row(case, d):
    """-> (first byte, end, longest record) in the stream of the row of 1234 copies"""
    name = next(ln for ln in case["bodies"][0].decode().split("\n") if ln.split("\t")[0].endswith("_1233")).split("\t")[0]
    seq = name.rsplit("_", 1)[0].encode()
    stream = b"".join(m["payload"] for m in d["members"])
    first, last = stream.find(seq + b"_0\0") - 36, stream.find(seq + b"_1233\0") - 36
    assert first >= 0 and last > first and stream.count(seq + b"_1233\0") == 1
    longest = int.from_bytes(stream[last:last + 4], "little") + 4
    assert int.from_bytes(stream[first:first + 4], "little") + 4 == longest - 3  # (one digit against four)
    return first, last + longest, longest


@pytest.mark.parametrize("block", [4096, 65280])
def test_copies_are_matched_one_record_back_and_the_file_is_smaller_than_the_dynamic_one(case, record_files, block):
    """structural for a row of 1234 copies: its nearest earlier copy lies one record back, the first copy in the block -- the other
    routes' only candidate -- up to a block back"""
    f = record_files[block]
    assert len(f["bam"]) < len(f["dynamic"]), (len(f["bam"]), len(f["dynamic"]))
    lo, hi, longest = heavy_row(case, f["d"])
    inside = [(u, m, s) for u, m, s in f["members"] if lo <= u and u + len(m["payload"]) <= hi]
    assert inside, (lo, hi)
    dists = [dist for _u, _m, s in inside for _at, length, dist in tp.matches_of(s) if length >= 32]
    print(f"block {block}: {len(f['bam'])} bytes against {len(f['dynamic'])} dynamic; {len(inside)} members inside the row, {len(dists)} matches of 32 bytes "
          f"or more, median distance {statistics.median(dists)}, longest record {longest}")
    assert len(dists) >= 10 and statistics.median(dists) <= longest


@pytest.mark.parametrize("block", [4096, 65280])
def test_the_same_stream_twice_gives_the_same_bytes(case, record_files, block):
    again, _d = sim_file(case, case["header"], block, 3)
    assert again == record_files[block]["bam"]


@pytest.mark.parametrize("block", [4096, dp.DEFAULT_BLOCK])
def test_repeated_unit_is_matched_across_segments(empty_sample, block):
    header, (lo, hi) = tp.repeated_unit()
    _bam, _d, members = tight_and_fixed(empty_sample, header, block)
    inside = [(u, m, s) for u, m, s in members if lo <= u and u + len(m["payload"]) <= hi]
    assert len(inside) >= 1
    for u, m, s in inside:  # (a block starts without a past: its first 700 bytes are literals)
        n = len(m["payload"])
        assert tp.crossing_matches(s, n), f"block at {u}: no match covers a multiple of {-(-n // dp.THREADS)}"
        assert all(dist % 700 == 0 for _at, _l, dist in tp.matches_of(s))


@pytest.mark.parametrize("block", [dp.DEFAULT_BLOCK, 256])
def test_equal_bytes(empty_sample, block):
    """the longest chain of overruns the prefix maximum can meet: every thread's first match runs into the next thread's bytes"""
    header, (lo, hi) = tp.equal_bytes(dp.DEFAULT_BLOCK, block)
    _bam, _d, members = tight_and_fixed(empty_sample, header, block)  # (check_tight: it decodes, no token beyond 258 or 32 768)
    inside = [(u, m, s) for u, m, s in members if lo <= u and u + len(m["payload"]) <= hi]
    assert len(inside) == dp.DEFAULT_BLOCK // block
    most = max(len(s) for _u, _m, s in inside)
    print(f"block {block}: at most {most} tokens per member of equal bytes")
    assert most <= 2 * dp.THREADS


@pytest.mark.parametrize("family,block", [("high_random", 4096), ("high_distinct", dp.DEFAULT_BLOCK), ("codes", dp.DEFAULT_BLOCK), ("codes", 4096)])
def test_payload_families(empty_sample, family, block):
    """(correctness only: a planted code need not survive another parse, and a match-free block is stored under any parse)"""
    header = {"high_random": dp.high_random, "high_distinct": dp.high_distinct, "codes": dp.codes_payload}[family]()[0]
    _bam, d, members = tight_and_fixed(empty_sample, header, block)
    assert b"".join(m["payload"] for m in d["members"]) == bam_export.header_blob(header)[0]
    print(f"{family}, block {block}: members stored / fixed / dynamic {tp.btypes(members)}")


@pytest.mark.parametrize("rem", dp.SHORT_REMAINDERS)
def test_short_last_member(empty_sample, rem):
    header, _span = dp.short_payload(rem)
    _bam, d, _members = tight_and_fixed(empty_sample, header, dp.SHORT_BLOCK)
    assert [len(m["payload"]) for m in d["members"][:-1]] == [dp.SHORT_BLOCK] * 2 + ([rem] if rem else [])
    assert b"".join(m["payload"] for m in d["members"]) == bam_export.header_blob(header)[0]


@pytest.mark.parametrize("block,want", [HEADER_CASES[5], HEADER_CASES[-1]], ids=lambda v: str(v))
def test_header_length_against_the_records(case, block, want):
    """(where the header ends decides in which thread's segment the first record starts)"""
    header = header_of_length(case["header"], block, want)
    assert len(bam_export.header_blob(header)[0]) % block == want
    _bam, d, _members = tight_and_fixed(case, header, block, sample=1)
    assert d["lines"] == expected_lines(case["bodies"][1], case["names"]) and len(d["lines"]) > 20


def test_bam_deflate_tight_needs_sorted_bam(tmp_path):
    from mirge3_amd.cli import parse_args
    base = ["-s", "x.fastq", "-lib", "L", "-on", "human"]
    hdr = tmp_path / "h.txt"
    hdr.write_text("@HD\tVN:1.0\n@SQ\tSN:chr1\tLN:1000\n")
    old = os.environ.get("MIRGE_BAM_DEFLATE")
    assert parse_args(base + ["--sorted-bam", "--sam-header", str(hdr), "--bam-deflate", "tight"]).bam_deflate == "tight"
    assert os.environ.get("MIRGE_BAM_DEFLATE") == old  # parsing alone sets nothing
    for bad in (["--bam-deflate", "tight"], ["--bam-deflate", "tight", "--sam-out"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
