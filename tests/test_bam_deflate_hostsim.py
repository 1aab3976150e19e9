"""The deflate of ``k_bam_blocks`` on payloads that BAM records cannot produce, on the CPU: ``csrc/kernels_bam.hpp`` compiled for the
host (tests/hostsim/bam_sim.cpp through ``test_sorted_bam_hostsim.run``).  The golden inputs with an all-zero count matrix select no
rows, so the stream is the header alone and an ``@CO`` line of the ``--sam-header`` file is the payload (tests/deflate_probe.py): the
stored fallback (BTYPE 00) and the edge of its decision, 9-bit literals, every length and distance code the parse can reach, last
members of 1 to 257 bytes.  tests/test_bam_deflate_gpu.py asserts the same of the device."""
import numpy as np
import pytest

import mirge3_amd  # noqa: F401

import bam_reader
import deflate_probe as dp
from test_sam_out import golden_inputs
from test_sam_out_hostsim import _oracle_annotation
from test_sorted_bam_hostsim import run


@pytest.fixture(scope="module")
def empty_sample():
    libs, _samples, seqs, counts = golden_inputs()
    return dict(libs=libs, seqs=seqs, ann=_oracle_annotation(libs, seqs), counts=np.zeros_like(counts), order=np.arange(len(seqs)))


def deflated(g, header, block):
    """-> (the file the members make with the EOF block, bam_reader.decode_bam of it)"""
    members, n_rec = run(g["libs"], g["seqs"], *g["ann"], g["counts"], g["order"], 0, header, block, 1)
    assert n_rec == 0
    bam = members + bam_reader.EOF_BLOCK
    return bam, bam_reader.decode_bam(bam)  # (every member's BSIZE, CRC-32 and ISIZE are checked there)


def test_fixed_symbols_reads_what_zlib_writes():
    """the decoder against zlib's own fixed-Huffman blocks (Z_FIXED): literals of 8 and 9 bits, every length up to 258, short and long
    distances"""
    import zlib
    rng = np.random.Generator(np.random.PCG64(3))
    unit = rng.integers(0, 256, size=700, dtype=np.uint8).tobytes()
    data = unit + b"".join(unit[k:k + 3 + k % 256] + bytes([k % 251]) for k in range(300)) + b"\xff" * 600 + unit[:300] + bytes(range(256))
    z = zlib.compressobj(9, zlib.DEFLATED, -15, 9, zlib.Z_FIXED)
    cdata = z.compress(data) + z.flush()
    syms = dp.fixed_symbols(cdata)
    assert dp.expand(syms) == data
    m = [s for s in syms if not isinstance(s, int)]
    assert {s[2] for s in m} >= set(range(258, 286)) and max(s[1] for s in m) > 16384 and min(s[1] for s in m) == 1
    assert all(dp.LEN_BASE[s[2] - 257] <= s[0] < dp.LEN_BASE[s[2] - 257] + (1 << dp.LEN_EXTRA[s[2] - 257]) for s in m)
    assert all(dp.DIST_BASE[s[3]] <= s[1] < dp.DIST_BASE[s[3]] + (1 << dp.DIST_EXTRA[s[3]]) for s in m)


def test_block_is_match_free():
    rng = np.random.Generator(np.random.PCG64(4))
    out = bytearray()
    dp.Fresh(rng, range(256)).fill(out, 70000)
    assert dp.block_is_match_free(out, 0, 65280) and dp.block_is_match_free(out, 5, 6) and b"@" not in out
    twice = bytearray(out); twice[30000:30004] = out[100:104]     # the same half
    assert not dp.block_is_match_free(twice, 0, 65280) and dp.block_is_match_free(twice, 101, 65280)
    halves = bytearray(out); halves[32800:32804] = out[100:104]   # one in either half: no source for a match
    assert dp.block_is_match_free(halves, 0, 65280) and not dp.block_is_match_free(halves, 100, 65280)
    run4 = bytearray(out); run4[500:504] = b"zzzz"
    assert not dp.block_is_match_free(run4, 0, 65280) and not dp.block_is_match_free(run4, 500, 504) and dp.block_is_match_free(run4, 501, 520)


@pytest.mark.parametrize("block", [64, 4096, dp.DEFAULT_BLOCK])
def test_high_bytes_are_stored(empty_sample, block):
    header, span = dp.high_distinct() if block == dp.DEFAULT_BLOCK else dp.high_random()
    bam, d = deflated(empty_sample, header, block)
    free, inside = dp.check_high(d, bam, header, span, block)
    print(f"block {block}: {free} of {inside} blocks inside the payload are match-free and stored")


@pytest.mark.parametrize("h", dp.EDGE_H)
def test_stored_exactly_when_the_fixed_form_is_no_shorter(empty_sample, h):
    header, span = dp.edge_payload(h)
    bam, d = deflated(empty_sample, header, dp.EDGE_BLOCK)
    dp.check_edge(d, bam, header, span, h)


@pytest.fixture(scope="module")
def codes():
    return dp.codes_payload()


@pytest.mark.parametrize("block", [dp.DEFAULT_BLOCK, 4096])
def test_every_length_and_distance_code(empty_sample, codes, block):
    header, _span, plants = codes
    bam, d = deflated(empty_sample, header, block)
    len_codes, dist_codes = dp.check_codes(d, bam, header, plants, block)
    print(f"block {block}: length codes {sorted(len_codes)}, distance codes {sorted(dist_codes)}")


@pytest.mark.parametrize("rem", dp.SHORT_REMAINDERS)
def test_short_last_member(empty_sample, rem):
    header, _span = dp.short_payload(rem)
    bam, d = deflated(empty_sample, header, dp.SHORT_BLOCK)
    dp.check_short(d, bam, header, rem)
