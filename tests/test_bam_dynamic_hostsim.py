"""``MIRGE_BAM_DEFLATE=dynamic`` on the CPU: ``k_bam_blocks`` with ``deflate == 2`` and the code-length builder ``bam_huff_lengths`` of
``csrc/kernels_bam.hpp`` compiled for the host (tests/hostsim/bam_sim.cpp through ``test_sorted_bam_hostsim.run``; tests/hostsim/
bam_huff_sim.cpp).  Every file is held against the file of ``deflate == 1`` on the same stream (tests/deflate_dyn_probe.py): the same
records, no member larger, the dynamic members' symbols those of the fixed members, the decision checked in both directions.
tests/test_bam_dynamic_gpu.py asserts the same of the device."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

import mirge3_amd  # noqa: F401
from mirge3_amd import bam_export

import bam_reader
import deflate_dyn_probe as dy
import deflate_probe as dp
from test_bam_deflate_hostsim import empty_sample  # noqa: F401  (a fixture)
from test_sorted_bam import HEADER_CASES, expected_lines, header_of_length
from test_sorted_bam_hostsim import case, run  # noqa: F401  (case: a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
HUFF_SRC = os.path.join(HERE, "hostsim", "bam_huff_sim.cpp")
HUFF_SO = os.path.join(HERE, "hostsim", "_build", "libbamhuffsim.so")


def both(g, header, block, sample=0):
    """-> ((file, decode_bam) of deflate == 2, the same of deflate == 1), the EOF block behind the members"""
    out = []
    for deflate in (2, 1):
        members, n_rec = run(g["libs"], g["seqs"], *g["ann"], g["counts"], g["order"], sample, header, block, deflate)
        bam = members + bam_reader.EOF_BLOCK
        d = bam_reader.decode_bam(bam)  # (every member's BSIZE, CRC-32 and ISIZE are checked there)
        assert n_rec == len(d["lines"])
        out.append((bam, d))
    return out


def test_dynamic_symbols_reads_what_zlib_writes():
    """the decoder against zlib's own dynamic block: the data of test_fixed_symbols_reads_what_zlib_writes at level 9"""
    rng = np.random.Generator(np.random.PCG64(3))
    unit = rng.integers(0, 256, size=700, dtype=np.uint8).tobytes()
    data = unit + b"".join(unit[k:k + 3 + k % 256] + bytes([k % 251]) for k in range(300)) + b"\xff" * 600 + unit[:300] + bytes(range(256))
    z = zlib.compressobj(9, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY)
    cdata = z.compress(data) + z.flush()
    assert cdata[0] & 7 == 5, "zlib did not write one final dynamic block"
    syms, ll, dd, cl = dy.dynamic_symbols(cdata)
    assert dp.expand(syms) == data
    m = [s for s in syms if not isinstance(s, int)]
    assert len(m) > 250 and max(s[1] for s in m) > 16384 and min(s[1] for s in m) == 1 and max(s[0] for s in m) == 258
    assert len(ll) == dy.N_LL and len(dd) == dy.N_D and len(cl) == dy.N_CL and max(cl) <= 7
    assert dy.crude_dynamic_bytes(syms) >= len(cdata) - 1 and dy.fixed_bytes(syms) > len(cdata)  # (zlib's header uses run symbols)


@pytest.mark.parametrize("block", [256, 4096, 65280])
def test_records(case, block):
    (bam, d), (fbam, fd) = both(case, case["header"], block)
    assert d["lines"] == fd["lines"] == expected_lines(case["bodies"][0], case["names"])
    res = dy.check_dynamic(d, bam, fd, fbam)
    print(f"block {block}: members stored / fixed / dynamic {res['btypes']}, left out {res['left_out']}; {len(bam)} bytes against {len(fbam)} fixed")
    if block >= 4096:
        assert res["btypes"][2] >= 1


@pytest.mark.parametrize("block", [64, 4096, dp.DEFAULT_BLOCK])
def test_high_bytes(empty_sample, block):
    header, span = dp.high_distinct() if block == dp.DEFAULT_BLOCK else dp.high_random()
    (bam, d), (fbam, fd) = both(empty_sample, header, block)
    res = dy.check_dynamic(d, bam, fd, fbam)
    free = dy.check_high_dynamic(res, d, header, span, block)
    sizes = sorted(m["bsize"] - 26 for _u, m, *_ in res["dynamic"])
    print(f"block {block}: {free} match-free blocks inside the payload; members stored / fixed / dynamic {res['btypes']}; dynamic cdata {sizes[:1]} .. {sizes[-1:]} bytes")


@pytest.fixture(scope="module")
def codes():
    return dp.codes_payload()


@pytest.mark.parametrize("block", [dp.DEFAULT_BLOCK, 4096])
def test_every_length_and_distance_code(empty_sample, codes, block):
    header, _span, plants = codes
    (bam, d), (fbam, fd) = both(empty_sample, header, block)
    res = dy.check_dynamic(d, bam, fd, fbam)
    len_codes, dist_codes = dy.check_plants(res, d, bam, plants) if block == dp.DEFAULT_BLOCK else dy.codes_seen(res)
    print(f"block {block}: members stored / fixed / dynamic {res['btypes']}; over the dynamic ones length codes {sorted(len_codes)}, distance codes {sorted(dist_codes)}")


@pytest.mark.parametrize("rem", dp.SHORT_REMAINDERS)
def test_short_last_member(empty_sample, rem):
    header, _span = dp.short_payload(rem)
    (bam, d), (fbam, fd) = both(empty_sample, header, dp.SHORT_BLOCK)
    res = dy.check_dynamic(d, bam, fd, fbam)
    blob = bam_export.header_blob(header)[0]
    want = [dp.SHORT_BLOCK] * 2 + ([rem] if rem else [])
    assert [len(m["payload"]) for m in d["members"][:-1]] == want and b"".join(m["payload"] for m in d["members"]) == blob
    assert res["btypes"][2] >= 2  # 16 byte values: the two whole blocks gain from a code of their own


@pytest.mark.parametrize("block,want", [HEADER_CASES[5], HEADER_CASES[-1]], ids=lambda v: str(v))
def test_header_length_against_the_records(case, block, want):
    assert {b for b, _ in HEADER_CASES} == {HEADER_CASES[5][0], HEADER_CASES[-1][0]}  # one case per block size
    header = header_of_length(case["header"], block, want)
    assert len(bam_export.header_blob(header)[0]) % block == want
    (bam, d), (fbam, fd) = both(case, header, block, sample=1)
    assert d["lines"] == fd["lines"] == expected_lines(case["bodies"][1], case["names"]) and len(d["lines"]) > 20
    dy.check_dynamic(d, bam, fd, fbam)


# ---------------------------------------------------------------------------------------------------------------------
# the builder alone
# ---------------------------------------------------------------------------------------------------------------------
def sim_lengths(counts, max_bits):
    """bam_huff_lengths through tests/hostsim/bam_huff_sim.cpp: uint32 [vectors, symbols] -> uint8 [vectors, symbols]"""
    csrc = os.path.join(HERE, "..", "mirge3.0_amd", "csrc")
    deps = [HUFF_SRC, os.path.join(csrc, "kernels_sam.hpp"), os.path.join(csrc, "kernels_bam.hpp")]
    if not os.path.exists(HUFF_SO) or os.path.getmtime(HUFF_SO) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(HUFF_SO), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-pthread", "-o", HUFF_SO, HUFF_SRC])
    sim = C.CDLL(HUFF_SO)
    counts = np.ascontiguousarray(counts, np.uint32)
    out = np.full(counts.shape, 0xEE, np.uint8)
    rc = sim.sim_huff(C.c_void_p(counts.ctypes.data), C.c_int(counts.shape[0]), C.c_int(counts.shape[1]), C.c_int(max_bits), C.c_void_p(out.ctypes.data))
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("name,max_bits,counts", dy.builder_cases(), ids=[c[0] for c in dy.builder_cases()])
def test_builder(name, max_bits, counts):
    lengths = sim_lengths(counts, max_bits)
    excess = [dy.check_lengths(c, x, max_bits) for c, x in zip(counts, lengths)]
    acted = [e for e in excess if e is not None]
    if name.startswith("fibonacci"):
        assert len(acted) == 1  # the limit acts
    print(f"{name}: {len(counts)} vectors, the limit acted on {len(acted)}; excess over package-merge: {sorted(acted)[-5:]} at most, {sum(1 for e in acted if e == 0)} optimal")


def test_bam_deflate_flag_needs_sorted_bam(tmp_path):
    from mirge3_amd.cli import parse_args
    base = ["-s", "x.fastq", "-lib", "L", "-on", "human"]
    hdr = tmp_path / "h.txt"
    hdr.write_text("@HD\tVN:1.0\n@SQ\tSN:chr1\tLN:1000\n")
    old = os.environ.get("MIRGE_BAM_DEFLATE")
    for route in ("device", "dynamic", "host"):
        assert parse_args(base + ["--sorted-bam", "--sam-header", str(hdr), "--bam-deflate", route]).bam_deflate == route
    assert parse_args(base + ["--sorted-bam", "--sam-header", str(hdr)]).bam_deflate is None
    assert os.environ.get("MIRGE_BAM_DEFLATE") == old  # parsing alone sets nothing
    for bad in (["--bam-deflate", "dynamic"], ["--bam-deflate", "dynamic", "--sam-out"], ["--sorted-bam", "--sam-header", str(hdr), "--bam-deflate", "fast"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
