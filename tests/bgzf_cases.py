"""The streams of the ``--bgzf-out`` tests (tests/test_bgzf.py, test_bgzf_hostsim.py, test_bgzf_gpu.py): ``name -> (S, B)``, and the checks
a file of the device kernel -- compiled for the host or run on the GPU -- has to pass (mirge3_amd/bgzf.py is the specification)."""
import functools
import gzip
import os

import numpy as np

import mirge3_amd  # noqa: F401
from mirge3_amd import bam_export, bgzf

import deflate_dyn_probe as dy
import deflate_probe as dp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sam_out")


def _text(rng, n):
    """n bytes that look like the exporters' text: tab-separated fields of letters and digits in lines"""
    out = bytearray()
    while len(out) < n:
        out += b"chr%d\t%d\t%d\t%d\n" % (rng.integers(1, 23), rng.integers(1, 10 ** 8), rng.integers(1, 10 ** 8), rng.integers(1, 999))
    return bytes(out[:n])


def no_repeated_4mer():
    """259 letters over ACGT in which every 4-mer occurs once: a de Bruijn sequence B(4, 4), unrolled"""
    k, n = 4, 4
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    s = "".join("ACGT"[x] for x in seq)
    s += s[:3]
    assert len(s) == 259 and len({s[i:i + 4] for i in range(256)}) == 256
    return s.encode()


@functools.lru_cache(maxsize=None)
def all_cases():
    from test_coverage import golden_bedgraph
    rng = np.random.Generator(np.random.PCG64(9101))
    cases = {}
    for n in (0, 1, 3, 255, 256, 257):          # segments of zero and one byte, threads without work
        cases[f"text{n}_b256"] = (_text(rng, n), 256)
    for n in (256, 257, 511):                    # exactly B, B + 1, 2 B - 1
        cases[f"blocks{n}_b256"] = (_text(rng, n), 256)
    cases["one_letter_b65280"] = (b"A" * 65280, 65280)   # a literal tree of two symbols, a distance tree of one
    cases["no_match_b4096"] = (no_repeated_4mer(), 4096)  # an empty distance tree; the dynamic form has to win
    cases["random_b4096"] = (rng.integers(0, 256, size=4096, dtype=np.uint8).tobytes(), 4096)  # stored
    cases["high_bytes_b1024"] = (rng.integers(144, 256, size=3000, dtype=np.uint8).tobytes(), 1024)  # the 9-bit fixed literals
    header, _span, _plants = dp.codes_payload()
    cases["codes_b65280"] = (bam_export.header_blob(header)[0], 65280)  # every length and distance code
    with open(os.path.join(GOLDEN, "S2.sam"), "rb") as fh:
        sam2 = fh.read()
    with open(os.path.join(GOLDEN, "S1.sam"), "rb") as fh:
        sam1 = fh.read()
    plus, minus = golden_bedgraph("S1", True)
    for b in (256, 4096):                        # boundaries inside numbers, names and a row's copies
        cases[f"sam_S2_b{b}"] = (sam2, b)
        cases[f"bedgraph_plus_b{b}"] = (plus, b)
        cases[f"bedgraph_minus_b{b}"] = (minus, b)
    cases["bedgraph_plus_b64"] = (plus, 64)     # (the golden bedGraph files are shorter than 256 bytes: boundaries at 64 as well)
    cases["bedgraph_minus_b64"] = (minus, 64)
    cases["sam_S1_b4096"] = (sam1, 4096)
    return cases


def check_device_file(s, block, gz, gzi, stats=None):
    """Everything the specification says of a file the device kernel wrote; -> [members stored, fixed, dynamic]"""
    assert gzip.decompress(gz) == s
    ms = bgzf.check_index(gz, gzi)  # (magic, BC, BSIZE, CRC-32, ISIZE, the EOF block; every .gzi pair on its member)
    assert len(ms) == (len(s) + block - 1) // block
    if not s:
        assert gz == bgzf.EOF_BLOCK and gzi == bytes(8)
    btypes, left_out = [0, 0, 0], 0
    for b, m in enumerate(ms):
        part = s[b * block:(b + 1) * block]
        n = len(part)
        assert m["payload"] == part and m["single"] and m["btype"] in (0, 1, 2), b
        assert m["bsize"] <= n + 31, (b, m["bsize"], n)
        btypes[m["btype"]] += 1
        cdata = gz[m["offset"] + 18:m["offset"] + m["bsize"] - 8]
        clen = len(cdata)
        if m["btype"] == 2:
            syms, _ll, _dd, _cl = dy.dynamic_symbols(cdata)
            assert dp.expand(syms) == part, b
            assert clen < dy.fixed_bytes(syms) and clen < n + 5, (b, clen, dy.fixed_bytes(syms), n + 5)
        else:
            syms = dp.fixed_symbols(cdata) if m["btype"] == 1 else list(part)
            if m["btype"] == 1:
                assert dp.expand(syms) == part and clen == dy.fixed_bytes(syms) and clen < n + 5, b
            else:
                assert clen == n + 5
            # the kernel's dynamic header is never longer than the crude coder's (no run symbols, all 19 code-length codes), so a
            # member that did not take the dynamic form is no larger than the crude dynamic form of its own symbols
            crude = dy.crude_dynamic_bytes(syms)
            if crude is None:
                left_out += 1
            else:
                assert crude >= clen, f"block {b}: BTYPE {m['btype']} of {clen} bytes, a crude dynamic form takes {crude}"
    assert left_out <= 0.05 * len(ms), (left_out, len(ms))  # (blocks whose crude trees do not fit 15 bits: deflate_dyn_probe.check_dynamic's bound)
    if stats is not None:
        assert [stats["stored"], stats["fixed"], stats["dynamic"]] == btypes and stats["members"] == len(ms)
        assert stats["file_bytes"] == len(gz) and stats["stream_bytes"] == len(s)
    return btypes
