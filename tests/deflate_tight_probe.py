"""What the tests of ``MIRGE_BAM_DEFLATE=tight`` (``k_bam_blocks`` with ``deflate == 3``, csrc/kernels_bam.hpp) read off its members: shared by
tests/test_bam_tight_hostsim.py (the kernels compiled for the host) and tests/test_bam_tight_gpu.py.  The tight route keeps the blocks of
the other routes and parses them anew, so a file is held against the STREAM (the payloads of the default route's members), never
against another route's tokens: every member is one final deflate block no larger than its stored form whose symbols -- read with
``deflate_probe.fixed_symbols`` or ``deflate_dyn_probe.dynamic_symbols`` by BTYPE -- expand to its payload, no match longer than 258 or
further than 32 768."""
import numpy as np

import deflate_dyn_probe as dy
import deflate_probe as dp

MAX_MATCH = 258
MAX_DIST = 32768


def symbols_of(bam, m):
    """the symbols of member m (a dict of bam_reader): literals as int, matches as tuples that start (length, distance)"""
    if m["btype"] == 0:
        return list(m["payload"])
    cdata = dp.cdata_of(bam, m)
    return dp.fixed_symbols(cdata) if m["btype"] == 1 else dy.dynamic_symbols(cdata)[0]


def matches_of(symbols):
    """[(position in the block, length, distance)]"""
    out, at = [], 0
    for s in symbols:
        if isinstance(s, int):
            at += 1
        else:
            out.append((at, s[0], s[1]))
            at += s[0]
    return out


def check_tight(d, bam, d_ref):
    """-> [(stream offset, member, symbols)] of a tight file (d = bam_reader.decode_bam(bam), which has checked every BSIZE, CRC-32 and
    ISIZE) against d_ref, the decoded file of another route on the same stream"""
    mt, mr = d["members"][:-1], d_ref["members"][:-1]
    assert [m["payload"] for m in mt] == [m["payload"] for m in mr], "the stream or the block boundaries differ"
    out, u = [], 0
    for m in mt:
        n = len(m["payload"])
        assert m["single"] and m["btype"] in (0, 1, 2)
        assert m["bsize"] <= n + 5 + 26, f"block at {u}: {m['bsize']} bytes, stored {n + 31}"
        syms = symbols_of(bam, m)
        assert dp.expand(syms) == m["payload"], f"block at {u}"
        for at, length, dist in matches_of(syms):
            assert 3 <= length <= MAX_MATCH and 1 <= dist <= min(MAX_DIST, at), (u, at, length, dist)
        out.append((u, m, syms))
        u += n
    return out


def btypes(members):
    return [sum(1 for _u, m, _s in members if m["btype"] == b) for b in range(3)]


def crossing_matches(symbols, n):
    """the matches that cover a multiple of a thread's segment, ceil(n / 256) bytes, strictly inside themselves"""
    seg = -(-n // dp.THREADS)
    return [(at, length, dist) for at, length, dist in matches_of(symbols) if (at + length - 1) // seg * seg > at]


# ---------------------------------------------------------------------------------------------------------------------
# payloads
# ---------------------------------------------------------------------------------------------------------------------
def repeated_unit(seed=7500, unit=700, n=150_000):
    """one random unit over and over: every match's source lies a multiple of `unit` in front, and nothing ends it but its limit"""
    rng = np.random.Generator(np.random.PCG64(seed))
    alphabet = np.asarray([b for b in range(1, 256) if b not in b"@\n\r\t"], dtype=np.uint8)
    u = alphabet[rng.integers(0, alphabet.size, size=unit)].tobytes()
    return dp.header_file((u * (n // unit + 1))[:n])


def equal_bytes(n, block, value=b"Q"):
    """a payload of n equal bytes that starts with a block of `block` bytes"""
    header, (lo, hi) = dp.header_file(value * n, pad=dp.pad_to(block))
    assert lo % block == 0
    return header, (lo, hi)
