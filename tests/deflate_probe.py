"""Payloads for the BAM deflate (``k_bam_blocks``, csrc/kernels_bam.hpp) that BAM records cannot produce, and what the tests read off
the members it writes: shared by tests/test_bam_deflate_hostsim.py (the kernel compiled for the host) and tests/test_bam_deflate_gpu.py.

The ``--sam-header`` file goes verbatim into the front of the uncompressed stream and only its ``@SQ`` lines are parsed, so an ``@CO``
line carries arbitrary bytes into the deflate; a sample without counts selects no rows, and the stream is the header alone.  Every
builder is seeded and returns ``(header file, (lo, hi))``: ``header_blob(header)[0][lo:hi]`` is the payload.  No payload holds the byte
``@`` (so no ``\\n@SQ`` either).

``fixed_symbols`` decodes a fixed-Huffman block into its symbols (RFC 1951, 3.2.5 and 3.2.6) -- only so that a test can prove which
codes a payload really exercised: whether the bytes are right stays with ``zlib`` and the CRC-32 in ``bam_reader.read_bgzf``."""
import struct

import numpy as np

from mirge3_amd import bam_export

import bam_reader

DEFAULT_BLOCK = bam_export.BLOCK_BYTES
THREADS = 256   # of a workgroup of k_bam_blocks: a block's segment is ceil(n / THREADS) bytes
HALF = 1 << 15  # a match's source lies in the same 32 KiB half of the block
MIN_MATCH = 4

FRONT = b"@HD\tVN:1.0\n@SQ\tSN:chr1\tLN:1000\n@CO\t"
N_REF = 1

# RFC 1951, 3.2.5: length codes 257..285 and distance codes 0..29: base value, extra bits
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
# what the kernel's parse can reach at the default block size: a segment is ceil(65280 / 256) = 255 bytes and a match ends with its
# segment, so no match is longer than 255 (never code 285 = 258 bytes); none is shorter than MIN_MATCH = 4 (never code 257 = 3 bytes)
REACHABLE_LEN_CODES = set(range(258, 285))
REACHABLE_DIST_CODES = set(range(30))


# ---------------------------------------------------------------------------------------------------------------------
# the symbol decoder
# ---------------------------------------------------------------------------------------------------------------------
def fixed_symbols(cdata):
    """the symbols of ONE final fixed-Huffman block that fills cdata: literals as int, matches as (length, distance, length code,
    distance code); the end-of-block symbol is checked and not returned"""
    stream = np.unpackbits(np.frombuffer(bytes(cdata), dtype=np.uint8), bitorder="little").tolist()  # bit k of the stream
    nbits = len(stream)
    at = 0

    def bits(n):  # a field other than a Huffman code: least significant bit first
        nonlocal at
        assert at + n <= nbits, "the block runs past cdata"
        v = 0
        for k in range(n):
            v |= stream[at + k] << k
        at += n
        return v

    def code(n, c=0):  # a Huffman code: most significant bit first
        nonlocal at
        assert at + n <= nbits, "the block runs past cdata"
        for k in range(n):
            c = (c << 1) | stream[at + k]
        at += n
        return c

    assert bits(1) == 1 and bits(2) == 1, "not a final block with BTYPE 01"
    out = []
    while True:
        c = code(7)
        if c <= 0b0010111:
            sym = 256 + c
        else:
            c = code(1, c)
            if 0b00110000 <= c <= 0b10111111:
                sym = c - 0b00110000
            elif 0b11000000 <= c <= 0b11000111:
                sym = 280 + c - 0b11000000
            else:
                c = code(1, c)
                assert 0b110010000 <= c <= 0b111111111
                sym = 144 + c - 0b110010000
        if sym < 256:
            out.append(sym)
            continue
        if sym == 256:
            break
        assert sym <= 285, f"length code {sym}"
        length = LEN_BASE[sym - 257] + bits(LEN_EXTRA[sym - 257])
        dc = code(5)
        assert dc <= 29, f"distance code {dc}"
        out.append((length, DIST_BASE[dc] + bits(DIST_EXTRA[dc]), sym, dc))
    assert nbits - at < 8 and not any(stream[at:]), "bits behind the end-of-block code"
    return out


def expand(symbols):
    """the bytes the symbols stand for"""
    out = bytearray()
    for s in symbols:
        if isinstance(s, int):
            out.append(s)
        else:
            length, dist = s[0], s[1]
            assert 1 <= dist <= len(out)
            for _ in range(length):
                out.append(out[-dist])
    return bytes(out)


def matches_at(symbols):
    """{position in the block: (length, distance)} of the block's matches"""
    out, at = {}, 0
    for s in symbols:
        if isinstance(s, int):
            at += 1
        else:
            out[at] = (s[0], s[1])
            at += s[0]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the header file around a payload
# ---------------------------------------------------------------------------------------------------------------------
def payload_start(pad=0):
    return 8 + len(bam_export.header_text(FRONT)) + pad


def pad_to(align):
    """filler bytes in front of the payload so that it starts on a multiple of align"""
    return -payload_start() % align


def header_file(payload, pad=0):
    assert b"@" not in payload
    header = FRONT + b"x" * pad + bytes(payload) + b"\n"
    lo = payload_start(pad)
    blob, refs = bam_export.header_blob(header)
    assert blob[lo:lo + len(payload)] == payload and len(refs) == N_REF
    return header, (lo, lo + len(payload))


def tail_bytes():
    """bytes of the stream behind a payload: the newline, n_ref, the reference"""
    return len(bam_export.header_blob(header_file(b"")[0])[0]) - payload_start()


class Fresh:
    """bytes of an alphabet such that no 4-gram of all it has written (across what others put between) comes twice, and no byte
    follows itself"""
    def __init__(self, rng, alphabet):
        self.rng, self.alphabet, self.seen = rng, np.asarray([a for a in alphabet if a != 0x40], dtype=np.uint8), set()

    def fill(self, out, n, avoid=None):
        """n more bytes onto bytearray out; the first of them is none of `avoid`"""
        need, avoid = n, set(avoid or ())
        while need > 0:
            for b in self.alphabet[self.rng.integers(0, len(self.alphabet), size=2 * need + 8)].tolist():
                if (out and out[-1] == b) or b in avoid:
                    continue
                if len(out) >= 3:
                    g = bytes(out[-3:]) + bytes([b])
                    if g in self.seen:
                        continue
                    self.seen.add(g)
                out.append(b)
                avoid = ()
                need -= 1
                if need == 0:
                    break


def block_is_match_free(stream, lo, hi):
    """the block stream[lo:hi] holds no 4-gram twice inside one 32 KiB half and no 4 equal bytes in a row: the kernel's parse (first
    position with the same hash in the same half, or the byte in front) can then emit only literals"""
    b = np.frombuffer(bytes(stream[lo:hi]), dtype=np.uint8)
    if b.size < MIN_MATCH:
        return True
    g = b[:-3].astype(np.uint32) | (b[1:-2].astype(np.uint32) << 8) | (b[2:-1].astype(np.uint32) << 16) | (b[3:].astype(np.uint32) << 24)
    if np.any((b[:-3] == b[1:-2]) & (b[1:-2] == b[2:-1]) & (b[2:-1] == b[3:])):
        return False
    return all(np.unique(g[h:h + HALF]).size == g[h:h + HALF].size for h in range(0, g.size, HALF))


# ---------------------------------------------------------------------------------------------------------------------
# a. high bytes: nothing to gain, every literal costs 9 bits
# ---------------------------------------------------------------------------------------------------------------------
HIGH_BYTES = 200_000


def high_random(seed=7104, n=HIGH_BYTES):
    rng = np.random.Generator(np.random.PCG64(seed))
    return header_file(rng.integers(144, 256, size=n, dtype=np.uint8).tobytes())


def high_distinct(seed=7102, n=HIGH_BYTES):
    """random 4-grams over 112 values repeat a few times per 32 KiB half, so at the default block size next to no block would pass
    block_is_match_free: here no 4-gram comes twice in the whole payload"""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = bytearray()
    Fresh(rng, range(144, 256)).fill(out, n)
    return header_file(bytes(out))


# ---------------------------------------------------------------------------------------------------------------------
# b. the decision's edge: blocks of 64 distinct bytes, h of them 144 and above
# ---------------------------------------------------------------------------------------------------------------------
EDGE_BLOCK = 64
EDGE_H = (0, 21, 22, 23, 24, 64)


def edge_payload(h, seed=7200, n_blocks=6):
    """n_blocks blocks of 64 distinct values (no 4-gram twice, no run), exactly h of them >= 144: without a match the fixed form has
    3 + 8 * 64 + h + 7 bits"""
    rng = np.random.Generator(np.random.PCG64(seed + h))
    low = np.asarray([v for v in range(144) if v != 0x40], dtype=np.uint8)
    high = np.arange(144, 256, dtype=np.uint8)
    out = bytearray()
    for _ in range(n_blocks):
        blk = rng.permutation(low)[:EDGE_BLOCK].copy()
        blk[rng.permutation(EDGE_BLOCK)[:h]] = rng.permutation(high)[:h]
        assert len(set(blk.tolist())) == EDGE_BLOCK and int((blk >= 144).sum()) == h
        out += blk.tobytes()
    return header_file(bytes(out), pad=pad_to(EDGE_BLOCK))


# ---------------------------------------------------------------------------------------------------------------------
# c. every code the parse can reach
# ---------------------------------------------------------------------------------------------------------------------
def _lo_hi(base, extra, codes):
    return [v for c in codes for v in (base[c], base[c] + (1 << extra[c]) - 1)]


def codes_payload(seed=7300):
    """Laid out for the default block size, where block 0's coordinates are the stream's and a segment is 255 bytes:
    - half 0: periodic stretches of period d for the least and the greatest distance of codes 0..15 (d = 1..256).  A 4-gram's source is
      the FIRST position of the half with its hash, so a stretch's first 4-grams may find another source's bucket taken and go out as
      literals; the next position tries again, and every match inside the stretch has distance d.
    - half 1 opens with a dictionary D of 256 bytes: its first 4-gram is the first position of the half, so it owns its bucket whatever
      the hash.  Copies D[:len] are planted at 32768 + dist for the least distance of codes 16..29 and one near the greatest (len 4; the next code's
      copy needs the room), and, between
      those, for the least and the greatest length of every length code 258..284; each is followed by a byte that is not D[len] and lies
      inside one segment, so the parse must emit exactly (len, dist) there: `plants` = {position: (len, dist)}.
    Everything else is filler without a repeated 4-gram, one byte in twenty of it 144 or above.
    -> (header file, (lo, hi), plants)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    seg = -(-DEFAULT_BLOCK // THREADS)
    fresh = Fresh(rng, [v for v in range(144) for _ in range(15)] + list(range(144, 256)))
    lo = payload_start()
    out = bytearray(bam_export.header_blob(header_file(b"")[0])[0][:lo])  # (l_text is not yet the final one: it plays no part)
    fresh.fill(out, seg - len(out))
    for d in [1, 2, 3, 4] + _lo_hi(DIST_BASE, DIST_EXTRA, range(4, 16)):
        unit = bytearray()
        fresh.fill(unit, d, avoid=[out[-1]])
        reps = bytes(unit) * (3 + 28 // d)
        out += reps[:d + max(d, 28)]
        fresh.fill(out, 3, avoid=[reps[d + max(d, 28)]])
    assert len(out) < HALF - 4
    fresh.fill(out, HALF - len(out))
    D = bytearray()
    fresh.fill(D, 256, avoid=[out[-1]])
    plan = {}
    for c in range(16, 30):
        for dist, step in ((DIST_BASE[c], 1), (min(DIST_BASE[c] + (1 << DIST_EXTRA[c]) - 8, DEFAULT_BLOCK - HALF - MIN_MATCH - 2), -1)):
            while (HALF + dist) % seg + MIN_MATCH > seg:  # the copy must lie inside one segment
                dist += step
            plan[HALF + dist] = MIN_MATCH
    at = HALF + len(D) + 1
    for length in _lo_hi(LEN_BASE, LEN_EXTRA, range(1, 28)):
        length = min(length, seg)
        while at % seg + length > seg or any(p - length - 2 < at < p + n + 2 for p, n in plan.items()):
            at += 1
        plan[at] = length
        at += length + 2
    assert at < DEFAULT_BLOCK - 2
    out += D
    plants, before = {}, {D[0]}
    for pos in sorted(plan):
        n = plan[pos]
        fresh.fill(out, pos - 1 - len(out))
        fresh.fill(out, 1, avoid=before)  # (the byte in front differs from copy to copy: no match may begin one byte early)
        before.add(out[-1])
        assert len(out) == pos and pos // seg == (pos + n - 1) // seg and pos // HALF == 1
        out += D[:n]
        fresh.fill(out, 1, avoid=[D[n]])
        plants[pos] = (n, pos - HALF)
    fresh.fill(out, DEFAULT_BLOCK + 50 - len(out))
    header, (lo2, hi) = header_file(bytes(out[lo:]))
    assert lo2 == lo
    return header, (lo, hi), plants


# ---------------------------------------------------------------------------------------------------------------------
# d. short last members
# ---------------------------------------------------------------------------------------------------------------------
SHORT_BLOCK = 4096
SHORT_REMAINDERS = (0, 1, 2, 3, 4, 5, 255, 256, 257)


def short_payload(rem, seed=7400):
    """a stream of two blocks of 4096 bytes and rem more: 16 byte values at random, so that matches of every kind occur"""
    rng = np.random.Generator(np.random.PCG64(seed + rem))
    n = 2 * SHORT_BLOCK + rem - payload_start() - tail_bytes()
    alphabet = np.asarray([1, 9, 32, 48, 65, 66, 97, 122, 127, 143, 144, 145, 200, 254, 255, 0], dtype=np.uint8)
    return header_file(alphabet[rng.integers(0, 16, size=n)].tobytes())


# ---------------------------------------------------------------------------------------------------------------------
# what every file must satisfy, and every family's own demands; d = bam_reader.decode_bam(file)
# ---------------------------------------------------------------------------------------------------------------------
def check_members(d, header, block):
    """-> [(stream offset, member)]: the payloads are the header blob cut into blocks, every member is one final deflate block, stored
    or fixed, and never larger than the stored form (18 header + 5 + n + 8 trailer bytes)"""
    blob, refs = bam_export.header_blob(header)
    body = d["members"][:-1]
    assert b"".join(m["payload"] for m in body) == blob and not d["lines"] and len(d["refs"]) == len(refs)
    assert [len(m["payload"]) for m in body] == [min(block, len(blob) - u) for u in range(0, len(blob), block)]
    out, u = [], 0
    for m in body:
        n = len(m["payload"])
        assert m["single"] and m["btype"] in (0, 1), (u, m["btype"])
        assert m["bsize"] <= n + 31, (u, m["bsize"], n)
        if m["btype"] == 0:
            assert m["bsize"] == n + 31, (u, m["bsize"], n)
        out.append((u, m))
        u += n
    return out


def cdata_of(bam, m):
    return bam[m["at"] + 18:m["at"] + m["bsize"] - 8]


def check_high(d, bam, header, span, block, max_excluded=0.05):
    """every block wholly inside the payload that the scan calls match-free is stored; the scan excludes at most 5 % of them"""
    blob = bam_export.header_blob(header)[0]
    inside = [(u, m) for u, m in check_members(d, header, block) if span[0] <= u and u + block <= span[1]]
    assert len(inside) >= (span[1] - span[0]) // block - 1
    free = [(u, m) for u, m in inside if block_is_match_free(blob, u, u + block)]
    assert len(inside) - len(free) <= max_excluded * len(inside), (len(free), len(inside))
    for u, m in free:
        assert m["btype"] == 0 and m["single"] and m["bsize"] == block + 31, (u, m["btype"], m["bsize"])
    return len(free), len(inside)


def check_edge(d, bam, header, span, h):
    """n = 64 literals and no match: 8 n + h + 10 bits.  (8 n + h + 17) // 8 bytes >= n + 5 exactly when h >= 23"""
    n = EDGE_BLOCK
    blob = bam_export.header_blob(header)[0]
    inside = [(u, m) for u, m in check_members(d, header, n) if span[0] <= u and u + n <= span[1]]
    assert len(inside) == (span[1] - span[0]) // n >= 4 and span[0] % n == 0
    for u, m in inside:
        assert block_is_match_free(blob, u, u + n) and sum(v >= 144 for v in blob[u:u + n]) == h
        if h <= 22:
            assert m["btype"] == 1 and m["bsize"] == 26 + (8 * n + h + 17) // 8, (u, m["btype"], m["bsize"])
            syms = fixed_symbols(cdata_of(bam, m))
            assert len(syms) == n and all(isinstance(s, int) for s in syms) and bytes(syms) == blob[u:u + n]
        else:
            assert m["btype"] == 0 and m["bsize"] == n + 31, (u, m["btype"], m["bsize"])


def check_codes(d, bam, header, plants, block):
    """-> (length codes, distance codes) of all BTYPE-01 members; at the default block size every planted copy is one match of exactly
    its length and distance, and the codes seen are exactly the reachable ones"""
    len_codes, dist_codes = set(), set()
    for u, m in check_members(d, header, block):
        if m["btype"] != 1:
            continue
        syms = fixed_symbols(cdata_of(bam, m))
        assert expand(syms) == m["payload"]
        len_codes |= {s[2] for s in syms if not isinstance(s, int)}
        dist_codes |= {s[3] for s in syms if not isinstance(s, int)}
        if block == DEFAULT_BLOCK and u == 0:
            got = matches_at(syms)
            assert {p: got.get(p) for p in plants} == plants
            assert any(isinstance(s, int) and s >= 144 for s in syms)
    if block == DEFAULT_BLOCK:
        # 257 (3 bytes: below MIN_MATCH) and 285 (258 bytes: longer than a segment of 255) are the two length codes the parse cannot emit
        assert len_codes == REACHABLE_LEN_CODES, sorted(REACHABLE_LEN_CODES ^ len_codes)
        assert dist_codes == REACHABLE_DIST_CODES, sorted(REACHABLE_DIST_CODES ^ dist_codes)
    return len_codes, dist_codes


def check_short(d, bam, header, rem):
    members = check_members(d, header, SHORT_BLOCK)
    blob = bam_export.header_blob(header)[0]
    assert len(blob) % SHORT_BLOCK == rem and len(blob) // SHORT_BLOCK == 2
    if rem == 0:
        assert [len(m["payload"]) for _, m in members] == [SHORT_BLOCK] * 2  # no short member
    else:
        assert [len(m["payload"]) for _, m in members] == [SHORT_BLOCK] * 2 + [rem]
        u, m = members[-1]
        assert m["payload"] == blob[-rem:]
        if m["btype"] == 1:
            syms = fixed_symbols(cdata_of(bam, m))
            assert expand(syms) == m["payload"]
            if rem < MIN_MATCH:  # never hashed: literals only
                assert all(isinstance(s, int) for s in syms)
    assert struct.unpack_from("<i", blob, len(blob) - tail_bytes() + 1)[0] == N_REF
    return members


EMPTY_BAI = bam_reader.build_bai(N_REF, [])
