"""What the tests of ``MIRGE_BAM_DEFLATE=dynamic`` (``k_bam_blocks`` with ``deflate == 2``, csrc/kernels_bam.hpp) read off its members and
off its code-length builder: shared by tests/test_bam_dynamic_hostsim.py (the kernels compiled for the host) and
tests/test_bam_dynamic_gpu.py.  Written from RFC 1951; nothing here imports or restates the product's builder.

- ``dynamic_symbols`` decodes one final dynamic-Huffman block (3.2.7) into the symbols ``deflate_probe.fixed_symbols`` returns, plus the
  three tables of code lengths it was sent with.  A code must be complete; the one exception is the RFC's: a distance code of a single
  code of length 1.
- ``crude_dynamic_bytes`` is the tests' own dynamic coder, good enough to catch a decision that leaves bytes on the table: plain
  ``heapq`` Huffman lengths, a header without run symbols and with all 19 three-bit entries.  ``fixed_bytes``: the same symbols under
  the fixed code.
- ``check_dynamic`` holds the assertions every file of the dynamic route must satisfy against the file of the fixed route.
- ``check_lengths`` holds the assertions on one vector of the builder's code lengths; ``BUILDER_CASES`` are the issue's inputs."""
import heapq

import numpy as np

import deflate_probe as dp

CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
N_LL, N_D, N_CL = 286, 30, 19


# ---------------------------------------------------------------------------------------------------------------------
# the decoder
# ---------------------------------------------------------------------------------------------------------------------
def kraft(lengths, max_bits=15):
    """the Kraft sum of the nonzero lengths in units of 2^-max_bits"""
    return sum(1 << (max_bits - n) for n in lengths if n)


def _decoder(lengths, what):
    """{(length, code): symbol} of the canonical code (RFC 1951, 3.2.2); complete, or -- distances only -- one code of length 1"""
    used = [n for n in lengths if n]
    assert used and max(used) <= 15, what
    k = kraft(lengths)
    if k != 1 << 15:
        assert what == "distance" and used == [1], f"{what} code: Kraft sum {k} / 32768 with lengths {sorted(used)}"
    bl = [0] * 17
    for n in used:
        bl[n] += 1
    code, nxt = 0, [0] * 17
    for n in range(1, 16):
        code = (code + bl[n - 1]) << 1
        nxt[n] = code
    table = {}
    for sym, n in enumerate(lengths):
        if n:
            table[(n, nxt[n])] = sym
            nxt[n] += 1
    return table


def dynamic_symbols(cdata):
    """the symbols of ONE final dynamic-Huffman block that fills cdata, as fixed_symbols gives them (literals as int, matches as
    (length, distance, length code, distance code); the end-of-block symbol checked and not returned)
    -> (symbols, the 286 literal/length code lengths, the 30 distance code lengths, the 19 code-length code lengths)"""
    stream = np.unpackbits(np.frombuffer(bytes(cdata), dtype=np.uint8), bitorder="little").tolist()
    nbits = len(stream)
    at = 0

    def bits(n):
        nonlocal at
        assert at + n <= nbits, "the block runs past cdata"
        v = 0
        for k in range(n):
            v |= stream[at + k] << k
        at += n
        return v

    def sym_of(table):
        nonlocal at
        c = 0
        for n in range(1, 16):
            assert at < nbits, "the block runs past cdata"
            c = (c << 1) | stream[at]
            at += 1
            if (n, c) in table:
                return table[(n, c)]
        raise AssertionError("no code of up to 15 bits")

    assert bits(1) == 1 and bits(2) == 2, "not a final block with BTYPE 10"
    hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
    assert hlit <= N_LL and hdist <= N_D, (hlit, hdist)
    cl = [0] * N_CL
    for k in range(hclen):
        cl[CL_ORDER[k]] = bits(3)
    cl_table = _decoder(cl, "code-length")
    seq = []
    while len(seq) < hlit + hdist:
        s = sym_of(cl_table)
        if s < 16:
            seq.append(s)
        elif s == 16:
            assert seq, "a repeat with nothing in front"
            seq += [seq[-1]] * (3 + bits(2))
        else:
            seq += [0] * (3 + bits(3) if s == 17 else 11 + bits(7))
    assert len(seq) == hlit + hdist, "a run past HLIT + HDIST"
    ll = seq[:hlit] + [0] * (N_LL - hlit)
    dd = seq[hlit:] + [0] * (N_D - hdist)
    assert ll[256], "no end-of-block code"
    ll_table, d_table = _decoder(ll, "literal/length"), _decoder(dd, "distance")
    out = []
    while True:
        sym = sym_of(ll_table)
        if sym < 256:
            out.append(sym)
            continue
        if sym == 256:
            break
        length = dp.LEN_BASE[sym - 257] + bits(dp.LEN_EXTRA[sym - 257])
        dc = sym_of(d_table)
        out.append((length, dp.DIST_BASE[dc] + bits(dp.DIST_EXTRA[dc]), sym, dc))
    assert nbits - at < 8 and not any(stream[at:]), "bits behind the end-of-block code"
    return out, ll, dd, cl


# ---------------------------------------------------------------------------------------------------------------------
# the tests' own coders: sizes only
# ---------------------------------------------------------------------------------------------------------------------
def huffman_lengths(counts):
    """plain heapq Huffman: {symbol: length} of the symbols with a count; one symbol alone gets length 1"""
    heap = [(int(c), s, (s,)) for s, c in enumerate(counts) if c]
    if len(heap) == 1:
        return {heap[0][1]: 1}
    heapq.heapify(heap)
    depth = {s: 0 for _, s, _ in heap}
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    return depth


def package_merge_cost(counts, max_bits):
    """the least sum count * length of a prefix code with no length above max_bits (Larmore and Hirschberg's package-merge)"""
    leaves = sorted((int(c), s) for s, c in enumerate(counts) if c)
    n = len(leaves)
    if n == 1:
        return leaves[0][0]
    assert n <= 1 << max_bits
    unit = [(c, np.bincount([k], minlength=n)) for k, (c, _) in enumerate(leaves)]
    items = list(unit)
    for _ in range(max_bits - 1):
        pairs = [(items[k][0] + items[k + 1][0], items[k][1] + items[k + 1][1]) for k in range(0, len(items) - 1, 2)]
        items = sorted(unit + pairs, key=lambda x: x[0])
    length = sum(v for _, v in items[:2 * n - 2])
    assert sum(1 << (max_bits - int(x)) for x in length) == 1 << max_bits
    return int(sum(int(x) * c for x, (c, _) in zip(length, leaves)))


def symbol_counts(symbols):
    ll, dd, extra = [0] * N_LL, [0] * N_D, 0
    for s in symbols:
        if isinstance(s, int):
            ll[s] += 1
        else:
            ll[s[2]] += 1
            dd[s[3]] += 1
            extra += dp.LEN_EXTRA[s[2] - 257] + dp.DIST_EXTRA[s[3]]
    ll[256] = 1
    return ll, dd, extra


def fixed_bytes(symbols):
    """the bytes of the symbols as one final fixed-Huffman block"""
    ll, dd, extra = symbol_counts(symbols)
    bits = 3 + extra + 5 * sum(dd)
    bits += sum(c * (8 if s < 144 else 9 if s < 256 else 7 if s < 280 else 8) for s, c in enumerate(ll))
    return (bits + 7) // 8


def crude_dynamic_bytes(symbols):
    """the bytes of the symbols as one final dynamic block of the tests' crude coder, or None where its plain Huffman trees do not fit
    15 bits (7 for the code-length code).  A block without a match sends one distance code of length 1."""
    ll, dd, extra = symbol_counts(symbols)
    ll_len, d_len = huffman_lengths(ll), huffman_lengths(dd if any(dd) else [1])
    if max(ll_len.values()) > 15 or max(d_len.values()) > 15:
        return None
    hlit = max(max(ll_len) + 1, 257)
    hdist = max(d_len) + 1
    seq = [ll_len.get(s, 0) for s in range(hlit)] + [d_len.get(s, 0) for s in range(hdist)]
    cl_len = huffman_lengths(np.bincount(seq, minlength=N_CL))
    if max(cl_len.values()) > 7:
        return None
    bits = 3 + 14 + 3 * N_CL + sum(cl_len[v] for v in seq) + extra
    bits += sum(c * ll_len[s] for s, c in enumerate(ll) if c) + sum(c * d_len[s] for s, c in enumerate(dd) if c)
    return (bits + 7) // 8


# ---------------------------------------------------------------------------------------------------------------------
# a file of the dynamic route against the file of the fixed route on the same stream
# ---------------------------------------------------------------------------------------------------------------------
def check_dynamic(d_dyn, bam_dyn, d_fix, bam_fix, max_left_out=0.05):
    """-> dict(btypes = [members per BTYPE 0, 1, 2], dynamic = [(stream offset, member, symbols, ll, dd, cl)], left_out).
    Member for member: the same payload; one final block of type 0, 1 or 2; never larger than under the fixed route.  A BTYPE 2 member
    decodes to the fixed member's own symbols (the parse is shared) and to the payload, and is smaller than both n + 5 and its symbols
    under the fixed code.  A member that is not BTYPE 2 is no larger than the crude dynamic form of its symbols (all literals for a
    stored one); blocks whose crude trees do not fit are left out, at most 5 % of all."""
    dyn, fix = d_dyn["members"][:-1], d_fix["members"][:-1]
    assert [m["payload"] for m in dyn] == [m["payload"] for m in fix]
    btypes, out, left_out, u = [0, 0, 0], [], 0, 0
    for md, mf in zip(dyn, fix):
        n = len(md["payload"])
        assert md["single"] and md["btype"] in (0, 1, 2), (u, md["btype"])
        assert md["bsize"] <= mf["bsize"] <= n + 31, (u, md["bsize"], mf["bsize"])
        btypes[md["btype"]] += 1
        clen = md["bsize"] - 26
        if md["btype"] == 2:
            syms, ll, dd, cl = dynamic_symbols(dp.cdata_of(bam_dyn, md))
            assert dp.expand(syms) == md["payload"], u
            if mf["btype"] == 1:
                assert syms == dp.fixed_symbols(dp.cdata_of(bam_fix, mf)), u
            assert clen < n + 5 and clen < fixed_bytes(syms), (u, clen, n + 5, fixed_bytes(syms))
            assert md["bsize"] < mf["bsize"], (u, md["bsize"], mf["bsize"])
            out.append((u, md, syms, ll, dd, cl))
        else:
            assert md["btype"] == mf["btype"] and md["bsize"] == mf["bsize"], (u, md["btype"], mf["btype"])
            syms = dp.fixed_symbols(dp.cdata_of(bam_dyn, md)) if md["btype"] == 1 else list(md["payload"])
            if md["btype"] == 1:
                assert syms == dp.fixed_symbols(dp.cdata_of(bam_fix, mf)), u
            crude = crude_dynamic_bytes(syms)
            if crude is None:
                left_out += 1
            else:
                assert crude >= clen, f"block at {u}: BTYPE {md['btype']} of {clen} bytes, a crude dynamic form takes {crude}"
        u += n
    assert left_out <= max_left_out * len(dyn), (left_out, len(dyn))
    return dict(btypes=btypes, dynamic=out, left_out=left_out)


def check_high_dynamic(res, d_dyn, header, span, block):
    """the blocks wholly inside a payload of high bytes that hold no match: stored at block 64 (the dynamic form of 64 distinct-ish
    literals ties with the stored one at best), BTYPE 2 and all literals above"""
    from mirge3_amd import bam_export
    blob = bam_export.header_blob(header)[0]
    by_offset = {u: (syms, ll, dd) for u, _m, syms, ll, dd, _cl in res["dynamic"]}
    n_free, u = 0, 0
    for m in d_dyn["members"][:-1]:
        n = len(m["payload"])
        if span[0] <= u and u + block <= span[1] and dp.block_is_match_free(blob, u, u + block):
            n_free += 1
            if block == 64:
                assert m["btype"] == 0 and m["bsize"] == n + 31, (u, m["btype"], m["bsize"])
            else:
                assert m["btype"] == 2, (u, m["btype"])
                syms, ll, dd = by_offset[u]
                assert all(isinstance(s, int) for s in syms) and bytes(syms) == blob[u:u + block]
                assert [x for x in dd if x] == [1]  # no match: the one distance code of length 1
        u += n
    inside = (span[1] - span[0]) // block - 1
    assert n_free >= 0.95 * inside, (n_free, inside)
    return n_free


def check_plants(res, d_dyn, bam_dyn, plants):
    """block 0 at the default size: every planted copy is one match of exactly its (length, distance), whichever type the member took
    -> (length codes, distance codes) over the BTYPE 2 members"""
    m0 = d_dyn["members"][0]
    if m0["btype"] == 2:
        syms = res["dynamic"][0][2]
        assert res["dynamic"][0][0] == 0
    else:
        assert m0["btype"] == 1
        syms = dp.fixed_symbols(dp.cdata_of(bam_dyn, m0))
    got = dp.matches_at(syms)
    assert {p: got.get(p) for p in plants} == plants
    return codes_seen(res)


def codes_seen(res):
    len_codes = {s[2] for _u, _m, syms, *_ in res["dynamic"] for s in syms if not isinstance(s, int)}
    dist_codes = {s[3] for _u, _m, syms, *_ in res["dynamic"] for s in syms if not isinstance(s, int)}
    return len_codes, dist_codes


# ---------------------------------------------------------------------------------------------------------------------
# the builder alone
# ---------------------------------------------------------------------------------------------------------------------
def _fib(k):
    out = [1, 1]
    while len(out) < k:
        out.append(out[-1] + out[-2])
    return out[:k]


def builder_cases():
    """-> [(name, max_bits, uint32 [vectors, symbols])]"""
    rng = np.random.Generator(np.random.PCG64(7500))
    fib286 = np.zeros(N_LL, np.uint32)
    fib286[rng.permutation(N_LL)[:20]] = _fib(20)
    assert int(fib286.sum()) == 17710 and max(huffman_lengths(fib286).values()) == 19
    fib19 = np.zeros(N_CL, np.uint32)
    fib19[rng.permutation(N_CL)[:10]] = _fib(10)
    assert max(huffman_lengths(fib19).values()) == 9
    one = np.zeros(N_LL, np.uint32); one[77] = 5
    two = np.zeros(N_LL, np.uint32); two[3] = 9; two[256] = 1
    hot = np.ones(N_LL, np.uint32); hot[200] = 65279
    # seeded vectors: a random number of used symbols, counts log-uniform over 1 .. 2^k so that both flat and steep trees occur
    rnd = np.zeros((200, N_LL), np.uint32)
    for v in range(200):
        used = rng.permutation(N_LL)[:int(rng.integers(2, N_LL + 1))]
        rnd[v, used] = np.floor(2.0 ** (rng.random(used.size) * float(rng.integers(1, 25)))).astype(np.uint32)
    rnd30 = np.zeros((40, N_D), np.uint32)
    for v in range(40):
        used = rng.permutation(N_D)[:int(rng.integers(1, N_D + 1))]
        rnd30[v, used] = np.floor(2.0 ** (rng.random(used.size) * float(rng.integers(1, 30)))).astype(np.uint32)
    rnd19 = np.zeros((40, N_CL), np.uint32)
    for v in range(40):
        used = rng.permutation(N_CL)[:int(rng.integers(2, N_CL + 1))]
        rnd19[v, used] = np.floor(2.0 ** (rng.random(used.size) * float(rng.integers(1, 12)))).astype(np.uint32)
    return [("fibonacci20of286", 15, fib286[None]), ("fibonacci10of19", 7, fib19[None]), ("one_symbol", 15, one[None]), ("two_symbols", 15, two[None]),
            ("equal286", 15, np.full((1, N_LL), 3, np.uint32)), ("hot_beside_ones", 15, hot[None]), ("seeded286", 15, rnd), ("seeded30", 15, rnd30),
            ("seeded19", 7, rnd19)]


def check_lengths(counts, lengths, max_bits):
    """-> (excess over the package-merge optimum where the limit acts, else None)"""
    counts, lengths = [int(c) for c in counts], [int(x) for x in lengths]
    assert max(lengths) <= max_bits
    assert [x == 0 for x in lengths] == [c == 0 for c in counts]
    used = sum(1 for c in counts if c)
    if used == 1:
        assert sorted(x for x in lengths if x) == [1]  # the documented single code
        return None
    assert kraft(lengths, max_bits) == 1 << max_bits, (kraft(lengths, max_bits), 1 << max_bits)
    cost = sum(c * x for c, x in zip(counts, lengths))
    plain = huffman_lengths(counts)
    if max(plain.values()) <= max_bits:
        assert cost == sum(counts[s] * x for s, x in plain.items()), "not the Huffman optimum although the plain tree fits"
        return None
    best = package_merge_cost(counts, max_bits)
    assert cost >= best, (cost, best)
    return cost - best
