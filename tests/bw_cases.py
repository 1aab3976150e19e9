"""Shared by the ``--coverage-bigwig`` tests (CPU, host simulation, GPU): chromosome sizes for the cases of ``cov_cases``, the directed
cases of the issue, and ``restate`` -- what a file must hold, worked out per covered base with NumPy and the sentences of the
specification, sharing no code with ``mirge3_amd/bigwig.py``, the kernels or the reader."""
import functools
import struct

import numpy as np

import cov_cases

S_TEST, BASE_TEST = 3, 4


def f32_bits(depth):
    """float32(depth), round to nearest even (a depth below 2^53 is exact as a double, so one rounding happens)"""
    assert 0 < depth < 2 ** 53
    return struct.unpack("<I", struct.pack("<f", float(depth)))[0]


def bits_to_float(b):
    return struct.unpack("<f", struct.pack("<I", b))[0]


def to_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def sizes_for(iv, n_rank):
    """an LN per rank: a few bases behind the last covered one, not a multiple of 4 where that is possible"""
    out = []
    for r in range(n_rank):
        pick = iv["rank"] == r
        end = int((iv["start"][pick] + iv["len"][pick]).max()) if pick.any() else 1000
        ln = min(end + 7, cov_cases.MAX_END)
        out.append(ln if ln % 4 or ln == end else ln - 1)
    return out


@functools.lru_cache(maxsize=None)
def directed():
    """name -> (intervals, names in rank (= @SQ) order, sizes, S, zoom base)"""
    W = 2 ** 32 - 1
    c = {}
    # @SQ order d, c, b, a is the opposite of the byte order; b has no run.  d: 3 runs (a section exactly full at S = 3), among them two
    # abutting runs inside one bin and a run that ends on a bin edge; c: 4 runs (full plus one), one spanning bins 75 .. 114 = 40 bins of
    # 4, the last one in the bin that LN = 999 clips; a: 256 one-base runs of alternating depth (so that levels are kept at all) and 7
    # more (last-short sections)
    rows = [(0, 8, 4, 2, 0), (0, 101, 1, 3, 1), (0, 102, 1, 5, 1)]
    rows += [(1, 0, 3, 7, 0), (1, 300, 160, 5, 1), (1, 600, 1, 1, 0), (1, 996, 3, 9, 0)]
    rows += [(3, x, 1, 1 + x % 3, x % 2) for x in range(256)] + [(3, 300 + 10 * i, 3, i + 1, i % 2) for i in range(7)]
    c["layout"] = (cov_cases.make(rows), ["d", "c", "b", "a"], [1003, 999, 77, 501], S_TEST, BASE_TEST)
    c["depths"] = (cov_cases.make([(0, 0, 4, 2 ** 24, 0), (0, 10, 4, 2 ** 24, 0), (0, 10, 2, 1, 1), (0, 20, 1, W, 0), (0, 20, 1, W, 1), (0, 20, 1, W, 0),
                                   (0, 19, 3, 1, 0)]), ["chr1"], [64], S_TEST, BASE_TEST)
    top = cov_cases.MAX_END
    c["extreme"] = (cov_cases.make([(0, 0, 5, 1, 0), (1, top - 4, 4, 2, 1), (1, top - 1, 1, 1, 0), (1, top - 9, 2, 1, 0)]), ["x", "y"], [5, top], S_TEST, BASE_TEST)
    # S = 1: 36 bytes a section, a lane per byte, so no match: all literals.  (What the form is: test_bigwig_hostsim's docstring.)
    c["single_items"] = (cov_cases.make([(0, 0x909190, 0x10101, 0x4D4D4E, 0), (0, 0xA0A1A2, 3, 7, 0)]), ["chr1"], [0xB0B0B0], 1, BASE_TEST)
    # three items whose starts, ends and values (float32 0x4A9A9A9C ...) are bytes of 144 and above, 33 of the section's 60: the fixed code
    # takes 3 + 60 * 8 + 33 + 7 bits = 66 bytes (a lane per byte: no match), the stored form 65
    c["incompressible"] = (cov_cases.make([(0, 0x909190, 0x010101, 0x4D4D4E, 0), (0, 0x9495A6, 0x010101, 0x55CDCF, 0), (0, 0x98A9AA, 0x010101, 0x5E4E48, 0)]),
                           ["chr1"], [0xB0B0B0], S_TEST, 1 << 20)
    c["ladder_1024"] = (cov_cases.make([(0, 16 * i, 8, 1 + i % 2, 0) for i in range(1024)]), ["chr1"], [16 * 1024], 1024, 64)
    c["empty"] = (cov_cases.make([]), ["chr2", "chr10", "chr1"], [10, 20, 30], S_TEST, BASE_TEST)
    return c


def strand_runs(runs, strand):
    """(rank, start, end, depth) of one strand (None: all) as Python lists, in the runs' order"""
    pick = np.ones(runs["chrom"].size, bool) if strand is None else runs["strand"] == strand
    return list(zip(runs["chrom"][pick].tolist(), runs["start"][pick].tolist(), runs["end"][pick].tolist(), runs["depth"][pick].tolist()))


def restate(rows, names, sizes, S, base):
    """rows: (rank, start, end, depth) -> dict(items, zoom [(R, records)], summary, sections) with float32 values as bit patterns"""
    order = sorted(range(len(names)), key=lambda r: names[r].encode("latin-1"))
    cid_of = {r: k for k, r in enumerate(order)}
    rows = sorted((cid_of[r], s, e, d) for r, s, e, d in rows)
    items = [(c, s, e, f32_bits(d)) for c, s, e, d in rows]
    ln_of = {cid_of[r]: sizes[r] for r in range(len(names))}
    # ---- every covered base: chromosome, position, the run that covers it
    if rows:
        lens = np.asarray([e - s for _, s, e, _ in rows], dtype=np.int64)
        rid = np.repeat(np.arange(len(rows)), lens)
        first = np.cumsum(lens) - lens
        pos = np.repeat(np.asarray([s for _, s, _, _ in rows], dtype=np.int64), lens) + (np.arange(int(lens.sum())) - np.repeat(first, lens))
        chrom = np.repeat(np.asarray([c for c, _, _, _ in rows], dtype=np.int64), lens)
    val = [float(bits_to_float(b)) for _, _, _, b in items]
    # ---- sections and the total summary
    sections, a = [], 0
    while a < len(rows):
        b = a
        while b < len(rows) and b - a < S and rows[b][0] == rows[a][0]:
            b += 1
        sections.append((a, b))
        a = b
    bases, vmin, vmax, tsum, tsq = 0, 0.0, 0.0, 0.0, 0.0
    for k, (a, b) in enumerate(sections):
        p_sum, p_sq = 0.0, 0.0
        for x in range(a, b):
            n = int(np.count_nonzero(rid == x)) if len(rows) < 2000 else rows[x][2] - rows[x][1]
            p_sum = p_sum + float(n) * val[x]
            p_sq = p_sq + float(n) * (val[x] * val[x])
            bases += n
        lo, hi = min(val[a:b]), max(val[a:b])
        vmin, vmax = (lo, hi) if k == 0 else (min(vmin, lo), max(vmax, hi))
        tsum, tsq = tsum + p_sum, tsq + p_sq
    # ---- zoom levels
    zoom, prev = [], len(rows)
    for k in range(8):
        R = base * 4 ** k
        if R > 2 ** 20 or not rows:
            break
        key = (chrom << 40) | ((pos // R) << 0)
        pair = np.stack([key, rid], axis=1)
        uniq, counts = np.unique(pair, axis=0, return_counts=True)  # (chromosome, bin) ascending, runs ascending inside
        recs = []
        last_key = None
        for (kk, x), ov in zip(uniq.tolist(), counts.tolist()):
            if kk != last_key:
                c, j = kk >> 40, kk & ((1 << 40) - 1)
                recs.append([c, j * R, min((j + 1) * R, ln_of[c]), 0, val[x], val[x], 0.0, 0.0])
                last_key = kk
            r = recs[-1]
            r[3] += ov
            r[4], r[5] = min(r[4], val[x]), max(r[5], val[x])
            r[6] = r[6] + float(ov) * val[x]
            r[7] = r[7] + float(ov) * (val[x] * val[x])
        if 2 * len(recs) > prev:
            break
        zoom.append((R, [(r[0], r[1], r[2], r[3], to_bits(r[4]), to_bits(r[5]), to_bits(np.float32(r[6])), to_bits(np.float32(r[7]))) for r in recs]))
        prev = len(recs)
    return dict(items=items, zoom=zoom, summary=(bases, vmin, vmax, tsum, tsq),
                sections=[(rows[a][0], rows[a][1], rows[b - 1][2], b - a) for a, b in sections])


def check(got, want):
    """a file read by bigwig_reader against ``restate``"""
    assert got["items"] == want["items"]
    assert got["sections"] == want["sections"]
    assert [z[0] for z in got["zoom"]] == [z[0] for z in want["zoom"]]
    for (_, a, _), (_, b) in zip(got["zoom"], want["zoom"]):
        assert a == b
    assert struct.pack("<Qdddd", *got["summary"]) == struct.pack("<Qdddd", *want["summary"])
