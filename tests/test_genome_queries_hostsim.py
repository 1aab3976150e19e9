"""``k_genome_queries`` on the CPU: ``csrc/kernels_genome.hpp`` itself compiled for the host (tests/hostsim/genome_sim.cpp, thread by
thread) against a restatement of the header's comment in Python integers: a query on a strand is a 128-bit pattern of 2-bit codes on
the forward text, with an N mask and a seed mask; the seed is cut into n_mm + 1 pieces at ``s0 + j * sl / P``; a piece's key is its
table (``min(piece length, kmax)``) above bit 32 and its first bases below, or NOKEY when it holds an N.  Every trimmed length of
1..64, seeds from 5 to 64, both strands, every piece holding an N in turn: a wrong word, shift or mask shows here without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostsim", "genome_sim.cpp")
HDR = os.path.join(HERE, "..", "mirge3.0_amd", "csrc", "kernels_genome.hpp")
SO = os.path.join(HERE, "hostsim", "_build", "libgenomesim.so")
NOKEY = 0xFFFFFFFFFFFFFFFF
EVEN = 0x5555555555555555
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
_RC = str.maketrans("ACGTN", "TGCAN")


def _sim():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in (SRC, HDR)):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", SO, SRC])
    return C.CDLL(SO)


def run(queries, n_mm, seedlen, trim5, trim3, kmax, norc=False):
    """-> per (query, strand) the GenomeQS fields as a dict, and keys / vals [2n, P]"""
    n, P = len(queries), n_mm + 1
    text = np.frombuffer("".join(queries).encode(), dtype=np.uint8).copy() if any(queries) else np.zeros(1, np.uint8)
    off = np.concatenate(([0], np.cumsum([len(q) for q in queries]))).astype(np.int64)
    qs = np.zeros((2 * n, 8), np.uint64)
    keys = np.zeros((2 * n, P), np.uint64)
    vals = np.zeros((2 * n, P), np.uint32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc = _sim().sim_queries(p(text), p(off), C.c_uint32(n), C.c_int(n_mm), C.c_int(seedlen), C.c_int(trim5), C.c_int(trim3), C.c_int(kmax),
                            C.c_int(1 if norc else 0), p(qs), p(keys), p(vals))
    assert rc == 0
    return qs, keys, vals


def restate(query, strand, n_mm, seedlen, trim5, trim3):
    """the header's comment: (q, nm, seed) as 128-bit integers, the length, [(lo, plen, piece's bases or None)]"""
    s = query[trim5:len(query) - trim3].upper() if len(query) > trim5 + trim3 else ""
    L, P = len(s), n_mm + 1
    if L < 1 or L <= n_mm or L > 64:
        return None
    pat = s if strand == 0 else s.translate(_RC)[::-1]
    q = sum(CODE[ch] << (2 * t) for t, ch in enumerate(pat) if ch != "N")
    nm = sum(1 << (2 * t) for t, ch in enumerate(pat) if ch == "N")
    sl = min(seedlen, L)
    s0 = 0 if strand == 0 else L - sl  # '-': the read's 5' end is the end of its reverse complement
    seed = sum(1 << (2 * t) for t in range(s0, s0 + sl))
    pieces = []
    for j in range(P):
        lo, hi = s0 + j * sl // P, s0 + (j + 1) * sl // P
        pieces.append((lo, hi - lo, None if "N" in pat[lo:hi] else [CODE[ch] for ch in pat[lo:hi]]))
    return q, nm, seed, L, pieces


def check(queries, n_mm, seedlen, trim5, trim3, kmaxes, norc=False):
    want = [[restate(q, s, n_mm, seedlen, trim5, trim3) if not (s == 1 and norc) else None for s in (0, 1)] for q in queries]
    lo64 = (1 << 64) - 1
    n_keys = 0
    for kmax in kmaxes:
        qs, keys, vals = run(queries, n_mm, seedlen, trim5, trim3, kmax, norc)
        P = n_mm + 1
        assert np.array_equal(vals, (np.arange(2 * len(queries), dtype=np.uint32) * 4)[:, None] + np.arange(P, dtype=np.uint32)[None, :])
        for i, q in enumerate(queries):
            for s in (0, 1):
                got, w = [int(x) for x in qs[2 * i + s]], want[i][s]
                ctx = (q, s, n_mm, seedlen, trim5, trim3, kmax)
                assert got[6] & 0xFFFFFFFF == i
                if w is None:
                    assert got[:6] == [0] * 6 and got[6] >> 32 == 0 and got[7] == 0 and keys[2 * i + s].tolist() == [NOKEY] * P, ctx
                    continue
                wq, wnm, wseed, L, pieces = w
                assert got[:6] == [wq & lo64, wq >> 64, wnm & lo64, wnm >> 64, wseed & lo64, wseed >> 64], ctx
                assert ((got[6] >> 32) & 0xFF, got[6] >> 40) == (L, P), ctx
                assert [(got[7] >> (8 * j)) & 0xFF for j in range(3)] == [p[0] for p in pieces] + [0] * (3 - P), ctx
                assert [(got[7] >> (24 + 8 * j)) & 0xFF for j in range(3)] == [p[1] for p in pieces] + [0] * (3 - P), ctx
                for j, (lo, plen, bases) in enumerate(pieces):
                    kk = min(plen, kmax)
                    key = NOKEY if bases is None else (kk << 32) | sum(c << (2 * t) for t, c in enumerate(bases[:kk]))
                    assert int(keys[2 * i + s, j]) == key, ctx + (j, lo, plen)
                    n_keys += bases is not None
    return want, n_keys


def queries_for(rng, n_mm, seedlen, trim5, trim3):
    """per trimmed length 1..64: a random read, and per strand and piece a read whose only N lies in that piece"""
    def rand(n):
        return "".join("ACGTacgt"[int(c)] for c in rng.integers(0, 8, n))
    qs = [rand(0), rand(trim5 + trim3), rand(max(0, trim5 + trim3 - 1))]  # nothing left after trimming
    for L in range(1, 65):
        qs.append(rand(trim5 + L + trim3))
        if L <= n_mm:
            continue
        for strand in (0, 1):
            for lo, plen, _ in restate("A" * (trim5 + L + trim3), strand, n_mm, seedlen, trim5, trim3)[4]:
                at = lo + int(rng.integers(0, plen))            # on the forward text
                at = at if strand == 0 else L - 1 - at          # in the read
                body = rand(L)
                qs.append(rand(trim5) + body[:at] + "N" + body[at + 1:] + rand(trim3))
    return qs


@pytest.mark.parametrize("n_mm", [0, 1, 2])
@pytest.mark.parametrize("seedlen", [5, 12, 15, 25, 28, 33, 64])
def test_query_encoding_equals_the_restatement(n_mm, seedlen):
    rng = np.random.default_rng(1000 * n_mm + seedlen)
    trim5, trim3 = (0, 0) if seedlen in (5, 15, 28, 64) else (1, 2)
    qs = queries_for(rng, n_mm, seedlen, trim5, trim3)
    want, n_keys = check(qs, n_mm, seedlen, trim5, trim3, (8, 12, 13))
    assert n_keys > 3 * 64 * (n_mm + 1)
    # the branches of the key extraction, from the restatement: a piece that starts in the second word, one that starts in the
    # first and whose key reaches into the second, one that starts at base 0 -- wherever the cut rule admits them
    los = {(lo, plen) for w in want for x in w if x for lo, plen, _ in x[4]}
    P, admits = n_mm + 1, set()
    for L in range(n_mm + 1, 65):
        sl = min(seedlen, L)
        for s0 in (0, L - sl):
            admits |= {(s0 + j * sl // P, s0 + (j + 1) * sl // P - (s0 + j * sl // P)) for j in range(P)}
    assert los == admits
    assert any(lo == 0 for lo, _ in los)
    assert any(0 < lo < 32 < lo + min(pl, 8) for lo, pl in los) == (seedlen < 64 or P > 1)  # -n 0 -l 64: one piece, at base 0
    assert any(lo >= 32 for lo, _ in los) == (seedlen <= 32 * P)  # the last piece of a 64-nt '-' read starts at 64 - ceil(sl / P)


def test_norc_leaves_the_minus_strand_empty_and_too_long_a_query_too():
    rng = np.random.default_rng(4)
    qs = ["".join("ACGT"[int(c)] for c in rng.integers(0, 4, n)) for n in (20, 64, 65, 66, 40)]
    want, _ = check(qs, 1, 28, 0, 0, (8,), norc=True)
    assert [w[0] is not None for w in want] == [True, True, False, False, True] and all(w[1] is None for w in want)
    want, _ = check(qs, 1, 28, 1, 1, (13,))
    assert [w[1] is not None for w in want] == [True, True, True, True, True]


def test_stand_alone_driver_under_the_sanitizers(tmp_path):
    """the same file as a program of its own, built with -fsanitize=address,undefined: every (pieces, seed, table length) once"""
    exe = str(tmp_path / "genome_sim")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DGENOME_SIM_MAIN",
                           "-Wno-unknown-pragmas", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("genome_sim ok"), r.stdout[-500:] + r.stderr[-3000:]
