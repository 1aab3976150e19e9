"""The kernels of ``--coverage-bigwig`` on the CPU: ``csrc/kernels_bw.hpp`` itself compiled for the host (tests/hostsim/bw_sim.cpp: the
launches of csrc/native_bw.hpp, the file assembled by csrc/bw_layout.hpp) on the brute-force runs of tests/cov_cases.py and the directed
cases of tests/bw_cases.py.  With ``MIRGE_BW_DEFLATE=none`` the files equal ``bigwig.write_host``'s byte for byte; the compressed files
decode through tests/bigwig_reader.py (Python's zlib judges stream and Adler-32) to the same payload.

The stored form.  The issue names "a section whose deflate is not smaller (S = 1)" for it.  By the issue's own rule (stored iff the
fixed-code block is not smaller than the payload + 5) a section of one item cannot be stored: of its 36 bytes, twelve are fixed (itemStep,
itemSpan, type, reserved, itemCount; all below 144, 8 bits each) and chromId < 2^24, start and end < 2^31 and a positive float leave at
most 3 + 3 + 3 + 3 + 3 = 15 bytes of 144 and above (9 bits), so the fixed code takes at most 3 + 36 * 8 + 15 + 7 = 313 bits = 40 bytes
against 41 stored.  ``single_items`` keeps that case (S = 1, fifteen such bytes: 40 bytes, fixed form, compared byte for byte like the
rest); ``incompressible`` is the smallest section that CAN be stored (S = 3, 33 such bytes of 60: 66 bytes fixed, 65 stored) and must be."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bigwig_reader
import bw_cases
import cov_cases
from mirge3_amd import bigwig

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostsim", "bw_sim.cpp")
SO = os.path.join(HERE, "hostsim", "_build", "libbwsim.so")
CSRC = os.path.join(HERE, "..", "mirge3.0_amd", "csrc")
SMALL = [n for n in sorted(cov_cases.all_cases()) if n not in ("count_65537", "many_equal")]


@pytest.fixture(scope="module")
def sim():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("kernels_bw.hpp", "bw_layout.hpp", "kernels_bam.hpp", "kernels_sam.hpp", "kernels_cov.hpp")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-pthread", "-o", SO, SRC])
    return C.CDLL(SO)


def run_sim(sim, runs, names, sizes, stranded, f, S, base, deflate):
    """-> (return code or the file's bytes, stats, err)"""
    n = int(runs["chrom"].size)
    arr = dict(strand=np.ascontiguousarray(runs["strand"], np.uint8), chrom=np.ascontiguousarray(runs["chrom"], np.int32),
               start=np.ascontiguousarray(runs["start"], np.int64), end=np.ascontiguousarray(runs["end"], np.int64),
               depth=np.ascontiguousarray(runs["depth"], np.int64))
    data = np.frombuffer("".join(names).encode(), np.uint8)
    off = np.zeros(len(names) + 1, np.int64)
    np.cumsum([len(x) for x in names], out=off[1:])
    ln = np.asarray(sizes, np.int64)
    cid = np.ascontiguousarray(bigwig.chrom_ids(names, sizes), np.int32)
    cap = (1 << 17) + 400 * n + 2 * len(names) * (max(len(x) for x in names) + 12)
    out, stats, err = np.zeros(cap, np.uint8), np.zeros(16, np.int64), np.zeros(4, np.int64)
    p = lambda a: C.c_void_p(a.ctypes.data)
    sim.sim_bigwig.restype = C.c_longlong
    rc = sim.sim_bigwig(C.c_uint32(n), p(arr["strand"]), p(arr["chrom"]), p(arr["start"]), p(arr["end"]), p(arr["depth"]), C.c_int32(len(names)),
                        p(data), p(off), p(ln), p(cid), C.c_int32(2 if stranded else 1), C.c_int32(f), C.c_uint32(S), C.c_uint32(base),
                        C.c_int32(deflate), p(out), C.c_longlong(cap), p(stats), p(err))
    return (bytes(out[:rc]) if rc > 0 else rc), stats.tolist(), err.tolist()


def sim_files(sim, iv, names, sizes, S, base, stranded, deflate):
    """the simulation's file(s) of a case: [(bytes, rows of that strand, stats)]"""
    runs = cov_cases.brute(iv, stranded)
    out = []
    for f, strand in enumerate((0, 1) if stranded else (None,)):
        blob, stats, _ = run_sim(sim, runs, names, sizes, stranded, f, S, base, deflate)
        assert not isinstance(blob, int), blob
        out.append((blob, bw_cases.strand_runs(runs, strand), stats))
    return out


def all_inputs():
    for name in SMALL:
        iv, names = cov_cases.all_cases()[name]
        yield name, (iv, names, bw_cases.sizes_for(iv, len(names)), bw_cases.S_TEST, bw_cases.BASE_TEST)
    for name, case in sorted(bw_cases.directed().items()):
        yield "directed_" + name, case


INPUTS = dict(all_inputs())


@pytest.mark.parametrize("stranded", [False, True], ids=["unstranded", "stranded"])
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_raw_files_equal_write_host_and_compressed_ones_decode_to_them(sim, name, stranded):
    iv, names, sizes, S, base = INPUTS[name]
    runs = cov_cases.brute(iv, stranded)
    raw = sim_files(sim, iv, names, sizes, S, base, stranded, 0)
    packed = sim_files(sim, iv, names, sizes, S, base, stranded, 1)
    for f, strand in enumerate((0, 1) if stranded else (None,)):
        assert raw[f][0] == bigwig.write_host(runs, names, sizes, strand, S, base), (name, f)
        want = bw_cases.restate(raw[f][1], names, sizes, S, base)
        a, b = bigwig_reader.read(raw[f][0]), bigwig_reader.read(packed[f][0])
        bw_cases.check(a, want)
        bw_cases.check(b, want)
        assert a["uncompress_buf"] == 0 and (b["uncompress_buf"] == a["largest"] or not raw[f][1])
        assert raw[f][2][:3] == [len(want["sections"]), len(want["items"]), len(want["zoom"])] and raw[f][2][3] == len(raw[f][0])
        assert raw[f][2][5:5 + len(want["zoom"])] == [len(z[1]) for z in want["zoom"]]


def test_stored_and_fixed_forms(sim):
    forms = {}
    for name in ("single_items", "incompressible", "ladder_1024"):
        iv, names, sizes, S, base = bw_cases.directed()[name]
        blob = sim_files(sim, iv, names, sizes, S, base, False, 1)[0][0]
        got = bigwig_reader.read(blob)
        forms[name] = got["forms"]
        print(name, "forms", got["forms"], "file bytes", len(blob))
    assert forms["incompressible"] == ["stored"]            # 66 bytes fixed against 65 stored
    assert forms["ladder_1024"] == ["fixed"]                # one section of 1024 items: 12 312 bytes, far smaller deflated
    assert forms["single_items"] == ["fixed", "fixed"]      # (a one-item section cannot reach the stored form: the docstring)


def test_a_run_beyond_its_chromosome_is_refused(sim):
    iv, names, sizes, S, base = bw_cases.directed()["extreme"]
    runs = cov_cases.brute(iv, False)
    rc, _, err = run_sim(sim, runs, names, [5, 2 ** 31 - 2], False, 0, S, base, 1)
    assert rc == -1 and err[:3] == [1, 2 ** 31 - 1, 2 ** 31 - 2]
    assert not isinstance(run_sim(sim, runs, names, sizes, False, 0, S, base, 1)[0], int)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 70000])
def test_the_chromosome_tree_of_the_layout_code_equals_write_host(sim, n):
    """csrc/bw_layout.hpp's B+ tree at one leaf, a full leaf, a second level and a third: the whole raw file against ``write_host``, and
    every name found from the root"""
    names = ["c%x" % ((k * 2654435761) % (1 << 32)) + "_" * (k % 3) for k in range(n)]
    sizes = [1000 + k for k in range(n)]
    runs = cov_cases.brute(cov_cases.make([(n // 2, 5, 7, 3, 0), (n - 1, 0, 2, 1, 0)]), False)
    blob, _, _ = run_sim(sim, runs, names, sizes, False, 0, bw_cases.S_TEST, bw_cases.BASE_TEST, 0)
    assert blob == bigwig.write_host(runs, names, sizes, None, bw_cases.S_TEST, bw_cases.BASE_TEST)
    got = bigwig_reader.read(blob)
    for k in list(range(0, n, 1 if n < 1000 else 997)) + [n - 1]:
        assert bigwig_reader.find_chrom(blob, got["tree_at"], names[k].encode())[1] == sizes[k]
