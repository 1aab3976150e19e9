"""The ``--sam-out`` kernels on the CPU: ``csrc/kernels_sam.hpp`` itself, compiled for the host (tests/hostsim/sam_sim.cpp: a workgroup's
threads are std::threads behind a barrier), against the reference's golden files and against ``format_sam_host`` -- at the default
tile / chunk sizes and at sizes that cut lines, QNAME digits and a row of many copies.  Reads and libraries are packed here the way
the kernels read them (2-bit words, N / invalid bitmaps); the cascade's answer comes from the oracle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
import mirge3_amd  # noqa: F401
from mirge3_amd import sam_export
from mirge3_amd.cascade import PASSES
from mirge3_amd.seqio import FlatSeqs

from test_sam_out import GOLDEN, ORG, golden_inputs, host_passes_of

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostsim", "sam_sim.cpp")
SO = os.path.join(HERE, "hostsim", "_build", "libsamsim.so")
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def _sim():
    deps = [SRC, os.path.join(HERE, "..", "mirge3.0_amd", "csrc", "kernels_sam.hpp")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-pthread", "-o", SO, SRC])
    sim = C.CDLL(SO)
    sim.sim_run.restype = C.c_longlong
    return sim


class SP(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("T", "inv", "ref_start", "chrom_of_ref", "minus", "seg_ptr", "seg_s", "seg_e", "cds_lo", "cds_hi", "chrom_data", "chrom_off")] + \
               [("n_refs", C.c_uint32), ("n_chrom", C.c_uint32), ("trim5", C.c_int32), ("trim3", C.c_int32), ("cls", C.c_int32), ("pad", C.c_int32)]

def pack_reads(reads):
    n = len(reads); W = max(1, (max(len(r) for r in reads) + 31) // 32)
    seq = np.zeros((W, n), np.uint64); nm = np.zeros((W, n), np.uint64)
    for i, r in enumerate(reads):
        for p, ch in enumerate(r):
            if ch == "N": nm[p >> 5, i] |= np.uint64(1) << np.uint64(2 * (p & 31))
            else: seq[p >> 5, i] |= np.uint64(CODE[ch]) << np.uint64(2 * (p & 31))
    return W, seq, nm, np.asarray([len(r) for r in reads], np.uint16)

def pack_lib(seqs):
    total = sum(len(s) + 1 for s in seqs)
    T = np.zeros(total // 32 + 8, np.uint64); inv = np.zeros(total // 64 + 4, np.uint64); rs = np.zeros(len(seqs) + 1, np.uint32)
    g = 0
    for r, s in enumerate(seqs):
        rs[r] = g
        for ch in s:
            if ch in CODE: T[g >> 5] |= np.uint64(CODE[ch]) << np.uint64(2 * (g & 31))
            else: inv[g >> 6] |= np.uint64(1) << np.uint64(g & 63)
            g += 1
        inv[g >> 6] |= np.uint64(1) << np.uint64(g & 63); g += 1
    rs[len(seqs)] = g
    return T, inv, rs

def run(libs, reads, ps, ref, off, mm, counts, order, sample, tile, chunk):
    sim = _sim()
    W, seq, nm, ln = pack_reads(reads)
    arr = (SP * 9)(); keep = []
    for p in range(9): arr[p].cls = -1
    for k, p in enumerate(sam_export.CLASS_PASSES):
        lib = libs[PASSES[p][1]]
        T, inv, rs = pack_lib(lib.seqs.to_list())
        t = sam_export.lift_tables(lib.names, lib.headers, ORG)
        a = dict(T=T, inv=inv, ref_start=rs, chrom_of_ref=t["chrom_of_ref"], minus=t["minus"], seg_ptr=t["seg_ptr"].astype(np.uint32),
                 seg_s=np.append(t["seg_s"], 0).astype(np.int32), seg_e=np.append(t["seg_e"], 0).astype(np.int32), cds_lo=np.append(t["cds_lo"], 0), cds_hi=np.append(t["cds_hi"], 0),
                 chrom_data=t["chrom_data"], chrom_off=t["chrom_off"].astype(np.uint32))
        keep.append(a)
        for f, v in a.items(): setattr(arr[p], f, v.ctypes.data)
        arr[p].n_refs, arr[p].n_chrom = len(lib), t["n_chrom"]
        arr[p].trim5, arr[p].trim3, arr[p].cls = PASSES[p][3].get("trim5", 0), PASSES[p][3].get("trim3", 0), k
    cnt = np.ascontiguousarray(counts, np.uint32); S = cnt.shape[1]
    out = np.zeros(64 << 20, np.uint8); nl = C.c_longlong(0)
    p8 = np.ascontiguousarray(ps, np.int8); r32 = np.ascontiguousarray(ref, np.int32); o32 = np.ascontiguousarray(off, np.int32); m8 = np.ascontiguousarray(mm, np.int8)
    od = np.ascontiguousarray(order, np.uint32)
    P = lambda a: C.c_void_p(a.ctypes.data)
    n = sim.sim_run(C.c_uint32(len(reads)), C.c_int(W), P(seq), P(nm), P(ln), P(cnt), P(p8), P(r32), P(o32), P(m8), C.c_int(S), C.c_int(sample), arr, C.c_int(9), P(od),
                    C.c_uint32(tile), C.c_uint32(chunk), P(out), C.c_longlong(out.size), C.byref(nl))
    assert n >= 0, n
    return out[:n].tobytes(), nl.value


def _oracle_annotation(libs, reads):
    fr = FlatSeqs.from_list(reads)
    olibs = [(libs[PASSES[p][1]].seqs.data, libs[PASSES[p][1]].seqs.offsets) for p in range(9)]
    return oracle.cascade(fr.data, fr.offsets, olibs, n_pass=9, indexed=True)


@pytest.mark.parametrize("tile,chunk", [(8160, 32 << 20), (256, 4096), (272, 544)])
def test_kernels_on_the_host_equal_the_reference_files(tile, chunk):
    libs, samples, seqs, counts = golden_inputs()
    ann = _oracle_annotation(libs, seqs)
    for s, name in enumerate(samples):
        body, n_lines = run(libs, seqs, *ann, counts, np.arange(len(seqs)), s, tile, chunk)
        with open(os.path.join(GOLDEN, name + ".sam"), "rb") as fh:
            exp = fh.read()[len(sam_export.DEFAULT_HEADER):]
        assert body == exp, name
        assert n_lines == exp.count(b"\n")


@pytest.mark.parametrize("tile,chunk", [(8160, 32 << 20), (256, 4096)])
def test_kernels_on_the_host_equal_format_sam_host(tile, chunk):
    """random libraries with one to four segments per reference, gaps, both strands, coordinates past 2^31, references without a
    lift; reads of 16, 25, 26, 64 and 300 nt, some with a mismatch or an N; zero counts and one row of 345 copies"""
    rng = np.random.Generator(np.random.PCG64(4242))

    def rnd(n):
        return "".join("ACGT"[int(c)] for c in rng.integers(0, 4, size=n))

    def head(name, length, i):
        kind = int(rng.integers(0, 8))
        if kind == 0:
            return name
        if kind == 1:
            return f"{name} chr{i}_PATCH segs:1-{length} cds:+:100-{99 + length}"
        cuts = sorted(set(int(x) for x in rng.integers(2, length, size=int(rng.integers(0, 4)))))
        bounds, g, minus, segs, cds = [1] + cuts + [length + 1], int(rng.integers(10_000_000, 5_000_000_000)), bool(rng.integers(0, 2)), [], []
        for a, b in zip(bounds[:-1], bounds[1:]):
            s = a + (3 if (rng.random() < 0.2 and b - a > 8) else 0)
            segs.append(f"{s}-{b - 1}"); cds.append(f"{g}-{g + (b - 1 - s)}")
            g = g - 3000 - (b - a) if minus else g + (b - a) + 3000
        return f"{name} chr{1 + i % 5} segs:{','.join(segs)} cds:{'-' if minus else '+'}:{','.join(cds)}"

    from mirge3_amd.seqio import Library

    def lib(prefix, n, length):
        names = [f"{prefix}{i}" for i in range(n)]
        return Library(names, FlatSeqs.from_list([rnd(length) for _ in range(n)]), [head(nm, length, i) for i, nm in enumerate(names)])
    libs = {"mirna": lib("miR-", 10, 22), "hairpin": lib("mir-", 6, 90), "mature_trna": lib("tRNA-", 2, 74), "pre_trna": lib("pre-", 2, 92),
            "snorna": lib("SNO", 6, 140), "rrna": lib("RR", 4, 400), "ncrna_others": lib("NC", 6, 420), "mrna": lib("ENST", 8, 600)}
    reads = set(libs["mirna"].seqs.to_list())
    for m in libs["mirna"].seqs.to_list():
        reads.add(rnd(1) + m[:20] + rnd(2))
    for key in ("snorna", "rrna", "ncrna_others", "mrna", "hairpin"):
        seqs = libs[key].seqs.to_list()
        for L in (16, 25, 26, 64, 300):
            for _ in range(5):
                q = seqs[int(rng.integers(0, len(seqs)))]
                if len(q) >= L:
                    o = int(rng.integers(0, len(q) - L + 1))
                    r = list(q[o:o + L])
                    u = rng.random()
                    if u < 0.3 and key != "mrna":
                        r[int(rng.integers(0, min(L, 28)))] = "N" if u < 0.12 else "ACGT"[int(rng.integers(0, 4))]
                    reads.add("".join(r))
    reads = sorted(reads) + [rnd(20), rnd(300)]
    ann = _oracle_annotation(libs, reads)
    assert set(sam_export.CLASS_PASSES) <= set(int(p) for p in ann[0])
    counts = rng.integers(0, 4, size=(len(reads), 3))
    counts[int(np.nonzero(ann[0] == 4)[0][0]), 1] = 345
    order = rng.permutation(len(reads))
    for s in range(3):
        body, n_lines = run(libs, reads, *ann, counts, order, s, tile, chunk)
        exp = sam_export.format_sam_host(reads, *ann, counts, order, s, host_passes_of(libs), ORG)
        assert len(exp) > 0 and body == exp, s
        assert n_lines == exp.count(b"\n")
