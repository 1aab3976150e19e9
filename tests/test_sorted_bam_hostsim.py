"""The ``--sorted-bam`` kernels on the CPU: ``csrc/kernels_bam.hpp`` itself, compiled for the host (tests/hostsim/bam_sim.cpp: a
workgroup's threads are std::threads behind a barrier).  The kernels use no wave-level steps, so not only the uncompressed stream
(block sizes 256 and 4096, against ``format_bam_host``; header lengths of every residue modulo the probe distance) but also the LDS
deflate, its bit offsets and the CRC-32 combination run here: the members are inflated and checked by tests/bam_reader.py.  Inputs:
the golden case of tests/golden/sam_out, one row raised to 1234 copies so that digit bands 1 to 4 occur and one row spans many blocks.
Records always shrink, so every member here is a fixed-Huffman block: the stored fallback and the edge of its decision, 9-bit literals
and every length and distance code run in tests/test_bam_deflate_hostsim.py, on payloads that records cannot produce."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mirge3_amd  # noqa: F401
from mirge3_amd import bam_export, sam_export
from mirge3_amd.cascade import PASSES
from mirge3_amd.seqio import FlatSeqs

import bam_reader
from test_sam_out import ORG, golden_inputs, host_passes_of
from test_sam_out_hostsim import SP, _oracle_annotation, pack_lib, pack_reads
from test_sorted_bam import HEADER_CASES, expected_lines, golden_header, header_of_length

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostsim", "bam_sim.cpp")
SO = os.path.join(HERE, "hostsim", "_build", "libbamsim.so")


def _sim():
    csrc = os.path.join(HERE, "..", "mirge3.0_amd", "csrc")
    deps = [SRC, os.path.join(csrc, "kernels_sam.hpp"), os.path.join(csrc, "kernels_bam.hpp")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-pthread", "-o", SO, SRC])
    sim = C.CDLL(SO)
    sim.sim_bam.restype = C.c_longlong
    return sim


def run(libs, reads, ps, ref, off, mm, counts, order, sample, header, block, deflate):
    sim = _sim()
    blob, refs = bam_export.header_blob(header)
    refid_of = {nm: k for k, (nm, _) in enumerate(refs)}
    W, seq, nm, ln = pack_reads(reads)
    arr = (SP * 9)(); keep = []
    rid = (C.c_void_p * 9)()
    for p in range(9): arr[p].cls = -1
    for k, p in enumerate(sam_export.CLASS_PASSES):
        lib = libs[PASSES[p][1]]
        T, inv, rs = pack_lib(lib.seqs.to_list())
        t = sam_export.lift_tables(lib.names, lib.headers, ORG)
        chroms = FlatSeqs(t["chrom_data"], t["chrom_off"]).to_list() if t["n_chrom"] else []
        a = dict(T=T, inv=inv, ref_start=rs, chrom_of_ref=t["chrom_of_ref"], minus=t["minus"], seg_ptr=t["seg_ptr"].astype(np.uint32),
                 seg_s=np.append(t["seg_s"], 0).astype(np.int32), seg_e=np.append(t["seg_e"], 0).astype(np.int32), cds_lo=np.append(t["cds_lo"], 0), cds_hi=np.append(t["cds_hi"], 0),
                 chrom_data=t["chrom_data"], chrom_off=t["chrom_off"].astype(np.uint32))
        r = np.asarray([refid_of.get(c, -1) for c in chroms] + [-1], dtype=np.int32)
        keep += [a, r]
        for f, v in a.items(): setattr(arr[p], f, v.ctypes.data)
        rid[p] = r.ctypes.data
        arr[p].n_refs, arr[p].n_chrom = len(lib), t["n_chrom"]
        arr[p].trim5, arr[p].trim3, arr[p].cls = PASSES[p][3].get("trim5", 0), PASSES[p][3].get("trim3", 0), k
    cnt = np.ascontiguousarray(counts, np.uint32); S = cnt.shape[1]
    out = np.zeros(16 << 20, np.uint8); nr = C.c_longlong(0)
    p8 = np.ascontiguousarray(ps, np.int8); r32 = np.ascontiguousarray(ref, np.int32); o32 = np.ascontiguousarray(off, np.int32); m8 = np.ascontiguousarray(mm, np.int8)
    od = np.ascontiguousarray(order, np.uint32)
    hb = np.frombuffer(blob, np.uint8)
    P = lambda a: C.c_void_p(a.ctypes.data)
    n = sim.sim_bam(C.c_uint32(len(reads)), C.c_int(W), P(seq), P(nm), P(ln), P(cnt), P(p8), P(r32), P(o32), P(m8), C.c_int(S), C.c_int(sample), arr, C.c_int(9), P(od),
                    rid, P(hb), C.c_longlong(len(blob)), C.c_uint32(block), C.c_int(deflate), P(out), C.c_longlong(out.size), C.byref(nr))
    assert n >= 0, n
    return out[:n].tobytes(), nr.value


@pytest.fixture(scope="module")
def case():
    libs, samples, seqs, counts = golden_inputs()
    ann = _oracle_annotation(libs, seqs)
    counts = counts.copy()
    header, names = golden_header()
    order = np.arange(len(seqs))
    body0 = sam_export.format_sam_host(seqs, *ann, counts, order, 0, host_passes_of(libs), ORG)
    heavy = seqs.index(body0.decode().split("\n")[3].split("\t")[0].rsplit("_", 1)[0])  # a read that writes lines in sample 0
    counts[heavy, 0] = 1234
    bodies = [sam_export.format_sam_host(seqs, *ann, counts, order, s, host_passes_of(libs), ORG) for s in range(len(samples))]
    assert bodies[0].count(b"_1233\t") == 1
    return dict(libs=libs, seqs=seqs, ann=ann, counts=counts, order=order, header=header, names=names, bodies=bodies)


@pytest.mark.parametrize("block", [256, 4096])
def test_uncompressed_stream_equals_format_bam_host(case, block):
    for s, body in enumerate(case["bodies"]):
        stream, n_rec = run(case["libs"], case["seqs"], *case["ann"], case["counts"], case["order"], s, case["header"], block, 0)
        bam, _ = bam_export.format_bam_host(body, case["header"], block_bytes=block)
        want = b"".join(m["payload"] for m in bam_reader.read_bgzf(bam))
        assert stream == want, s
        assert n_rec == body.count(b"\n")


@pytest.mark.parametrize("block,want", HEADER_CASES, ids=[f"block{b}_H{w}" for b, w in HEADER_CASES])
def test_header_length_against_the_records(case, block, want):
    """where the header ends inside a block and inside a probe's 32 bytes decides which probe writes the first records (the sample
    without the 1234-copy row: a few blocks each)"""
    header = header_of_length(case["header"], block, want)
    H = len(bam_export.header_blob(header)[0])
    assert H % block == want and (block != 256 or H % 32 == want % 32)
    body = case["bodies"][1]
    stream, n_rec = run(case["libs"], case["seqs"], *case["ann"], case["counts"], case["order"], 1, header, block, 0)
    bam, _ = bam_export.format_bam_host(body, header, block_bytes=block)
    assert stream == b"".join(m["payload"] for m in bam_reader.read_bgzf(bam))
    assert n_rec == body.count(b"\n") > 20 and len(stream) > H + 4 * block


@pytest.mark.parametrize("block", [256, 4096, 65280])
def test_deflated_members_inflate_to_the_same_records(case, block):
    s, body = 0, case["bodies"][0]
    members, n_rec = run(case["libs"], case["seqs"], *case["ann"], case["counts"], case["order"], s, case["header"], block, 1)
    d = bam_reader.decode_bam(members + bam_reader.EOF_BLOCK)  # (every member's BSIZE, CRC-32 and ISIZE are checked there)
    assert d["lines"] == expected_lines(body, case["names"]) and n_rec == len(d["lines"])
    assert all(m["single"] and m["btype"] in (0, 1) for m in d["members"][:-1])
    stream_bytes = sum(len(m["payload"]) for m in d["members"])
    if block >= 4096:  # a row of 1234 copies: the copies are matches of one record's distance
        assert len(members) < stream_bytes // 4, (len(members), stream_bytes)
