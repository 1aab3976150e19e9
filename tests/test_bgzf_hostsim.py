"""``k_bgzf_text`` (csrc/kernels_bgzf.hpp) on the CPU: the kernel compiled for the host (tests/hostsim/bgzf_sim.cpp: one workgroup of 256
std::threads behind a futex barrier), every stream of tests/bgzf_cases.py held against the specification of mirge3_amd/bgzf.py -- the file
inflates to the stream, every member to its slice with its CRC-32 and ISIZE, none beyond n + 31 bytes, the form chosen as the rule says in
both directions, the tallies what the call reports.  tests/test_bgzf_gpu.py holds the device's files against these byte for byte."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import bgzf_cases

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostsim", "bgzf_sim.cpp")
SO = os.path.join(HERE, "hostsim", "_build", "libbgzfsim.so")
CSRC = os.path.join(HERE, "..", "mirge3.0_amd", "csrc")


def _sim():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("kernels_sam.hpp", "kernels_bam.hpp", "kernels_bgzf.hpp")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-pthread", "-o", SO, SRC])
    sim = C.CDLL(SO)
    sim.sim_bgzf.restype = C.c_longlong
    return sim


@functools.lru_cache(maxsize=None)
def run(s: bytes, block: int, shift: int = 0):
    """-> (the .gz file, its .gzi, stats as ``bgzf.stats_dict`` spells them) of the kernel on the host"""
    sim = _sim()
    n_blocks = (len(s) + block - 1) // block
    src = np.frombuffer(s, dtype=np.uint8) if s else np.zeros(1, np.uint8)
    out = np.full(len(s) + 31 * n_blocks + 64, 0xEE, np.uint8)
    gzi = np.zeros(2 * n_blocks + 2, np.uint64)
    stats = np.zeros(4, np.int64)
    n = sim.sim_bgzf(C.c_void_p(src.ctypes.data), C.c_longlong(len(s)), C.c_uint32(block), C.c_uint32(shift), C.c_void_p(out.ctypes.data),
                     C.c_longlong(out.size), C.c_void_p(gzi.ctypes.data), C.c_longlong(gzi.size), C.c_void_p(stats.ctypes.data))
    assert n >= 28, n
    st = dict(file_bytes=int(stats[0]), stored=int(stats[1]), fixed=int(stats[2]), dynamic=int(stats[3]), members=n_blocks, stream_bytes=len(s))
    return out[:n].tobytes(), gzi[:1 + 2 * int(gzi[0])].astype("<u8").tobytes(), st


@pytest.mark.parametrize("name", sorted(bgzf_cases.all_cases()))
def test_every_stream(name):
    s, block = bgzf_cases.all_cases()[name]
    gz, gzi, st = run(s, block)
    btypes = bgzf_cases.check_device_file(s, block, gz, gzi, st)
    print(f"{name}: {len(s)} -> {len(gz)} bytes; members stored / fixed / dynamic {btypes}")
    if name.startswith("random"):
        assert btypes == [1, 0, 0]
    if name.startswith(("one_letter", "no_match", "high_bytes")):
        assert btypes[0] == 0 and btypes[1] == 0  # a code of the block's own has to win
    if name.startswith("codes"):
        import deflate_dyn_probe as dy
        import deflate_probe as dp
        from mirge3_amd import bgzf
        lens, dists = set(), set()
        for m in bgzf.members(gz):
            cdata = gz[m["offset"] + 18:m["offset"] + m["bsize"] - 8]
            syms = dy.dynamic_symbols(cdata)[0] if m["btype"] == 2 else dp.fixed_symbols(cdata) if m["btype"] == 1 else []
            lens |= {x[2] for x in syms if not isinstance(x, int)}
            dists |= {x[3] for x in syms if not isinstance(x, int)}
        assert lens >= dp.REACHABLE_LEN_CODES and dists >= dp.REACHABLE_DIST_CODES, (sorted(lens), sorted(dists))


@pytest.mark.parametrize("shift", [1, 7, 15])
def test_the_file_does_not_depend_on_where_the_buffer_lies(shift):
    """the source's offset in its 16 bytes decides which bytes go through the kernel's wide loads"""
    for name in ("text3_b256", "text257_b256", "sam_S2_b256", "sam_S2_b4096"):
        s, block = bgzf_cases.all_cases()[name]
        assert run(s, block, shift)[:2] == run(s, block)[:2], name


def test_the_stand_alone_program_builds(tmp_path):
    """-DBGZF_SIM_MAIN: the program the sanitizer build runs (here without a sanitizer: that it builds and ends with 0)"""
    exe = str(tmp_path / "bgzf_main")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-pthread", "-DBGZF_SIM_MAIN", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "dynamic" in r.stdout, r.stderr[-2000:]
