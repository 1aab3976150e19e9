"""CPU tests of the ctypes binding's signature table (``_ffi.SIGNATURES``): it is include/mirge_native.h, ``_ffi.bind`` declares it on
whatever library it is handed, and a call through it is checked before it is made."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mirge3_amd  # noqa: F401
from mirge3_amd import _ffi

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def header_prototypes():
    """[(name, return type, [parameter types])] of include/mirge_native.h in its order: comments and struct bodies stripped, parameter
    names dropped, ``[N]`` read as ``*``, ``T * x`` / ``T *x`` spelt ``T*``"""
    text = open(os.path.join(ROOT, "include", "mirge_native.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"typedef\s+struct\s+\w*\s*\{.*?\}\s*\w+\s*;", " ", text, flags=re.S)

    def spell(t):
        t = re.sub(r"\s*\*\s*", "* ", " ".join(t.split())).strip()
        return re.sub(r"\* (?=\*)", "*", t)

    out = []
    for ret, name, params in re.findall(r"^\s*([A-Za-z_][\w \t\*]*?)\b(mirge_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        types = []
        for p in params.split(","):
            p = " ".join(p.split())
            if p == "void":
                continue
            m = re.fullmatch(r"(.*?)(\w+)\s*(\[\d*\])?", p)
            assert m and m.group(1).strip(), (name, p)  # every parameter of the header is named
            types.append(spell(m.group(1) + ("*" if m.group(3) else "")))
        out.append((name, spell(ret), types))
    return out


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return _ffi.load()


def test_the_table_is_the_header():
    hdr = header_prototypes()
    assert len(hdr) >= 96 and len({n for n, _, _ in hdr}) == len(hdr)
    assert [n for n, _, _ in hdr] == list(_ffi.SIGNATURES) == _ffi.EXPORTS
    for name, ret, params in hdr:
        assert _ffi.SIGNATURES[name] == (ret, tuple(params)), name
    # the spellings the table must keep apart
    assert _ffi.SIGNATURES["mirge_ctx_pool_stats"] == ("int", ("mirge_ctx*", "int64_t*"))  # int64_t out[3]
    assert _ffi.SIGNATURES["mirge_last_error"] == ("const char*", ())
    assert _ffi.SIGNATURES["mirge_reads_concat"][1][1] == "const mirge_reads* const*"


def test_every_symbol_of_the_built_library_is_declared(lib):
    for name, (ret, params) in _ffi.SIGNATURES.items():
        fn = getattr(lib, name)  # the built library has them all (test_abi_exports_every_declared_symbol)
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), name
        assert [_ffi._ctype(t) for t in params] == list(fn.argtypes), name
        want = {"void": None, "int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "const char*": C.c_char_p}[ret]
        assert fn.restype is want, name
    assert lib.mirge_reads_count.restype is C.c_int64 and lib.mirge_ctx_destroy.restype is None
    assert lib.mirge_cascade_run.argtypes[3] is C.POINTER(_ffi.MirgePolicy) and lib.mirge_sam_write_device.argtypes[7] is C.POINTER(_ffi.SamPass)
    from mirge3_amd import sam_export
    assert sam_export.SamPass is _ffi.SamPass


def test_a_library_without_the_symbols_binds_without_error():
    libc = C.CDLL("libc.so.6")
    assert _ffi.bind(libc) is libc
    assert not any(hasattr(libc, n) for n in _ffi.EXPORTS)
    assert libc.memcpy.argtypes is None  # nothing else was touched


def test_calls_without_a_gpu_answer_as_the_c_code_says(lib):
    assert lib.mirge_reads_count(None) == -1  # (an int64_t return)
    assert lib.mirge_reads_n_samples(None) == -1
    assert lib.mirge_umi_cluster_stats(np.zeros(5, np.int64)) == 0
    assert lib.mirge_kmer_correct_stats(np.zeros(192, np.int64)) >= 0
    cls, ex, iso = np.zeros((9, 1), np.int64), np.zeros((10, 1), np.int64), np.zeros((10, 1), np.int64)
    assert lib.mirge_count_join(None, None, None, 0, 8, 10, cls, ex, iso) == -1
    assert b"mirge_count_join" in lib.mirge_last_error()
    # numpy integers and bool are integers
    assert lib.mirge_count_join(None, None, None, np.int32(0), True, np.int64(10), cls, ex, iso) == -1
    assert _ffi.umi_cluster_stats().keys() == {"tagged", "eligible", "linked", "rounds", "slots"} and isinstance(_ffi.kmer_correct_stats(), list)


def test_wrong_arguments_are_refused_before_the_call(lib):
    a = np.zeros(8, np.int64)
    frozen = np.zeros(8, np.int64)
    frozen.flags.writeable = False
    join = lambda *args: lib.mirge_count_join(None, None, None, *args)
    for bad in (a.astype(np.int32), a.astype(np.uint64), np.zeros(16, np.int64)[::2], frozen, b"12345678", "text", 2.5):
        with pytest.raises(C.ArgumentError, match="argument 1"):
            lib.mirge_umi_cluster_stats(bad)  # int64_t*
        with pytest.raises(C.ArgumentError, match="argument 8"):
            join(0, 8, 10, a, bad, a)
    with pytest.raises(C.ArgumentError, match="int64"):  # the message names the dtype wanted
        lib.mirge_umi_cluster_stats(a.astype(np.int32))
    # a const pointer takes the read-only array (and refuses the rest all the same); const bytes take bytes
    gz = lambda src, dst: lib.mirge_gz_inflate(src, 8, dst, 8, C.byref(C.c_int64()), 1)
    assert gz(np.frombuffer(b"\0" * 8, np.uint8), np.zeros(8, np.uint8)) != 0 and gz(b"\0" * 8, np.zeros(8, np.uint8)) != 0
    for src, dst, n in ((frozen, np.zeros(8, np.uint8), 1), (np.zeros(8, np.int8), np.zeros(8, np.uint8), 1),
                        (np.zeros(8, np.uint8), np.frombuffer(b"\0" * 8, np.uint8), 3), (np.zeros(8, np.uint8), b"\0" * 8, 3)):
        with pytest.raises(C.ArgumentError, match=f"argument {n}"):
            gz(src, dst)
    for bad in (2.5, None, "8", C.c_int32(1), C.c_double(1)):  # ... for an int64_t
        with pytest.raises(C.ArgumentError, match="argument 6"):
            join(0, 8, bad, a, a, a)
    for bad in (2.5, None, C.c_int64(1)):  # ... for an int32_t
        with pytest.raises(C.ArgumentError, match="argument 4"):
            join(bad, 8, 10, a, a, a)
    with pytest.raises(C.ArgumentError, match="argument 6"):  # a struct pointer takes its own struct only
        lib.mirge_reads_parse_trim(None, None, 0, 0, 0, _ffi.MirgeUmi(), None, None)


def test_every_pointer_takes_null_an_address_and_byref(lib):
    a = np.zeros(8, np.int64)
    for ok in (C.c_void_p(a.ctypes.data), (C.c_int64 * 8)()):  # (five numbers are written)
        assert lib.mirge_umi_cluster_stats(ok) == 0
    for ok in (None, C.c_void_p(a.ctypes.data), C.byref(C.c_int64()), C.c_void_p(0)):
        # a handle and arrays alike; the C side refuses the call for its NULL read set before it looks at any of them
        assert lib.mirge_count_join(ok, None, None, 0, 8, 10, ok, ok, ok) == -1
    assert lib.mirge_count_join(None, None, None, C.c_int32(0), C.c_int32(8), C.c_int64(10), a, a, a) == -1  # wrapped at the right width
    assert lib.mirge_reads_parse_trim(None, None, 0, 0, 0, _ffi.MirgeTrim.make(), None, None) != 0  # the struct itself, or None
    assert lib.mirge_reads_parse_trim(None, None, 0, 0, 0, None, None, None) != 0
