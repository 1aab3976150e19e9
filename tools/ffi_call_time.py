"""What the declared signatures of ``_ffi.load()`` cost per call, on the CPU: two entry points that return before any HIP call
(``mirge_count_join`` on a NULL context, ``mirge_reads_count`` on a NULL read set), each timed through the typed binding with bare
arguments and through a second, plain ``CDLL`` of the same library with every argument wrapped by hand, as the wrappers did before the
signatures were declared.  Needs the built library, no GPU.  profiles/ffi_signatures.md holds a run.

    python tools/ffi_call_time.py [--calls 200000] [--repeats 7]
"""
import argparse
import ctypes as C
import json
import os
import sys
import timeit

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import mirge3_amd  # noqa: E402,F401
from mirge3_amd import _ffi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200000)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    typed, plain = _ffi.load(), C.CDLL(_ffi.SO_PATH)
    plain.mirge_reads_count.restype = C.c_int64
    cls, ex, iso = np.zeros((9, 1), np.int64), np.zeros((10, 1), np.int64), np.zeros((10, 1), np.int64)
    null, exact_pass, iso_pass, n_mirna = C.c_void_p(), 0, 8, 10
    p = lambda arr: C.c_void_p(arr.ctypes.data) if arr is not None else C.c_void_p(0)
    cases = {
        "count_join typed": lambda: typed.mirge_count_join(null, null, null, exact_pass, iso_pass, n_mirna, cls, ex, iso),
        "count_join hand-wrapped": lambda: plain.mirge_count_join(null, null, null, C.c_int32(exact_pass), C.c_int32(iso_pass),
                                                                  C.c_int64(n_mirna), p(cls), p(ex), p(iso)),
        "count_join typed, arrays as addresses": lambda: typed.mirge_count_join(
            null, null, null, exact_pass, iso_pass, n_mirna, C.c_void_p(cls.ctypes.data), C.c_void_p(ex.ctypes.data), C.c_void_p(iso.ctypes.data)),
        "reads_count typed": lambda: typed.mirge_reads_count(null),
        "reads_count hand-wrapped": lambda: plain.mirge_reads_count(null),
    }
    for fn in cases.values():
        assert fn() == -1
    out = {}
    for name, fn in cases.items():
        t = sorted(x / a.calls * 1e6 for x in timeit.repeat(fn, number=a.calls, repeat=a.repeats))
        out[name] = {"median_us": round(t[len(t) // 2], 3), "min_us": round(t[0], 3), "max_us": round(t[-1], 3)}
        print(f"{name:40s} {out[name]['median_us']:7.3f} us per call (min {t[0]:.3f}, max {t[-1]:.3f})")
    print(json.dumps({"calls": a.calls, "repeats": a.repeats, "us_per_call": out}))


if __name__ == "__main__":
    main()
