"""ctypes bindings to tests/cpp/mat_mul_check.c, the plain-C checker of apps/cuda_mat_mul — TEST INFRASTRUCTURE ONLY, the sibling of
hexagon_benchmarks_checker.py.

The checker is one fmaf chain per output, the contract in both canonical float forms: it needs neither check_canon.c nor a
canonical-form switch.  It is built into a shared object of its own, once per process, in a temporary directory, with
-ffp-contract=off; where the host has the FMA instruction (the `fma` flag of /proc/cpuinfo) the compiler may emit it for fmaf
(-mfma: the same correctly rounded operation, five times as fast at 1024^3 as the call into libm), otherwise fmaf stays libm's.
tests/test_mat_mul.py and scripts/fuzz_parity.py both come here.  Imports neither the product nor torch."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = ("mat_mul_check.c",)

_lock = threading.Lock()
_lib = []


def host_has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return any(line.startswith("flags") and " fma " in line + " " for line in f)
    except OSError:
        return False


def lib():
    """The loaded shared object (the raw ctypes library), built on the first call."""
    with _lock:
        if not _lib:
            so = os.path.join(tempfile.mkdtemp(prefix="hlmi_mat_mul_checker"), "libmatmulcheck.so")
            flags = ["-O2", "-ftree-vectorize", "-ffp-contract=off", "-Wall", "-Werror"] + (["-mfma"] if host_has_fma() else [])
            subprocess.run(["gcc"] + flags + ["-shared", "-fPIC", "-o", so] + [os.path.join(ROOT, "tests", "cpp", s) for s in SOURCES] + ["-lm"], check=True)
            L = C.CDLL(so)
            L.mm_check.restype, L.mm_check.argtypes = None, [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_int]
            _lib.append(L)
    return _lib[0]


def _square(m):
    m = np.asarray(m)
    assert m.ndim == 2 and m.dtype == np.float32 and m.shape[0] == m.shape[1] and m.shape[0] > 0 and (m.strides[1] == 4 or m.shape[1] == 1)
    return m, (m.strides[0] // 4 if m.shape[0] > 1 else m.shape[1])


def run(A, B):
    """out[y][x] = the chain over r of fmaf(A[r][x], B[y][r], .) from +0: (n, n) float32 arrays (rows may be padded), the row-major
    product B @ A in the contract's order.  Returns a dense (n, n) float32 array."""
    A, sa = _square(A)
    B, sb = _square(B)
    n = A.shape[0]
    assert B.shape == A.shape
    out = np.empty((n, n), np.float32)
    lib().mm_check(A.ctypes.data, sa, B.ctypes.data, sb, out.ctypes.data, n, n)
    return out
