"""ctypes bindings to tests/cpp/mat_mul_check.c, the plain-C checker of apps/cuda_mat_mul — TEST INFRASTRUCTURE ONLY.

The checker is one fmaf chain per output, the contract in both canonical float forms: a checker_lib.Checker without float forms,
so without a canonical-form switch, but built with -ffp-contract=off; where the host has the FMA instruction (the `fma` flag of
/proc/cpuinfo) the compiler may emit it for fmaf (-mfma), otherwise fmaf stays libm's.  tests/test_mat_mul.py and scripts/fuzz_parity.py both come here.  Imports neither the product nor torch."""
from __future__ import annotations

import ctypes as C

import numpy as np

from checker_lib import Checker, host_has_fma


def _bind(L):
    L.mm_check.restype, L.mm_check.argtypes = None, [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_int]


lib = Checker("mat_mul", ("mat_mul_check.c",), _bind, flags=["-ftree-vectorize", "-ffp-contract=off"] + (["-mfma"] if host_has_fma() else [])).lib


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
