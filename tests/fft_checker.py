"""ctypes bindings to tests/cpp/fft_check.c, the plain-C checker of the four 2-D transforms of apps/fft — TEST INFRASTRUCTURE ONLY.

A checker_lib.Checker with float forms: a shared object and a canonical-form switch of its own.  tests/test_fft.py and
scripts/fuzz_parity.py both come here.  Imports neither the product nor torch: use_twiddles() takes the address of the library's
table function from whoever has loaded the library."""
from __future__ import annotations

import ctypes as C

import numpy as np

from checker_lib import Checker

KINDS = ("c2c_forward", "c2c_inverse", "r2c", "c2r")
V = 8   # FC_V
f32 = np.float32


def _bind(L):
    I, P = C.c_int, C.c_void_p
    L.fc_twiddles.restype, L.fc_twiddles.argtypes = None, [I, I, C.c_float, P]
    L.fc_set_twiddle_fn.restype, L.fc_set_twiddle_fn.argtypes = None, [P]
    L.fc_radix_factor.argtypes = [I, P]
    L.fc_size_ok.argtypes = [I]
    L.fc_zip_width.argtypes = [I, I, I, I]
    L.fc_fft2d.argtypes = [I, I, I, C.c_float, I, P, C.c_long, P, C.c_long]


checker = Checker("fft", ("fft_check.c",), _bind, float_forms=True)
lib, set_canon, get_canon, canon = checker.lib, checker.set_canon, checker.get_canon, checker.canon


def use_twiddles(fn_address) -> None:
    """Build the tables with the function at this address (the library's hlmi_fft_twiddles) from now on; None = the checker's own."""
    lib().fc_set_twiddle_fn(C.c_void_p(fn_address) if fn_address else None)


def twiddles(n, sign, gain):
    """the table of (n = R S, sign, gain) as the checker's own function builds it: (n, 2) float32"""
    out = np.empty((n, 2), f32)
    lib().fc_twiddles(int(n), int(sign), float(gain), out.ctypes.data)
    return out


def radix_factor(n):
    R = (C.c_int * 16)()
    k = lib().fc_radix_factor(int(n), R)
    return list(R[:k])


def size_ok(n):
    return bool(lib().fc_size_ok(int(n)))


def zip_width(kind, n0, n1, v=V):
    return int(lib().fc_zip_width(KINDS.index(kind), n0, n1, v))


def out_shape(kind, n0, n1):
    return {"r2c": (n1 // 2 + 1, n0, 2), "c2r": (n1, n0)}.get(kind, (n1, n0, 2))


def in_shape(kind, n0, n1):
    return {"r2c": (n1, n0), "c2r": (n1 // 2 + 1, n0, 2)}.get(kind, (n1, n0, 2))


def run(kind, x, n1=None, gain=1.0, v=V, expect=0):
    """The transform `kind` of x: complex arrays are float32 [rows, N0, 2], real ones float32 [rows, N0].  n1: the transform's N1
    (default: what x's rows imply; a c2r input may be taller than N1/2 + 1).  Returns a dense float32 array of out_shape()."""
    x = np.ascontiguousarray(x, f32)
    n0 = x.shape[1]
    if n1 is None:
        n1 = 2 * (x.shape[0] - 1) if kind == "c2r" else x.shape[0]
    assert x.shape[0] >= in_shape(kind, n0, n1)[0] and x.shape[1:] == in_shape(kind, n0, n1)[1:], (kind, x.shape, n1)
    out = np.zeros(out_shape(kind, n0, n1), f32)
    r = lib().fc_fft2d(KINDS.index(kind), n0, n1, float(gain), int(v), x.ctypes.data, x.strides[0] // 4, out.ctypes.data, out.strides[0] // 4)
    assert r == expect, r
    return out
