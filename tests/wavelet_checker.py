"""ctypes bindings to tests/cpp/wavelet_check.c, the plain-C checker of haar_x, inverse_haar_x, daubechies_x and
inverse_daubechies_x — TEST INFRASTRUCTURE ONLY.

A checker_lib.Checker with float forms: a shared object of its own, with a canonical-form switch of its own, separate from every
other checker's and the oracle's.  tests/test_wavelet.py and scripts/fuzz_parity.py both come here.  Imports neither the product
nor torch."""
from __future__ import annotations

import ctypes as C

import numpy as np

from checker_lib import Checker

NAMES = ("haar_x", "inverse_haar_x", "daubechies_x", "inverse_daubechies_x")
f32 = np.float32


def _bind(L):
    I, P = C.c_int, C.c_void_p
    L.wc_constant.restype, L.wc_constant.argtypes = C.c_float, [I]
    L.wc_forward.argtypes = [I, P, I, I, I, I, P, I, I, I, I, I, I]
    L.wc_inverse.argtypes = [I, P, I, I, I, I, I, I, P, I, I, I, I]


checker = Checker("wavelet", ("wavelet_check.c",), _bind, float_forms=True)
lib, set_canon, get_canon, canon = checker.lib, checker.set_canon, checker.get_canon, checker.canon


def constants():
    """D0 .. D3 as the checker holds them"""
    return [f32(lib().wc_constant(i)) for i in range(4)]


def is_inverse(name):
    assert name in NAMES, name
    return name.startswith("inverse_")


def forward(name, img, out_shape=None, out_min=None, in_min=(0, 0), expect=0):
    """img: (H, W) at mins in_min = (x, y); the output (C, H', W') at out_min = (x, y, c), default the driver's: (2, H, W // 2)
    at (0, 0, 0) (apps/wavelet/wavelet.cpp:61)"""
    assert not is_inverse(name)
    img = np.ascontiguousarray(img, f32)
    out_shape = (2, img.shape[0], img.shape[1] // 2) if out_shape is None else out_shape
    out_min = (0, 0, 0) if out_min is None else out_min
    out = np.zeros(out_shape, f32)
    r = lib().wc_forward(int(name == "daubechies_x"), img.ctypes.data, in_min[0], in_min[1], img.shape[1], img.shape[0], out.ctypes.data,
                         out_min[0], out_min[1], out_min[2], out_shape[2], out_shape[1], out_shape[0])
    assert r == expect, r
    return out


def inverse(name, img, out_shape=None, out_min=None, in_min=(0, 0, 0), expect=0):
    """img: (C, H, W2) at mins in_min = (x, y, c); the output (H', W') at out_min = (x, y), default the driver's: (H, 2 * W2) at
    (0, 0) (apps/wavelet/wavelet.cpp:62)"""
    assert is_inverse(name)
    img = np.ascontiguousarray(img, f32)
    out_shape = (img.shape[1], 2 * img.shape[2]) if out_shape is None else out_shape
    out_min = (0, 0) if out_min is None else out_min
    out = np.zeros(out_shape, f32)
    r = lib().wc_inverse(int(name == "inverse_daubechies_x"), img.ctypes.data, in_min[0], in_min[1], in_min[2], img.shape[2], img.shape[1],
                         img.shape[0], out.ctypes.data, out_min[0], out_min[1], out_shape[1], out_shape[0])
    assert r == expect, r
    return out


def run(name, img, **kw):
    return (inverse if is_inverse(name) else forward)(name, img, **kw)
