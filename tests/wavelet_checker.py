"""ctypes bindings to tests/cpp/wavelet_check.c, the plain-C checker of haar_x, inverse_haar_x, daubechies_x and
inverse_daubechies_x — TEST INFRASTRUCTURE ONLY, the sibling of checker_lib.py.

The checker is built with tests/cpp/check_canon.c into a shared object of its own, with checker_lib.py's build line, once per
process, in a temporary directory; tests/test_wavelet.py and scripts/fuzz_parity.py both come here.  Its canonical-form switch is
its own copy of check_canon.c's (-Wl,-Bsymbolic), separate from checker_lib's and the oracle's.  Imports neither the product nor
torch."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = ("check_canon.c", "wavelet_check.c")
NAMES = ("haar_x", "inverse_haar_x", "daubechies_x", "inverse_daubechies_x")

_lock = threading.Lock()
_lib = []
f32 = np.float32


def lib():
    """The loaded shared object (the raw ctypes library), built on the first call."""
    with _lock:
        if not _lib:
            so = os.path.join(tempfile.mkdtemp(prefix="hlmi_wavelet_checker"), "libwaveletcheck.so")
            subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-Wl,-Bsymbolic", "-I", os.path.join(ROOT, "oracle"), "-o", so]
                           + [os.path.join(ROOT, "tests", "cpp", s) for s in SOURCES] + ["-lm"], check=True)
            L = C.CDLL(so)
            I, P = C.c_int, C.c_void_p
            L.ck_set_canon.argtypes = [I]
            L.ck_get_canon.restype = I
            L.wc_constant.restype, L.wc_constant.argtypes = C.c_float, [I]
            L.wc_forward.argtypes = [I, P, I, I, I, I, P, I, I, I, I, I, I]
            L.wc_inverse.argtypes = [I, P, I, I, I, I, I, I, P, I, I, I, I]
            _lib.append(L)
    return _lib[0]


def set_canon(fma: int) -> None:
    """The checker's canonical form (oracle/oracle_common.h): 0 = one rounding per operator, 1 = mul+add pairs contracted."""
    lib().ck_set_canon(int(fma))


def get_canon() -> int:
    return int(lib().ck_get_canon())


class canon:
    """with wavelet_checker.canon(0): ...   — evaluates the checker in the given form, then restores the one in force."""

    def __init__(self, fma: int):
        self.fma = int(fma)

    def __enter__(self):
        self.prev = get_canon()
        set_canon(self.fma)
        return self

    def __exit__(self, *exc):
        set_canon(self.prev)
        return False


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
