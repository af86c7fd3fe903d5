"""The plain-C checkers of the pipelines oracle/ does not restate (tests/cpp/*_check.c) — TEST INFRASTRUCTURE ONLY, the sibling of
oracle_lib.py.

Checker is the one place that knows how a checker object comes to exist: the build line, the temporary directory, the load, and the
canonical-form switch of an object with float forms.  Every *_checker.py declares one Checker and keeps its ctypes signatures, name
tables and numpy conveniences; the bindings of resize, gaussian_blur and linear_blur / simple_blur, three files in one object, are
below.  tests/test_*.py and scripts/fuzz_parity.py both come here.  A further checker-held pipeline costs its C file, a Checker and
its bindings.  Imports neither the product nor torch."""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import subprocess
import tempfile
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RESIZE_KERNELS = ("box", "linear", "cubic", "lanczos")        # rc_* take the index
RESIZE_TAPS = {"box": 1, "linear": 2, "cubic": 4, "lanczos": 6}
RESIZE_TYPE_INDEX = {"float32": 0, "uint8": 1, "uint16": 2}   # rc_resize's `type`

f32 = np.float32


def host_has_fma():
    """whether gcc may emit the FMA instruction for fmaf / fma (-mfma: the same correctly rounded operation, five times as fast at
    1024^3 as the call into libm)"""
    try:
        with open("/proc/cpuinfo") as f:
            return any(line.startswith("flags") and " fma " in line + " " for line in f)
    except OSError:
        return False


class Checker:
    """One shared object of tests/cpp/ `sources`, built with -O2 -Wall -Werror and `flags` on first use, once per process, under one
    lock, in a temporary directory; `bind(L)` sets its ctypes signatures.  float_forms: the object evaluates the canonical float forms
    of oracle/oracle_common.h, so it is built with check_canon.c and -ffp-contract=off, holds an o_canon_fma of its own beside
    liboracle.so's and every other checker's in the same process (-Wl,-Bsymbolic), and has the switch below."""
    _lock = threading.Lock()

    def __init__(self, name, sources, bind, float_forms=False, flags=()):
        self.name, self.bind, self.float_forms, self._lib = name, bind, float_forms, None
        self.sources = (("check_canon.c",) if float_forms else ()) + tuple(sources)
        self.flags = list(flags) + (["-ffp-contract=off", "-Wl,-Bsymbolic", "-I", os.path.join(ROOT, "oracle")] if float_forms else [])

    def lib(self):
        """The loaded shared object (the raw ctypes library)."""
        with Checker._lock:
            if self._lib is None:
                so = os.path.join(tempfile.mkdtemp(prefix=f"hlmi_{self.name}_checker"), f"lib{self.name}.so")
                subprocess.run(["gcc", "-O2", "-Wall", "-Werror", *self.flags, "-shared", "-fPIC", "-o", so]
                               + [os.path.join(ROOT, "tests", "cpp", s) for s in self.sources] + ["-lm"], check=True)
                L = C.CDLL(so)
                if self.float_forms:
                    L.ck_set_canon.argtypes = [C.c_int]
                    L.ck_get_canon.restype = C.c_int
                self.bind(L)
                self._lib = L
        return self._lib

    def set_canon(self, fma: int) -> None:
        """The object's canonical form: 0 = one rounding per operator, 1 = mul+add pairs contracted into fma.  One switch for every
        checker in the object; every other object's, and the oracle's (oracle_lib.set_canon), is a separate one."""
        self.lib().ck_set_canon(int(fma))

    def get_canon(self) -> int:
        return int(self.lib().ck_get_canon())

    @contextlib.contextmanager
    def canon(self, fma: int):
        """with xx.canon(0): ...   — evaluates the object's checkers in the given form, then restores the one in force."""
        prev = self.get_canon()
        self.set_canon(fma)
        try:
            yield self
        finally:
            self.set_canon(prev)


def _bind(L):
    I, F, P = C.c_int, C.c_float, C.c_void_p
    L.rc_halide_sin.restype = F
    L.rc_halide_sin.argtypes = [F]
    L.rc_sin_array.argtypes = [P, P, C.c_size_t]
    L.rc_sin_sweep.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.POINTER(F)]
    L.rc_tables.argtypes = [I, I, F, I, I, I, I, P, P, P]
    L.rc_resize.argtypes = [I, I, I, F, P, P, P, P, P, P]
    L.rc_taps_f.restype = F
    L.rc_taps_f.argtypes = [I, I, F]
    L.gc_radius.argtypes = [F, I]
    L.gc_kernel_table.argtypes = [F, I, P, P]
    L.gc_resampling_kernel.argtypes = [I, I, P]
    L.gc_variance.restype = F
    L.gc_variance.argtypes = [I, I]
    L.gc_sigma_lo.restype = F
    L.gc_sigma_lo.argtypes = [I, I, I, F]
    L.gc_direct.argtypes = [P, I, I, I, I, F, I, P, I, I, I, I]
    L.gc_resampled.argtypes = [I, I, I, P, I, I, I, I, F, I, P, I, I]
    L.lc_blur.argtypes = [I, P, I, I, I, I, I, I, I, P, I, I, I, I]
    for fn in (L.lc_to_linear, L.lc_to_srgb):
        fn.restype, fn.argtypes = F, [F]


checker = Checker("resize_blur", ("resize_check.c", "gaussian_blur_check.c", "linear_blur_check.c"), _bind, float_forms=True)
lib, set_canon, get_canon, canon = checker.lib, checker.set_canon, checker.get_canon, checker.canon


class _Checker:
    @property
    def lib(self):
        return lib()


# ---------------------------------------------------------------------------------------------------- resize_check.c
def resize_out_size(w, h, scale):
    """apps/resize/resize.cpp:77-78: int out_width = in.width() * scale_factor (int * float, truncated)"""
    return int(f32(w) * f32(scale)), int(f32(h) * f32(scale))


def i3(v):
    """three ints (x, y, c) as rc_resize takes its mins and extents"""
    return (C.c_int * 3)(*[int(a) for a in v])


class Resize(_Checker):
    def sin(self, x):
        x = np.ascontiguousarray(x, f32)
        out = np.empty_like(x)
        self.lib.rc_sin_array(x.ctypes.data, out.ctypes.data, x.size)
        return out

    def tables(self, kernel, up, scale, out_min, n, in_min, in_extent):
        taps = int(self.lib.rc_taps_f(RESIZE_KERNELS.index(kernel), int(up), scale))
        begin, w, sums = np.zeros(n, np.int32), np.zeros((taps, n), f32), np.zeros(n, f32)
        r = self.lib.rc_tables(RESIZE_KERNELS.index(kernel), int(up), scale, out_min, n, in_min, in_extent, begin.ctypes.data, w.ctypes.data, sums.ctypes.data)
        assert r == taps, r
        return begin, w, sums

    def resize(self, kernel, img, scale, up, out_shape=None, out_min=(0, 0, 0), in_min=(0, 0, 0)):
        """img: (C, H, W); out_shape: (C', H', W'), default the driver's int(W * scale), int(H * scale)"""
        img = np.ascontiguousarray(img)
        if out_shape is None:
            out_shape = (img.shape[0],) + resize_out_size(img.shape[2], img.shape[1], scale)[::-1]
        out = np.zeros(out_shape, img.dtype)
        r = self.lib.rc_resize(RESIZE_KERNELS.index(kernel), RESIZE_TYPE_INDEX[img.dtype.name], int(up), scale, img.ctypes.data, i3(in_min),
                               i3(img.shape[::-1]), out.ctypes.data, i3(out_min), i3(out.shape[::-1]))
        assert r == 0, r
        return out


# ---------------------------------------------------------------------------------------------------- gaussian_blur_check.c
class GaussianBlur(_Checker):
    def radius(self, sigma, trunc):
        return int(self.lib.gc_radius(sigma, trunc))

    def kernel_table(self, sigma, radius):
        kn, s = np.zeros(2 * radius + 1, f32), np.zeros(1, f32)
        self.lib.gc_kernel_table(sigma, radius, kn.ctypes.data, s.ctypes.data)
        return kn, s[0]

    def resampling_kernel(self, order, factor):
        k = np.zeros(order * factor, f32)
        self.lib.gc_resampling_kernel(order, factor, k.ctypes.data)
        return k

    def sigma_lo(self, u, d, f, sigma):
        return float(self.lib.gc_sigma_lo(u, d, f, sigma))

    def direct(self, img, sigma, trunc, out_shape=None, out_min=None, in_min=(0, 0)):
        """img: (H, W); out_shape: (H', W'), default the image's own region"""
        img = np.ascontiguousarray(img, f32)
        out_shape = img.shape if out_shape is None else out_shape
        out_min = in_min if out_min is None else out_min
        out = np.zeros(out_shape, f32)
        r = self.lib.gc_direct(img.ctypes.data, in_min[0], in_min[1], img.shape[1], img.shape[0], sigma, trunc, out.ctypes.data, out_min[0], out_min[1],
                               out.shape[1], out.shape[0])
        assert r == 0, r
        return out

    def resampled(self, udf, img, sigma, trunc, out_shape=None, in_min=(0, 0)):
        img = np.ascontiguousarray(img, f32)
        out = np.zeros(img.shape if out_shape is None else out_shape, f32)
        r = self.lib.gc_resampled(*udf, img.ctypes.data, in_min[0], in_min[1], img.shape[1], img.shape[0], sigma, trunc, out.ctypes.data, out.shape[1],
                                  out.shape[0])
        assert r == 0, r
        return out


# ---------------------------------------------------------------------------------------------------- linear_blur_check.c
class LinearBlur(_Checker):
    def to_linear(self, s):
        return f32(self.lib.lc_to_linear(float(s)))

    def to_srgb(self, l):
        return f32(self.lib.lc_to_srgb(float(l)))

    def blur(self, name, img, width=None, height=None, out_shape=None, out_min=None, in_min=(0, 0, 0), expect=0):
        """img: (C, H, W) at mins in_min = (x, y, c); out_shape: (C', H', W') at out_min, default the image's own region.  width and
        height (simple_blur): default the image's."""
        img = np.asarray(img, f32)
        out_shape = img.shape if out_shape is None else out_shape
        out_min = in_min if out_min is None else out_min
        c0 = out_min[2] - in_min[2]
        assert 0 <= c0 and c0 + out_shape[0] <= img.shape[0]
        mine = np.ascontiguousarray(img[c0:c0 + out_shape[0]])
        out = np.zeros(out_shape, f32)
        r = self.lib.lc_blur(int(name == "linear_blur"), mine.ctypes.data, in_min[0], in_min[1], img.shape[2], img.shape[1], out_shape[0],
                             img.shape[2] if width is None else width, img.shape[1] if height is None else height, out.ctypes.data,
                             out_min[0], out_min[1], out_shape[2], out_shape[1])
        assert r == expect, r
        return out


resize, gaussian_blur, linear_blur = Resize(), GaussianBlur(), LinearBlur()
