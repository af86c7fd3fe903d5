"""ctypes bindings to tests/cpp/linear_algebra_check.c, the plain-C checker of the pipelines of apps/linear_algebra, twelve f32 and twelve
f64 — TEST INFRASTRUCTURE ONLY.

A checker_lib.Checker with float forms: one shared object and one canonical-form switch for both element types; where the host has the
FMA instruction the compiler may emit it for fmaf / fma (-mfma).  The bindings are one class, LinearAlgebra, with an instance per element
type: `f32` (la_*, the s routines, V = 8) and `f64` (ld_*, the d routines, V = 4).  Each routine is there under its plain name (f32.dot)
and its BLAS name (f32.sdot, f64.ddot).  tests/test_linear_algebra.py, tests/test_linear_algebra_f64.py and scripts/fuzz_parity.py come
here.  Imports neither the product nor torch.

Arrays: a vector is a 1-D array of the element type; a matrix with Halide extents (w, h) — dimension 0 innermost, column-major in BLAS
terms — is a numpy array of shape (h, w) whose rows may be padded: A(i, k) is A[k, i]."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from checker_lib import Checker, host_has_fma
from parity_helpers import DevArray, HostArray

ROUTINES = ("copy", "scal", "axpy", "dot", "asum", "gemv", "ger", "gemm")


def _bind(L):
    I, P, N = C.c_int, C.c_void_p, C.c_long
    for p, F in (("la_", C.c_float), ("ld_", C.c_double)):
        for name, restype, argtypes in (("v", I, []), ("axpy", None, [I, F, P, P, P, N]), ("dot_v", F, [P, P, N, I]), ("asum_v", F, [P, N, I]),
                                        ("gemv", None, [I, F, P, N, I, I, P, F, P, P, I]), ("ger", None, [F, P, I, P, I, P, N]),
                                        ("gemm", None, [I, I, F, P, N, P, N, F, P, N, P, N, I, I, I, P]), ("compare", I, [F, F, F]),
                                        ("compare_all", F, [P, P, N, F, C.POINTER(I)])):
            fn = getattr(L, p + name)
            fn.restype, fn.argtypes = restype, argtypes


checker = Checker("linear_algebra", ("linear_algebra_check.c",), _bind, float_forms=True, flags=["-ftree-vectorize"] + (["-mfma"] if host_has_fma() else []))


def _p(a):
    return a.ctypes.data


class LinearAlgebra:
    """The checker's routines for one element type: `letter` is the BLAS one (s, d), `prefix` the C one (la_, ld_), V the generators'
    vector width (asserted against the checker's and the kernels' constant by the tests)."""
    lib, set_canon, get_canon, canon = checker.lib, checker.set_canon, checker.get_canon, checker.canon

    def __init__(self, dtype, letter, prefix, V):
        self.dtype, self.prefix, self.V, self.EPS = np.dtype(dtype), prefix, V, float(np.finfo(dtype).eps)
        h = f"halide_{letter}"
        self.NAMES = (h + "copy_impl", h + "scal_impl", h + "axpy_impl", h + "dot", h + "asum", h + "gemv_notrans", h + "gemv_trans", h + "ger_impl",
                      h + "gemm_notrans", h + "gemm_transA", h + "gemm_transB", h + "gemm_transAB")
        self.GEMM_FLAGS = {h + "gemm_notrans": (0, 0), h + "gemm_transA": (1, 0), h + "gemm_transB": (0, 1), h + "gemm_transAB": (1, 1)}
        for r in ROUTINES:
            setattr(self, letter + r, getattr(self, r))
        self.Arr = functools.partial(Arr, self.dtype)

    def _fn(self, name):
        return getattr(checker.lib(), self.prefix + name)

    def _vec(self, x):
        x = np.asarray(x)
        assert x.ndim == 1 and x.dtype == self.dtype and (x.size <= 1 or x.strides[0] == x.itemsize), (x.shape, x.dtype, x.strides)
        return x

    def _mat(self, m):
        """(array, column stride in elements); rows of the numpy array are the matrix's columns and may be padded"""
        m = np.asarray(m)
        assert m.ndim == 2 and m.dtype == self.dtype and (m.shape[1] <= 1 or m.strides[1] == m.itemsize), (m.shape, m.dtype, m.strides)
        return m, (m.strides[0] // m.itemsize if m.shape[0] > 1 else max(m.shape[1], 1))

    def copy(self, x):
        x = self._vec(x)
        out = np.empty(x.size, self.dtype)
        self._fn("axpy")(0, 0.0, _p(x), None, _p(out), x.size)
        return out

    def scal(self, a, x):
        x = self._vec(x)
        out = np.empty(x.size, self.dtype)
        self._fn("axpy")(1, a, _p(x), None, _p(out), x.size)
        return out

    def axpy(self, a, x, y):
        x, y = self._vec(x), self._vec(y)
        assert x.size == y.size
        out = np.empty(x.size, self.dtype)
        self._fn("axpy")(2, a, _p(x), _p(y), _p(out), x.size)
        return out

    def dot(self, x, y, v=None):
        """0-dimensional array"""
        x, y = self._vec(x), self._vec(y)
        assert x.size == y.size
        return np.array(self._fn("dot_v")(_p(x), _p(y), x.size, self.V if v is None else v), self.dtype)

    def asum(self, x, v=None):
        x = self._vec(x)
        return np.array(self._fn("asum_v")(_p(x), x.size, self.V if v is None else v), self.dtype)

    def gemv(self, trans, a, A, x, b, y, v=None):
        """A: shape (h, w).  notrans: x[h], y[w]; trans: x[w], y[h]"""
        (A, lda), x, y = self._mat(A), self._vec(x), self._vec(y)
        h, w = A.shape
        assert (x.size, y.size) == ((w, h) if trans else (h, w)), (A.shape, x.size, y.size, trans)
        out = np.empty(y.size, self.dtype)
        self._fn("gemv")(int(bool(trans)), a, _p(A), lda, w, h, _p(x), b, _p(y), _p(out), self.V if v is None else v)
        return out

    def ger(self, a, x, y, R):
        """R: shape (n, m) for x[m], y[n]; returns the updated matrix, dense; R is not written"""
        x, y = self._vec(x), self._vec(y)
        out = np.ascontiguousarray(R, self.dtype).copy()
        assert out.shape == (y.size, x.size)
        self._fn("ger")(a, _p(x), x.size, _p(y), y.size, _p(out), max(x.size, 1))
        return out

    def gemm(self, ta, tb, a, A, B, b, Cm):
        """A: shape (K, M) as stored, B: (N, K), C: (N, M); the transposed operands square (asserted here: the checker's C leaves it to us)"""
        (A, lda), (B, ldb), (Cm, ldc) = self._mat(A), self._mat(B), self._mat(Cm)
        K, M = A.shape
        N = B.shape[0]
        assert B.shape == (N, K) and Cm.shape == (N, M) and (not ta or M == K) and (not tb or N == K), (A.shape, B.shape, Cm.shape, ta, tb)
        out, scratch = np.empty((N, M), self.dtype), np.empty(max(M, 1), self.dtype)
        self._fn("gemm")(int(bool(ta)), int(bool(tb)), a, _p(A), lda, _p(B), ldb, b, _p(Cm), ldc, _p(out), max(M, 1), M, N, K, _p(scratch))
        return out

    def compare(self, expected, actual, eps_multiple):
        """compareScalars over two arrays of one shape with epsilon = eps_multiple * the type's epsilon: (every pair accepted, the worst
        |x - y| / (|x| + |y|) in units of that epsilon)"""
        e, a = np.ascontiguousarray(expected, self.dtype).ravel(), np.ascontiguousarray(actual, self.dtype).ravel()
        assert e.size == a.size
        ok = C.c_int(0)
        worst = self._fn("compare_all")(_p(e), _p(a), e.size, eps_multiple * self.EPS, C.byref(ok))
        return bool(ok.value), float(worst)


class Arr:
    """f32.Arr(hl, kind, shape, ...): a vector (n,), a matrix (h, w) or a scalar () of the element type laid out by parity_helpers' HostArray ("host") or DevArray ("dev") —
    padded columns, a first element `offset` bytes off the allocation's start, sentinels all around — behind a buffer of the right
    dimensionality (those two classes are 2-D and up: a vector is their one-row matrix).  `hl` is the product module."""

    def __init__(self, dtype, hl, kind, shape, col_stride=None, offset=0, fill=None):
        self.kind, self.shape = kind, tuple(shape)
        shape2 = self.shape if len(shape) == 2 else (1, shape[0] if shape else 1)
        self.inner = (HostArray if kind == "host" else DevArray)(hl, shape2, dtype, col_stride, offset=offset,
                                                                 fill=None if fill is None else np.asarray(fill, dtype).reshape(shape2))
        if len(shape) == 2:
            self.buf = self.inner.buf
        elif kind == "host":
            self.buf = hl.Buffer(self.inner.host[0] if shape else self.inner.host[0, 0:1].reshape(()))
        else:
            self.buf = hl.Buffer.wrap_device(self.inner.p.value + offset, dtype.type, list(self.shape))

    def address(self):
        """the address the kernels see (after the call, for a host array)"""
        return self.buf.raw.device

    def result(self):
        """the array as the library left it, dense; every byte around it must be as it was"""
        if self.buf is not self.inner.buf:
            if self.kind == "host":
                self.buf.numpy()
                return self.inner._checked(self.inner.flat.copy(), self.inner.before).reshape(self.shape)
            self.buf.device_sync()
        return self.inner.result().reshape(self.shape)

    def free(self):
        if self.buf is not self.inner.buf:
            if self.kind == "host":
                self.buf.device_free()
            else:
                self.buf.device_detach()
        self.inner.free()


f32 = LinearAlgebra(np.float32, "s", "la_", 8)
f64 = LinearAlgebra(np.float64, "d", "ld_", 4)
