"""ctypes bindings to tests/cpp/linear_algebra_check.c, the plain-C checker of the twelve f32 pipelines of apps/linear_algebra — TEST
INFRASTRUCTURE ONLY, the sibling of wavelet_checker.py.

Built with tests/cpp/check_canon.c into a shared object of its own, once per process, in a temporary directory, with
-ffp-contract=off; where the host has the FMA instruction the compiler may emit it for fmaf (-mfma, as mat_mul_checker.py).  Its
canonical-form switch is its own copy of check_canon.c's.  tests/test_linear_algebra.py and scripts/fuzz_parity.py both come here.
Imports neither the product nor torch.

Arrays: a vector is a 1-D float32 array; a matrix with Halide extents (w, h) — dimension 0 innermost, column-major in BLAS terms — is
a numpy array of shape (h, w) whose rows may be padded: A(i, k) is A[k, i]."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile
import threading

import numpy as np

from mat_mul_checker import host_has_fma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = ("check_canon.c", "linear_algebra_check.c")
NAMES = ("halide_scopy_impl", "halide_sscal_impl", "halide_saxpy_impl", "halide_sdot", "halide_sasum", "halide_sgemv_notrans",
         "halide_sgemv_trans", "halide_sger_impl", "halide_sgemm_notrans", "halide_sgemm_transA", "halide_sgemm_transB", "halide_sgemm_transAB")
GEMM_FLAGS = {"halide_sgemm_notrans": (0, 0), "halide_sgemm_transA": (1, 0), "halide_sgemm_transB": (0, 1), "halide_sgemm_transAB": (1, 1)}

_lock = threading.Lock()
_lib = []
f32 = np.float32
EPS = float(np.finfo(f32).eps)


def lib():
    """The loaded shared object (the raw ctypes library), built on the first call."""
    with _lock:
        if not _lib:
            so = os.path.join(tempfile.mkdtemp(prefix="hlmi_linear_algebra_checker"), "liblacheck.so")
            flags = ["-O2", "-ftree-vectorize", "-ffp-contract=off", "-Wall", "-Werror"] + (["-mfma"] if host_has_fma() else [])
            subprocess.run(["gcc"] + flags + ["-shared", "-fPIC", "-Wl,-Bsymbolic", "-I", os.path.join(ROOT, "oracle"), "-o", so]
                           + [os.path.join(ROOT, "tests", "cpp", s) for s in SOURCES] + ["-lm"], check=True)
            L = C.CDLL(so)
            I, F, P, N = C.c_int, C.c_float, C.c_void_p, C.c_long
            L.ck_set_canon.argtypes = [I]
            L.ck_get_canon.restype = I
            L.la_v.restype = I
            L.la_axpy.restype, L.la_axpy.argtypes = None, [I, F, P, P, P, N]
            L.la_dot_v.restype, L.la_dot_v.argtypes = F, [P, P, N, I]
            L.la_asum_v.restype, L.la_asum_v.argtypes = F, [P, N, I]
            L.la_gemv.restype, L.la_gemv.argtypes = None, [I, F, P, N, I, I, P, F, P, P, I]
            L.la_ger.restype, L.la_ger.argtypes = None, [F, P, I, P, I, P, N]
            L.la_gemm.restype, L.la_gemm.argtypes = None, [I, I, F, P, N, P, N, F, P, N, P, N, I, I, I, P]
            L.la_compare.restype, L.la_compare.argtypes = I, [F, F, F]
            L.la_compare_all.restype, L.la_compare_all.argtypes = F, [P, P, N, F, C.POINTER(I)]
            _lib.append(L)
    return _lib[0]


def set_canon(fma: int) -> None:
    """The checker's canonical form (oracle/oracle_common.h): 0 = one rounding per operator, 1 = mul+add pairs contracted."""
    lib().ck_set_canon(int(fma))


def get_canon() -> int:
    return int(lib().ck_get_canon())


class canon:
    """with linear_algebra_checker.canon(0): ...   — evaluates the checker in the given form, then restores the one in force."""

    def __init__(self, fma: int):
        self.fma = int(fma)

    def __enter__(self):
        self.prev = get_canon()
        set_canon(self.fma)
        return self

    def __exit__(self, *exc):
        set_canon(self.prev)
        return False


V = 8   # asserted against the checker's and the kernels' constant by the tests


def _vec(x):
    x = np.asarray(x)
    assert x.ndim == 1 and x.dtype == f32 and (x.size <= 1 or x.strides[0] == 4), (x.shape, x.dtype, x.strides)
    return x


def _mat(m):
    """(array, column stride in elements); rows of the numpy array are the matrix's columns and may be padded"""
    m = np.asarray(m)
    assert m.ndim == 2 and m.dtype == f32 and (m.shape[1] <= 1 or m.strides[1] == 4), (m.shape, m.dtype, m.strides)
    return m, (m.strides[0] // 4 if m.shape[0] > 1 else max(m.shape[1], 1))


def _p(a):
    return a.ctypes.data


def scopy(x):
    x = _vec(x)
    out = np.empty(x.size, f32)
    lib().la_axpy(0, 0.0, _p(x), None, _p(out), x.size)
    return out


def sscal(a, x):
    x = _vec(x)
    out = np.empty(x.size, f32)
    lib().la_axpy(1, a, _p(x), None, _p(out), x.size)
    return out


def saxpy(a, x, y):
    x, y = _vec(x), _vec(y)
    assert x.size == y.size
    out = np.empty(x.size, f32)
    lib().la_axpy(2, a, _p(x), _p(y), _p(out), x.size)
    return out


def sdot(x, y, v=V):
    """0-dimensional float32 array"""
    x, y = _vec(x), _vec(y)
    assert x.size == y.size
    return np.array(lib().la_dot_v(_p(x), _p(y), x.size, v), f32)


def sasum(x, v=V):
    x = _vec(x)
    return np.array(lib().la_asum_v(_p(x), x.size, v), f32)


def sgemv(trans, a, A, x, b, y, v=V):
    """A: shape (h, w).  notrans: x[h], y[w]; trans: x[w], y[h]"""
    (A, lda), x, y = _mat(A), _vec(x), _vec(y)
    h, w = A.shape
    assert (x.size, y.size) == ((w, h) if trans else (h, w)), (A.shape, x.size, y.size, trans)
    out = np.empty(y.size, f32)
    lib().la_gemv(int(bool(trans)), a, _p(A), lda, w, h, _p(x), b, _p(y), _p(out), v)
    return out


def sger(a, x, y, R):
    """R: shape (n, m) for x[m], y[n]; returns the updated matrix, dense; R is not written"""
    x, y = _vec(x), _vec(y)
    out = np.ascontiguousarray(R, f32).copy()
    assert out.shape == (y.size, x.size)
    lib().la_ger(a, _p(x), x.size, _p(y), y.size, _p(out), max(x.size, 1))
    return out


def sgemm(ta, tb, a, A, B, b, Cm):
    """A: shape (K, M) as stored, B: (N, K), C: (N, M); the transposed operands square (asserted here: the checker's C leaves it to us)"""
    (A, lda), (B, ldb), (Cm, ldc) = _mat(A), _mat(B), _mat(Cm)
    K, M = A.shape
    N = B.shape[0]
    assert B.shape == (N, K) and Cm.shape == (N, M) and (not ta or M == K) and (not tb or N == K), (A.shape, B.shape, Cm.shape, ta, tb)
    out, scratch = np.empty((N, M), f32), np.empty(max(M, 1), f32)
    lib().la_gemm(int(bool(ta)), int(bool(tb)), a, _p(A), lda, _p(B), ldb, b, _p(Cm), ldc, _p(out), max(M, 1), M, N, K, _p(scratch))
    return out


class Arr:
    """A vector (n,), a matrix (h, w) or a scalar () of float32 laid out by parity_helpers' HostArray ("host") or DevArray ("dev") — padded
    columns, a first element `offset` bytes off the allocation's start, sentinels all around — behind a buffer of the right
    dimensionality (those two classes are 2-D and up: a vector is their one-row matrix).  `hl` is the product module."""

    def __init__(self, hl, kind, shape, col_stride=None, offset=0, fill=None):
        from parity_helpers import DevArray, HostArray
        self.kind, self.shape = kind, tuple(shape)
        shape2 = self.shape if len(shape) == 2 else (1, shape[0] if shape else 1)
        self.inner = (HostArray if kind == "host" else DevArray)(hl, shape2, f32, col_stride, offset=offset,
                                                                 fill=None if fill is None else np.asarray(fill, f32).reshape(shape2))
        if len(shape) == 2:
            self.buf = self.inner.buf
        elif kind == "host":
            self.buf = hl.Buffer(self.inner.host[0] if shape else self.inner.host[0, 0:1].reshape(()))
        else:
            self.buf = hl.Buffer.wrap_device(self.inner.p.value + offset, f32, list(self.shape))

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


def compare(expected, actual, eps_multiple):
    """compareScalars over two float32 arrays of one shape with epsilon = eps_multiple * FLT_EPSILON: (every pair accepted, the worst
    |x - y| / (|x| + |y|) in units of FLT_EPSILON)"""
    e, a = np.ascontiguousarray(expected, f32).ravel(), np.ascontiguousarray(actual, f32).ravel()
    assert e.size == a.size
    ok = C.c_int(0)
    worst = lib().la_compare_all(_p(e), _p(a), e.size, eps_multiple * EPS, C.byref(ok))
    return bool(ok.value), float(worst)
