"""ctypes bindings to tests/cpp/linear_algebra_f64_check.c, the plain-C checker of the twelve f64 pipelines of apps/linear_algebra — TEST
INFRASTRUCTURE ONLY, the sibling of linear_algebra_checker.py.

Built with tests/cpp/check_canon.c into a shared object of its own, once per process, in a temporary directory, with
-ffp-contract=off; where the host has the FMA instruction the compiler may emit it for fma (-mfma).  Its canonical-form switch is its
own copy of check_canon.c's.  tests/test_linear_algebra_f64.py and scripts/fuzz_parity.py both come here.  Imports neither the product
nor torch.

Arrays: a vector is a 1-D float64 array; a matrix with Halide extents (w, h) — dimension 0 innermost, column-major in BLAS terms — is
a numpy array of shape (h, w) whose rows may be padded: A(i, k) is A[k, i]."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile
import threading

import numpy as np

import parity_helpers
from mat_mul_checker import host_has_fma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = ("check_canon.c", "linear_algebra_f64_check.c")
NAMES = ("halide_dcopy_impl", "halide_dscal_impl", "halide_daxpy_impl", "halide_ddot", "halide_dasum", "halide_dgemv_notrans",
         "halide_dgemv_trans", "halide_dger_impl", "halide_dgemm_notrans", "halide_dgemm_transA", "halide_dgemm_transB", "halide_dgemm_transAB")
GEMM_FLAGS = {"halide_dgemm_notrans": (0, 0), "halide_dgemm_transA": (1, 0), "halide_dgemm_transB": (0, 1), "halide_dgemm_transAB": (1, 1)}

_lock = threading.Lock()
_lib = []
f64 = np.float64
EPS = float(np.finfo(f64).eps)
# the padding value of parity_helpers' strided arrays for this element type (its table has the types the older pipelines use)
parity_helpers.SENTINEL.setdefault(np.dtype(f64), f64(-1234.5))


def lib():
    """The loaded shared object (the raw ctypes library), built on the first call."""
    with _lock:
        if not _lib:
            so = os.path.join(tempfile.mkdtemp(prefix="hlmi_linear_algebra_f64_checker"), "libldcheck.so")
            flags = ["-O2", "-ftree-vectorize", "-ffp-contract=off", "-Wall", "-Werror"] + (["-mfma"] if host_has_fma() else [])
            subprocess.run(["gcc"] + flags + ["-shared", "-fPIC", "-Wl,-Bsymbolic", "-o", so]
                           + [os.path.join(ROOT, "tests", "cpp", s) for s in SOURCES] + ["-lm"], check=True)
            L = C.CDLL(so)
            I, D, P, N = C.c_int, C.c_double, C.c_void_p, C.c_long
            L.ck_set_canon.argtypes = [I]
            L.ck_get_canon.restype = I
            L.ld_v.restype = I
            L.ld_axpy.restype, L.ld_axpy.argtypes = None, [I, D, P, P, P, N]
            L.ld_dot_v.restype, L.ld_dot_v.argtypes = D, [P, P, N, I]
            L.ld_asum_v.restype, L.ld_asum_v.argtypes = D, [P, N, I]
            L.ld_gemv.restype, L.ld_gemv.argtypes = None, [I, D, P, N, I, I, P, D, P, P, I]
            L.ld_ger.restype, L.ld_ger.argtypes = None, [D, P, I, P, I, P, N]
            L.ld_gemm.restype, L.ld_gemm.argtypes = None, [I, I, D, P, N, P, N, D, P, N, P, N, I, I, I, P]
            L.ld_compare.restype, L.ld_compare.argtypes = I, [D, D, D]
            L.ld_compare_all.restype, L.ld_compare_all.argtypes = D, [P, P, N, D, C.POINTER(I)]
            _lib.append(L)
    return _lib[0]


def set_canon(fma: int) -> None:
    """The checker's canonical form: 0 = one rounding per operator, 1 = mul+add pairs contracted."""
    lib().ck_set_canon(int(fma))


def get_canon() -> int:
    return int(lib().ck_get_canon())


class canon:
    """with linear_algebra_f64_checker.canon(0): ...   — evaluates the checker in the given form, then restores the one in force."""

    def __init__(self, fma: int):
        self.fma = int(fma)

    def __enter__(self):
        self.prev = get_canon()
        set_canon(self.fma)
        return self

    def __exit__(self, *exc):
        set_canon(self.prev)
        return False


V = 4   # asserted against the checker's, the kernels' and the Python binding's constant by the tests


def _vec(x):
    x = np.asarray(x)
    assert x.ndim == 1 and x.dtype == f64 and (x.size <= 1 or x.strides[0] == 8), (x.shape, x.dtype, x.strides)
    return x


def _mat(m):
    """(array, column stride in elements); rows of the numpy array are the matrix's columns and may be padded"""
    m = np.asarray(m)
    assert m.ndim == 2 and m.dtype == f64 and (m.shape[1] <= 1 or m.strides[1] == 8), (m.shape, m.dtype, m.strides)
    return m, (m.strides[0] // 8 if m.shape[0] > 1 else max(m.shape[1], 1))


def _p(a):
    return a.ctypes.data


def dcopy(x):
    x = _vec(x)
    out = np.empty(x.size, f64)
    lib().ld_axpy(0, 0.0, _p(x), None, _p(out), x.size)
    return out


def dscal(a, x):
    x = _vec(x)
    out = np.empty(x.size, f64)
    lib().ld_axpy(1, a, _p(x), None, _p(out), x.size)
    return out


def daxpy(a, x, y):
    x, y = _vec(x), _vec(y)
    assert x.size == y.size
    out = np.empty(x.size, f64)
    lib().ld_axpy(2, a, _p(x), _p(y), _p(out), x.size)
    return out


def ddot(x, y, v=V):
    """0-dimensional float64 array"""
    x, y = _vec(x), _vec(y)
    assert x.size == y.size
    return np.array(lib().ld_dot_v(_p(x), _p(y), x.size, v), f64)


def dasum(x, v=V):
    x = _vec(x)
    return np.array(lib().ld_asum_v(_p(x), x.size, v), f64)


def dgemv(trans, a, A, x, b, y, v=V):
    """A: shape (h, w).  notrans: x[h], y[w]; trans: x[w], y[h]"""
    (A, lda), x, y = _mat(A), _vec(x), _vec(y)
    h, w = A.shape
    assert (x.size, y.size) == ((w, h) if trans else (h, w)), (A.shape, x.size, y.size, trans)
    out = np.empty(y.size, f64)
    lib().ld_gemv(int(bool(trans)), a, _p(A), lda, w, h, _p(x), b, _p(y), _p(out), v)
    return out


def dger(a, x, y, R):
    """R: shape (n, m) for x[m], y[n]; returns the updated matrix, dense; R is not written"""
    x, y = _vec(x), _vec(y)
    out = np.ascontiguousarray(R, f64).copy()
    assert out.shape == (y.size, x.size)
    lib().ld_ger(a, _p(x), x.size, _p(y), y.size, _p(out), max(x.size, 1))
    return out


def dgemm(ta, tb, a, A, B, b, Cm):
    """A: shape (K, M) as stored, B: (N, K), C: (N, M); the transposed operands square (asserted here: the checker's C leaves it to us)"""
    (A, lda), (B, ldb), (Cm, ldc) = _mat(A), _mat(B), _mat(Cm)
    K, M = A.shape
    N = B.shape[0]
    assert B.shape == (N, K) and Cm.shape == (N, M) and (not ta or M == K) and (not tb or N == K), (A.shape, B.shape, Cm.shape, ta, tb)
    out, scratch = np.empty((N, M), f64), np.empty(max(M, 1), f64)
    lib().ld_gemm(int(bool(ta)), int(bool(tb)), a, _p(A), lda, _p(B), ldb, b, _p(Cm), ldc, _p(out), max(M, 1), M, N, K, _p(scratch))
    return out


class Arr:
    """A vector (n,), a matrix (h, w) or a scalar () of float64 laid out by parity_helpers' HostArray ("host") or DevArray ("dev") — padded
    columns, a first element `offset` bytes off the allocation's start, sentinels all around — behind a buffer of the right
    dimensionality (those two classes are 2-D and up: a vector is their one-row matrix).  `hl` is the product module."""

    def __init__(self, hl, kind, shape, col_stride=None, offset=0, fill=None):
        from parity_helpers import DevArray, HostArray
        self.kind, self.shape = kind, tuple(shape)
        shape2 = self.shape if len(shape) == 2 else (1, shape[0] if shape else 1)
        self.inner = (HostArray if kind == "host" else DevArray)(hl, shape2, f64, col_stride, offset=offset,
                                                                 fill=None if fill is None else np.asarray(fill, f64).reshape(shape2))
        if len(shape) == 2:
            self.buf = self.inner.buf
        elif kind == "host":
            self.buf = hl.Buffer(self.inner.host[0] if shape else self.inner.host[0, 0:1].reshape(()))
        else:
            self.buf = hl.Buffer.wrap_device(self.inner.p.value + offset, f64, list(self.shape))

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


def same_bits(got, want, what):
    """bit patterns, not values: -0 is not 0, and a NaN equals itself"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == f64, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = got.view(np.uint64) != want.view(np.uint64)
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} of {got.size} differ, first at {tuple(np.argwhere(bad)[0])}"


def same_bits_or_nan(got, want, what):
    """same_bits, except where the checker has a NaN: there the library must have a NaN, and nothing else is compared (sign and payload
    of a NaN that an operation produces belong to the processor)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == f64, what
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), f"{what}: {np.count_nonzero(~np.isnan(got[nan]))} of the checker's {np.count_nonzero(nan)} NaNs are numbers"
    bad = (got.view(np.uint64) != want.view(np.uint64)) & ~nan
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} of {got.size} differ, first at {tuple(np.argwhere(bad)[0])}"


def call_argv(hl, name, *args):
    """The call through `<name>_argv`: every scalar boxed by its metadata type (parity_helpers.call_argv for entry points that take
    doubles)"""
    md = hl.metadata(name)
    assert len(args) == md.num_arguments, (name, len(args))
    fn = getattr(hl.lib, name + "_argv")
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(C.c_void_p)]
    argv, keep = (C.c_void_p * len(args))(), []
    for j, v in enumerate(args):
        a = md.arguments[j]
        if a.kind != 0:
            argv[j] = None if v is None else C.cast(v.ptr, C.c_void_p)
        else:
            keep.append({(2, 32): C.c_float, (2, 64): C.c_double, (0, 32): C.c_int32}[(a.type.code, a.type.bits)](v))
            argv[j] = C.cast(C.pointer(keep[-1]), C.c_void_p)
    return fn(argv)


def compare(expected, actual, eps_multiple):
    """compareScalars over two float64 arrays of one shape with epsilon = eps_multiple * DBL_EPSILON: (every pair accepted, the worst
    |x - y| / (|x| + |y|) in units of DBL_EPSILON)"""
    e, a = np.ascontiguousarray(expected, f64).ravel(), np.ascontiguousarray(actual, f64).ravel()
    assert e.size == a.size
    ok = C.c_int(0)
    worst = lib().ld_compare_all(_p(e), _p(a), e.size, eps_multiple * EPS, C.byref(ok))
    return bool(ok.value), float(worst)
