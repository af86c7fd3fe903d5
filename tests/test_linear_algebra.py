"""linear_algebra: the twelve f32 pipelines of apps/linear_algebra (scopy, sscal, saxpy, sdot, sasum, sgemv x 2, sger, sgemm x 4), the
hblas_s* interface over them (include/hlmi_blas.h), the Python calls and the torch ops.

The contract is restated in include/hlmi_pipelines.h and DESIGN.md 5.8 and, line by line against the generators, in the header of the
checker tests/cpp/linear_algebra_check.c (bound by tests/linear_algebra_checker.py).  The CPU tests hold the checker to independent
evaluations (float64 where every partial result is exact, libm's fmaf and numpy's float32 operators one output at a time elsewhere,
both canonical forms), show that the inputs used on the GPU tell a wrong order or association from the right one, state the -0 traps
in numbers, hold the checker to the reference's own acceptance (compareScalars against float64 at N = 768) and the entry points to
their protocol.  The GPU tests hold the tuned path and the one-thread-per-output path to the checker bit for bit, NaN for NaN.

Arrays: a matrix with Halide extents (w, h), column-major in BLAS terms, is a numpy array of shape (h, w)."""
import ctypes as C
import ctypes.util
import functools
import os
import subprocess
import threading

import numpy as np
import pytest

from linear_algebra_checker import f32 as la
from parity_helpers import ROOT, call_argv, call_direct, kernel_const, load_fuzz_parity
from parity_helpers import gpu_present as _gpu_present, launches as _launches, same_bits as _same, same_bits_or_nan as _same_or_nan

Arr = la.Arr

f32, f64, u32 = np.float32, np.float64, np.uint32
HIP = "linear_algebra.hip"
V, MAX_VECTOR, MAX_EXTENT, SMALL_TILE, LARGE_TILE, LARGE_FROM_WGS, KC, GEMV_WG = (
    kernel_const(HIP, n) for n in ("V", "MAX_VECTOR", "MAX_EXTENT", "SMALL_TILE", "LARGE_TILE", "LARGE_FROM_WGS", "KC", "GEMV_WG"))
NAMES = la.NAMES
VEC3 = ("halide_scopy_impl", "halide_sscal_impl", "halide_saxpy_impl")
GEMMS = tuple(la.GEMM_FLAGS)
PREFIX = {"halide_scopy_impl": "scopy", "halide_sscal_impl": "sscal", "halide_saxpy_impl": "saxpy", "halide_sger_impl": "sger"}


@pytest.fixture(params=[0, 1], ids=["canon0", "canon1"])
def each_canon(request):
    with la.canon(request.param):
        yield request.param


@pytest.fixture
def canon_lib(hl):
    """the checker in the form the loaded library was built for"""
    with la.canon(hl.canon_fma()):
        yield la


def test_v_is_one_constant():
    assert V == 8 == la.V == la.lib().la_v() and MAX_VECTOR == 2 ** 27 and MAX_EXTENT == 8192


# ---------------------------------------------------------------------------------------------------- inputs
def _noise(shape, seed):
    """[-1, 1)"""
    return (np.random.default_rng(seed).random(shape, dtype=f32) * 2 - 1).astype(f32)


def _uniform(shape, rng):
    return rng.random(shape, dtype=f32)


def _order_sensitive(shape, seed):
    """a mix of +-2^24, +-1, +-2^-24 and noise: 2^24 + 1 + ... - 2^24 depends on the order of the additions"""
    rng = np.random.default_rng(seed)
    pool = np.array([2.0 ** 24, -2.0 ** 24, 1.0, -1.0, 2.0 ** -24, -2.0 ** -24], f32)
    m = rng.choice(pool, shape).astype(f32)
    pick = rng.random(shape) < 0.3
    m[pick] = _noise(shape, seed + 1)[pick]
    return m


def _signs(shape, seed):
    rng = np.random.default_rng(seed)
    m = np.where(rng.random(shape) < 0.5, f32(1), f32(-1)).astype(f32)
    pick = rng.random(shape) < 0.3
    m[pick] = _noise(shape, seed + 1)[pick]
    return m


def _subnormal(shape, seed, exp):
    return (_noise(shape, seed) * f32(2.0 ** exp)).astype(f32)


SPECIALS = np.array([0.0, -0.0, 1e-40, -3e-39, np.inf, -np.inf, np.nan, 3e38, -2e38, 2.0 ** 100, -2.0 ** 100], f32)


# ---------------------------------------------------------------------------------------------------- independent evaluations
def _libm_fmaf():
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype, libm.fmaf.argtypes = C.c_float, [C.c_float, C.c_float, C.c_float]
    return libm.fmaf


FMAF = _libm_fmaf()


def _mad(a, b, c, fma):
    with np.errstate(all="ignore"):
        return f32(FMAF(float(a), float(b), float(c))) if fma else f32(f32(a) * f32(b)) + f32(c)


def _mad2(a, b, c, d, fma):
    with np.errstate(all="ignore"):
        cd = f32(c) * f32(d)
        return f32(FMAF(float(a), float(b), float(cd))) if fma else f32(f32(a) * f32(b)) + cd


def _py_dot(x, y, fma, v=8, asum=False):
    lanes = [f32(0)] * v
    nvec = len(x) // v
    step = (lambda xv, yv, acc: acc + abs(f32(xv))) if asum else (lambda xv, yv, acc: _mad(xv, yv, acc, fma))
    for k in range(nvec):
        for i in range(v):
            lanes[i] = step(x[k * v + i], y[k * v + i], lanes[i])
    s = f32(0)
    for i in range(v):
        s = s + lanes[i]
    t = f32(0)
    for e in range(nvec * v, len(x)):
        t = step(x[e], y[e], t)
    return f32(s + t)


def _py_gemv(trans, a, A, x, b, y, fma, alt=False):
    """alt: notrans with a * (A * x) in place of (a * A) * x"""
    h, w = A.shape
    a, b = f32(a), f32(b)
    with np.errstate(all="ignore"):
        if not trans:
            out = np.empty(w, f32)
            for i in range(w):
                acc = b * y[i]
                for k in range(h):
                    acc = _mad(a, A[k, i] * x[k], acc, fma) if alt else _mad(a * A[k, i], x[k], acc, fma)
                out[i] = acc
            return out
        out = np.empty(h, f32)
        for i in range(h):
            lanes = [f32(0)] * 8
            for k in range(w // 8):
                for j in range(8):
                    lanes[j] = _mad(A[i, k * 8 + j], x[k * 8 + j], lanes[j], fma)
            s = f32(0)
            for j in range(8):
                s = s + lanes[j]
            for t in range(w // 8 * 8, w):
                s = _mad(A[i, t], x[t], s, fma)
            out[i] = _mad2(b, y[i], a, s, fma)
        return out


def _py_gemm(ta, tb, a, A, B, b, Cm, fma, alt=False):
    """alt: the epilogue as mad2(b, C, a, ab) in place of mad2(a, ab, b, C)"""
    K, M = A.shape
    N = B.shape[0]
    out = np.empty((N, M), f32)
    for j in range(N):
        for i in range(M):
            ab = f32(0)
            for k in range(K):
                ab = _mad(A[i, k] if ta else A[k, i], B[k, j] if tb else B[j, k], ab, fma)
            out[j, i] = _mad2(b, Cm[j, i], a, ab, fma) if alt else _mad2(a, ab, b, Cm[j, i], fma)
    return out


def _opA(ta, A):
    return A.T if ta else A


def _f64_gemm(ta, tb, a, A, B, b, Cm):
    """result[j, i] = a sum_k opA(i, k) opB(k, j) + b C[j, i] with opA(i, k) = A[k, i] (A[i, k] transposed), opB(k, j) = B[j, k] (B[k, j])"""
    A64, B64 = A.astype(f64), B.astype(f64)
    return f64(a) * ((B64.T if tb else B64) @ (A64.T if ta else A64)) + f64(b) * Cm.astype(f64)


def _f64_gemv(trans, a, A, x, b, y):
    A64 = A.astype(f64)
    return f64(a) * ((A64 @ x.astype(f64)) if trans else (A64.T @ x.astype(f64))) + f64(b) * y.astype(f64)


def _gemm_shapes(name, M, N, K):
    """(A, B, C) numpy shapes; the transposed operands square"""
    ta, tb = la.GEMM_FLAGS[name]
    assert (not ta or M == K) and (not tb or N == K)
    return (K, M), (N, K), (N, M)


# ---------------------------------------------------------------------------------------------------- CPU 1: the checker
def test_the_checker_equals_float64_where_every_partial_result_is_exact(each_canon):
    rng = np.random.default_rng(1)
    ints = lambda shape: rng.integers(-8, 9, shape).astype(f32)
    for n in (0, 1, 7, 8, 9, 33, 100):
        x, y = ints(n), ints(n)
        for a in (2.0, -0.5, 3.0):
            _same(la.scopy(x), x, "scopy")
            _same(la.sscal(a, x), (f64(a) * x).astype(f32), "sscal")
            _same(la.saxpy(a, x, y), (f64(a) * x + y).astype(f32), "saxpy")
        _same(la.sdot(x, y), np.array(x.astype(f64) @ y.astype(f64), f32), "sdot")
        _same(la.sasum(x), np.array(np.abs(x.astype(f64)).sum(), f32), "sasum")
    for w, h in ((1, 1), (7, 9), (9, 7), (33, 17), (16, 40)):
        A = ints((h, w))
        for trans in (False, True):
            x, y = ints(w if trans else h), ints(h if trans else w)
            _same(la.sgemv(trans, 2.0, A, x, -0.5, y), _f64_gemv(trans, 2.0, A, x, -0.5, y).astype(f32), f"sgemv {trans} {w}x{h}")
        x, y = ints(w), ints(h)
        _same(la.sger(0.5, x, y, A), (A.astype(f64) + 0.5 * np.outer(y, x)).astype(f32), "sger")
    for name in GEMMS:
        ta, tb = la.GEMM_FLAGS[name]
        for M, N, K in ((1, 1, 1), (7, 7, 7), (33, 33, 33)) + (((5, 9, 13),) if name == "halide_sgemm_notrans" else ()) + \
                (((9, 4, 9),) if name == "halide_sgemm_transA" else ()) + (((4, 9, 9),) if name == "halide_sgemm_transB" else ()):
            sa, sb, sc = _gemm_shapes(name, M, N, K)
            A, B, Cm = ints(sa), ints(sb), ints(sc)
            _same(la.sgemm(ta, tb, 2.0, A, B, -0.5, Cm), _f64_gemm(ta, tb, 2.0, A, B, -0.5, Cm).astype(f32), f"{name} {M} {N} {K}")


def test_the_checker_equals_the_chains_stepped_through_libm(each_canon):
    fma = each_canon
    for n, seed in ((1, 1), (7, 2), (8, 3), (19, 4), (70, 5)):
        for mk in (_noise, _order_sensitive):
            x, y = mk(n, seed), mk(n, seed + 50)
            _same(la.sdot(x, y), np.array(_py_dot(x, y, fma), f32), f"sdot n {n}")
            _same(la.sasum(x), np.array(_py_dot(x, x, fma, asum=True), f32), f"sasum n {n}")
            a = f32(0.37)
            _same(la.saxpy(a, x, y), np.array([_mad(a, x[i], y[i], fma) for i in range(n)], f32), "saxpy")
            _same(la.sscal(a, x), (a * x).astype(f32), "sscal")
    for w, h in ((1, 3), (9, 5), (20, 11)):
        A, a, b = _noise((h, w), w), f32(0.7), f32(-1.3)
        for trans in (False, True):
            x, y = _noise(w if trans else h, 7), _noise(h if trans else w, 8)
            _same(la.sgemv(trans, a, A, x, b, y), _py_gemv(trans, a, A, x, b, y, fma), f"sgemv {trans} {w}x{h}")
        x, y = _noise(w, 9), _noise(h, 10)
        with np.errstate(all="ignore"):
            want = np.array([[_mad(a * y[j], x[i], A[j, i], fma) for i in range(w)] for j in range(h)], f32)
        _same(la.sger(a, x, y, A), want, "sger")
    for name in GEMMS:
        ta, tb = la.GEMM_FLAGS[name]
        M, N, K = (6, 9, 11) if name == "halide_sgemm_notrans" else (9, 9, 9)
        sa, sb, sc = _gemm_shapes(name, M, N, K)
        A, B, Cm = _order_sensitive(sa, 3), _signs(sb, 4), _noise(sc, 5)
        _same(la.sgemm(ta, tb, 0.7, A, B, -1.3, Cm), _py_gemm(ta, tb, f32(0.7), A, B, f32(-1.3), Cm, fma), name)


def test_the_checker_reads_padded_columns(each_canon):
    A, B, Cm = _noise((9, 7), 1), _noise((5, 9), 2), _noise((5, 7), 3)
    wide = lambda m, pad: np.concatenate([m, np.full((m.shape[0], pad), 9e9, f32)], axis=1)[:, :m.shape[1]]
    _same(la.sgemm(0, 0, 0.5, wide(A, 3), wide(B, 1), 2.0, wide(Cm, 2)), la.sgemm(0, 0, 0.5, A, B, 2.0, Cm), "padded sgemm")
    x, y = _noise(9, 4), _noise(7, 5)
    _same(la.sgemv(False, 0.5, wide(A, 3), x, 2.0, y), la.sgemv(False, 0.5, A, x, 2.0, y), "padded sgemv")


# ---------------------------------------------------------------------------------------------------- CPU 2: the tests can tell
ORDER_N = 257


@functools.lru_cache(maxsize=None)
def _order_vectors(n=ORDER_N):
    """(x, y): x holds as many +2^24 as -2^24 (else their sum, near 10^8, swallows every difference of order), shuffled among +-1,
    +-2^-24 and noise; y is +-1.  The first seed whose vectors tell V = 8 from 4, 16 and 1 for sdot and sasum in both canonical forms:
    the test below states what was searched for, the GPU tests run these vectors."""
    for seed in range(300, 400):
        rng = np.random.default_rng(seed)
        big = np.repeat(np.array([2.0 ** 24, -2.0 ** 24], f32), n // 8)
        rest = _order_sensitive(n - big.size, seed + 1000)
        rest[np.abs(rest) > 2] = 1.0
        x = rng.permutation(np.concatenate([big, rest])).astype(f32)
        y = np.where(rng.random(n) < 0.5, f32(1), f32(-1)).astype(f32)
        y[np.abs(x) > 2] = 1.0
        # sasum adds magnitudes, nothing cancels: what tells the orders apart is the rounding of a growing sum of uneven terms
        xs = (x * f32(2.0 ** -12) + _noise(n, seed)).astype(f32)
        ok = True
        for form in (0, 1):
            with la.canon(form):
                for fn, args in ((la.sdot, (x, y)), (la.sasum, (xs,))):
                    ok &= all(fn(*args, v=v).view(u32) != fn(*args).view(u32) for v in (4, 16, 1))
        if ok:
            for m in (x, y, xs):
                m.setflags(write=False)
            return x, y, xs
    raise AssertionError("no seed separates the vector widths")


def test_the_order_sensitive_vectors_tell_v_8_from_4_16_and_a_sequential_sum(each_canon):
    x, y, xs = _order_vectors()
    for fn, args in ((la.sdot, (x, y)), (la.sasum, (xs,))):
        want = fn(*args)
        assert np.isfinite(want)
        for v in (4, 16, 1):   # v = 1: one chain over everything, the lane sum and the tail add nothing
            assert fn(*args, v=v).view(u32) != want.view(u32), (fn.__name__, v)
    A, xv, yv = _order_gemv_trans()
    want = la.sgemv(True, 0.7, A, xv, -1.3, yv)
    for v in (4, 16, 1):
        assert np.count_nonzero(la.sgemv(True, 0.7, A, xv, -1.3, yv, v=v).view(u32) != want.view(u32)) > 0, v


def _order_gemv_trans():
    """A's columns are shuffles of the order-sensitive vector, x is +-1 (+1 against the 2^24s): each output is such a dot product"""
    x, y, _ = _order_vectors()
    rng = np.random.default_rng(302)
    perm = rng.permutation(ORDER_N)
    A = np.stack([np.roll(x[perm], 3 * i) for i in range(9)]).astype(f32)
    xv = np.where(rng.random(ORDER_N) < 0.5, f32(1), f32(-1)).astype(f32)
    return A, xv, _noise(9, 303)


def test_the_gemv_input_tells_which_product_is_rounded_first(each_canon):
    A, x, y = _noise((40, 24), 304), _noise(40, 305), _noise(24, 306)
    a, b = f32(0.7), f32(-1.3)
    want = la.sgemv(False, a, A, x, b, y)
    _same(want, _py_gemv(False, a, A, x, b, y, each_canon), "the contract")
    assert np.count_nonzero(_py_gemv(False, a, A, x, b, y, each_canon, alt=True).view(u32) != want.view(u32)) > 0


def test_the_gemm_input_tells_which_product_the_epilogue_fuses():
    """only the contracted form has a choice: with one rounding per operator a * ab + b * C is one expression"""
    A, B, Cm = _noise((12, 12), 307), _noise((12, 12), 308), _noise((12, 12), 309)
    with la.canon(1):
        want = la.sgemm(0, 0, 0.7, A, B, -1.3, Cm)
    _same(want, _py_gemm(0, 0, f32(0.7), A, B, f32(-1.3), Cm, 1), "the contract")
    assert np.count_nonzero(_py_gemm(0, 0, f32(0.7), A, B, f32(-1.3), Cm, 1, alt=True).view(u32) != want.view(u32)) > 0
    with la.canon(0):
        _same(la.sgemm(0, 0, 0.7, A, B, -1.3, Cm), _py_gemm(0, 0, f32(0.7), A, B, f32(-1.3), Cm, 0, alt=True), "form 0 has one epilogue")


# ---------------------------------------------------------------------------------------------------- CPU 3: the -0 traps
NEG0 = 0x80000000


def _gemm_trap(M, N, K, i0, j0):
    """all zero but A(i0, K - 1) = -2^-100, B(K - 1, j0) = 2^-100 and C = -0: the chain at (i0, j0) is +0 until its last step, whose
    product underflows to -0; with a = b = 1 the result there is -0 + -0 = -0 and +0 + -0 = +0 everywhere else"""
    A, B, Cm = np.zeros((K, M), f32), np.zeros((N, K), f32), np.full((N, M), -0.0, f32)
    A[K - 1, i0], B[j0, K - 1] = -2.0 ** -100, 2.0 ** -100
    return A, B, Cm


def test_the_minus_zero_traps_in_numbers(each_canon):
    # a chain that ends in -0 survives the epilogue only against a -0 from b * C; a zero-padded further step makes it +0
    A, B, Cm = _gemm_trap(5, 4, 3, 2, 1)
    got = la.sgemm(0, 0, 1.0, A, B, 1.0, Cm).view(u32)
    if each_canon:
        assert got[1, 2] == NEG0 and np.count_nonzero(got) == 1
    else:   # the product rounds to -0 on its own and +0 + -0 = +0: with one rounding per operator no chain from +0 ends in -0
        assert not got.any()
    assert np.array([FMAF(0.0, 0.0, -0.0)], f32).view(u32)[0] == 0
    # +0 + -0: every product of this dot product is -0, every lane and the tail stay +0, and so does the result; x * y alone is -0
    for n in (1, 8, 9):
        x, y = np.full(n, -1.0, f32), np.zeros(n, f32)
        assert la.sdot(x, y).view(u32) == 0 and (x[0] * y[0]).view(u32) == NEG0
    # gemv_notrans starts from b * y, which may be -0, and keeps it through products that are -0
    Az, xz, yz = np.zeros((3, 2), f32), np.full(3, -1.0, f32), np.ones(2, f32)
    assert list(la.sgemv(False, 1.0, Az, xz, -0.0, yz).view(u32)) == [NEG0, NEG0]
    # gemv_trans: mad2(b, y, a, +0) with a < 0 and b * y = -0
    assert list(la.sgemv(True, -1.0, Az, np.ones(2, f32), -0.0, np.ones(3, f32)).view(u32)) == [NEG0] * 3


# ---------------------------------------------------------------------------------------------------- CPU 4: the reference's acceptance
@functools.lru_cache(maxsize=None)
def _acceptance_inputs(seed, n=768):
    rng = np.random.default_rng(seed)
    d = dict(a=float(rng.random(dtype=f32)), b=float(rng.random(dtype=f32)), x=_uniform(n, rng), y=_uniform(n, rng), A=_uniform((n, n), rng),
             B=_uniform((n, n), rng), C=_uniform((n, n), rng))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _acceptance_expected(name, d):
    """float64, rounded to float32 once: the reference's expected value comes from a float BLAS; float64 is the stricter stand-in"""
    a, b, x, y, A, B, Cm = (d[k] for k in "abxyABC")
    x64, y64 = x.astype(f64), y.astype(f64)
    if name == "halide_scopy_impl":
        return x
    if name == "halide_sscal_impl":
        return (a * x64).astype(f32)
    if name == "halide_saxpy_impl":
        return (a * x64 + y64).astype(f32)
    if name == "halide_sdot":
        return np.array(x64 @ y64, f32)
    if name == "halide_sasum":
        return np.array(np.abs(x64).sum(), f32)
    if name.startswith("halide_sgemv"):
        return _f64_gemv(name.endswith("_trans"), a, A, x, b, y).astype(f32)
    if name == "halide_sger_impl":
        return (A.astype(f64) + a * np.outer(y64, x64)).astype(f32)
    return _f64_gemm(*la.GEMM_FLAGS[name], a, A, B, b, Cm).astype(f32)


def _acceptance_checker(name, d):
    a, b, x, y, A, B, Cm = (d[k] for k in "abxyABC")
    if name in VEC3:
        return {"halide_scopy_impl": lambda: la.scopy(x), "halide_sscal_impl": lambda: la.sscal(a, x), "halide_saxpy_impl": lambda: la.saxpy(a, x, y)}[name]()
    if name == "halide_sdot":
        return la.sdot(x, y)
    if name == "halide_sasum":
        return la.sasum(x)
    if name.startswith("halide_sgemv"):
        return la.sgemv(name.endswith("_trans"), a, A, x, b, y)
    if name == "halide_sger_impl":
        return la.sger(a, x, y, A)
    return la.sgemm(*la.GEMM_FLAGS[name], a, A, B, b, Cm)


@pytest.mark.parametrize("seed", [11, 12, 13])
@pytest.mark.parametrize("name", NAMES)
def test_the_checker_meets_the_references_acceptance_at_768(each_canon, name, seed):
    d = _acceptance_inputs(seed)
    eps = 32 if name in ("halide_sdot", "halide_sasum") else 16
    ok, worst = la.compare(_acceptance_expected(name, d), _acceptance_checker(name, d), eps)
    print(f"{name} form {each_canon} seed {seed}: worst {worst:.2f} eps of {eps}")
    assert ok, (worst, eps)


def test_compare_scalars_as_the_reference_writes_it():
    e = la.EPS
    cmp = lambda x, y, k: bool(la.lib().la_compare(x, y, k * e))
    assert cmp(1.0, 1.0, 16) and cmp(0.0, -0.0, 16) and cmp(1.0, 1.0 + 8 * e, 16) and not cmp(1.0, 1.0 + 64 * e, 16)
    assert not cmp(0.0, 1e-30, 16) and cmp(0.0, 1e-44, 16) and cmp(1e-40, 1.00001e-40, 16)
    assert not cmp(float("nan"), 1.0, 16) and cmp(float("inf"), float("inf"), 16)


# ---------------------------------------------------------------------------------------------------- CPU 5: the library's surface
def _buffers(name):
    """names of the buffer arguments in signature order"""
    if name in VEC3 or name == "halide_sger_impl":
        return ("x", "y", "result")
    if name == "halide_sdot":
        return ("x", "y", "result")
    if name == "halide_sasum":
        return ("x", "result")
    if name.startswith("halide_sgemv"):
        return ("A", "x", "y", "output")
    return ("A_", "B_", "C_", "result")


def _shapes(name, n=20, w=12, h=9):
    """numpy shapes of the buffer arguments of a small valid call"""
    if name in VEC3:
        return {"x": (n,), "y": (n,), "result": (n,)}
    if name == "halide_sdot":
        return {"x": (n,), "y": (n,), "result": ()}
    if name == "halide_sasum":
        return {"x": (n,), "result": ()}
    if name == "halide_sgemv_notrans":
        return {"A": (h, w), "x": (h,), "y": (w,), "output": (w,)}
    if name == "halide_sgemv_trans":
        return {"A": (h, w), "x": (w,), "y": (h,), "output": (h,)}
    if name == "halide_sger_impl":
        return {"x": (w,), "y": (h,), "result": (h, w)}
    M, N, K = {"halide_sgemm_notrans": (10, 9, 7), "halide_sgemm_transA": (10, 9, 10), "halide_sgemm_transB": (10, 7, 7), "halide_sgemm_transAB": (8, 8, 8)}[name]
    sa, sb, sc = _gemm_shapes(name, M, N, K)
    return {"A_": sa, "B_": sb, "C_": sc, "result": sc}


def _scalars(name):
    return {"halide_sdot": 0, "halide_sasum": 0}.get(name, 2 if name.startswith(("halide_sgemv", "halide_sgemm")) else 1)


def _arguments(hl, name, bufs, a=0.5, b=-2.0):
    """the C signature's arguments in order from {buffer name: Buffer or None}"""
    order = [bufs[k] for k in _buffers(name)]
    if _scalars(name) == 0:
        return order
    if _scalars(name) == 1:
        return [a] + order
    return [a, order[0], order[1], b, order[2], order[3]]


def _valid(hl, name, **over):
    bufs = {k: hl.Buffer(np.zeros(s, f32)) for k, s in _shapes(name).items()}
    bufs.update(over)
    return bufs


def _call(hl, how, name, **over):
    return how(hl, name, *_arguments(hl, name, _valid(hl, name, **over)))


def _general(hl, name, *args):
    try:
        return hl.debug_linear_algebra_general(name, *args)
    except hl.HalideError as e:
        return e.code


def _ok():
    return 0 if _gpu_present() else -29   # with everything in order only the device can be missing


HOW = pytest.mark.parametrize("how", [call_direct, call_argv], ids=["direct_call", "argv"])
EACH = pytest.mark.parametrize("name", NAMES)


@EACH
def test_the_entry_points_are_exported_with_argv_and_metadata(hl, name):
    lib = C.CDLL(hl.LIB_PATH)
    for suffix in ("", "_argv", "_metadata"):
        assert hasattr(lib, name + suffix), name + suffix
    assert not hasattr(lib, name + "_auto_schedule") and hasattr(lib, "hlmi_linear_algebra_general")
    for sym in ("hblas_scopy", "hblas_sscal", "hblas_saxpy", "hblas_sdot", "hblas_snrm2", "hblas_sasum", "hblas_sgemv", "hblas_sger", "hblas_sgemm"):
        assert hasattr(lib, sym), sym
    assert hl._fn[name] is not None and name in hl.LINEAR_ALGEBRA
    for fn in ("scopy", "sscal", "saxpy", "sdot", "sasum", "sgemv", "sger", "sgemm", "debug_linear_algebra_general", "debug_sgemm_general", "debug_sgemv_general"):
        assert callable(getattr(hl, fn)), fn


@EACH
def test_metadata(hl, name):
    md = hl.metadata(name)
    bufs, ns = _buffers(name), _scalars(name)
    assert md.version == 1 and md.num_arguments == len(bufs) + ns and md.name.decode() == name and b"hip" in md.target
    args = [md.arguments[i] for i in range(md.num_arguments)]
    want_names = list(_arguments(hl, name, {k: k for k in bufs}, a="a_" if name in GEMMS else "a", b="b_" if name in GEMMS else "b"))
    assert [x.name.decode() for x in args] == want_names
    assert [x.kind for x in args] == [0 if n in ("a", "b", "a_", "b_") else 2 if n in ("result", "output") else 1 for n in want_names]
    assert all((x.type.code, x.type.bits) == (2, 32) for x in args)
    shapes = _shapes(name)
    assert [x.dimensions for x in args] == [0 if n in ("a", "b", "a_", "b_") else len(shapes[n]) for n in want_names]
    assert all(not x.buffer_estimates for x in args)


def test_the_headers_compile_as_c(tmp_path):
    src = tmp_path / "c.c"
    src.write_text("".join(f'#include "aot/{n}.h"\n' for n in NAMES) + '#include "hlmi_blas.h"\n'
                   + "".join(f"int (*const a_{n})(void **) = {n}_argv;\nconst struct halide_filter_metadata_t *(*const m_{n})(void) = {n}_metadata;\n" for n in NAMES)
                   + "int (*const g)(float, struct halide_buffer_t *, struct halide_buffer_t *, float, struct halide_buffer_t *, struct halide_buffer_t *) = halide_sgemm_transAB;\n"
                   + "int use(struct halide_buffer_t *b) { return halide_scopy(b, b) + halide_sscal(1.0f, b) + halide_saxpy(1.0f, b, b) + halide_sgemv(1, 1.0f, b, b, 1.0f, b)"
                     " + halide_sger(1.0f, b, b, b) + halide_sgemm(0, 1, 1.0f, b, b, 1.0f, b) + HblasColMajor + HblasTrans; }\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "c.o")], check=True)
    subprocess.run(["g++", "-Wall", "-Werror", "-x", "c++", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "cc.o")], check=True)
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "tests", "cpp", "blas_consumer.c"), "-o",
                    str(tmp_path / "consumer.o")], check=True)


@HOW
@EACH
def test_a_call_in_order_reaches_the_device(hl, how, name):
    assert _call(hl, how, name) == _ok()
    assert _general(hl, name, *_arguments(hl, name, _valid(hl, name))) == _ok()


@HOW
@EACH
def test_a_null_buffer_is_refused_except_the_unused_y(hl, how, name):
    for which in _buffers(name):
        code = _call(hl, how, name, **{which: None})
        if which == "y" and name in ("halide_scopy_impl", "halide_sscal_impl"):
            assert code == _ok(), (name, which)
        else:
            assert code == -12 and which in hl.last_error(), (name, which)
    if name in ("halide_scopy_impl", "halide_sscal_impl"):   # nor is a y of any other kind looked at
        assert _call(hl, how, name, y=hl.Buffer(np.zeros((3, 3), np.uint16))) == _ok()


@HOW
@EACH
def test_a_wrong_type_or_dimensionality_is_refused(hl, how, name):
    shapes = _shapes(name)
    for which in _buffers(name):
        if which == "y" and name in ("halide_scopy_impl", "halide_sscal_impl"):
            continue
        assert _call(hl, how, name, **{which: hl.Buffer(np.zeros(shapes[which], np.int32))}) == -3 and which in hl.last_error(), (name, which)
        assert _call(hl, how, name, **{which: hl.Buffer(np.zeros(shapes[which], np.float64))}) == -3
        assert _call(hl, how, name, **{which: hl.Buffer(np.zeros((1,) + shapes[which], f32))}) == -43 and which in hl.last_error(), (name, which)


@HOW
@EACH
def test_stride_min_and_extent_are_pinned(hl, how, name):
    shapes = _shapes(name)
    for which in _buffers(name):
        s = shapes[which]
        if not s or (which == "y" and name in ("halide_scopy_impl", "halide_sscal_impl")):
            continue
        wide = hl.Buffer(np.zeros(s[:-1] + (2 * s[-1],), f32)[..., ::2])
        assert wide.dim(0).stride == 2
        assert _call(hl, how, name, **{which: wide}) == -8 and f"{which}.stride.0" in hl.last_error(), (name, which)
        for d in range(len(s)):
            mins = [0] * len(s)
            mins[d] = 1
            assert _call(hl, how, name, **{which: hl.Buffer(np.zeros(s, f32), mins=mins)}) == -8 and f"{which}.min.{d}" in hl.last_error(), (name, which, d)
            if name == "halide_sasum":
                continue   # its one vector has no other extent to disagree with
            longer = list(s)
            longer[len(s) - 1 - d] += 1
            code = _call(hl, how, name, **{which: hl.Buffer(np.zeros(longer, f32))})
            assert code == -8 and ".extent." in hl.last_error(), (name, which, d, code, hl.last_error())
        if len(s) == 2:
            b = hl.Buffer(np.zeros(s, f32))
            b.dim(1).stride = s[1] - 1   # columns that overlap
            assert _call(hl, how, name, **{which: b}) == -8 and f"{which}.stride.1" in hl.last_error()
            padded = hl.Buffer(np.zeros((s[0], s[1] + 5), f32)[:, :s[1]])
            assert _call(hl, how, name, **{which: padded}) == _ok()


def test_the_transposed_variants_take_square_operands_only(hl):
    mk = lambda *s: hl.Buffer(np.zeros(s, f32))
    # A stored (K, M) in numpy terms: extents M x K
    call = lambda name, M, N, K: call_direct(hl, name, 1.0, mk(K, M), mk(N, K), 1.0, mk(N, M), mk(N, M))
    assert call("halide_sgemm_notrans", 5, 6, 7) == _ok()
    assert call("halide_sgemm_transA", 5, 6, 5) == _ok() and call("halide_sgemm_transA", 5, 6, 7) == -8 and "A_.extent.1" in hl.last_error()
    assert call("halide_sgemm_transB", 5, 7, 7) == _ok() and call("halide_sgemm_transB", 5, 6, 7) == -8 and "B_.extent.1" in hl.last_error()
    assert call("halide_sgemm_transAB", 6, 6, 6) == _ok() and call("halide_sgemm_transAB", 5, 7, 7) == -8 and call("halide_sgemm_transAB", 7, 6, 7) == -8


def test_the_limits(hl):
    v = hl.Buffer(np.zeros(4, f32))
    v.dim(0).extent = MAX_VECTOR + 1
    assert call_direct(hl, "halide_sasum", v, hl.Buffer(np.zeros((), f32))) == -8 and "must be 0 .." in hl.last_error()
    assert call_direct(hl, "halide_saxpy_impl", 1.0, v, v, v) == -8
    m = hl.Buffer(np.zeros((4, 4), f32))
    m.dim(1).extent = MAX_EXTENT + 1
    assert call_direct(hl, "halide_sgemm_notrans", 1.0, m, m, 1.0, m, m) == -8 and "must be 0 .." in hl.last_error()
    assert call_direct(hl, "halide_sger_impl", 1.0, hl.Buffer(np.zeros(4, f32)), v, m) == -8
    # zero extents are calls in order
    # (numpy gives an empty array strides of its own: cut the empty ones out of larger arrays, whose strides they keep)
    z = lambda *s: hl.Buffer(np.zeros(tuple(max(e, 1) for e in s), f32)[tuple(slice(0, e) for e in s)] if s else np.zeros((), f32))
    assert z(0).dim(0).stride == 1 and z(3, 0).dim(0).stride == 1
    assert call_direct(hl, "halide_sdot", z(0), z(0), z()) == _ok() and call_direct(hl, "halide_sscal_impl", 2.0, z(0), None, z(0)) == _ok()
    assert call_direct(hl, "halide_sgemm_notrans", 1.0, z(0, 5), z(4, 0), 1.0, z(4, 5), z(4, 5)) == _ok()
    assert call_direct(hl, "halide_sgemv_notrans", 1.0, z(3, 0), z(3), 1.0, z(0), z(0)) == _ok()


def test_exact_aliasing_is_the_normal_call_and_partial_overlap_is_refused(hl):
    z = lambda *s: hl.Buffer(np.zeros(s, f32))
    whole = np.zeros(64, f32)
    head, shifted, tail = hl.Buffer(whole[:20]), hl.Buffer(whole[10:30]), hl.Buffer(whole[20:40])
    twin = hl.Buffer(whole[:20])   # another descriptor of the same elements
    y = z(20)
    assert call_direct(hl, "halide_saxpy_impl", 1.0, z(20), y, y) == _ok()
    assert call_direct(hl, "halide_saxpy_impl", 1.0, z(20), head, twin) == _ok()
    assert call_direct(hl, "halide_saxpy_impl", 1.0, z(20), head, shifted) == -8 and "overlap" in hl.last_error()
    assert call_direct(hl, "halide_saxpy_impl", 1.0, head, z(20), twin) == -8 and "x" in hl.last_error()
    assert call_direct(hl, "halide_saxpy_impl", 1.0, z(20), head, tail) == _ok()   # neighbours in one allocation
    x = z(20)
    assert call_direct(hl, "halide_sscal_impl", 2.0, x, None, x) == _ok() and call_direct(hl, "halide_sscal_impl", 2.0, head, None, shifted) == -8
    assert call_direct(hl, "halide_scopy_impl", 0.0, head, None, shifted) == -8 and call_direct(hl, "halide_scopy_impl", 0.0, head, None, tail) == _ok()
    assert call_direct(hl, "halide_sdot", head, z(20), hl.Buffer(whole[5:6].reshape(()))) == -8
    for name in ("halide_sgemv_notrans", "halide_sgemv_trans"):
        yv = z(8)
        assert call_direct(hl, name, 1.0, z(8, 8), z(8), 1.0, yv, yv) == _ok()
        assert call_direct(hl, name, 1.0, z(8, 8), yv, 1.0, z(8), yv) == -8 and "x" in hl.last_error()
        w8 = np.zeros(32, f32)
        assert call_direct(hl, name, 1.0, z(8, 8), z(8), 1.0, hl.Buffer(w8[:8]), hl.Buffer(w8[4:12])) == -8
    big = np.zeros((20, 8), f32)
    for name in GEMMS:
        Cm = z(8, 8)
        assert call_direct(hl, name, 1.0, z(8, 8), z(8, 8), 1.0, Cm, Cm) == _ok()
        assert call_direct(hl, name, 1.0, Cm, z(8, 8), 1.0, z(8, 8), Cm) == -8 and "A_" in hl.last_error()
        assert call_direct(hl, name, 1.0, z(8, 8), Cm, 1.0, z(8, 8), Cm) == -8 and "B_" in hl.last_error()
        assert call_direct(hl, name, 1.0, z(8, 8), z(8, 8), 1.0, hl.Buffer(big[:8]), hl.Buffer(big[4:12])) == -8 and "C_" in hl.last_error()
        assert call_direct(hl, name, 1.0, z(8, 8), z(8, 8), 1.0, hl.Buffer(big[:8]), hl.Buffer(big[:8])) == _ok()
        a = z(8, 8)
        assert call_direct(hl, name, 1.0, a, a, 1.0, z(8, 8), z(8, 8)) == _ok()   # the inputs may be one matrix
    r = z(8, 8)
    assert call_direct(hl, "halide_sger_impl", 1.0, hl.Buffer(r.array[0]), z(8), r) == -8 and "overlap" in hl.last_error()


def test_the_order_of_the_checks(hl):
    z = lambda *s: hl.Buffer(np.zeros(s, f32))
    assert call_direct(hl, "halide_sgemm_notrans", 1.0, None, hl.Buffer(np.zeros((4, 4), np.uint16)), 1.0, z(4, 4), z(4, 4)) == -12   # null before type
    assert call_direct(hl, "halide_sgemm_notrans", 1.0, hl.Buffer(np.zeros((1, 4, 4), np.uint16)), z(4, 4), 1.0, z(4, 4), z(4, 4)) == -3   # type before dimensionality
    Cm = z(4, 4)
    assert call_direct(hl, "halide_sgemm_notrans", 1.0, Cm, z(5, 4), 1.0, z(5, 4), Cm) == -8 and ".extent." in hl.last_error()   # the pins before the alias check


@HOW
@EACH
def test_bounds_queries_are_answered(hl, how, name):
    shapes = _shapes(name)
    dims = lambda b: [(b.raw.dim[i].min, b.raw.dim[i].extent, b.raw.dim[i].stride) for i in range(b.raw.dimensions)]
    dense = lambda s: [(0, e, int(np.prod(s[::-1][:i], dtype=int))) for i, e in enumerate(s[::-1])]
    for which in _buffers(name):
        if not shapes[which] or (which == "y" and name in ("halide_scopy_impl", "halide_sscal_impl")):
            continue
        q = hl.Buffer.bounds_query(f32, len(shapes[which]), mins=(3,) * len(shapes[which]))
        assert _call(hl, how, name, **{which: q}) == 0
        # (sasum's x is the one buffer that has a size: queried, there is nothing to derive it from)
        assert dims(q) == ([(0, 0, 1)] if name == "halide_sasum" else dense(shapes[which])), (name, which, dims(q))
        q = hl.Buffer.bounds_query(np.uint16, len(shapes[which]))
        assert _call(hl, how, name, **{which: q}) == 0 and (q.raw.type.code, q.raw.type.bits) == (2, 32)
        assert _call(hl, how, name, **{which: hl.Buffer.bounds_query(f32, len(shapes[which]) + 1)}) == -43


def test_without_a_gpu_the_python_calls_refuse_to_run(hl):
    if _gpu_present():
        return   # the statement is about a machine without one
    z = lambda *s: hl.Buffer(np.zeros(s, f32))
    for fn in (lambda: hl.scopy(z(4), z(4)), lambda: hl.sscal(2.0, z(4)), lambda: hl.saxpy(2.0, z(4), z(4)), lambda: hl.sdot(z(4), z(4), z()),
               lambda: hl.sasum(z(4), z()), lambda: hl.sgemv(True, 1.0, z(4, 3), z(3), 1.0, z(4)), lambda: hl.sger(1.0, z(3), z(4), z(4, 3)),
               lambda: hl.sgemm(True, False, 1.0, z(4, 4), z(3, 4), 1.0, z(3, 4)), lambda: hl.debug_sgemm_general(False, False, 1.0, z(4, 4), z(3, 4), 1.0, z(3, 4))):
        with pytest.raises(hl.HalideError) as e:
            fn()
        assert e.value.code == -29


def _hblas(hl):
    L = C.CDLL(hl.LIB_PATH)
    I, F, P = C.c_int, C.c_float, C.c_void_p
    L.hblas_scopy.restype, L.hblas_scopy.argtypes = None, [I, P, I, P, I]
    L.hblas_sscal.restype, L.hblas_sscal.argtypes = None, [I, F, P, I]
    L.hblas_saxpy.restype, L.hblas_saxpy.argtypes = None, [I, F, P, I, P, I]
    L.hblas_sdot.restype, L.hblas_sdot.argtypes = F, [I, P, I, P, I]
    L.hblas_snrm2.restype, L.hblas_snrm2.argtypes = F, [I, P, I]
    L.hblas_sasum.restype, L.hblas_sasum.argtypes = F, [I, P, I]
    L.hblas_sgemv.restype, L.hblas_sgemv.argtypes = None, [I, I, I, I, F, P, I, P, I, F, P, I]
    L.hblas_sger.restype, L.hblas_sger.argtypes = None, [I, I, I, F, P, I, P, I, P, I]
    L.hblas_sgemm.restype, L.hblas_sgemm.argtypes = None, [I, I, I, I, I, I, F, P, I, P, I, F, P, I]
    return L


ROW, COL, NOT, TR = 101, 102, 111, 112


def test_hblas_refuses_increments_and_row_major(hl, capfd):
    L = _hblas(hl)
    x, y, m = np.ones(8, f32), np.full(8, 3.0, f32), np.full((4, 4), 5.0, f32)
    p = lambda a: a.ctypes.data
    capfd.readouterr()
    for fn, args in ((L.hblas_sdot, (4, p(x), 2, p(y), 1)), (L.hblas_sdot, (4, p(x), 1, p(y), 2)), (L.hblas_snrm2, (4, p(x), 2)), (L.hblas_sasum, (4, p(x), 0))):
        assert np.isnan(fn(*args))
        assert "increments of 1" in capfd.readouterr().err
    for fn, args in ((L.hblas_scopy, (4, p(x), 2, p(y), 1)), (L.hblas_sscal, (4, 2.0, p(y), 2)), (L.hblas_saxpy, (4, 2.0, p(x), 1, p(y), 2)),
                     (L.hblas_sgemv, (COL, NOT, 4, 4, 1.0, p(m), 4, p(x), 2, 1.0, p(y), 1)), (L.hblas_sger, (COL, 4, 4, 1.0, p(x), 1, p(y), 3, p(m), 4))):
        fn(*args)
        assert "increments of 1" in capfd.readouterr().err
    for fn, args in ((L.hblas_sgemv, (ROW, NOT, 4, 4, 1.0, p(m), 4, p(x), 1, 1.0, p(y), 1)), (L.hblas_sger, (ROW, 4, 4, 1.0, p(x), 1, p(y), 1, p(m), 4)),
                     (L.hblas_sgemm, (ROW, NOT, NOT, 4, 4, 4, 1.0, p(m), 4, p(m), 4, 1.0, p(m), 4))):
        fn(*args)
        assert "HblasColMajor" in capfd.readouterr().err
    rect = np.zeros((4, 8), f32)
    L.hblas_sgemm(COL, TR, NOT, 4, 4, 8, 1.0, p(rect), 8, p(rect), 8, 1.0, p(m), 4)
    assert "square" in capfd.readouterr().err
    assert (y == 3.0).all() and (m == 5.0).all() and (x == 1.0).all()   # nothing was computed


def test_torch_shape_functions_and_refusals():
    import torch
    import halide_amd.torch_ops  # noqa: F401
    ops = torch.ops.hlmi
    meta = lambda *s: torch.empty(s, dtype=torch.float32, device="meta")
    assert ops.saxpy(2.0, meta(9), meta(9)).shape == (9,) and ops.sdot(meta(9), meta(9)).shape == () and ops.sasum(meta(9)).shape == ()
    assert ops.sgemv(False, 1.0, meta(5, 7), meta(5), 1.0, meta(7)).shape == (7,) and ops.sgemv(True, 1.0, meta(5, 7), meta(7), 1.0, meta(5)).shape == (5,)
    assert ops.sger(1.0, meta(7), meta(5), meta(5, 7)).shape == (5, 7) and ops.sgemm(False, False, 1.0, meta(4, 7), meta(5, 4), 1.0, meta(5, 7)).shape == (5, 7)
    z = lambda *s: torch.zeros(s)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.saxpy(1.0, z(4), z(4))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.sgemm(False, False, 1.0, z(4, 7), z(5, 4), 1.0, z(5, 7))
    for bad in (lambda: ops.saxpy(1.0, z(4), z(5)), lambda: ops.sdot(z(4), z(4, 1)), lambda: ops.sasum(torch.zeros(4, dtype=torch.float64)),
                lambda: ops.sgemv(False, 1.0, z(5, 7), z(7), 1.0, z(5)), lambda: ops.sger(1.0, z(7), z(5), z(7, 5)),
                lambda: ops.sgemm(True, False, 1.0, z(4, 7), z(5, 4), 1.0, z(5, 7)), lambda: ops.sgemm(False, False, 1.0, z(4, 7), z(5, 3), 1.0, z(5, 7))):
        with pytest.raises(TypeError):
            bad()


def test_the_fuzzer_has_the_case():
    src = open(os.path.join(ROOT, "scripts", "fuzz_parity.py")).read()
    assert "def fuzz_linear_algebra(rng):" in src and 'CASES["linear_algebra"] = fuzz_linear_algebra' in src


# ---------------------------------------------------------------------------------------------------- GPU: one driver for all twelve
def _want(name, a, b, ins):
    """the checker's output for the call's inputs (dense numpy arrays by buffer name)"""
    if name == "halide_scopy_impl":
        return la.scopy(ins["x"])
    if name == "halide_sscal_impl":
        return la.sscal(a, ins["x"])
    if name == "halide_saxpy_impl":
        return la.saxpy(a, ins["x"], ins["y"])
    if name == "halide_sdot":
        return la.sdot(ins["x"], ins["y"])
    if name == "halide_sasum":
        return la.sasum(ins["x"])
    if name.startswith("halide_sgemv"):
        return la.sgemv(name.endswith("_trans"), a, ins["A"], ins["x"], b, ins["y"])
    if name == "halide_sger_impl":
        return la.sger(a, ins["x"], ins["y"], ins["result"])
    return la.sgemm(*la.GEMM_FLAGS[name], a, ins["A_"], ins["B_"], b, ins["C_"])


def _out_name(name):
    return _buffers(name)[-1]


def _aliased_input(name):
    """the input the wrappers of hlmi_blas.h pass as the output too"""
    return {"halide_sscal_impl": "x", "halide_saxpy_impl": "y", "halide_sgemv_notrans": "y", "halide_sgemv_trans": "y"}.get(name, "C_" if name in GEMMS else None)


def _expected_launches(hl, name, general, arrs, shapes):
    """the plan predicates of linear_algebra.hip restated; arrs: {buffer name: Arr} after the call"""
    out = shapes[_out_name(name)]
    al = lambda k: arrs[k].address() % 16 == 0
    if name in PREFIX:
        if 0 in out:
            return []
        if general:
            return [PREFIX[name] + "_general"]
        vec = al("x") and al("result") and (name != "halide_saxpy_impl" or al("y")) and (name != "halide_sger_impl" or arrs["result"].buf.dim(1).stride % 4 == 0)
        return [PREFIX[name] + ("_vec4" if vec else "_scalar")]
    if name in ("halide_sdot", "halide_sasum"):
        return [] if shapes["x"][0] == 0 else [name[7:] + ("_general" if general else "_wave")]
    if name.startswith("halide_sgemv"):
        return [] if out[0] == 0 else [name[7:] + ("_general" if general else "_wave")]
    (K, M), N = shapes["A_"], shapes["B_"][0]
    if M == 0 or N == 0:
        return []
    tile = LARGE_TILE if -(-M // LARGE_TILE) * -(-N // LARGE_TILE) >= LARGE_FROM_WGS else SMALL_TILE
    if general or not hl.canon_fma() or K == 0:
        return ["sgemm_general"]
    fast = M % tile == 0 and N % tile == 0 and K % KC == 0 and all(al(k) and arrs[k].buf.dim(1).stride % 4 == 0 for k in ("A_", "B_", "C_", "result"))
    return ["sgemm_mfma" if fast else "sgemm_mfma_edge"]


def _run(hl, name, ins, a=0.5, b=-2.0, general=False, kinds="dev", layouts=None, alias=False, check_launch=True, nan=False):
    """One call with every buffer in host or device memory ("host" / "dev", or a dict by buffer name), each with (column stride or None,
    byte offset) from `layouts`; alias: the output IS the wrapper's input.  Asserts the launch names, the bits of the output, the
    sentinels around every buffer and that the inputs are as they were.  Returns the launch names."""
    shapes = {k: tuple(np.shape(v)) for k, v in ins.items()}
    out = _out_name(name)
    if out not in shapes:
        shapes[out] = tuple(np.shape(_want(name, a, b, ins)))
    want = _want(name, a, b, ins)
    layouts = layouts or {}
    kind = (lambda k: kinds) if isinstance(kinds, str) else (lambda k: kinds.get(k, "dev"))
    al_in = _aliased_input(name) if alias else None
    arrs = {}
    try:
        for k in _buffers(name):
            if k == "y" and name in ("halide_scopy_impl", "halide_sscal_impl"):
                arrs[k] = None
                continue
            if k == out and al_in:
                arrs[k] = arrs[al_in]
                continue
            lay = layouts.get(k, (None, 0))
            arrs[k] = Arr(hl, kind(k), shapes[k], lay[0], lay[1], fill=ins.get(k))
        bufs = {k: (None if v is None else v.buf) for k, v in arrs.items()}
        args = _arguments(hl, name, bufs, a, b)
        fn = (lambda: hl.debug_linear_algebra_general(name, *args)) if general else (lambda: hl._check(call_direct(hl, name, *args)))
        ran = _launches(hl, fn)
        real = {k: v for k, v in arrs.items() if v is not None}
        if check_launch:
            assert ran == _expected_launches(hl, name, general, real, shapes), (name, ran, shapes)
        what = f"{name} {shapes} general {general} kinds {kinds} layouts {layouts} alias {alias} a {a} b {b}"
        (_same_or_nan if nan else _same)(np.asarray(arrs[out].result()).reshape(want.shape), want, what)
        for k, v in real.items():
            if k != out and v is not arrs[out]:
                assert np.array_equal(v.result().view(u32), np.asarray(ins[k], f32).reshape(shapes[k]).view(u32)), f"{what}: input {k} was written"
        return ran
    finally:
        for v in {id(v): v for v in arrs.values() if v is not None}.values():
            v.free()


def _inputs(name, dims, mk=_noise, seed=0):
    """inputs by buffer name.  dims: n for the vector routines, (w, h) for gemv and ger, (M, N, K) for gemm"""
    if name in VEC3 or name in ("halide_sdot", "halide_sasum"):
        ins = {"x": mk((dims,), seed + 1)}
        if name in ("halide_saxpy_impl", "halide_sdot"):
            ins["y"] = mk((dims,), seed + 2)
        return ins
    if name.startswith("halide_sgemv"):
        w, h = dims
        t = name.endswith("_trans")
        return {"A": mk((h, w), seed + 1), "x": mk((w if t else h,), seed + 2), "y": mk((h if t else w,), seed + 3)}
    if name == "halide_sger_impl":
        w, h = dims
        return {"x": mk((w,), seed + 1), "y": mk((h,), seed + 2), "result": mk((h, w), seed + 3)}
    sa, sb, sc = _gemm_shapes(name, *dims)
    return {"A_": mk(sa, seed + 1), "B_": mk(sb, seed + 2), "C_": mk(sc, seed + 3)}


PATHS = pytest.mark.parametrize("general", [False, True], ids=["default", "general"])
VECTOR_NS = (0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1000, 4099)
GEMV_DIMS = ((1, 1), (1, 65), (64, 1), (7, 8), (8, 7), (9, 64), (65, 9), (130, 257), (257, 130), (64, 64), (8, 130))


@pytest.mark.gpu
@PATHS
@pytest.mark.parametrize("name", VEC3 + ("halide_sdot", "halide_sasum"))
def test_vector_sizes(hl, canon_lib, name, general):
    for n in VECTOR_NS:
        _run(hl, name, _inputs(name, n, seed=n), general=general)


@pytest.mark.gpu
@PATHS
@pytest.mark.parametrize("name", ("halide_sgemv_notrans", "halide_sgemv_trans", "halide_sger_impl"))
def test_matrix_vector_sizes(hl, canon_lib, name, general):
    for dims in GEMV_DIMS:
        _run(hl, name, _inputs(name, dims, seed=sum(dims)), general=general)


def _gemm_dims(name):
    """M, N, K from {1, 2, 31, 32, 33, 64, 65, 96, 129, 130} over the shapes the variant's rule allows, always with an odd K and a K < KC"""
    if name == "halide_sgemm_notrans":
        return ((1, 1, 1), (2, 31, 33), (33, 2, 31), (64, 65, 1), (65, 64, 129), (96, 130, 2), (130, 96, 65), (129, 129, 32), (32, 33, 96), (31, 1, 130))
    if name == "halide_sgemm_transA":   # M == K
        return ((1, 1, 1), (33, 2, 33), (31, 64, 31), (65, 96, 65), (129, 31, 129), (2, 130, 2), (64, 33, 64), (130, 1, 130), (96, 65, 96))
    if name == "halide_sgemm_transB":   # N == K
        return ((1, 1, 1), (2, 33, 33), (64, 31, 31), (96, 65, 65), (31, 129, 129), (130, 2, 2), (33, 64, 64), (1, 130, 130), (65, 96, 96))
    return ((1, 1, 1), (2, 2, 2), (31, 31, 31), (32, 32, 32), (33, 33, 33), (64, 64, 64), (65, 65, 65), (96, 96, 96), (129, 129, 129), (130, 130, 130))


@pytest.mark.gpu
@PATHS
@pytest.mark.parametrize("name", GEMMS)
def test_gemm_sizes(hl, canon_lib, name, general):
    for dims in _gemm_dims(name):
        _run(hl, name, _inputs(name, dims, seed=sum(dims)), a=0.75, b=-1.5, general=general)


@pytest.mark.gpu
@pytest.mark.parametrize("name", GEMMS)
def test_gemm_aligned_cases_take_the_fast_kernel_of_each_tile(hl, canon_lib, name):
    fast = ["sgemm_mfma"] if hl.canon_fma() else ["sgemm_general"]
    edge = ["sgemm_mfma_edge"] if hl.canon_fma() else ["sgemm_general"]
    assert _run(hl, name, _inputs(name, (128, 128, 128), seed=5)) == fast
    assert _run(hl, name, _inputs(name, (128, 128, 128), seed=5), layouts={"A_": (132, 16), "C_": (140, 32), "result": (136, 0)}) == fast
    assert _run(hl, name, _inputs(name, (128, 128, 128), seed=5), layouts={"B_": (129, 0)}) == edge
    assert _run(hl, name, _inputs(name, (128, 128, 128), seed=5), layouts={"result": (132, 4)}) == edge
    if name == "halide_sgemm_notrans":   # the large tile at its threshold: 16 x 16 workgroups of 128 x 128
        assert (2048 // LARGE_TILE) ** 2 >= LARGE_FROM_WGS > (2048 // LARGE_TILE) * (1920 // LARGE_TILE)
        assert _run(hl, name, _inputs(name, (2048, 2048, 64), seed=6)) == fast
        assert _run(hl, name, _inputs(name, (2048, 2047, 33), seed=7)) == edge
        assert _run(hl, name, _inputs(name, (2048, 1920, 32), seed=8)) == fast   # below it: the small tile


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("halide_sgemm_transA", "halide_sgemm_transB", "halide_sgemm_transAB"))
def test_gemm_large_tile_of_the_transposed_variants(hl, canon_lib, name):
    """the smallest shapes their rules allow that reach 256 workgroups of 128 x 128"""
    dims = {"halide_sgemm_transA": (512, 8192, 512), "halide_sgemm_transB": (8192, 512, 512), "halide_sgemm_transAB": (2048, 2048, 2048)}[name]
    assert -(-dims[0] // LARGE_TILE) * -(-dims[1] // LARGE_TILE) >= LARGE_FROM_WGS
    ran = _run(hl, name, _inputs(name, dims, seed=9))
    assert ran == (["sgemm_mfma"] if hl.canon_fma() else ["sgemm_general"])


LARGE_EDGE_DIMS = {"halide_sgemm_transA": (385, 8065, 385), "halide_sgemm_transB": (8065, 385, 385), "halide_sgemm_transAB": (1921, 1921, 1921)}


def test_the_large_tile_edge_shapes_are_the_smallest_their_rules_allow():
    """256 workgroups of 128 x 128 with no extent above MAX_EXTENT are 4 x 64 tiles where only one of M, N is tied to K (one extent more
    than 3 and than 63 tiles: 385 and 8065, both off the tile, K = 385 odd) and 16 x 16 where both are (one more than 15 tiles: 1921)"""
    wgs = lambda M, N: -(-M // LARGE_TILE) * -(-N // LARGE_TILE)
    for name, (M, N, K) in LARGE_EDGE_DIMS.items():
        tA, tB = la.GEMM_FLAGS[name]
        assert (not tA or M == K) and (not tB or N == K) and max(M, N, K) <= MAX_EXTENT
        assert wgs(M, N) >= LARGE_FROM_WGS and K % 2 == 1 and (M % LARGE_TILE or N % LARGE_TILE)
        assert wgs(M - 1, N) < LARGE_FROM_WGS and wgs(M, N - 1) < LARGE_FROM_WGS   # one less either way and the plan takes the small tile


@pytest.mark.gpu
@pytest.mark.parametrize("name", tuple(LARGE_EDGE_DIMS))
def test_gemm_large_tile_edge_kernel_of_the_transposed_variants(hl, canon_lib, name):
    """sgemm_mfma<2, false, ., .> of each transposed variant: ragged tiles, a short last chunk and the odd last step on the VALU"""
    ran = _run(hl, name, _inputs(name, LARGE_EDGE_DIMS[name], seed=10))
    assert ran == (["sgemm_mfma_edge"] if hl.canon_fma() else ["sgemm_general"])


@pytest.mark.gpu
@PATHS
@EACH
def test_layouts_host_and_device_padded_and_off_the_grid(hl, canon_lib, name, general):
    dims = 261 if name in VEC3 + ("halide_sdot", "halide_sasum") else (67, 35) if name.startswith(("halide_sgemv", "halide_sger")) else \
        {"halide_sgemm_notrans": (67, 35, 41), "halide_sgemm_transA": (67, 35, 67), "halide_sgemm_transB": (67, 35, 35), "halide_sgemm_transAB": (67, 67, 67)}[name]
    ins = _inputs(name, dims, seed=3)
    shapes = _shapes_of(name, ins)
    for kinds in ("dev", "host"):
        _run(hl, name, ins, general=general, kinds=kinds)
    for el in (1, 2, 3):
        for which in shapes:
            pad = (shapes[which][1] + el) if len(shapes[which]) == 2 else None
            _run(hl, name, ins, general=general, layouts={which: (pad, 4 * el)})
    mixed = {k: ("host" if i % 2 else "dev") for i, k in enumerate(shapes)}
    _run(hl, name, ins, general=general, kinds=mixed, layouts={k: ((s[1] + 5) if len(s) == 2 else None, 0) for k, s in shapes.items()})


def _shapes_of(name, ins):
    shapes = {k: tuple(v.shape) for k, v in ins.items()}
    out = _out_name(name)
    if out not in shapes:
        shapes[out] = tuple(np.shape(_want(name, 0.5, -2.0, ins)))
    return {k: s for k, s in shapes.items() if s}


@pytest.mark.gpu
@PATHS
@pytest.mark.parametrize("name", [n for n in NAMES if _aliased_input(n)])
def test_in_place_calls_on_host_and_device_buffers(hl, canon_lib, name, general):
    dims = 261 if name in VEC3 else (67, 35) if name.startswith("halide_sgemv") else \
        {"halide_sgemm_notrans": (67, 35, 41), "halide_sgemm_transA": (64, 64, 64), "halide_sgemm_transB": (67, 35, 35), "halide_sgemm_transAB": (65, 65, 65)}[name]
    ins = _inputs(name, dims, seed=4)
    for kinds in ("dev", "host"):
        _run(hl, name, ins, general=general, kinds=kinds, alias=True)
        _run(hl, name, ins, general=general, kinds=kinds, alias=False)   # a separate output leaves y / C as it was (asserted by _run)


@pytest.mark.gpu
@PATHS
def test_two_descriptors_of_one_array_are_an_exact_alias_too(hl, canon_lib, general):
    y0, x = _noise(100, 1), _noise(100, 2)
    y = y0.copy()
    args = (0.5, hl.Buffer(x.copy()), hl.Buffer(y), hl.Buffer(y))
    (hl.debug_linear_algebra_general if general else lambda n, *a: hl._check(call_direct(hl, n, *a)))("halide_saxpy_impl", *args)
    _same(args[3].numpy(), la.saxpy(0.5, x, y0), "saxpy through two descriptors")


@pytest.mark.gpu
@PATHS
@EACH
def test_order_sensitive_subnormal_and_special_values(hl, canon_lib, name, general):
    dims = 1000 if name in VEC3 + ("halide_sdot", "halide_sasum") else (130, 65) if name.startswith(("halide_sgemv", "halide_sger")) else \
        {"halide_sgemm_notrans": (65, 33, 97), "halide_sgemm_transA": (65, 33, 65), "halide_sgemm_transB": (65, 33, 33), "halide_sgemm_transAB": (65, 65, 65)}[name]
    _run(hl, name, _inputs(name, dims, _order_sensitive, seed=20), a=0.7, b=-1.3, general=general)
    sub = _inputs(name, dims, lambda s, seed: _subnormal(s, seed, -70), seed=30)
    _run(hl, name, sub, a=2.0 ** -60, b=2.0 ** -62, general=general)
    # the special values: a handful per buffer, in at most a sixteenth of the rows and columns
    ins = _inputs(name, dims, seed=40)
    rng = np.random.default_rng(41)
    for k, m in ins.items():
        flat = m.reshape(-1)
        if m.ndim == 2:
            rows, cols = rng.choice(m.shape[0], max(1, m.shape[0] // 16), replace=False), rng.choice(m.shape[1], max(1, m.shape[1] // 16), replace=False)
            m[rows[0], rng.integers(0, m.shape[1], 3)] = rng.choice(SPECIALS, 3)
            m[rng.integers(0, m.shape[0], 3), cols[0]] = rng.choice(SPECIALS, 3)
        else:
            flat[rng.choice(flat.size, max(1, flat.size // 64), replace=False)] = rng.choice(SPECIALS, max(1, flat.size // 64))
    want = _want(name, 0.7, -1.3, ins)
    if want.ndim:
        assert np.count_nonzero(np.isnan(want)) <= want.size // 8 + 1, np.count_nonzero(np.isnan(want))
    _run(hl, name, ins, a=0.7, b=-1.3, general=general, nan=True)


@pytest.mark.gpu
@PATHS
def test_the_inputs_that_tell_the_vector_width(hl, canon_lib, general):
    x, y, xs = _order_vectors()
    _run(hl, "halide_sdot", {"x": x, "y": y}, general=general)
    _run(hl, "halide_sasum", {"x": xs}, general=general)
    A, xv, yv = _order_gemv_trans()
    _run(hl, "halide_sgemv_trans", {"A": A, "x": xv, "y": yv}, a=0.7, b=-1.3, general=general)
    A, xn, yn = _noise((40, 24), 304), _noise(40, 305), _noise(24, 306)   # (a * A) * x against a * (A * x)
    _run(hl, "halide_sgemv_notrans", {"A": A, "x": xn, "y": yn}, a=0.7, b=-1.3, general=general)
    ins = {"A_": _noise((12, 12), 307), "B_": _noise((12, 12), 308), "C_": _noise((12, 12), 309)}   # which product the epilogue fuses
    _run(hl, "halide_sgemm_notrans", ins, a=0.7, b=-1.3, general=general)


@pytest.mark.gpu
@PATHS
@pytest.mark.parametrize("name", ("halide_saxpy_impl", "halide_sscal_impl", "halide_sgemv_notrans", "halide_sgemv_trans", "halide_sger_impl") + GEMMS)
def test_the_scalars(hl, canon_lib, name, general):
    dims = 70 if name in VEC3 else (33, 17) if name.startswith(("halide_sgemv", "halide_sger")) else (33, 33, 33)
    ins = _inputs(name, dims, seed=50)
    noise = float(_noise(1, 51)[0])
    for a in (0.0, -0.0, 1.0, -1.0, noise, float("inf")):
        for b in ((0.0, -0.0, 1.0, -1.0, noise, float("inf")) if _scalars(name) == 2 else (0.0,)):
            _run(hl, name, ins, a=a, b=b, general=general, nan=True, check_launch=False)
    if _scalars(name) == 2:   # b = 0 does not hide a NaN in y / C
        k = _aliased_input(name)
        ins[k].reshape(-1)[3] = np.nan
        want = _want(name, 1.0, 0.0, ins)
        assert np.isnan(want.reshape(-1)[3]) and np.count_nonzero(np.isnan(want)) == 1
        _run(hl, name, ins, a=1.0, b=0.0, general=general, nan=True)


@pytest.mark.gpu
@PATHS
def test_minus_zero_on_the_device(hl, canon_lib, general):
    for M, N, K in ((33, 33, 33), (64, 64, 64), (65, 40, 31)):
        A, B, Cm = _gemm_trap(M, N, K, M // 3, N // 2)
        _run(hl, "halide_sgemm_notrans", {"A_": A, "B_": B, "C_": Cm}, a=1.0, b=1.0, general=general)
    Az = np.zeros((3, 70), f32)
    _run(hl, "halide_sgemv_notrans", {"A": Az, "x": np.full(3, -1.0, f32), "y": np.ones(70, f32)}, a=1.0, b=-0.0, general=general)
    _run(hl, "halide_sgemv_trans", {"A": Az, "x": np.ones(70, f32), "y": np.ones(3, f32)}, a=-1.0, b=-0.0, general=general)
    for n in (1, 8, 9, 300):
        _run(hl, "halide_sdot", {"x": np.full(n, -1.0, f32), "y": np.zeros(n, f32)}, general=general)


@pytest.mark.gpu
def test_argv_equals_the_direct_call(hl, canon_lib):
    for name in NAMES:
        ins = _inputs(name, 100 if name in VEC3 + ("halide_sdot", "halide_sasum") else (33, 17) if name.startswith(("halide_sgemv", "halide_sger")) else (33, 33, 33), seed=60)
        shapes = _shapes_of(name, ins)
        out = _out_name(name)
        bufs = {k: hl.Buffer(np.array(ins[k]) if k in ins else np.zeros(shapes.get(k, ()), f32)) for k in _buffers(name)
                if not (k == "y" and name in ("halide_scopy_impl", "halide_sscal_impl"))}
        bufs.setdefault("y", None)
        assert call_argv(hl, name, *_arguments(hl, name, bufs, 0.7, -1.3)) == 0
        _same(bufs[out].numpy(), _want(name, 0.7, -1.3, ins), f"{name} through argv")


# ---------------------------------------------------------------------------------------------------- GPU: hblas, the consumer, torch
@pytest.mark.gpu
def test_the_references_protocol_at_768_through_hblas(hl):
    L, d = _hblas(hl), _acceptance_inputs(11)
    a, b, x, y, A, B, Cm = (d[k] for k in "abxyABC")
    n, p = 768, lambda m: m.ctypes.data
    results = {}
    w = np.full(n, -1.0, f32)
    L.hblas_scopy(n, p(x), 1, p(w), 1)
    results["halide_scopy_impl"] = w
    w = x.copy()
    L.hblas_sscal(n, a, p(w), 1)
    results["halide_sscal_impl"] = w
    w = y.copy()
    L.hblas_saxpy(n, a, p(x), 1, p(w), 1)
    results["halide_saxpy_impl"] = w
    results["halide_sdot"] = np.array(L.hblas_sdot(n, p(x), 1, p(y), 1), f32)
    results["halide_sasum"] = np.array(L.hblas_sasum(n, p(x), 1), f32)
    for t, name in ((NOT, "halide_sgemv_notrans"), (TR, "halide_sgemv_trans")):
        w = y.copy()
        L.hblas_sgemv(COL, t, n, n, a, p(A), n, p(x), 1, b, p(w), 1)
        results[name] = w
    w = A.copy()
    L.hblas_sger(COL, n, n, a, p(x), 1, p(y), 1, p(w), n)
    results["halide_sger_impl"] = w
    for name, (ta, tb) in la.GEMM_FLAGS.items():
        w = Cm.copy()
        L.hblas_sgemm(COL, TR if ta else NOT, TR if tb else NOT, n, n, n, a, p(A), n, p(B), n, b, p(w), n)
        results[name] = w
    for name in NAMES:
        eps = 32 if name in ("halide_sdot", "halide_sasum") else 16
        ok, worst = la.compare(_acceptance_expected(name, d), results[name], eps)
        print(f"{name}: worst {worst:.2f} eps of {eps}")
        assert ok, (name, worst)
    nrm = L.hblas_snrm2(n, p(x), 1)
    assert la.compare(np.array(np.sqrt(x.astype(f64) @ x.astype(f64)), f32), np.array(nrm, f32), 32)[0]
    assert np.array_equal(x, d["x"]) and np.array_equal(A, d["A"])


@pytest.mark.gpu
def test_a_plain_c_consumer_of_hlmi_blas_h(hl, tmp_path):
    exe = tmp_path / "blas_consumer"
    libdir, libname = os.path.split(hl.LIB_PATH)
    subprocess.run(["gcc", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "blas_consumer.c"), "-o", str(exe),
                    "-L", libdir, "-l:" + libname, "-Wl,-rpath," + libdir, "-lm"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.count(" ok") == 13 and "FAIL" not in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_torch_ops_equal_the_checker(hl, canon_lib):
    import torch
    import halide_amd.torch_ops  # noqa: F401
    ops = torch.ops.hlmi
    cu = lambda m: torch.from_numpy(np.array(m)).cuda()
    back = lambda t: t.cpu().numpy()
    x, y, A = _noise(300, 1), _noise(300, 2), _noise((70, 300), 3)
    tx, ty, tA = cu(x), cu(y), cu(A)
    _same(back(ops.saxpy(0.7, tx, ty)), la.saxpy(0.7, x, y), "saxpy")
    _same(back(ops.sdot(tx, ty)), la.sdot(x, y), "sdot")
    _same(back(ops.sasum(tx)), la.sasum(x), "sasum")
    y70 = _noise(70, 4)
    _same(back(ops.sgemv(True, 0.7, tA, tx, -1.3, cu(y70))), la.sgemv(True, 0.7, A, x, -1.3, y70), "sgemv trans")
    _same(back(ops.sgemv(False, 0.7, tA, cu(y70), -1.3, ty)), la.sgemv(False, 0.7, A, y70, -1.3, y), "sgemv notrans")
    _same(back(ops.sger(0.7, tx, cu(y70), tA)), la.sger(0.7, x, y70, A), "sger")
    for name, (ta, tb) in la.GEMM_FLAGS.items():
        M, N, K = (70, 45, 96) if name == "halide_sgemm_notrans" else (64, 64, 64)
        sa, sb, sc = _gemm_shapes(name, M, N, K)
        Am, Bm, Cm = _noise(sa, 5), _noise(sb, 6), _noise(sc, 7)
        tC = cu(Cm)
        out = ops.sgemm(bool(ta), bool(tb), 0.7, cu(Am), cu(Bm), -1.3, tC)
        _same(back(out), la.sgemm(ta, tb, 0.7, Am, Bm, -1.3, Cm), name)
        assert np.array_equal(back(tC), Cm)
    assert np.array_equal(back(tx), x) and np.array_equal(back(ty), y) and np.array_equal(back(tA), A)
    # views with longer rows and a first element off the 16-byte grid
    big = torch.zeros((80, 313), dtype=torch.float32).cuda()
    big[3:73, 5:305] = tA
    _same(back(ops.sgemv(True, 0.7, big[3:73, 5:305], tx, -1.3, cu(y70))), la.sgemv(True, 0.7, A, x, -1.3, y70), "sgemv on a view")


@pytest.mark.gpu
def test_seeded_fuzz_slice_of_linear_algebra(on_stream):
    """scripts/fuzz_parity.py's linear_algebra case, a fixed number of cases from a fixed seed"""
    mod = load_fuzz_parity()
    rng = np.random.default_rng(20261019)
    for i in range(60):
        desc, ok = mod.CASES["linear_algebra"](rng)
        assert ok, f"case {i}: {desc}"


@pytest.mark.gpu
def test_two_host_threads_call_different_routines_at_once(hl, canon_lib):
    jobs = [("halide_sgemm_notrans", _inputs("halide_sgemm_notrans", (96, 65, 70), seed=1)), ("halide_sdot", _inputs("halide_sdot", 5000, seed=2))]
    wants = [_want(n, 0.7, -1.3, ins) for n, ins in jobs]
    errors = []

    def worker(i):
        try:
            name, ins = jobs[i]
            for rep in range(6):
                bufs = {k: hl.Buffer(np.array(ins[k]) if k in ins else np.zeros(wants[i].shape, f32)) for k in _buffers(name)}
                args = _arguments(hl, name, bufs, 0.7, -1.3)
                if rep % 2:
                    hl.debug_linear_algebra_general(name, *args)
                else:
                    hl._check(call_direct(hl, name, *args))
                got = bufs[_out_name(name)].numpy()
                if not np.array_equal(got.view(u32), wants[i].view(u32)):
                    errors.append(f"thread {i} rep {rep}: differs")
        except Exception as e:  # noqa: BLE001
            errors.append(f"thread {i}: {e!r}")

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
