"""linear_algebra, the f64 half: the twelve `halide_d*` pipelines of apps/linear_algebra (dcopy, dscal, daxpy, ddot, dasum, dgemv x 2,
dger, dgemm x 4), the hblas_d* interface over them (include/hlmi_blas.h), the Python calls and the torch ops.

The contract is restated in include/hlmi_pipelines.h and DESIGN.md 5.10 and, derived from the generators at T = double, in the header of
the checker tests/cpp/linear_algebra_check.c (its ld_* half, bound by tests/linear_algebra_checker.py).  The CPU tests hold the checker to
independent evaluations (numpy float64 where every partial result is exact, libm's fma and Python's float operators one output at a time
elsewhere, both canonical forms), show that the inputs used on the GPU tell V = 4 from 2, 8 and a sequential sum, state the -0 traps in
numbers, hold the checker to the reference's own acceptance (compareScalars in double against numpy.longdouble at N = 768) and the
entry points to their protocol.  The GPU tests hold the tuned path and the one-thread-per-output path to the checker bit for bit, NaN
for NaN.

Arrays: a matrix with Halide extents (w, h), column-major in BLAS terms, is a numpy array of shape (h, w)."""
import ctypes as C
import ctypes.util
import functools
import os
import subprocess
import threading

import numpy as np
import pytest

from linear_algebra_checker import f64 as ld
from parity_helpers import ROOT, call_argv, call_direct, kernel_const, load_fuzz_parity
from parity_helpers import gpu_present as _gpu_present, launches as _launches, same_bits as _same, same_bits_or_nan as _same_or_nan

Arr = ld.Arr

f32, f64, u64, ext = np.float32, np.float64, np.uint64, np.longdouble
HIP = "linear_algebra_f64.hip"
V, MAX_VECTOR, MAX_EXTENT, SMALL_TILE, LARGE_TILE, TILE_N, LARGE_FROM_WGS, KC, GEMV_WG, GEMV_U, RED_BLOCK, ELEM_BLOCK = (
    kernel_const(HIP, n) for n in ("V", "MAX_VECTOR", "MAX_EXTENT", "SMALL_TILE", "LARGE_TILE", "TILE_N", "LARGE_FROM_WGS", "KC", "GEMV_WG", "GEMV_U",
                                   "RED_BLOCK", "ELEM_BLOCK"))
NAMES = ld.NAMES
VEC3 = ("halide_dcopy_impl", "halide_dscal_impl", "halide_daxpy_impl")
REDS = ("halide_ddot", "halide_dasum")
GEMMS = tuple(ld.GEMM_FLAGS)
PREFIX = {"halide_dcopy_impl": "dcopy", "halide_dscal_impl": "dscal", "halide_daxpy_impl": "daxpy", "halide_dger_impl": "dger"}


@pytest.fixture(params=[0, 1], ids=["canon0", "canon1"])
def each_canon(request):
    with ld.canon(request.param):
        yield request.param


@pytest.fixture
def canon_lib(hl):
    """the checker in the form the loaded library was built for"""
    with ld.canon(hl.canon_fma()):
        yield ld


def test_v_is_one_constant(hl):
    assert V == 4 == ld.V == ld.lib().ld_v() == hl.LINEAR_ALGEBRA_F64_V and MAX_VECTOR == 2 ** 27 and MAX_EXTENT == 8192
    assert tuple(hl.LINEAR_ALGEBRA_F64) == NAMES


# ---------------------------------------------------------------------------------------------------- inputs
def _noise(shape, seed):
    """[-1, 1)"""
    return np.random.default_rng(seed).random(shape) * 2 - 1


def _order_sensitive(shape, seed):
    """a mix of +-2^53, +-1, +-2^-53 and noise: 2^53 + 1 + ... - 2^53 depends on the order of the additions"""
    rng = np.random.default_rng(seed)
    pool = np.array([2.0 ** 53, -2.0 ** 53, 1.0, -1.0, 2.0 ** -53, -2.0 ** -53], f64)
    m = rng.choice(pool, shape).astype(f64)
    pick = rng.random(shape) < 0.3
    m[pick] = _noise(shape, seed + 1)[pick]
    return m


def _signs(shape, seed):
    rng = np.random.default_rng(seed)
    m = np.where(rng.random(shape) < 0.5, 1.0, -1.0).astype(f64)
    pick = rng.random(shape) < 0.3
    m[pick] = _noise(shape, seed + 1)[pick]
    return m


def _subnormal(shape, seed, exp):
    return _noise(shape, seed) * 2.0 ** exp


SPECIALS = np.array([0.0, -0.0, 1e-310, -3e-309, np.inf, -np.inf, np.nan, 1.5e308, -1e308, 2.0 ** 600, -2.0 ** 600], f64)


# ---------------------------------------------------------------------------------------------------- independent evaluations
def _libm_fma():
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fma.restype, libm.fma.argtypes = C.c_double, [C.c_double, C.c_double, C.c_double]
    return libm.fma


FMA = _libm_fma()


def _mad(a, b, c, fma):
    """Python floats are binary64 and every operator on them rounds once"""
    a, b, c = float(a), float(b), float(c)
    return FMA(a, b, c) if fma else a * b + c


def _mad2(a, b, c, d, fma):
    cd = float(c) * float(d)
    return FMA(float(a), float(b), cd) if fma else float(a) * float(b) + cd


def _py_dot(x, y, fma, v=4, asum=False):
    lanes = [0.0] * v
    nvec = len(x) // v
    step = (lambda xv, yv, acc: acc + abs(float(xv))) if asum else (lambda xv, yv, acc: _mad(xv, yv, acc, fma))
    for k in range(nvec):
        for i in range(v):
            lanes[i] = step(x[k * v + i], y[k * v + i], lanes[i])
    s = 0.0
    for i in range(v):
        s = s + lanes[i]
    t = 0.0
    for e in range(nvec * v, len(x)):
        t = step(x[e], y[e], t)
    return s + t


def _py_gemv(trans, a, A, x, b, y, fma, alt=False):
    """alt: notrans with a * (A * x) in place of (a * A) * x"""
    h, w = A.shape
    a, b = float(a), float(b)
    if not trans:
        out = np.empty(w, f64)
        for i in range(w):
            acc = b * float(y[i])
            for k in range(h):
                acc = _mad(a, float(A[k, i]) * float(x[k]), acc, fma) if alt else _mad(a * float(A[k, i]), x[k], acc, fma)
            out[i] = acc
        return out
    out = np.empty(h, f64)
    for i in range(h):
        lanes = [0.0] * 4
        for k in range(w // 4):
            for j in range(4):
                lanes[j] = _mad(A[i, k * 4 + j], x[k * 4 + j], lanes[j], fma)
        s = 0.0
        for j in range(4):
            s = s + lanes[j]
        for t in range(w // 4 * 4, w):
            s = _mad(A[i, t], x[t], s, fma)
        out[i] = _mad2(b, y[i], a, s, fma)
    return out


def _py_gemm(ta, tb, a, A, B, b, Cm, fma, alt=False):
    """alt: the epilogue as mad2(b, C, a, ab) in place of mad2(a, ab, b, C)"""
    K, M = A.shape
    N = B.shape[0]
    out = np.empty((N, M), f64)
    for j in range(N):
        for i in range(M):
            ab = 0.0
            for k in range(K):
                ab = _mad(A[i, k] if ta else A[k, i], B[k, j] if tb else B[j, k], ab, fma)
            out[j, i] = _mad2(b, Cm[j, i], a, ab, fma) if alt else _mad2(a, ab, b, Cm[j, i], fma)
    return out


def _wide_gemm(ta, tb, a, A, B, b, Cm, t=f64):
    """result[j, i] = a sum_k opA(i, k) opB(k, j) + b C[j, i] in type t"""
    Aw, Bw = A.astype(t), B.astype(t)
    return t(a) * ((Bw.T if tb else Bw) @ (Aw.T if ta else Aw)) + t(b) * Cm.astype(t)


def _wide_gemv(trans, a, A, x, b, y, t=f64):
    Aw = A.astype(t)
    return t(a) * ((Aw @ x.astype(t)) if trans else (Aw.T @ x.astype(t))) + t(b) * y.astype(t)


def _gemm_shapes(name, M, N, K):
    """(A, B, C) numpy shapes; the transposed operands square"""
    ta, tb = ld.GEMM_FLAGS[name]
    assert (not ta or M == K) and (not tb or N == K)
    return (K, M), (N, K), (N, M)


# ---------------------------------------------------------------------------------------------------- CPU 1: the checker
def test_the_checker_equals_float64_where_every_partial_result_is_exact(each_canon):
    rng = np.random.default_rng(1)
    ints = lambda shape: rng.integers(-8, 9, shape).astype(f64)
    for n in (0, 1, 3, 4, 5, 33, 100):
        x, y = ints(n), ints(n)
        for a in (2.0, -0.5, 3.0):
            _same(ld.dcopy(x), x, "dcopy")
            _same(ld.dscal(a, x), a * x, "dscal")
            _same(ld.daxpy(a, x, y), a * x + y, "daxpy")
        _same(ld.ddot(x, y), np.array(x @ y if n else 0.0, f64), "ddot")
        _same(ld.dasum(x), np.array(np.abs(x).sum(), f64), "dasum")
    for w, h in ((1, 1), (7, 9), (9, 7), (33, 17), (16, 40)):
        A = ints((h, w))
        for trans in (False, True):
            x, y = ints(w if trans else h), ints(h if trans else w)
            _same(ld.dgemv(trans, 2.0, A, x, -0.5, y), _wide_gemv(trans, 2.0, A, x, -0.5, y), f"dgemv {trans} {w}x{h}")
        x, y = ints(w), ints(h)
        _same(ld.dger(0.5, x, y, A), A + 0.5 * np.outer(y, x), "dger")
    for name in GEMMS:
        ta, tb = ld.GEMM_FLAGS[name]
        for M, N, K in ((1, 1, 1), (7, 7, 7), (33, 33, 33)) + (((5, 9, 13),) if name == "halide_dgemm_notrans" else ()) + \
                (((9, 4, 9),) if name == "halide_dgemm_transA" else ()) + (((4, 9, 9),) if name == "halide_dgemm_transB" else ()):
            sa, sb, sc = _gemm_shapes(name, M, N, K)
            A, B, Cm = ints(sa), ints(sb), ints(sc)
            _same(ld.dgemm(ta, tb, 2.0, A, B, -0.5, Cm), _wide_gemm(ta, tb, 2.0, A, B, -0.5, Cm), f"{name} {M} {N} {K}")


def test_the_checker_equals_the_chains_stepped_through_libm(each_canon):
    fma = each_canon
    for n, seed in ((1, 1), (3, 2), (4, 3), (19, 4), (70, 5)):
        for mk in (_noise, _order_sensitive):
            x, y = mk(n, seed), mk(n, seed + 50)
            _same(ld.ddot(x, y), np.array(_py_dot(x, y, fma), f64), f"ddot n {n}")
            _same(ld.dasum(x), np.array(_py_dot(x, x, fma, asum=True), f64), f"dasum n {n}")
            a = 0.37
            _same(ld.daxpy(a, x, y), np.array([_mad(a, x[i], y[i], fma) for i in range(n)], f64), "daxpy")
            _same(ld.dscal(a, x), a * x, "dscal")
    for w, h in ((1, 3), (9, 5), (20, 11)):
        A, a, b = _noise((h, w), w), 0.7, -1.3
        for trans in (False, True):
            x, y = _noise(w if trans else h, 7), _noise(h if trans else w, 8)
            _same(ld.dgemv(trans, a, A, x, b, y), _py_gemv(trans, a, A, x, b, y, fma), f"dgemv {trans} {w}x{h}")
        x, y = _noise(w, 9), _noise(h, 10)
        want = np.array([[_mad(a * float(y[j]), x[i], A[j, i], fma) for i in range(w)] for j in range(h)], f64)
        _same(ld.dger(a, x, y, A), want, "dger")
    for name in GEMMS:
        ta, tb = ld.GEMM_FLAGS[name]
        M, N, K = (6, 9, 11) if name == "halide_dgemm_notrans" else (9, 9, 9)
        sa, sb, sc = _gemm_shapes(name, M, N, K)
        A, B, Cm = _order_sensitive(sa, 3), _signs(sb, 4), _noise(sc, 5)
        _same(ld.dgemm(ta, tb, 0.7, A, B, -1.3, Cm), _py_gemm(ta, tb, 0.7, A, B, -1.3, Cm, fma), name)


def test_the_checker_reads_padded_columns(each_canon):
    A, B, Cm = _noise((9, 7), 1), _noise((5, 9), 2), _noise((5, 7), 3)
    wide = lambda m, pad: np.concatenate([m, np.full((m.shape[0], pad), 9e99, f64)], axis=1)[:, :m.shape[1]]
    assert wide(A, 3).strides[0] == 8 * 10
    _same(ld.dgemm(0, 0, 0.5, wide(A, 3), wide(B, 1), 2.0, wide(Cm, 2)), ld.dgemm(0, 0, 0.5, A, B, 2.0, Cm), "padded dgemm")
    x, y = _noise(9, 4), _noise(7, 5)
    _same(ld.dgemv(False, 0.5, wide(A, 3), x, 2.0, y), ld.dgemv(False, 0.5, A, x, 2.0, y), "padded dgemv")


# ---------------------------------------------------------------------------------------------------- CPU 2: the tests can tell
ORDER_N = 257
OTHER_WIDTHS = (2, 8, 1)   # v = 1: one chain over everything, the lane sum and the tail add nothing


@functools.lru_cache(maxsize=None)
def _order_vectors(n=ORDER_N):
    """(x, y, xs): x holds as many +2^53 as -2^53 (else their sum swallows every difference of order), shuffled among +-1, +-2^-53 and
    noise; y is +-1.  The first seed whose vectors tell V = 4 from 2, 8 and 1 for ddot and dasum in both canonical forms: the test
    below states what was searched for, the GPU tests run these vectors."""
    for seed in range(300, 500):
        rng = np.random.default_rng(seed)
        big = np.repeat(np.array([2.0 ** 53, -2.0 ** 53], f64), n // 8)
        rest = _order_sensitive(n - big.size, seed + 1000)
        rest[np.abs(rest) > 2] = 1.0
        x = rng.permutation(np.concatenate([big, rest]))
        y = np.where(rng.random(n) < 0.5, 1.0, -1.0).astype(f64)
        y[np.abs(x) > 2] = 1.0
        # dasum adds magnitudes, nothing cancels: what tells the orders apart is the rounding of a growing sum of uneven terms
        xs = x * 2.0 ** -41 + _noise(n, seed)
        ok = True
        for form in (0, 1):
            with ld.canon(form):
                for fn, args in ((ld.ddot, (x, y)), (ld.dasum, (xs,))):
                    ok &= all(fn(*args, v=v).view(u64) != fn(*args).view(u64) for v in OTHER_WIDTHS)
        if ok:
            for m in (x, y, xs):
                m.setflags(write=False)
            return x, y, xs
    raise AssertionError("no seed separates the vector widths")


def _order_gemv_trans():
    """A's columns are shuffles of the order-sensitive vector, x is +-1: each output is such a dot product"""
    x, y, _ = _order_vectors()
    rng = np.random.default_rng(302)
    perm = rng.permutation(ORDER_N)
    A = np.stack([np.roll(x[perm], 3 * i) for i in range(9)])
    xv = np.where(rng.random(ORDER_N) < 0.5, 1.0, -1.0).astype(f64)
    return A, xv, _noise(9, 303)


def test_the_order_sensitive_vectors_tell_v_4_from_2_8_and_a_sequential_sum(each_canon):
    x, y, xs = _order_vectors()
    assert np.abs(x).max() == 2.0 ** 53
    for fn, args in ((ld.ddot, (x, y)), (ld.dasum, (xs,))):
        want = fn(*args)
        assert np.isfinite(want)
        for v in OTHER_WIDTHS:
            assert fn(*args, v=v).view(u64) != want.view(u64), (fn.__name__, v)
    A, xv, yv = _order_gemv_trans()
    want = ld.dgemv(True, 0.7, A, xv, -1.3, yv)
    for v in OTHER_WIDTHS:
        assert np.count_nonzero(ld.dgemv(True, 0.7, A, xv, -1.3, yv, v=v).view(u64) != want.view(u64)) > 0, v


def test_the_gemv_input_tells_which_product_is_rounded_first(each_canon):
    A, x, y = _noise((40, 24), 304), _noise(40, 305), _noise(24, 306)
    want = ld.dgemv(False, 0.7, A, x, -1.3, y)
    _same(want, _py_gemv(False, 0.7, A, x, -1.3, y, each_canon), "the contract")
    assert np.count_nonzero(_py_gemv(False, 0.7, A, x, -1.3, y, each_canon, alt=True).view(u64) != want.view(u64)) > 0


def test_the_gemm_input_tells_which_product_the_epilogue_fuses():
    """only the contracted form has a choice: with one rounding per operator a * ab + b * C is one expression"""
    A, B, Cm = _noise((12, 12), 307), _noise((12, 12), 308), _noise((12, 12), 309)
    with ld.canon(1):
        want = ld.dgemm(0, 0, 0.7, A, B, -1.3, Cm)
    _same(want, _py_gemm(0, 0, 0.7, A, B, -1.3, Cm, 1), "the contract")
    assert np.count_nonzero(_py_gemm(0, 0, 0.7, A, B, -1.3, Cm, 1, alt=True).view(u64) != want.view(u64)) > 0
    with ld.canon(0):
        _same(ld.dgemm(0, 0, 0.7, A, B, -1.3, Cm), _py_gemm(0, 0, 0.7, A, B, -1.3, Cm, 0, alt=True), "form 0 has one epilogue")


# ---------------------------------------------------------------------------------------------------- CPU 3: the -0 traps
NEG0 = 0x8000000000000000


def _gemm_trap(M, N, K, i0, j0):
    """all zero but A(i0, K - 1) = -2^-600, B(K - 1, j0) = 2^-600 and C = -0: the chain at (i0, j0) is +0 until its last step, whose
    product underflows to -0; with a = b = 1 the result there is -0 + -0 = -0 and +0 + -0 = +0 everywhere else"""
    A, B, Cm = np.zeros((K, M), f64), np.zeros((N, K), f64), np.full((N, M), -0.0, f64)
    A[K - 1, i0], B[j0, K - 1] = -2.0 ** -600, 2.0 ** -600
    return A, B, Cm


def test_the_minus_zero_traps_in_numbers(each_canon):
    # a chain that ends in -0 survives the epilogue only against a -0 from b * C; a zero-padded further step makes it +0
    A, B, Cm = _gemm_trap(5, 4, 3, 2, 1)
    got = ld.dgemm(0, 0, 1.0, A, B, 1.0, Cm).view(u64)
    if each_canon:
        assert got[1, 2] == NEG0 and np.count_nonzero(got) == 1
    else:   # the product rounds to -0 on its own and +0 + -0 = +0: with one rounding per operator no chain from +0 ends in -0
        assert not got.any()
    assert np.array([FMA(0.0, 0.0, -0.0)], f64).view(u64)[0] == 0
    # +0 + -0: every product of this dot product is -0, every lane and the tail stay +0, and so does the result; x * y alone is -0
    for n in (1, 4, 5):
        x, y = np.full(n, -1.0, f64), np.zeros(n, f64)
        assert ld.ddot(x, y).view(u64) == 0 and (x[0] * y[0]).view(u64) == NEG0
    # gemv_notrans starts from b * y, which may be -0, and keeps it through products that are -0
    Az, xz, yz = np.zeros((3, 2), f64), np.full(3, -1.0, f64), np.ones(2, f64)
    assert list(ld.dgemv(False, 1.0, Az, xz, -0.0, yz).view(u64)) == [NEG0, NEG0]
    # gemv_trans: mad2(b, y, a, +0) with a < 0 and b * y = -0
    assert list(ld.dgemv(True, -1.0, Az, np.ones(2, f64), -0.0, np.ones(3, f64)).view(u64)) == [NEG0] * 3


# ---------------------------------------------------------------------------------------------------- CPU 4: the reference's acceptance
@functools.lru_cache(maxsize=None)
def _acceptance_inputs(seed, n=768):
    rng = np.random.default_rng(seed)
    d = dict(a=float(rng.random()), b=float(rng.random()), x=rng.random(n), y=rng.random(n), A=rng.random((n, n)), B=rng.random((n, n)), C=rng.random((n, n)))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _acceptance_expected(name, seed):
    """numpy.longdouble, rounded to float64 once: the reference's expected value comes from a double BLAS; the wider type is the stricter
    stand-in"""
    a, b, x, y, A, B, Cm = (_acceptance_inputs(seed)[k] for k in "abxyABC")
    xw, yw = x.astype(ext), y.astype(ext)
    if name == "halide_dcopy_impl":
        return x
    if name == "halide_dscal_impl":
        return (ext(a) * xw).astype(f64)
    if name == "halide_daxpy_impl":
        return (ext(a) * xw + yw).astype(f64)
    if name == "halide_ddot":
        return np.array((xw * yw).sum(), f64)
    if name == "halide_dasum":
        return np.array(np.abs(xw).sum(), f64)
    if name.startswith("halide_dgemv"):
        return _wide_gemv(name.endswith("_trans"), a, A, x, b, y, ext).astype(f64)
    if name == "halide_dger_impl":
        return (A.astype(ext) + ext(a) * np.outer(yw, xw)).astype(f64)
    return _wide_gemm(*ld.GEMM_FLAGS[name], a, A, B, b, Cm, ext).astype(f64)


def _acceptance_checker(name, d):
    a, b, x, y, A, B, Cm = (d[k] for k in "abxyABC")
    if name in VEC3:
        return {"halide_dcopy_impl": lambda: ld.dcopy(x), "halide_dscal_impl": lambda: ld.dscal(a, x), "halide_daxpy_impl": lambda: ld.daxpy(a, x, y)}[name]()
    if name == "halide_ddot":
        return ld.ddot(x, y)
    if name == "halide_dasum":
        return ld.dasum(x)
    if name.startswith("halide_dgemv"):
        return ld.dgemv(name.endswith("_trans"), a, A, x, b, y)
    if name == "halide_dger_impl":
        return ld.dger(a, x, y, A)
    return ld.dgemm(*ld.GEMM_FLAGS[name], a, A, B, b, Cm)


@pytest.mark.parametrize("seed", [11, 12, 13])
@pytest.mark.parametrize("name", NAMES)
def test_the_checker_meets_the_references_acceptance_at_768(each_canon, name, seed):
    assert np.finfo(ext).eps < 2 ** -60, "numpy.longdouble is no wider than double here: there is nothing to evaluate against"
    eps = 32 if name in REDS else 16
    ok, worst = ld.compare(_acceptance_expected(name, seed), _acceptance_checker(name, _acceptance_inputs(seed)), eps)
    print(f"{name} form {each_canon} seed {seed}: worst {worst:.2f} eps of {eps}")
    assert ok, (worst, eps)


def test_compare_scalars_as_the_reference_writes_it():
    e = ld.EPS
    cmp = lambda x, y, k: bool(ld.lib().ld_compare(x, y, k * e))
    assert cmp(1.0, 1.0, 16) and cmp(0.0, -0.0, 16) and cmp(1.0, 1.0 + 8 * e, 16) and not cmp(1.0, 1.0 + 64 * e, 16)
    # zero against a number: only a difference below 16 epsilon of DBL_MIN (a few subnormal steps) is accepted
    assert not cmp(0.0, 1e-300, 16) and cmp(0.0, 5e-324, 16) and not cmp(0.0, 1e-322, 16)
    # both below DBL_MIN: the absolute criterion (16 epsilon of DBL_MIN is sixteen subnormal steps), not the relative one
    assert 16 * e * 2.2250738585072014e-308 == 16 * 5e-324
    assert cmp(1e-310, 1e-310 + 5 * 5e-324, 16) and not cmp(1e-310, 1e-310 + 17 * 5e-324, 16) and not cmp(1e-310, 2e-310, 16)
    assert not cmp(float("nan"), 1.0, 16) and cmp(float("inf"), float("inf"), 16)


# ---------------------------------------------------------------------------------------------------- CPU 5: the library's surface
def _buffers(name):
    """names of the buffer arguments in signature order"""
    if name in VEC3 or name in ("halide_dger_impl", "halide_ddot"):
        return ("x", "y", "result")
    if name == "halide_dasum":
        return ("x", "result")
    if name.startswith("halide_dgemv"):
        return ("A", "x", "y", "output")
    return ("A_", "B_", "C_", "result")


def _shapes(name, n=20, w=12, h=9):
    """numpy shapes of the buffer arguments of a small valid call"""
    if name in VEC3:
        return {"x": (n,), "y": (n,), "result": (n,)}
    if name == "halide_ddot":
        return {"x": (n,), "y": (n,), "result": ()}
    if name == "halide_dasum":
        return {"x": (n,), "result": ()}
    if name == "halide_dgemv_notrans":
        return {"A": (h, w), "x": (h,), "y": (w,), "output": (w,)}
    if name == "halide_dgemv_trans":
        return {"A": (h, w), "x": (w,), "y": (h,), "output": (h,)}
    if name == "halide_dger_impl":
        return {"x": (w,), "y": (h,), "result": (h, w)}
    M, N, K = {"halide_dgemm_notrans": (10, 9, 7), "halide_dgemm_transA": (10, 9, 10), "halide_dgemm_transB": (10, 7, 7), "halide_dgemm_transAB": (8, 8, 8)}[name]
    sa, sb, sc = _gemm_shapes(name, M, N, K)
    return {"A_": sa, "B_": sb, "C_": sc, "result": sc}


def _scalars(name):
    return 0 if name in REDS else 2 if name.startswith(("halide_dgemv", "halide_dgemm")) else 1


def _arguments(name, bufs, a=0.5, b=-2.0):
    """the C signature's arguments in order from {buffer name: Buffer or None}"""
    order = [bufs[k] for k in _buffers(name)]
    if _scalars(name) == 0:
        return order
    if _scalars(name) == 1:
        return [a] + order
    return [a, order[0], order[1], b, order[2], order[3]]


def _valid(hl, name, **over):
    bufs = {k: hl.Buffer(np.zeros(s, f64)) for k, s in _shapes(name).items()}
    bufs.update(over)
    return bufs


def _call(hl, how, name, **over):
    return how(hl, name, *_arguments(name, _valid(hl, name, **over)))


def _general(hl, name, *args):
    try:
        return hl.debug_linear_algebra_general_f64(name, *args)
    except hl.HalideError as e:
        return e.code


def _ok():
    return 0 if _gpu_present() else -29   # with everything in order only the device can be missing


HOW = pytest.mark.parametrize("how", [call_direct, call_argv], ids=["direct_call", "argv"])
EACH = pytest.mark.parametrize("name", NAMES)
HBLAS = ("hblas_dcopy", "hblas_dscal", "hblas_daxpy", "hblas_ddot", "hblas_dnrm2", "hblas_dasum", "hblas_dgemv", "hblas_dger", "hblas_dgemm")


@EACH
def test_the_entry_points_are_exported_with_argv_and_metadata(hl, name):
    lib = C.CDLL(hl.LIB_PATH)
    for suffix in ("", "_argv", "_metadata"):
        assert hasattr(lib, name + suffix), name + suffix
    assert not hasattr(lib, name + "_auto_schedule") and hasattr(lib, "hlmi_linear_algebra_general_f64")
    for sym in HBLAS:
        assert hasattr(lib, sym), sym
    assert hl._fn[name] is not None and name in hl.LINEAR_ALGEBRA_F64
    for fn in ("dcopy", "dscal", "daxpy", "ddot", "dasum", "dgemv", "dger", "dgemm", "dgemm_name", "debug_linear_algebra_general_f64"):
        assert callable(getattr(hl, fn)), fn


@EACH
def test_metadata_states_float64_buffers_and_scalars(hl, name):
    md = hl.metadata(name)
    bufs, ns = _buffers(name), _scalars(name)
    assert md.version == 1 and md.num_arguments == len(bufs) + ns and md.name.decode() == name and b"hip" in md.target
    args = [md.arguments[i] for i in range(md.num_arguments)]
    want_names = list(_arguments(name, {k: k for k in bufs}, a="a_" if name in GEMMS else "a", b="b_" if name in GEMMS else "b"))
    assert [x.name.decode() for x in args] == want_names
    assert [x.kind for x in args] == [0 if n in ("a", "b", "a_", "b_") else 2 if n in ("result", "output") else 1 for n in want_names]
    assert all((x.type.code, x.type.bits) == (2, 64) for x in args)
    shapes = _shapes(name)
    assert [x.dimensions for x in args] == [0 if n in ("a", "b", "a_", "b_") else len(shapes[n]) for n in want_names]
    assert all(not x.buffer_estimates for x in args)
    assert all(not (x.scalar_def or x.scalar_min or x.scalar_max or x.scalar_estimate) for x in args)
    assert hl._fn[name].argtypes == [C.c_double if x.kind == 0 else hl._BP for x in args]


def test_an_f64_scalar_round_trips_through_the_argument_table(tmp_path):
    """A scalar_f64 line of hlmi_internal.h's argument table: def / min / max / estimate are stored and read back as doubles, a value
    no float holds included, the float and int lines beside it behave as before, and argv_call reads all eight bytes of a double
    parameter.  (No d* table gives a default or a range, so the library's own metadata cannot show this: a host program does.)"""
    src = tmp_path / "table.cpp"
    src.write_text(r'''
#include "hlmi_internal.h"
#include <math.h>
using namespace hlmi;
static double got_a; static float got_f; static int got_i;
static int entry(double a, float f, int32_t i) { got_a = a, got_f = f, got_i = i; return 7; }
int main() {
    Arg d = scalar_f64("a").def(0.1).range(-1e300, 1e300).estimate(1.0 / 3.0);
    Arg f = scalar_f32("f").def(0.1);
    Arg i = scalar_i32("i").def(3);
    if (d.type != T_F64 || d.sv[Arg::DEF].u.f64 != 0.1 || d.sv[Arg::MIN].u.f64 != -1e300 || d.sv[Arg::MAX].u.f64 != 1e300) return 1;
    if (d.sv[Arg::EST].u.f64 != 1.0 / 3.0 || d.get(Arg::EST) != 1.0 / 3.0 || d.get(Arg::MIN) != -1e300 || d.has != 15u) return 2;
    if (f.sv[Arg::DEF].u.f32 != 0.1f || f.get(Arg::DEF) != (double)0.1f || i.sv[Arg::DEF].u.i32 != 3 || i.get(Arg::DEF) != 3.0) return 3;
    if (type_abi(2, 64) != T_F64 || (T_F64 & 0xff) != 2 || ((T_F64 >> 8) & 0xff) != 64) return 4;
    double a = 1.0 + ldexp(1.0, -40); float fv = 2.5f; int32_t iv = -9;
    void *argv[3] = {&a, &fv, &iv};
    if (argv_call(entry, argv) != 7 || got_a != a || (float)got_a == got_a || got_f != 2.5f || got_i != -9) return 5;
    return 0;
}
''')
    exe = tmp_path / "table"
    # compiled as the library's sources are (halide_amd/csrc/Makefile); the program launches nothing and needs no device
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-x", "hip", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "halide_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_the_headers_compile_as_c(tmp_path):
    src = tmp_path / "c.c"
    src.write_text("".join(f'#include "aot/{n}.h"\n' for n in NAMES) + '#include "hlmi_blas.h"\n'
                   + "".join(f"int (*const a_{n})(void **) = {n}_argv;\nconst struct halide_filter_metadata_t *(*const m_{n})(void) = {n}_metadata;\n" for n in NAMES)
                   + "int (*const g)(double, struct halide_buffer_t *, struct halide_buffer_t *, double, struct halide_buffer_t *, struct halide_buffer_t *) = halide_dgemm_transAB;\n"
                   + "double (*const d)(const int, const double *, const int, const double *, const int) = hblas_ddot;\n"
                   + "int use(struct halide_buffer_t *b) { return halide_dcopy(b, b) + halide_dscal(1.0, b) + halide_daxpy(1.0, b, b) + halide_dgemv(1, 1.0, b, b, 1.0, b)"
                     " + halide_dger(1.0, b, b, b) + halide_dgemm(0, 1, 1.0, b, b, 1.0, b) + HblasColMajor + HblasTrans; }\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "c.o")], check=True)
    subprocess.run(["g++", "-Wall", "-Werror", "-x", "c++", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "cc.o")], check=True)
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "tests", "cpp", "blas_consumer_f64.c"), "-o",
                    str(tmp_path / "consumer.o")], check=True)


@HOW
@EACH
def test_a_call_in_order_reaches_the_device(hl, how, name):
    assert _call(hl, how, name) == _ok()
    assert _general(hl, name, *_arguments(name, _valid(hl, name))) == _ok()


@HOW
@EACH
def test_a_null_buffer_is_refused_except_the_unused_y(hl, how, name):
    for which in _buffers(name):
        code = _call(hl, how, name, **{which: None})
        if which == "y" and name in ("halide_dcopy_impl", "halide_dscal_impl"):
            assert code == _ok(), (name, which)
        else:
            assert code == -12 and which in hl.last_error(), (name, which)
    if name in ("halide_dcopy_impl", "halide_dscal_impl"):   # nor is a y of any other kind looked at
        assert _call(hl, how, name, y=hl.Buffer(np.zeros((3, 3), np.uint16))) == _ok()


@HOW
@EACH
def test_a_wrong_type_or_dimensionality_is_refused(hl, how, name):
    shapes = _shapes(name)
    for which in _buffers(name):
        if which == "y" and name in ("halide_dcopy_impl", "halide_dscal_impl"):
            continue
        # a float32 buffer is the case that matters: half the bytes behind the same shape
        assert _call(hl, how, name, **{which: hl.Buffer(np.zeros(shapes[which], f32))}) == -3 and which in hl.last_error() and "float64" in hl.last_error(), (name, which)
        assert _call(hl, how, name, **{which: hl.Buffer(np.zeros(shapes[which], np.int32))}) == -3
        assert _call(hl, how, name, **{which: hl.Buffer(np.zeros((1,) + shapes[which], f64))}) == -43 and which in hl.last_error(), (name, which)


@HOW
@EACH
def test_stride_min_and_extent_are_pinned(hl, how, name):
    shapes = _shapes(name)
    for which in _buffers(name):
        s = shapes[which]
        if not s or (which == "y" and name in ("halide_dcopy_impl", "halide_dscal_impl")):
            continue
        wide = hl.Buffer(np.zeros(s[:-1] + (2 * s[-1],), f64)[..., ::2])
        assert wide.dim(0).stride == 2
        assert _call(hl, how, name, **{which: wide}) == -8 and f"{which}.stride.0" in hl.last_error(), (name, which)
        for d in range(len(s)):
            mins = [0] * len(s)
            mins[d] = 1
            assert _call(hl, how, name, **{which: hl.Buffer(np.zeros(s, f64), mins=mins)}) == -8 and f"{which}.min.{d}" in hl.last_error(), (name, which, d)
            if name == "halide_dasum":
                continue   # its one vector has no other extent to disagree with
            longer = list(s)
            longer[len(s) - 1 - d] += 1
            code = _call(hl, how, name, **{which: hl.Buffer(np.zeros(longer, f64))})
            assert code == -8 and ".extent." in hl.last_error(), (name, which, d, code, hl.last_error())
        if len(s) == 2:
            b = hl.Buffer(np.zeros(s, f64))
            b.dim(1).stride = s[1] - 1   # columns that overlap
            assert _call(hl, how, name, **{which: b}) == -8 and f"{which}.stride.1" in hl.last_error()
            padded = hl.Buffer(np.zeros((s[0], s[1] + 5), f64)[:, :s[1]])
            assert _call(hl, how, name, **{which: padded}) == _ok()


def test_the_transposed_variants_take_square_operands_only(hl):
    mk = lambda *s: hl.Buffer(np.zeros(s, f64))
    # A stored (K, M) in numpy terms: extents M x K
    call = lambda name, M, N, K: call_direct(hl, name, 1.0, mk(K, M), mk(N, K), 1.0, mk(N, M), mk(N, M))
    assert call("halide_dgemm_notrans", 5, 6, 7) == _ok()
    assert call("halide_dgemm_transA", 5, 6, 5) == _ok() and call("halide_dgemm_transA", 5, 6, 7) == -8 and "A_.extent.1" in hl.last_error()
    assert call("halide_dgemm_transB", 5, 7, 7) == _ok() and call("halide_dgemm_transB", 5, 6, 7) == -8 and "B_.extent.1" in hl.last_error()
    assert call("halide_dgemm_transAB", 6, 6, 6) == _ok() and call("halide_dgemm_transAB", 5, 7, 7) == -8 and call("halide_dgemm_transAB", 7, 6, 7) == -8


def test_the_limits(hl):
    v = hl.Buffer(np.zeros(4, f64))
    v.dim(0).extent = MAX_VECTOR + 1
    assert call_direct(hl, "halide_dasum", v, hl.Buffer(np.zeros((), f64))) == -8 and "must be 0 .." in hl.last_error()
    assert call_direct(hl, "halide_daxpy_impl", 1.0, v, v, v) == -8
    m = hl.Buffer(np.zeros((4, 4), f64))
    m.dim(1).extent = MAX_EXTENT + 1
    assert call_direct(hl, "halide_dgemm_notrans", 1.0, m, m, 1.0, m, m) == -8 and "must be 0 .." in hl.last_error()
    assert call_direct(hl, "halide_dger_impl", 1.0, hl.Buffer(np.zeros(4, f64)), v, m) == -8
    # zero extents are calls in order
    # (numpy gives an empty array strides of its own: cut the empty ones out of larger arrays, whose strides they keep)
    z = lambda *s: hl.Buffer(np.zeros(tuple(max(e, 1) for e in s), f64)[tuple(slice(0, e) for e in s)] if s else np.zeros((), f64))
    assert z(0).dim(0).stride == 1 and z(3, 0).dim(0).stride == 1
    assert call_direct(hl, "halide_ddot", z(0), z(0), z()) == _ok() and call_direct(hl, "halide_dscal_impl", 2.0, z(0), None, z(0)) == _ok()
    assert call_direct(hl, "halide_dgemm_notrans", 1.0, z(0, 5), z(4, 0), 1.0, z(4, 5), z(4, 5)) == _ok()
    assert call_direct(hl, "halide_dgemv_notrans", 1.0, z(3, 0), z(3), 1.0, z(0), z(0)) == _ok()


def test_exact_aliasing_is_the_normal_call_and_partial_overlap_is_refused(hl):
    z = lambda *s: hl.Buffer(np.zeros(s, f64))
    whole = np.zeros(64, f64)
    head, shifted, tail = hl.Buffer(whole[:20]), hl.Buffer(whole[10:30]), hl.Buffer(whole[20:40])
    last = hl.Buffer(whole[19:39])   # shares its first element with head's last: the ranges are measured in 8-byte elements
    twin = hl.Buffer(whole[:20])   # another descriptor of the same elements
    y = z(20)
    assert call_direct(hl, "halide_daxpy_impl", 1.0, z(20), y, y) == _ok()
    assert call_direct(hl, "halide_daxpy_impl", 1.0, z(20), head, twin) == _ok()
    assert call_direct(hl, "halide_daxpy_impl", 1.0, z(20), head, shifted) == -8 and "overlap" in hl.last_error()
    assert call_direct(hl, "halide_daxpy_impl", 1.0, head, z(20), twin) == -8 and "x" in hl.last_error()
    assert call_direct(hl, "halide_daxpy_impl", 1.0, z(20), head, tail) == _ok()   # neighbours in one allocation
    assert call_direct(hl, "halide_dcopy_impl", 0.0, head, None, last) == -8
    x = z(20)
    assert call_direct(hl, "halide_dscal_impl", 2.0, x, None, x) == _ok() and call_direct(hl, "halide_dscal_impl", 2.0, head, None, shifted) == -8
    assert call_direct(hl, "halide_dcopy_impl", 0.0, head, None, shifted) == -8 and call_direct(hl, "halide_dcopy_impl", 0.0, head, None, tail) == _ok()
    assert call_direct(hl, "halide_ddot", head, z(20), hl.Buffer(whole[5:6].reshape(()))) == -8
    for name in ("halide_dgemv_notrans", "halide_dgemv_trans"):
        yv = z(8)
        assert call_direct(hl, name, 1.0, z(8, 8), z(8), 1.0, yv, yv) == _ok()
        assert call_direct(hl, name, 1.0, z(8, 8), yv, 1.0, z(8), yv) == -8 and "x" in hl.last_error()
        w8 = np.zeros(32, f64)
        assert call_direct(hl, name, 1.0, z(8, 8), z(8), 1.0, hl.Buffer(w8[:8]), hl.Buffer(w8[4:12])) == -8
    big = np.zeros((20, 8), f64)
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
    assert call_direct(hl, "halide_dger_impl", 1.0, hl.Buffer(r.array[0]), z(8), r) == -8 and "overlap" in hl.last_error()


def test_the_order_of_the_checks(hl):
    z = lambda *s: hl.Buffer(np.zeros(s, f64))
    assert call_direct(hl, "halide_dgemm_notrans", 1.0, None, hl.Buffer(np.zeros((4, 4), f32)), 1.0, z(4, 4), z(4, 4)) == -12   # null before type
    assert call_direct(hl, "halide_dgemm_notrans", 1.0, hl.Buffer(np.zeros((1, 4, 4), f32)), z(4, 4), 1.0, z(4, 4), z(4, 4)) == -3   # type before dimensionality
    Cm = z(4, 4)
    assert call_direct(hl, "halide_dgemm_notrans", 1.0, Cm, z(5, 4), 1.0, z(5, 4), Cm) == -8 and ".extent." in hl.last_error()   # the pins before the alias check


@HOW
@EACH
def test_bounds_queries_are_answered(hl, how, name):
    shapes = _shapes(name)
    dims = lambda b: [(b.raw.dim[i].min, b.raw.dim[i].extent, b.raw.dim[i].stride) for i in range(b.raw.dimensions)]
    dense = lambda s: [(0, e, int(np.prod(s[::-1][:i], dtype=int))) for i, e in enumerate(s[::-1])]
    for which in _buffers(name):
        if not shapes[which] or (which == "y" and name in ("halide_dcopy_impl", "halide_dscal_impl")):
            continue
        q = hl.Buffer.bounds_query(f64, len(shapes[which]), mins=(3,) * len(shapes[which]))
        assert _call(hl, how, name, **{which: q}) == 0
        # (dasum's x is the one buffer that has a size: queried, there is nothing to derive it from)
        assert dims(q) == ([(0, 0, 1)] if name == "halide_dasum" else dense(shapes[which])), (name, which, dims(q))
        q = hl.Buffer.bounds_query(f32, len(shapes[which]))
        assert _call(hl, how, name, **{which: q}) == 0 and (q.raw.type.code, q.raw.type.bits) == (2, 64)
        assert _call(hl, how, name, **{which: hl.Buffer.bounds_query(f64, len(shapes[which]) + 1)}) == -43


def test_without_a_gpu_the_python_calls_refuse_to_run(hl):
    if _gpu_present():
        return   # the statement is about a machine without one
    z = lambda *s: hl.Buffer(np.zeros(s, f64))
    for fn in (lambda: hl.dcopy(z(4), z(4)), lambda: hl.dscal(2.0, z(4)), lambda: hl.daxpy(2.0, z(4), z(4)), lambda: hl.ddot(z(4), z(4), z()),
               lambda: hl.dasum(z(4), z()), lambda: hl.dgemv(True, 1.0, z(4, 3), z(3), 1.0, z(4)), lambda: hl.dger(1.0, z(3), z(4), z(4, 3)),
               lambda: hl.dgemm(True, False, 1.0, z(4, 4), z(3, 4), 1.0, z(3, 4)),
               lambda: hl.debug_linear_algebra_general_f64(hl.dgemm_name(False, False), 1.0, z(4, 4), z(3, 4), 1.0, z(3, 4), z(3, 4))):
        with pytest.raises(hl.HalideError) as e:
            fn()
        assert e.value.code == -29
    with pytest.raises(ValueError):
        hl.debug_linear_algebra_general_f64("halide_sdot", z(4), z(4), z())


def _hblas(hl):
    L = C.CDLL(hl.LIB_PATH)
    I, D, P = C.c_int, C.c_double, C.c_void_p
    L.hblas_dcopy.restype, L.hblas_dcopy.argtypes = None, [I, P, I, P, I]
    L.hblas_dscal.restype, L.hblas_dscal.argtypes = None, [I, D, P, I]
    L.hblas_daxpy.restype, L.hblas_daxpy.argtypes = None, [I, D, P, I, P, I]
    L.hblas_ddot.restype, L.hblas_ddot.argtypes = D, [I, P, I, P, I]
    L.hblas_dnrm2.restype, L.hblas_dnrm2.argtypes = D, [I, P, I]
    L.hblas_dasum.restype, L.hblas_dasum.argtypes = D, [I, P, I]
    L.hblas_dgemv.restype, L.hblas_dgemv.argtypes = None, [I, I, I, I, D, P, I, P, I, D, P, I]
    L.hblas_dger.restype, L.hblas_dger.argtypes = None, [I, I, I, D, P, I, P, I, P, I]
    L.hblas_dgemm.restype, L.hblas_dgemm.argtypes = None, [I, I, I, I, I, I, D, P, I, P, I, D, P, I]
    return L


ROW, COL, NOT, TR = 101, 102, 111, 112


def test_hblas_refuses_increments_and_row_major(hl, capfd):
    L = _hblas(hl)
    x, y, m = np.ones(8, f64), np.full(8, 3.0, f64), np.full((4, 4), 5.0, f64)
    p = lambda a: a.ctypes.data
    capfd.readouterr()
    for fn, args in ((L.hblas_ddot, (4, p(x), 2, p(y), 1)), (L.hblas_ddot, (4, p(x), 1, p(y), 2)), (L.hblas_dnrm2, (4, p(x), 2)), (L.hblas_dasum, (4, p(x), 0))):
        assert np.isnan(fn(*args))
        assert "increments of 1" in capfd.readouterr().err
    for fn, args in ((L.hblas_dcopy, (4, p(x), 2, p(y), 1)), (L.hblas_dscal, (4, 2.0, p(y), 2)), (L.hblas_daxpy, (4, 2.0, p(x), 1, p(y), 2)),
                     (L.hblas_dgemv, (COL, NOT, 4, 4, 1.0, p(m), 4, p(x), 2, 1.0, p(y), 1)), (L.hblas_dger, (COL, 4, 4, 1.0, p(x), 1, p(y), 3, p(m), 4))):
        fn(*args)
        assert "increments of 1" in capfd.readouterr().err
    for fn, args in ((L.hblas_dgemv, (ROW, NOT, 4, 4, 1.0, p(m), 4, p(x), 1, 1.0, p(y), 1)), (L.hblas_dger, (ROW, 4, 4, 1.0, p(x), 1, p(y), 1, p(m), 4)),
                     (L.hblas_dgemm, (ROW, NOT, NOT, 4, 4, 4, 1.0, p(m), 4, p(m), 4, 1.0, p(m), 4))):
        fn(*args)
        assert "HblasColMajor" in capfd.readouterr().err
    rect = np.zeros((4, 8), f64)
    L.hblas_dgemm(COL, TR, NOT, 4, 4, 8, 1.0, p(rect), 8, p(rect), 8, 1.0, p(m), 4)
    assert "square" in capfd.readouterr().err
    assert (y == 3.0).all() and (m == 5.0).all() and (x == 1.0).all()   # nothing was computed


def test_torch_shape_functions_and_refusals():
    import torch
    import halide_amd.torch_ops  # noqa: F401
    ops = torch.ops.hlmi
    meta = lambda *s: torch.empty(s, dtype=torch.float64, device="meta")
    assert ops.daxpy(2.0, meta(9), meta(9)).shape == (9,) and ops.ddot(meta(9), meta(9)).shape == () and ops.dasum(meta(9)).shape == ()
    assert ops.ddot(meta(9), meta(9)).dtype == torch.float64
    assert ops.dgemv(False, 1.0, meta(5, 7), meta(5), 1.0, meta(7)).shape == (7,) and ops.dgemv(True, 1.0, meta(5, 7), meta(7), 1.0, meta(5)).shape == (5,)
    assert ops.dger(1.0, meta(7), meta(5), meta(5, 7)).shape == (5, 7) and ops.dgemm(False, False, 1.0, meta(4, 7), meta(5, 4), 1.0, meta(5, 7)).shape == (5, 7)
    z = lambda *s: torch.zeros(s, dtype=torch.float64)
    z32 = lambda *s: torch.zeros(s, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.daxpy(1.0, z(4), z(4))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.dgemm(False, False, 1.0, z(4, 7), z(5, 4), 1.0, z(5, 7))
    for bad in (lambda: ops.daxpy(1.0, z(4), z(5)), lambda: ops.ddot(z(4), z(4, 1)), lambda: ops.dasum(z32(4)), lambda: ops.daxpy(1.0, z32(4), z(4)),
                lambda: ops.ddot(z(4), z32(4)), lambda: ops.dgemv(False, 1.0, z32(5, 7), z(5), 1.0, z(7)), lambda: ops.dger(1.0, z(7), z(5), z32(5, 7)),
                lambda: ops.dgemm(False, False, 1.0, z(4, 7), z(5, 4), 1.0, z32(5, 7)),
                lambda: ops.dgemv(False, 1.0, z(5, 7), z(7), 1.0, z(5)), lambda: ops.dger(1.0, z(7), z(5), z(7, 5)),
                lambda: ops.dgemm(True, False, 1.0, z(4, 7), z(5, 4), 1.0, z(5, 7)), lambda: ops.dgemm(False, False, 1.0, z(4, 7), z(5, 3), 1.0, z(5, 7))):
        with pytest.raises(TypeError):
            bad()


def test_the_fuzzer_has_the_case():
    src = open(os.path.join(ROOT, "scripts", "fuzz_parity.py")).read()
    assert "def fuzz_linear_algebra_f64(rng):" in src and 'CASES["linear_algebra_f64"] = fuzz_linear_algebra_f64' in src
    assert "def fuzz_linear_algebra(rng):" in src and 'CASES["linear_algebra"] = fuzz_linear_algebra ' in src


# ---------------------------------------------------------------------------------------------------- GPU: one driver for all twelve
def _want(name, a, b, ins):
    """the checker's output for the call's inputs (dense numpy arrays by buffer name)"""
    if name == "halide_dcopy_impl":
        return ld.dcopy(ins["x"])
    if name == "halide_dscal_impl":
        return ld.dscal(a, ins["x"])
    if name == "halide_daxpy_impl":
        return ld.daxpy(a, ins["x"], ins["y"])
    if name == "halide_ddot":
        return ld.ddot(ins["x"], ins["y"])
    if name == "halide_dasum":
        return ld.dasum(ins["x"])
    if name.startswith("halide_dgemv"):
        return ld.dgemv(name.endswith("_trans"), a, ins["A"], ins["x"], b, ins["y"])
    if name == "halide_dger_impl":
        return ld.dger(a, ins["x"], ins["y"], ins["result"])
    return ld.dgemm(*ld.GEMM_FLAGS[name], a, ins["A_"], ins["B_"], b, ins["C_"])


def _out_name(name):
    return _buffers(name)[-1]


def _aliased_input(name):
    """the input the wrappers of hlmi_blas.h pass as the output too"""
    return {"halide_dscal_impl": "x", "halide_daxpy_impl": "y", "halide_dgemv_notrans": "y", "halide_dgemv_trans": "y"}.get(name, "C_" if name in GEMMS else None)


def _gemm_tile(M, N):
    return LARGE_TILE if -(-M // LARGE_TILE) * -(-N // TILE_N) >= LARGE_FROM_WGS else SMALL_TILE


def _expected_launches(name, general, arrs, shapes):
    """the plan predicates of linear_algebra_f64.hip restated; arrs: {buffer name: Arr} after the call"""
    out = shapes[_out_name(name)]
    al = lambda k: arrs[k].address() % 16 == 0
    if name in PREFIX:
        if 0 in out:
            return []
        if general:
            return [PREFIX[name] + "_general"]
        vec = al("x") and al("result") and (name != "halide_daxpy_impl" or al("y")) and (name != "halide_dger_impl" or arrs["result"].buf.dim(1).stride % 2 == 0)
        return [PREFIX[name] + ("_vec2" if vec else "_scalar")]
    if name in REDS:
        return [] if shapes["x"][0] == 0 else [name[7:] + ("_general" if general else "_wave")]
    if name.startswith("halide_dgemv"):
        return [] if out[0] == 0 else [name[7:] + ("_general" if general else "_wave")]
    (K, M), N = shapes["A_"], shapes["B_"][0]
    if M == 0 or N == 0:
        return []
    if general or K == 0:   # the tiled kernel steps dev::mad: it serves both canonical forms
        return ["dgemm_general"]
    fast = M % _gemm_tile(M, N) == 0 and N % TILE_N == 0 and K % KC == 0 and all(al(k) and arrs[k].buf.dim(1).stride % 2 == 0 for k in ("A_", "B_", "C_", "result"))
    return ["dgemm_tile" if fast else "dgemm_tile_edge"]


def _run(hl, name, ins, a=0.5, b=-2.0, general=False, kinds="dev", layouts=None, alias=False, check_launch=True, nan=False):
    """One call with every buffer in host or device memory ("host" / "dev", or a dict by buffer name), each with (column stride or None,
    byte offset) from `layouts`; alias: the output IS the wrapper's input.  Asserts the launch names, the bits of the output, the
    sentinels around every buffer and that the inputs are as they were.  Returns the launch names."""
    shapes = {k: tuple(np.shape(v)) for k, v in ins.items()}
    out = _out_name(name)
    want = _want(name, a, b, ins)
    shapes.setdefault(out, tuple(np.shape(want)))
    layouts = layouts or {}
    kind = (lambda k: kinds) if isinstance(kinds, str) else (lambda k: kinds.get(k, "dev"))
    al_in = _aliased_input(name) if alias else None
    arrs = {}
    try:
        for k in _buffers(name):
            if k == "y" and name in ("halide_dcopy_impl", "halide_dscal_impl"):
                arrs[k] = None
                continue
            if k == out and al_in:
                arrs[k] = arrs[al_in]
                continue
            lay = layouts.get(k, (None, 0))
            arrs[k] = Arr(hl, kind(k), shapes[k], lay[0], lay[1], fill=ins.get(k))
        bufs = {k: (None if v is None else v.buf) for k, v in arrs.items()}
        args = _arguments(name, bufs, a, b)
        fn = (lambda: hl.debug_linear_algebra_general_f64(name, *args)) if general else (lambda: hl._check(call_direct(hl, name, *args)))
        ran = _launches(hl, fn)
        real = {k: v for k, v in arrs.items() if v is not None}
        if check_launch:
            assert ran == _expected_launches(name, general, real, shapes), (name, ran, shapes)
        what = f"{name} {shapes} general {general} kinds {kinds} layouts {layouts} alias {alias} a {a} b {b}"
        (_same_or_nan if nan else _same)(np.asarray(arrs[out].result()).reshape(want.shape), want, what)
        for k, v in real.items():
            if k != out and v is not arrs[out]:
                assert np.array_equal(v.result().view(u64), np.asarray(ins[k], f64).reshape(shapes[k]).view(u64)), f"{what}: input {k} was written"
        return ran
    finally:
        for v in {id(v): v for v in arrs.values() if v is not None}.values():
            v.free()


def _inputs(name, dims, mk=_noise, seed=0):
    """inputs by buffer name.  dims: n for the vector routines, (w, h) for gemv and ger, (M, N, K) for gemm"""
    if name in VEC3 or name in REDS:
        ins = {"x": mk((dims,), seed + 1)}
        if name in ("halide_daxpy_impl", "halide_ddot"):
            ins["y"] = mk((dims,), seed + 2)
        return ins
    if name.startswith("halide_dgemv"):
        w, h = dims
        t = name.endswith("_trans")
        return {"A": mk((h, w), seed + 1), "x": mk((w if t else h,), seed + 2), "y": mk((h if t else w,), seed + 3)}
    if name == "halide_dger_impl":
        w, h = dims
        return {"x": mk((w,), seed + 1), "y": mk((h,), seed + 2), "result": mk((h, w), seed + 3)}
    sa, sb, sc = _gemm_shapes(name, *dims)
    return {"A_": mk(sa, seed + 1), "B_": mk(sb, seed + 2), "C_": mk(sc, seed + 3)}


PATHS = pytest.mark.parametrize("general", [False, True], ids=["default", "general"])
# 0 .. 9; around the wave and the wave x access width; the reduction block +- 1 and twice it +- 1; the elementwise block +- 1; past 4096
VECTOR_NS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4097)
# (w, h): w < 4, w % 4 != 0, h no multiple of the 16 outputs of a gemv_trans wave, the unroll depth +- 1 along k (h for notrans, w / 4 for trans)
GEMV_DIMS = ((1, 1), (1, 65), (64, 1), (2, 3), (3, 17), (7, 8), (8, 7), (9, 64), (65, 9), (28, 15), (32, 16), (36, 17), (130, 257), (257, 130), (64, 64), (4, 130))


def test_the_sizes_cover_the_kernels_own_constants():
    assert {RED_BLOCK - 1, RED_BLOCK, RED_BLOCK + 1, 2 * RED_BLOCK - 1, 2 * RED_BLOCK + 1, ELEM_BLOCK - 1, ELEM_BLOCK + 1, 64 * 2 + 1} <= set(VECTOR_NS)
    hs, nvecs = {h for _, h in GEMV_DIMS}, {w // V for w, _ in GEMV_DIMS}
    assert {GEMV_U - 1, GEMV_U, GEMV_U + 1, 2 * GEMV_U - 1, 2 * GEMV_U, 2 * GEMV_U + 1} <= hs and {GEMV_U - 1, GEMV_U, GEMV_U + 1} <= nvecs
    assert any(h % (GEMV_WG // V) for h in hs) and SMALL_TILE == 64 == TILE_N and LARGE_TILE == 128 and KC == 16


@pytest.mark.gpu
@PATHS
@pytest.mark.parametrize("name", VEC3 + REDS)
def test_vector_sizes(hl, canon_lib, name, general):
    for n in VECTOR_NS:
        _run(hl, name, _inputs(name, n, seed=n), general=general)


@pytest.mark.gpu
@PATHS
@pytest.mark.parametrize("name", ("halide_dgemv_notrans", "halide_dgemv_trans", "halide_dger_impl"))
def test_matrix_vector_sizes(hl, canon_lib, name, general):
    for dims in GEMV_DIMS:
        _run(hl, name, _inputs(name, dims, seed=sum(dims)), general=general)


def _gemm_dims(name):
    """M, N, K from 1 to one past two workgroup tiles (129) over the shapes the variant's rule allows, always with an odd K, a K = 1 and a
    K < KC"""
    if name == "halide_dgemm_notrans":
        return ((1, 1, 1), (2, 31, 33), (33, 2, 15), (64, 65, 1), (65, 64, 129), (96, 129, 2), (129, 96, 17), (129, 129, 16), (32, 33, 48), (31, 1, 129))
    if name == "halide_dgemm_transA":   # M == K
        return ((1, 1, 1), (33, 2, 33), (15, 64, 15), (65, 96, 65), (129, 31, 129), (2, 129, 2), (64, 33, 64), (128, 1, 128), (17, 65, 17))
    if name == "halide_dgemm_transB":   # N == K
        return ((1, 1, 1), (2, 33, 33), (64, 15, 15), (96, 65, 65), (31, 129, 129), (129, 2, 2), (33, 64, 64), (1, 128, 128), (65, 17, 17))
    return ((1, 1, 1), (2, 2, 2), (15, 15, 15), (16, 16, 16), (17, 17, 17), (64, 64, 64), (65, 65, 65), (96, 96, 96), (128, 128, 128), (129, 129, 129))


@pytest.mark.gpu
@PATHS
@pytest.mark.parametrize("name", GEMMS)
def test_gemm_sizes(hl, canon_lib, name, general):
    for dims in _gemm_dims(name):
        _run(hl, name, _inputs(name, dims, seed=sum(dims)), a=0.75, b=-1.5, general=general)


@pytest.mark.gpu
@pytest.mark.parametrize("name", GEMMS)
def test_gemm_aligned_cases_take_the_fast_kernel_of_each_tile(hl, canon_lib, name):
    fast, edge = ["dgemm_tile"], ["dgemm_tile_edge"]
    assert _run(hl, name, _inputs(name, (128, 128, 128), seed=5)) == fast
    assert _run(hl, name, _inputs(name, (128, 128, 128), seed=5), layouts={"A_": (130, 16), "C_": (140, 32), "result": (136, 0)}) == fast
    assert _run(hl, name, _inputs(name, (128, 128, 128), seed=5), layouts={"B_": (129, 0)}) == edge
    assert _run(hl, name, _inputs(name, (128, 128, 128), seed=5), layouts={"result": (130, 8)}) == edge
    if name == "halide_dgemm_notrans":   # the large tile at its threshold: 16 x 16 workgroups of 128 x 64, K two chunks (+ 1)
        assert _gemm_tile(2048, 1024) == LARGE_TILE and _gemm_tile(2048, 960) == SMALL_TILE == _gemm_tile(1920, 1024)
        assert _run(hl, name, _inputs(name, (2048, 1024, 2 * KC), seed=6)) == fast
        assert _run(hl, name, _inputs(name, (2048, 1023, 2 * KC + 1), seed=7)) == edge
        assert _run(hl, name, _inputs(name, (2048, 960, KC), seed=8)) == fast   # below it: the small tile


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("halide_dgemm_transA", "halide_dgemm_transB", "halide_dgemm_transAB"))
def test_gemm_large_tile_of_the_transposed_variants(hl, canon_lib, name):
    """the smallest shapes their rules allow that reach 256 workgroups of 128 x 64 (K is tied to M or N there)"""
    dims = {"halide_dgemm_transA": (256, 8192, 256), "halide_dgemm_transB": (8192, 256, 256), "halide_dgemm_transAB": (1472, 1472, 1472)}[name]
    assert _gemm_tile(dims[0], dims[1]) == LARGE_TILE
    assert _run(hl, name, _inputs(name, dims, seed=9)) == ["dgemm_tile" if dims[0] % LARGE_TILE == 0 else "dgemm_tile_edge"]


def _shapes_of(name, ins):
    shapes = {k: tuple(v.shape) for k, v in ins.items()}
    shapes.setdefault(_out_name(name), tuple(np.shape(_want(name, 0.5, -2.0, ins))))
    return {k: s for k, s in shapes.items() if s}


@pytest.mark.gpu
@PATHS
@EACH
def test_layouts_host_and_device_padded_and_off_the_grid(hl, canon_lib, name, general):
    dims = 261 if name in VEC3 + REDS else (67, 35) if name.startswith(("halide_dgemv", "halide_dger")) else \
        {"halide_dgemm_notrans": (67, 35, 41), "halide_dgemm_transA": (67, 35, 67), "halide_dgemm_transB": (67, 35, 35), "halide_dgemm_transAB": (67, 67, 67)}[name]
    ins = _inputs(name, dims, seed=3)
    shapes = _shapes_of(name, ins)
    for kinds in ("dev", "host"):
        _run(hl, name, ins, general=general, kinds=kinds)
    # 8 bytes off a 16-byte boundary is the only misalignment a double array can have; column strides odd and even in elements
    for el in (1, 2, 3):
        for which in shapes:
            pad = (shapes[which][1] + el) if len(shapes[which]) == 2 else None
            _run(hl, name, ins, general=general, layouts={which: (pad, 8 * (el & 1))})
    mixed = {k: ("host" if i % 2 else "dev") for i, k in enumerate(shapes)}
    _run(hl, name, ins, general=general, kinds=mixed, layouts={k: ((s[1] + 5) if len(s) == 2 else None, 0) for k, s in shapes.items()})
    _run(hl, name, ins, general=general, layouts={k: ((s[1] + 1) if len(s) == 2 else None, 8) for k, s in shapes.items()})


@pytest.mark.gpu
@PATHS
@pytest.mark.parametrize("name", [n for n in NAMES if _aliased_input(n)])
def test_in_place_calls_on_host_and_device_buffers(hl, canon_lib, name, general):
    dims = 261 if name in VEC3 else (67, 35) if name.startswith("halide_dgemv") else \
        {"halide_dgemm_notrans": (67, 35, 41), "halide_dgemm_transA": (64, 64, 64), "halide_dgemm_transB": (67, 35, 35), "halide_dgemm_transAB": (65, 65, 65)}[name]
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
    (hl.debug_linear_algebra_general_f64 if general else lambda n, *a: hl._check(call_direct(hl, n, *a)))("halide_daxpy_impl", *args)
    _same(args[3].numpy(), ld.daxpy(0.5, x, y0), "daxpy through two descriptors")


@pytest.mark.gpu
@PATHS
@EACH
def test_order_sensitive_subnormal_and_special_values(hl, canon_lib, name, general):
    dims = 1000 if name in VEC3 + REDS else (130, 65) if name.startswith(("halide_dgemv", "halide_dger")) else \
        {"halide_dgemm_notrans": (65, 33, 97), "halide_dgemm_transA": (65, 33, 65), "halide_dgemm_transB": (65, 33, 33), "halide_dgemm_transAB": (65, 65, 65)}[name]
    _run(hl, name, _inputs(name, dims, _order_sensitive, seed=20), a=0.7, b=-1.3, general=general)
    sub = _inputs(name, dims, lambda s, seed: _subnormal(s, seed, -520), seed=30)
    _run(hl, name, sub, a=2.0 ** -515, b=2.0 ** -517, general=general)
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
    _run(hl, "halide_ddot", {"x": x, "y": y}, general=general)
    _run(hl, "halide_dasum", {"x": xs}, general=general)
    A, xv, yv = _order_gemv_trans()
    _run(hl, "halide_dgemv_trans", {"A": A, "x": xv, "y": yv}, a=0.7, b=-1.3, general=general)
    A, xn, yn = _noise((40, 24), 304), _noise(40, 305), _noise(24, 306)   # (a * A) * x against a * (A * x)
    _run(hl, "halide_dgemv_notrans", {"A": A, "x": xn, "y": yn}, a=0.7, b=-1.3, general=general)
    ins = {"A_": _noise((12, 12), 307), "B_": _noise((12, 12), 308), "C_": _noise((12, 12), 309)}   # which product the epilogue fuses
    _run(hl, "halide_dgemm_notrans", ins, a=0.7, b=-1.3, general=general)


@pytest.mark.gpu
@PATHS
@pytest.mark.parametrize("name", ("halide_daxpy_impl", "halide_dscal_impl", "halide_dgemv_notrans", "halide_dgemv_trans", "halide_dger_impl") + GEMMS)
def test_the_scalars(hl, canon_lib, name, general):
    dims = 70 if name in VEC3 else (33, 17) if name.startswith(("halide_dgemv", "halide_dger")) else (33, 33, 33)
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
    """a zero-padded k step turns the chain's -0 into +0: K = 33 and 31 leave the last chunk partly filled, K = 17 starts a chunk with it"""
    for M, N, K in ((33, 33, 33), (64, 64, 64), (65, 40, 31), (128, 64, 17)):
        A, B, Cm = _gemm_trap(M, N, K, M // 3, N // 2)
        _run(hl, "halide_dgemm_notrans", {"A_": A, "B_": B, "C_": Cm}, a=1.0, b=1.0, general=general)
    Az = np.zeros((3, 70), f64)
    _run(hl, "halide_dgemv_notrans", {"A": Az, "x": np.full(3, -1.0, f64), "y": np.ones(70, f64)}, a=1.0, b=-0.0, general=general)
    _run(hl, "halide_dgemv_trans", {"A": Az, "x": np.ones(70, f64), "y": np.ones(3, f64)}, a=-1.0, b=-0.0, general=general)
    for n in (1, 4, 5, 300):
        _run(hl, "halide_ddot", {"x": np.full(n, -1.0, f64), "y": np.zeros(n, f64)}, general=general)


@pytest.mark.gpu
def test_the_empty_reductions_write_all_eight_bytes_of_plus_zero(hl):
    z = lambda n: np.zeros(max(n, 1), f64)[:n]
    for name, args in (("halide_ddot", lambda r: (hl.Buffer(z(0)), hl.Buffer(z(0)), r)), ("halide_dasum", lambda r: (hl.Buffer(z(0)), r))):
        out = np.full((), np.nan, f64)
        r = hl.Buffer(out)
        hl._check(call_direct(hl, name, *args(r)))
        assert r.numpy().view(u64) == 0, name


@pytest.mark.gpu
def test_argv_equals_the_direct_call(hl, canon_lib):
    for name in NAMES:
        ins = _inputs(name, 100 if name in VEC3 + REDS else (33, 17) if name.startswith(("halide_dgemv", "halide_dger")) else (33, 33, 33), seed=60)
        shapes = _shapes_of(name, ins)
        out = _out_name(name)
        bufs = {k: hl.Buffer(np.array(ins[k]) if k in ins else np.zeros(shapes.get(k, ()), f64)) for k in _buffers(name)
                if not (k == "y" and name in ("halide_dcopy_impl", "halide_dscal_impl"))}
        bufs.setdefault("y", None)
        a = 0.7 + 2.0 ** -40   # a value no float holds: the scalar crosses argv as eight bytes
        assert call_argv(hl, name, *_arguments(name, bufs, a, -1.3)) == 0
        _same(bufs[out].numpy(), _want(name, a, -1.3, ins), f"{name} through argv")


# ---------------------------------------------------------------------------------------------------- GPU: hblas, the consumer, torch
@pytest.mark.gpu
def test_the_references_protocol_at_768_through_hblas(hl):
    assert np.finfo(ext).eps < 2 ** -60
    L, d = _hblas(hl), _acceptance_inputs(11)
    a, b, x, y, A, B, Cm = (d[k] for k in "abxyABC")
    n, p = 768, lambda m: m.ctypes.data
    results = {}
    w = np.full(n, -1.0, f64)
    L.hblas_dcopy(n, p(x), 1, p(w), 1)
    results["halide_dcopy_impl"] = w
    w = x.copy()
    L.hblas_dscal(n, a, p(w), 1)
    results["halide_dscal_impl"] = w
    w = y.copy()
    L.hblas_daxpy(n, a, p(x), 1, p(w), 1)
    results["halide_daxpy_impl"] = w
    results["halide_ddot"] = np.array(L.hblas_ddot(n, p(x), 1, p(y), 1), f64)
    results["halide_dasum"] = np.array(L.hblas_dasum(n, p(x), 1), f64)
    for t, name in ((NOT, "halide_dgemv_notrans"), (TR, "halide_dgemv_trans")):
        w = y.copy()
        L.hblas_dgemv(COL, t, n, n, a, p(A), n, p(x), 1, b, p(w), 1)
        results[name] = w
    w = A.copy()
    L.hblas_dger(COL, n, n, a, p(x), 1, p(y), 1, p(w), n)
    results["halide_dger_impl"] = w
    for name, (ta, tb) in ld.GEMM_FLAGS.items():
        w = Cm.copy()
        L.hblas_dgemm(COL, TR if ta else NOT, TR if tb else NOT, n, n, n, a, p(A), n, p(B), n, b, p(w), n)
        results[name] = w
    for name in NAMES:
        eps = 32 if name in REDS else 16
        ok, worst = ld.compare(_acceptance_expected(name, 11), results[name], eps)
        print(f"{name}: worst {worst:.2f} eps of {eps}")
        assert ok, (name, worst)
    nrm = L.hblas_dnrm2(n, p(x), 1)
    assert ld.compare(np.array(np.sqrt((x.astype(ext) * x.astype(ext)).sum()), f64), np.array(nrm, f64), 32)[0]
    assert np.array_equal(x, d["x"]) and np.array_equal(A, d["A"])


@pytest.mark.gpu
def test_a_plain_c_consumer_of_hlmi_blas_h(hl, tmp_path):
    exe = tmp_path / "blas_consumer_f64"
    libdir, libname = os.path.split(hl.LIB_PATH)
    subprocess.run(["gcc", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "blas_consumer_f64.c"), "-o", str(exe),
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
    _same(back(ops.daxpy(0.7, tx, ty)), ld.daxpy(0.7, x, y), "daxpy")
    _same(back(ops.ddot(tx, ty)), ld.ddot(x, y), "ddot")
    _same(back(ops.dasum(tx)), ld.dasum(x), "dasum")
    y70 = _noise(70, 4)
    _same(back(ops.dgemv(True, 0.7, tA, tx, -1.3, cu(y70))), ld.dgemv(True, 0.7, A, x, -1.3, y70), "dgemv trans")
    _same(back(ops.dgemv(False, 0.7, tA, cu(y70), -1.3, ty)), ld.dgemv(False, 0.7, A, y70, -1.3, y), "dgemv notrans")
    _same(back(ops.dger(0.7, tx, cu(y70), tA)), ld.dger(0.7, x, y70, A), "dger")
    for name, (ta, tb) in ld.GEMM_FLAGS.items():
        M, N, K = (70, 45, 96) if name == "halide_dgemm_notrans" else (64, 64, 64)
        sa, sb, sc = _gemm_shapes(name, M, N, K)
        Am, Bm, Cm = _noise(sa, 5), _noise(sb, 6), _noise(sc, 7)
        tC = cu(Cm)
        out = ops.dgemm(bool(ta), bool(tb), 0.7, cu(Am), cu(Bm), -1.3, tC)
        _same(back(out), ld.dgemm(ta, tb, 0.7, Am, Bm, -1.3, Cm), name)
        assert np.array_equal(back(tC), Cm)
    assert np.array_equal(back(tx), x) and np.array_equal(back(ty), y) and np.array_equal(back(tA), A)
    # views with longer rows and a first element off the 16-byte grid
    big = torch.zeros((80, 313), dtype=torch.float64).cuda()
    big[3:73, 5:305] = tA
    _same(back(ops.dgemv(True, 0.7, big[3:73, 5:305], tx, -1.3, cu(y70))), ld.dgemv(True, 0.7, A, x, -1.3, y70), "dgemv on a view")
    with pytest.raises(TypeError):   # a float32 tensor is refused, not converted
        ops.daxpy(0.7, tx.float(), ty)


@pytest.mark.gpu
def test_seeded_fuzz_slice_of_linear_algebra_f64(on_stream):
    """scripts/fuzz_parity.py's linear_algebra_f64 case, a fixed number of cases from a fixed seed"""
    mod = load_fuzz_parity()
    rng = np.random.default_rng(20261019)
    for i in range(60):
        desc, ok = mod.CASES["linear_algebra_f64"](rng)
        assert ok, f"case {i}: {desc}"


@pytest.mark.gpu
def test_two_host_threads_call_an_s_and_a_d_routine_at_once(hl, canon_lib):
    from linear_algebra_checker import f32 as la
    rng = np.random.default_rng(5)
    A32, B32, C32 = ((rng.random(s, dtype=f32) * 2 - 1).astype(f32) for s in ((70, 96), (65, 70), (65, 96)))
    with la.canon(hl.canon_fma()):
        want32 = la.sgemm(0, 0, 0.7, A32, B32, -1.3, C32)
    ins = _inputs("halide_dgemm_notrans", (96, 65, 70), seed=1)
    want64 = _want("halide_dgemm_notrans", 0.7, -1.3, ins)
    errors = []

    def worker(i):
        try:
            for rep in range(6):
                if i == 0:
                    bufs = [hl.Buffer(m.copy()) for m in (A32, B32, C32)] + [hl.Buffer(np.zeros_like(want32))]
                    (hl.debug_sgemm_general if rep % 2 else hl.sgemm)(False, False, 0.7, bufs[0], bufs[1], -1.3, bufs[2], bufs[3])
                    same = np.array_equal(bufs[3].numpy().view(np.uint32), want32.view(np.uint32))
                else:
                    bufs = [hl.Buffer(ins[k].copy()) for k in ("A_", "B_", "C_")] + [hl.Buffer(np.zeros_like(want64))]
                    if rep % 2:
                        hl.debug_linear_algebra_general_f64("halide_dgemm_notrans", 0.7, bufs[0], bufs[1], -1.3, bufs[2], bufs[3])
                    else:
                        hl.dgemm(False, False, 0.7, bufs[0], bufs[1], -1.3, bufs[2], bufs[3])
                    same = np.array_equal(bufs[3].numpy().view(u64), want64.view(u64))
                if not same:
                    errors.append(f"thread {i} rep {rep}: differs")
        except Exception as e:  # noqa: BLE001
            errors.append(f"thread {i}: {e!r}")

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
