"""mat_mul: the square f32 matrix product of apps/cuda_mat_mul as an exact k-ordered fmaf chain.

The contract (include/hlmi_pipelines.h): out(x, y) = acc_n with acc_0 = +0 and acc_{r+1} = fmaf(A(x, r), B(r, y), acc_r);
dimension 0 is innermost, so with row-major arrays out = B @ A.  It is the same chain in both canonical float forms: both library
builds face the same checker output.  The checker is tests/cpp/mat_mul_check.c, plain C, built and bound by tests/mat_mul_checker.py.
The CPU tests hold the checker to independent evaluations (float64 where every partial sum is exact, libm's fmaf one output at a
time elsewhere), show that the inputs used on the GPU can tell a wrong order of summation from the right one, state the -0 trap in
numbers, and hold the entry points to their protocol; the GPU tests hold hl.mat_mul / hl.mat_mul_sized (the MFMA kernels) and
hl.debug_mat_mul_general (one thread per output) to the checker bit for bit."""
import ctypes as C
import ctypes.util
import functools
import os
import subprocess

import numpy as np
import pytest

import mat_mul_checker as mm
from parity_helpers import ROOT, DevArray, HostArray, address, call_argv, call_direct, kernel_const, load_fuzz_parity
from parity_helpers import gpu_present as _gpu_present, launches as _launches, same_bits as _same, same_bits_or_nan as _same_or_nan

f32, f64, u32 = np.float32, np.float64, np.uint32

# the plan's constants, read from the source: a kernel without them fails here
SMALL_TILE, LARGE_TILE, LARGE_FROM, KC, MAX_SIZE = (kernel_const("mat_mul.hip", n) for n in ("SMALL_TILE", "LARGE_TILE", "LARGE_FROM", "KC", "MAX_SIZE"))
FAST, EDGE, GENERAL = "mat_mul_mfma", "mat_mul_mfma_edge", "mat_mul_general"


def _tile(n):
    """mm_tile() of mat_mul.hip restated"""
    return LARGE_TILE if n >= LARGE_FROM else SMALL_TILE


def _expected_launch(n, general, layouts):
    """mm_plan() of mat_mul.hip restated; layouts: (device address, row stride in elements) of A, B and out"""
    if general:
        return GENERAL
    fast = n % _tile(n) == 0 and n % KC == 0 and all(addr % 16 == 0 and stride % 4 == 0 for addr, stride in layouts)
    return FAST if fast else EDGE


# ---------------------------------------------------------------------------------------------------- inputs
def _noise(n, seed):
    """[-1, 1)"""
    return (np.random.default_rng(seed).random((n, n), dtype=f32) * 2 - 1).astype(f32)


def _order_sensitive(n, seed):
    """(A, B): the products of an output mix +-2^24, +-1, +-2^-24 and noise, so that 2^24 + 1 + ... - 2^24 depends on the order of the
    additions and a wider accumulator keeps what f32 drops; the right half of A's columns holds no 2^24, so that there the sums stay
    small enough for the rounding of a noise x noise product (a multiply rounded before the add) to show"""
    rng = np.random.default_rng(seed)
    pool = np.array([2.0 ** 24, -2.0 ** 24, 1.0, -1.0, 2.0 ** -24, -2.0 ** -24], f32)
    A = rng.choice(pool, (n, n)).astype(f32)
    A[:, n // 2:] = rng.choice(pool[2:], (n, n - n // 2))
    B = np.where(rng.random((n, n)) < 0.5, f32(1), f32(-1)).astype(f32)
    for m in (A, B):
        pick = rng.random((n, n)) < 0.3
        m[pick] = (rng.random((n, n), dtype=f32) * 2 - 1)[pick]
    return A, B


def _minus_zero_trap(n, x0, y0):
    """all zero except A(x0, n - 1) = -2^-100 and B(n - 1, y0) = 2^-100: the chain at (x0, y0) is +0 until its last step, whose product
    underflows to -0"""
    A, B = np.zeros((n, n), f32), np.zeros((n, n), f32)
    A[n - 1, x0] = -2.0 ** -100
    B[y0, n - 1] = 2.0 ** -100
    return A, B


def _subnormal(n, seed):
    """products near 2^-145 and sums below n * 2^-145 < 2^-126: everything after the inputs is subnormal"""
    rng = np.random.default_rng(seed)
    A = ((rng.random((n, n), dtype=f32) * 2 - 1) * f32(2.0 ** -75)).astype(f32)
    B = ((rng.random((n, n), dtype=f32) * 2 - 1) * f32(2.0 ** -70)).astype(f32)
    return A, B


SPECIALS = np.array([0.0, -0.0, 1e-40, -3e-39, np.inf, -np.inf, np.nan, 3e38, -2e38, 2.0 ** 100, -2.0 ** 100], f32)


def _special_values(n, seed):
    """Noise with a handful of +-0, subnormals, +-Inf, NaN and magnitudes whose products overflow.  A special in A(x, r) reaches every
    output of column x and one in B(r, y) every output of row y, so they sit in at most n // 16 columns of A and n // 16 rows of B: at
    most an eighth of the outputs can be NaN"""
    rng = np.random.default_rng(seed)
    A, B = _noise(n, seed + 1), _noise(n, seed + 2)
    k = max(1, n // 16)
    cols, rows = rng.choice(n, k, replace=False), rng.choice(n, k, replace=False)
    for c in cols:
        r = rng.integers(0, n, 3)
        A[r, c] = rng.choice(SPECIALS, 3)
    for y in rows:
        r = rng.integers(0, n, 3)
        B[y, r] = rng.choice(SPECIALS, 3)
    # one of each in a known place
    A[0, cols[0]], A[1, cols[0]] = np.inf, -np.inf
    B[rows[0], 2], B[rows[0], 3] = np.nan, 2.0 ** 100
    A[3, cols[-1]] = 2.0 ** 100
    return A, B


@functools.lru_cache(maxsize=None)
def _case(kind, n, seed=0):
    """(A, B, the checker's output), computed once per module and never written to"""
    if kind == "noise":
        A, B = _noise(n, 100 + seed), _noise(n, 200 + seed)
    elif kind == "order":
        A, B = _order_sensitive(n, 300 + seed)
    elif kind == "subnormal":
        A, B = _subnormal(n, 400 + seed)
    elif kind == "special":
        A, B = _special_values(n, 500 + seed)
    elif kind == "runner":   # the reference's runner.cpp: entries (rand & 3) - 1
        rng = np.random.default_rng(600 + seed)
        A, B = ((rng.integers(0, 2 ** 31, (n, n)) & 3) - 1).astype(f32), ((rng.integers(0, 2 ** 31, (n, n)) & 3) - 1).astype(f32)
    else:
        raise KeyError(kind)
    want = mm.run(A, B)
    for m in (A, B, want):
        m.setflags(write=False)
    return A, B, want


# ---------------------------------------------------------------------------------------------------- independent evaluations
def _libm_fmaf():
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype, libm.fmaf.argtypes = C.c_float, [C.c_float, C.c_float, C.c_float]
    return libm.fmaf


def _chain_by_libm(A, B):
    """the chain stepped one output at a time through libm's fmaf"""
    fmaf = _libm_fmaf()
    n = A.shape[0]
    out = np.zeros((n, n), f32)
    for y in range(n):
        for x in range(n):
            acc = 0.0
            for r in range(n):
                acc = fmaf(float(A[r, x]), float(B[y, r]), acc)
            out[y, x] = acc
    return out


def _products(A, B):
    """P[r][y][x] = A(x, r) * B(r, y) in float64 (exact: 24 x 24 bits)"""
    return A.astype(f64)[:, None, :] * B.astype(f64).T[:, :, None]


def _descending(A, B):
    """the same fmaf chain with r running downward, stepped through libm as well"""
    return _chain_by_libm(A[::-1], B[:, ::-1])


def _pairwise(A, B):
    """products rounded to f32, then a balanced tree of f32 additions"""
    with np.errstate(all="ignore"):
        t = _products(A, B).astype(f32)
        while t.shape[0] > 1:
            if t.shape[0] % 2:
                t = np.concatenate([t, np.zeros((1,) + t.shape[1:], f32)])
            t = (t[0::2] + t[1::2]).astype(f32)
    return t[0]


def _f64_once(A, B):
    with np.errstate(all="ignore"):
        return (B.astype(f64) @ A.astype(f64)).astype(f32)


def _mul_then_add(A, B):
    """one rounding per operator: acc = round(round(a * b) + acc), r upward"""
    n = A.shape[0]
    acc = np.zeros((n, n), f32)
    with np.errstate(all="ignore"):
        for r in range(n):
            acc = ((A[r][None, :] * B[:, r][:, None]).astype(f32) + acc).astype(f32)
    return acc


# ---------------------------------------------------------------------------------------------------- CPU 1: the checker
def test_the_checker_equals_float64_where_every_partial_sum_is_exact():
    rng = np.random.default_rng(1)
    for n in (1, 2, 7, 33, 64, 100):
        ints = [rng.integers(-8, 9, (n, n)).astype(f32) for _ in range(2)]
        dyadic = [(rng.integers(-15, 16, (n, n)) * 2.0 ** rng.integers(-3, 4, (n, n))).astype(f32) for _ in range(2)]   # 4 bits at 2^-3 .. 2^3
        for A, B in (ints, dyadic):
            want = B.astype(f64) @ A.astype(f64)
            assert np.abs(want).max() < 2 ** 24 / 64   # every partial sum is a multiple of 2^-6 below 2^18: exact in f32
            _same(mm.run(A, B), want.astype(f32), f"exact inputs n {n}")
    A, B, want = _case("runner", 96)
    _same(want, (B.astype(f64) @ A.astype(f64)).astype(f32), "runner's entries")


def test_the_checker_equals_the_chain_stepped_through_libm():
    for n, seed in ((1, 1), (2, 2), (5, 3), (32, 4), (33, 5)):
        A, B = _noise(n, seed), _noise(n, seed + 50)
        _same(mm.run(A, B), _chain_by_libm(A, B), f"noise n {n}")
    A, B = _order_sensitive(17, 9)
    _same(mm.run(A, B), _chain_by_libm(A, B), "order-sensitive n 17")
    A, B = _subnormal(9, 9)
    _same(mm.run(A, B), _chain_by_libm(A, B), "subnormal n 9")


def test_the_checker_reads_padded_rows():
    n = 19
    A, B = _noise(n, 1), _noise(n, 2)
    wide = lambda m, pad: np.lib.stride_tricks.as_strided(np.concatenate([np.concatenate([m, np.full((n, pad), 9e9, f32)], axis=1).ravel(), np.zeros(8, f32)]),
                                                         (n, n), (4 * (n + pad), 4))
    _same(mm.run(wide(A, 3), wide(B, 1)), mm.run(A, B), "padded rows")


# ---------------------------------------------------------------------------------------------------- CPU 2: the tests can tell
ORDER_NS = (33, 64)   # the odd and the even size the GPU runs the order-sensitive input at


@pytest.mark.parametrize("n", ORDER_NS)
def test_the_order_sensitive_input_tells_every_wrong_association(n):
    A, B, want = _case("order", n)
    assert np.isfinite(want).all()
    differs = lambda other: np.count_nonzero(other.view(u32) != want.view(u32))
    assert differs(_descending(A, B)) > 0, "a descending-k chain"
    assert differs(_pairwise(A, B)) > 0, "a pairwise sum"
    assert differs(_f64_once(A, B)) > 0, "a float64 sum rounded once"
    assert differs(_mul_then_add(A, B)) > 0, "a mul-then-add chain"


# ---------------------------------------------------------------------------------------------------- CPU 3: the -0 trap
@pytest.mark.parametrize("n", [1, 3, 33, 65])
def test_the_minus_zero_trap_in_numbers(n):
    x0, y0 = n // 3, n // 2
    A, B = _minus_zero_trap(n, x0, y0)
    got = mm.run(A, B).view(u32)
    assert got[y0, x0] == 0x80000000
    got[y0, x0] = 0
    assert not got.any()   # every other output is +0
    # one further, zero-padded step turns it into +0
    fmaf = _libm_fmaf()
    assert np.array([fmaf(0.0, 0.0, -0.0)], f32).view(u32)[0] == 0x00000000
    assert np.array([fmaf(-2.0 ** -100, 2.0 ** -100, 0.0)], f32).view(u32)[0] == 0x80000000


def test_the_subnormal_input_stays_subnormal():
    for n in (33, 64):
        A, B, want = _case("subnormal", n)
        tiny = np.finfo(f32).tiny
        assert (np.abs(want) < tiny).all() and np.count_nonzero(want) > 0.9 * want.size
        assert (np.abs(_products(A, B)) < tiny).all()


# ---------------------------------------------------------------------------------------------------- CPU 4: cap on NaN
SPECIAL_NS = (65, 128)


@pytest.mark.parametrize("n", SPECIAL_NS)
def test_the_special_values_leave_most_outputs_numbers(n):
    A, B, want = _case("special", n)
    for v in (np.inf, -np.inf):
        assert (A == v).any() or (B == v).any()
    assert np.isnan(B).any() and (np.abs(want) == np.inf).any()
    nan = np.count_nonzero(np.isnan(want))
    assert 0 < nan <= 0.25 * want.size, nan


# ---------------------------------------------------------------------------------------------------- CPU 5: the library's surface
def test_the_entry_point_is_exported_with_argv_and_metadata(hl):
    lib = C.CDLL(hl.LIB_PATH)
    for sym in ("mat_mul", "mat_mul_argv", "mat_mul_metadata", "hlmi_mat_mul_sized", "hlmi_mat_mul_general"):
        assert hasattr(lib, sym), sym
    assert not hasattr(lib, "mat_mul_auto_schedule")
    assert hl._fn["mat_mul"] is not None and callable(hl.mat_mul) and callable(hl.mat_mul_sized) and callable(hl.debug_mat_mul_general)


def test_metadata_states_three_square_f32_buffers(hl):
    md = hl.metadata("mat_mul")
    assert md.version == 1 and md.num_arguments == 3 and md.name.decode() == "mat_mul" and b"hip" in md.target
    a = [md.arguments[i] for i in range(3)]
    assert [x.name.decode() for x in a] == ["A", "B", "out"]
    assert [x.kind for x in a] == [1, 1, 2]
    assert [(x.type.code, x.type.bits) for x in a] == [(2, 32)] * 3
    assert [x.dimensions for x in a] == [2] * 3
    for x in a:
        assert [x.buffer_estimates[i][0] for i in range(4)] == [0, 1024, 0, 1024]


def test_the_aot_header_compiles_as_c(tmp_path):
    decl = " ".join(open(os.path.join(ROOT, "include", "hlmi_pipelines.h")).read().split())
    assert "int mat_mul(struct halide_buffer_t *A, struct halide_buffer_t *B, struct halide_buffer_t *out);" in decl
    src = tmp_path / "c.c"
    src.write_text('#include "aot/mat_mul.h"\nint (*const f)(struct halide_buffer_t *, struct halide_buffer_t *, struct halide_buffer_t *) = mat_mul;\n'
                   "int (*const a)(void **) = mat_mul_argv;\nconst struct halide_filter_metadata_t *(*const m)(void) = mat_mul_metadata;\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "c.o")], check=True)


# ---- the entry protocol
S0 = 20   # the size the sized entry point is asked for below


def _mk(hl, n=S0, dtype=f32, mins=None, shape=None):
    return hl.Buffer(np.zeros(shape or (n, n), dtype), mins=mins)


def _sized(hl, size=S0, symbol="hlmi_mat_mul_sized", **over):
    """hlmi_mat_mul_sized(size, ...) on three size x size buffers, with the named arguments replaced; returns the code"""
    args = {"A": _mk(hl, size), "B": _mk(hl, size), "out": _mk(hl, size)}
    args.update(over)
    return hl._mat_mul_hook(symbol)(size, *[None if args[k] is None else args[k].ptr for k in ("A", "B", "out")])


HOW = pytest.mark.parametrize("how", [call_direct, call_argv], ids=["direct_call", "argv"])
NAMES3 = ("A", "B", "out")


def _full(hl, how, **over):
    """mat_mul itself (size 1024) on three 1024 x 1024 buffers (untouched zero pages), with the named arguments replaced"""
    args = {k: _mk(hl, 1024) for k in NAMES3}
    args.update(over)
    return how(hl, "mat_mul", *[args[k] for k in NAMES3])


def _ok():
    return 0 if _gpu_present() else -29   # with everything in order only the device can be missing


@HOW
def test_a_call_in_order_reaches_the_device(hl, how):
    assert _full(hl, how) == _ok()
    assert _sized(hl) == _ok() and _sized(hl, symbol="hlmi_mat_mul_general") == _ok()


@HOW
@pytest.mark.parametrize("which", NAMES3)
def test_a_bounds_query_on_any_buffer_fills_all_three(hl, how, which):
    dims = lambda b: [(b.raw.dim[i].min, b.raw.dim[i].extent, b.raw.dim[i].stride) for i in range(2)]
    q = hl.Buffer.bounds_query(f32, 2, mins=(5, 6), extents=(7, 8))
    others = {k: hl.Buffer.bounds_query(f32, 2) for k in NAMES3 if k != which}
    assert _full(hl, how, **{which: q}, **others) == 0
    for b in [q] + list(others.values()):
        assert dims(b) == [(0, 1024, 1), (0, 1024, 1024)]
    # real buffers beside the query stay as they are, whatever their shape
    q, small = hl.Buffer.bounds_query(f32, 2), _mk(hl, 9)
    other = [k for k in NAMES3 if k != which]
    assert _full(hl, how, **{which: q, other[0]: small}) == 0
    assert dims(q) == [(0, 1024, 1), (0, 1024, 1024)] and dims(small) == [(0, 9, 1), (0, 9, 9)]
    # the sized entry point answers its own size
    q = hl.Buffer.bounds_query(f32, 2)
    assert _sized(hl, 48, **{which: q}) == 0 and dims(q) == [(0, 48, 1), (0, 48, 48)]
    # a query buffer of the wrong type is rewritten, one of the wrong dimensionality stays an error
    q = hl.Buffer.bounds_query(np.uint16, 2)
    assert _full(hl, how, **{which: q}) == 0 and (q.raw.type.code, q.raw.type.bits) == (2, 32)
    assert _full(hl, how, **{which: hl.Buffer.bounds_query(f32, 3)}) == -43


@HOW
@pytest.mark.parametrize("which", NAMES3)
def test_a_null_argument_is_refused(hl, how, which):
    assert _full(hl, how, **{which: None}) == -12 and which in hl.last_error()
    assert _sized(hl, **{which: None}) == -12


@HOW
@pytest.mark.parametrize("which", NAMES3)
def test_a_wrong_type_is_refused(hl, how, which):
    assert _full(hl, how, **{which: _mk(hl, 1024, np.uint16)}) == -3 and which in hl.last_error()
    assert _full(hl, how, **{which: _mk(hl, 1024, np.int32)}) == -3
    assert _full(hl, how, **{which: _mk(hl, 512, np.float64)}) == -3


@HOW
@pytest.mark.parametrize("which", NAMES3)
def test_a_3d_buffer_is_refused(hl, how, which):
    assert _full(hl, how, **{which: _mk(hl, shape=(1, 1024, 1024))}) == -43 and which in hl.last_error()
    assert _full(hl, how, **{which: hl.Buffer(np.zeros(1024, f32))}) == -43


@HOW
@pytest.mark.parametrize("which", NAMES3)
def test_extent_1023_is_refused(hl, how, which):
    assert _full(hl, how, **{which: _mk(hl, shape=(1024, 1023))}) == -8 and f"{which}.extent.0" in hl.last_error()
    assert _full(hl, how, **{which: _mk(hl, shape=(1023, 1024))}) == -8 and f"{which}.extent.1" in hl.last_error()
    assert _full(hl, how, **{which: _mk(hl, shape=(1025, 1025))}) == -8
    assert _sized(hl, 1023, **{which: _mk(hl, 1024)}) == -8 and _sized(hl, 1023) == _ok()


@HOW
@pytest.mark.parametrize("which", NAMES3)
def test_min_1_is_refused(hl, how, which):
    assert _full(hl, how, **{which: _mk(hl, 1024, mins=(1, 0))}) == -8 and f"{which}.min.0" in hl.last_error()
    assert _full(hl, how, **{which: _mk(hl, 1024, mins=(0, 1))}) == -8 and f"{which}.min.1" in hl.last_error()
    assert _full(hl, how, **{which: _mk(hl, 1024, mins=(0, -1))}) == -8


@HOW
@pytest.mark.parametrize("which", NAMES3)
def test_stride_2_in_dimension_0_is_refused(hl, how, which):
    b = hl.Buffer(np.zeros((1024, 2048), f32)[:, ::2])
    assert b.dim(0).stride == 2
    assert _full(hl, how, **{which: b}) == -8 and f"{which}.stride.0" in hl.last_error()


@HOW
@pytest.mark.parametrize("which", NAMES3)
def test_a_row_stride_below_the_size_is_refused_and_one_above_it_is_not(hl, how, which):
    b = _mk(hl, 1024)
    b.dim(1).stride = 1023   # rows that overlap
    assert _full(hl, how, **{which: b}) == -8 and f"{which}.stride.1" in hl.last_error()
    b.dim(1).stride = 0
    assert _full(hl, how, **{which: b}) == -8
    padded = hl.Buffer(np.zeros((1024, 1031), f32)[:, :1024])
    assert padded.dim(1).stride == 1031
    assert _full(hl, how, **{which: padded}) == _ok()


def test_sizes_0_and_8193_are_refused(hl):
    assert MAX_SIZE == 8192
    for symbol in ("hlmi_mat_mul_sized", "hlmi_mat_mul_general"):
        for size in (0, -1, MAX_SIZE + 1):
            fn = hl._mat_mul_hook(symbol)
            a, b, o = _mk(hl, 4), _mk(hl, 4), _mk(hl, 4)
            assert fn(size, a.ptr, b.ptr, o.ptr) == -8 and "size" in hl.last_error()
    assert _sized(hl, 1) == _ok()


def test_out_may_not_alias_an_input(hl):
    a = _mk(hl)
    assert _sized(hl, A=a, out=a) == -8 and "alias" in hl.last_error()
    assert _sized(hl, B=a, out=a) == -8
    whole = np.zeros((2 * S0, S0), f32)
    top, shifted = hl.Buffer(whole[:S0]), hl.Buffer(whole[S0 - 1:2 * S0 - 1])   # one shared row
    assert _sized(hl, A=top, out=shifted) == -8
    assert _sized(hl, A=a, B=a) == _ok()   # the inputs may be one matrix
    assert _sized(hl, A=hl.Buffer(whole[:S0]), out=hl.Buffer(whole[S0:])) == _ok()   # neighbours in one allocation


def test_the_order_of_the_checks(hl):
    assert _sized(hl, A=None, B=_mk(hl, dtype=np.uint16)) == -12                           # null before type
    assert _sized(hl, A=_mk(hl, shape=(2, S0, S0), dtype=np.uint16)) == -3                 # type before dimensionality
    assert _sized(hl, A=_mk(hl, shape=(2, S0, S0)), B=_mk(hl, mins=(1, 0))) == -43         # dimensionality before the pins
    a = _mk(hl)
    assert _sized(hl, A=a, out=a, B=_mk(hl, S0 + 1)) == -8 and "B.extent" in hl.last_error()   # the pins before the alias check


def test_without_a_gpu_the_python_calls_refuse_to_run(hl):
    if _gpu_present():
        return   # the statement is about a machine without one
    a, b, o = _mk(hl), _mk(hl), _mk(hl)
    for fn in (lambda: hl.mat_mul_sized(S0, a, b, o), lambda: hl.debug_mat_mul_general(S0, a, b, o), lambda: hl.mat_mul(_mk(hl, 1024), _mk(hl, 1024), _mk(hl, 1024))):
        with pytest.raises(hl.HalideError) as e:
            fn()
        assert e.value.code == -29


def test_torch_shape_function_and_refusals():
    import torch
    import halide_amd.torch_ops  # noqa: F401
    op = torch.ops.hlmi.mat_mul
    out = op(torch.empty((45, 45), dtype=torch.float32, device="meta"), torch.empty((45, 45), dtype=torch.float32, device="meta"))
    assert out.shape == (45, 45) and out.dtype == torch.float32
    sq = torch.zeros((8, 8))
    with pytest.raises(RuntimeError, match="GPU"):
        op(sq, sq)
    for bad in (torch.zeros((8, 9)), torch.zeros((9, 9)), torch.zeros((8, 8), dtype=torch.float64), torch.zeros((8, 8), dtype=torch.int32),
                torch.zeros(64), torch.zeros((1, 8, 8))):
        with pytest.raises(TypeError):
            op(sq, bad)
        with pytest.raises(TypeError):
            op(bad, sq)


def test_the_fuzzer_has_the_case():
    src = open(os.path.join(ROOT, "scripts", "fuzz_parity.py")).read()
    assert "def fuzz_mat_mul(rng):" in src and 'CASES["mat_mul"] = fuzz_mat_mul' in src and "def case_mat_mul" not in src


# ---------------------------------------------------------------------------------------------------- GPU
PATHS = pytest.mark.parametrize("general", [False, True], ids=["default", "general"])


def _run(hl, n, a, b, o, general=False):
    (hl.debug_mat_mul_general if general else hl.mat_mul_sized)(n, a, b, o)


def _gpu(hl, A, B, general=False):
    """the call on dense host buffers; returns out"""
    n = A.shape[0]
    o = hl.Buffer(np.zeros((n, n), f32))
    _run(hl, n, hl.Buffer(np.ascontiguousarray(A)), hl.Buffer(np.ascontiguousarray(B)), o, general)
    return o.numpy()


# the issue's sizes, and one below, at and one above each tile and chunk constant of mat_mul.hip and the size the plan changes tile at
SIZES = sorted({1, 2, 3, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 191}
               | {c + d for c in (SMALL_TILE, LARGE_TILE, KC, KC // 2, LARGE_FROM) for d in (-1, 0, 1)})


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_sizes(hl, n):
    A, B, want = _case("noise", n)
    for general in (False, True):
        _same(_gpu(hl, A, B, general), want, f"n {n} general {general}")


@pytest.mark.gpu
def test_1024_through_mat_mul_and_mat_mul_argv(hl, on_stream):
    """the runner's own check — entries (rand & 3) - 1, the result equal to float64 B @ A exactly — and once noise against the checker"""
    A, B, want = _case("runner", 1024)
    _same(want, (B.astype(f64) @ A.astype(f64)).astype(f32), "the checker on the runner's entries")
    for how in (call_direct, call_argv):
        o = hl.Buffer(np.zeros((1024, 1024), f32))
        assert how(hl, "mat_mul", hl.Buffer(A.copy()), hl.Buffer(B.copy()), o) == 0
        _same(o.numpy(), want, f"runner {how.__name__}")
    A, B, want = _case("noise", 1024)
    a, b, o = hl.Buffer(A.copy()), hl.Buffer(B.copy()), hl.Buffer(np.zeros((1024, 1024), f32))
    ran = _launches(hl, lambda: hl.mat_mul(a, b, o))
    assert ran == [_expected_launch(1024, False, [(t.raw.device, 1024) for t in (a, b, o)])]
    _same(o.numpy(), want, "noise")


@pytest.mark.gpu
@PATHS
@pytest.mark.parametrize("n,x0,y0,r0", [(96, 5, 40, 70), (97, 70, 5, 96), (128, 5, 40, 100), (128, 100, 70, 5)])
def test_orientation(hl, general, n, x0, y0, r0):
    """a swapped operand or C/D map hides behind symmetric matrices: identity against an asymmetric matrix on either side, and a single
    non-zero product that may land in one place only"""
    eye, M = np.eye(n, dtype=f32), _noise(n, 7)
    assert not np.array_equal(M, M.T)
    _same(_gpu(hl, eye, M, general), M, "A = I gives B")
    _same(_gpu(hl, M, eye, general), M, "B = I gives A")
    assert len({x0 // 32, y0 // 32, r0 // 32}) == 3
    A, B = np.zeros((n, n), f32), np.zeros((n, n), f32)
    A[r0, x0], B[y0, r0] = 3.0, 5.0   # A(x0, r0), B(r0, y0)
    want = np.zeros((n, n), f32)
    want[y0, x0] = 15.0
    _same(mm.run(A, B), want, "the checker")
    _same(_gpu(hl, A, B, general), want, "one-hot")


@pytest.mark.gpu
@PATHS
@pytest.mark.parametrize("n", ORDER_NS)
def test_the_order_sensitive_input(hl, general, n):
    A, B, want = _case("order", n)
    _same(_gpu(hl, A, B, general), want, f"order-sensitive n {n}")


@pytest.mark.gpu
@PATHS
@pytest.mark.parametrize("n", [33, 64, 65, 128])
def test_minus_zero_and_subnormals(hl, general, n):
    x0, y0 = n // 3, n // 2
    A, B = _minus_zero_trap(n, x0, y0)
    got = _gpu(hl, A, B, general)
    assert got.view(u32)[y0, x0] == 0x80000000, hex(got.view(u32)[y0, x0])
    _same(got, mm.run(A, B), f"-0 n {n}")
    A, B, want = _case("subnormal", n)
    _same(_gpu(hl, A, B, general), want, f"subnormal n {n}")


@pytest.mark.gpu
@PATHS
@pytest.mark.parametrize("n", SPECIAL_NS)
def test_special_values(hl, general, n):
    A, B, want = _case("special", n)
    _same_or_nan(_gpu(hl, A, B, general), want, f"special values n {n}")


def _layout_case(hl, n, kinds, la, lb, lo, general, data=None):
    """One call with A, B and out each in host memory ("host": the library's own device mirror) or in a device allocation of the test's
    own ("dev"), with (row stride or None, byte offset).  Asserts the launch the restated predicate names, the bits, and the sentinels."""
    A, B, want = data or _case("noise", n)
    mk = lambda kind, lay, fill: (HostArray if kind == "host" else DevArray)(hl, (n, n), f32, lay[0], offset=lay[1], fill=fill)
    a, b, o = mk(kinds[0], la, A), mk(kinds[1], lb, B), mk(kinds[2], lo, None)
    try:
        ran = _launches(hl, lambda: _run(hl, n, a.buf, b.buf, o.buf, general))
        layouts = [(address(t), t.buf.dim(1).stride) for t in (a, b, o)]
        assert ran == [_expected_launch(n, general, layouts)], (ran, layouts)
        _same(o.result(), want, f"n {n} {kinds} A {la} B {lb} out {lo} general {general}")
        for t in (a, b):
            if isinstance(t, DevArray):
                t.result()   # the inputs and the bytes around them are as they were
        return ran[0]
    finally:
        a.free(), b.free(), o.free()


DENSE = (None, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [1, 3])
@pytest.mark.parametrize("which", ["A", "B", "out", "all"])
def test_padded_rows(hl, on_stream, which, pad):
    n = 64
    lay = lambda k: (n + pad, 0) if which in (k, "all") else DENSE
    assert _layout_case(hl, n, ("dev",) * 3, lay("A"), lay("B"), lay("out"), False) == EDGE
    assert _layout_case(hl, n, ("dev",) * 3, lay("A"), lay("B"), lay("out"), True) == GENERAL


@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 128])
def test_aligned_layouts_take_the_fast_kernel_padded_rows_included(hl, on_stream, n):
    assert _layout_case(hl, n, ("dev",) * 3, DENSE, DENSE, DENSE, False) == FAST
    assert _layout_case(hl, n, ("dev",) * 3, (n + 4, 0), (n + 12, 16), (n + 8, 32), False) == FAST
    assert _layout_case(hl, n, ("host",) * 3, DENSE, DENSE, DENSE, False) in (FAST, EDGE)   # as the predicate says of the mirrors' addresses


@pytest.mark.gpu
@pytest.mark.parametrize("elements", [1, 2, 3])
@pytest.mark.parametrize("which", ["A", "B", "out"])
def test_pointers_off_the_16_byte_grid(hl, which, elements):
    n = 64
    lay = lambda k: (n + 4, 4 * elements) if which == k else DENSE
    assert _layout_case(hl, n, ("dev",) * 3, lay("A"), lay("B"), lay("out"), False) == EDGE
    assert _layout_case(hl, n, ("dev",) * 3, lay("A"), lay("B"), lay("out"), True) == GENERAL


@pytest.mark.gpu
@PATHS
def test_host_and_device_buffers_mix(hl, general):
    for n in (64, 65):
        for kinds in (("host", "dev", "dev"), ("dev", "host", "host"), ("host", "host", "dev")):
            _layout_case(hl, n, kinds, (n + 3, 0) if kinds[0] == "host" else DENSE, DENSE, (n + 1, 4) if kinds[2] == "dev" else (n + 5, 0), general)


@pytest.mark.gpu
def test_a_size_off_the_tile_takes_the_edge_kernel(hl):
    for n in (KC, SMALL_TILE + 1, SMALL_TILE + KC, 2 * SMALL_TILE - 1):
        assert _layout_case(hl, n, ("dev",) * 3, DENSE, DENSE, DENSE, False) == (FAST if n % SMALL_TILE == 0 else EDGE)


@pytest.mark.gpu
def test_the_large_tile_on_padded_and_offset_buffers(hl):
    """the sizes from LARGE_FROM on run the 2 x 2 wave tile, which no smaller size reaches: its aligned kernel on padded rows and its edge
    variant on an aligned size with rows and a pointer off the grid"""
    n = LARGE_FROM
    assert _layout_case(hl, n, ("dev",) * 3, (n + 4, 16), DENSE, (n + 8, 0), False) == FAST
    assert _layout_case(hl, n, ("dev",) * 3, (n + 1, 0), (n + 4, 4), (n + 3, 8), False) == EDGE


@pytest.mark.gpu
def test_argv_equals_the_direct_call_on_both_internal_entry_points(hl):
    A, B, want = _case("noise", 96)
    for symbol in ("hlmi_mat_mul_sized", "hlmi_mat_mul_general"):
        o = hl.Buffer(np.zeros((96, 96), f32))
        assert hl._mat_mul_hook(symbol)(96, hl.Buffer(A.copy()).ptr, hl.Buffer(B.copy()).ptr, o.ptr) == 0
        _same(o.numpy(), want, symbol)


@pytest.mark.gpu
def test_torch_op(hl):
    import torch
    import halide_amd.torch_ops  # noqa: F401
    op = torch.ops.hlmi.mat_mul
    for n in (96, 1024):
        A, B, want = _case("noise", n)
        ta, tb = torch.from_numpy(A.copy()).cuda(), torch.from_numpy(B.copy()).cuda()
        out = op(ta, tb)
        torch.cuda.synchronize()
        assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (n, n)
        o = hl.Buffer(np.zeros((n, n), f32))
        hl.mat_mul_sized(n, hl.Buffer(A.copy()), hl.Buffer(B.copy()), o)
        _same(out.cpu().numpy(), o.numpy(), f"torch against hl.mat_mul_sized n {n}")
        _same(out.cpu().numpy(), want, f"torch against the checker n {n}")
        assert np.array_equal(ta.cpu().numpy(), A) and np.array_equal(tb.cpu().numpy(), B)
        # which way round: B @ A, to float64's accuracy
        ref = B.astype(f64) @ A.astype(f64)
        assert np.abs(out.cpu().numpy() - ref).max() < 1e-3 and np.abs(out.cpu().numpy() - (A.astype(f64) @ B.astype(f64))).max() > 1.0
    # views with longer rows and a first element off the 16-byte grid
    n = 96
    A, B, want = _case("noise", n)
    big = torch.zeros((2, n + 2, n + 13), dtype=torch.float32).cuda()
    big[0, 1:n + 1, 3:n + 3], big[1, 1:n + 1, 5:n + 5] = torch.from_numpy(A.copy()).cuda(), torch.from_numpy(B.copy()).cuda()
    _same(op(big[0, 1:n + 1, 3:n + 3], big[1, 1:n + 1, 5:n + 5]).cpu().numpy(), want, "torch views")
    for bad in (torch.zeros((8, 9)).cuda(), torch.zeros((9, 9)).cuda(), torch.zeros((8, 8), dtype=torch.float64).cuda()):
        with pytest.raises(TypeError):
            op(torch.zeros((8, 8)).cuda(), bad)


@pytest.mark.gpu
def test_seeded_fuzz_slice_of_mat_mul(on_stream):
    """scripts/fuzz_parity.py's mat_mul case, a fixed number of cases from a fixed seed"""
    mod = load_fuzz_parity()
    rng = np.random.default_rng(20261019)
    for i in range(40):
        desc, ok = mod.CASES["mat_mul"](rng)
        assert ok, f"case {i}: {desc}"
