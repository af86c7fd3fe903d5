"""hannk's pooling, mean, add, mul, softmax and l2_normalization ops (halide_amd/csrc/hannk_nn.hip).

CPU: the plain-C checker against an independent numpy evaluator (explicit wrap and saturate helpers), the reference's own acceptance of
approx_log2 / approx_exp2 on its full grids, closeness to float64, known answers for the traps, the entry protocol, the consumer build.
GPU (-m gpu): the library, its general path and _argv byte for byte against the checker."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hannk_nn_checker as hk
from parity_helpers import DevTensor, gpu_present, launches, load_fuzz_parity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NN_OPS = ("average_pool_uint8", "max_pool_uint8", "mean_uint8", "add_uint8_uint8", "mul_uint8_uint8_uint8", "softmax_uint8", "l2_normalization_uint8")


# ------------------------------------------------------------------------------------------------------------------ the numpy evaluator
def i64(v):
    return np.asarray(v, np.int64)


def wr(v, bits):
    m = 1 << bits
    v = i64(v) & (m - 1)
    return np.where(v >= (m >> 1), v - m, v)


def wru(v, bits):
    return i64(v) & ((1 << bits) - 1)


def st(v, bits):
    return np.clip(i64(v), -(1 << (bits - 1)), (1 << (bits - 1)) - 1)


def stu(v, bits):
    return np.clip(i64(v), 0, (1 << bits) - 1)


def fdiv(a, b):
    a, b = np.broadcast_arrays(i64(a), i64(b))
    return np.where(b == 0, 0, np.floor_divide(a, np.where(b == 0, 1, b)))


def shl(a, c, bits):
    a, c = np.broadcast_arrays(i64(a), i64(c))
    left = np.where(c >= bits, 0, wr(a << np.clip(c, 0, bits - 1), bits))
    right = np.where(-c >= bits, np.where(a < 0, -1, 0), a >> np.clip(-c, 0, bits - 1))
    return np.where(c >= 0, left, right)


def rsr(a, s, bits):
    a, s = np.broadcast_arrays(i64(a), i64(s))
    sp = np.clip(s, 1, bits)
    pos = np.where(s > bits, 0, (a >> np.minimum(sp, 62)) + ((a >> (sp - 1)) & 1))
    return np.where(s > 0, pos, shl(a, -s, bits))


def m2h(a, b, bits):
    return st((i64(a) * i64(b) + (1 << (bits - 2))) >> (bits - 1), bits)


def clz32(x):
    y = wru(x, 32).copy()
    n = np.zeros(y.shape, np.int64)
    for s in (16, 8, 4, 2, 1):
        big = (y >> s) != 0
        y = np.where(big, y >> s, y)
        n += np.where(big, s, 0)
    return 32 - (n + (y != 0))


def np_approx_log2(q, x, q_x, tb):
    x = i64(x)
    fl = 31 - clz32(x)
    frac1 = wr(shl(x, 15 - fl, 32), 16) & 0x7fff
    frac2 = m2h(frac1, frac1, 16)
    frac3 = m2h(frac2, frac1, 16)
    poly = wr(m2h(2555, frac3, 16) + m2h(-9421, frac2, 16) + m2h(23249, frac1, 16) + 5, 16)
    frac_result = wr(rsr(poly, 14 - q, 16), tb) if q < 14 else shl(wr(poly, tb), q - 14, tb)
    floor_result = shl(wr(wr(fl - q_x, 16), tb), q, tb)
    return st(floor_result + frac_result, tb)


def np_approx_exp2(q, x, xb, q_x, tb):
    x = i64(x)
    floor_x = wr(x >> min(int(q_x), xb - 1) if q_x < xb else np.where(x < 0, -1, 0), tb)
    e = st(shl(1, wr(floor_x + q, tb), 32), tb)
    d = wr(x - (floor_x << int(q_x) if q_x < 32 else 0), 16)
    frac1 = shl(d, wr(15 - wr(q_x, 16), 16), 16)
    frac2 = m2h(frac1, frac1, 16)
    frac3 = m2h(frac2, frac1, 16)
    poly = wr(m2h(2592, frac3, 16) + m2h(7363, frac2, 16) + m2h(22812, frac1, 16), 16)
    poly = shl(poly, tb - 16, tb)
    return st(e + m2h(e, poly, tb), tb)


def np_approx_reciprocal(q, x, tb):
    return np_approx_exp2(q, wr(-np_approx_log2(15, x, 0, 32), 32), 32, 15, tb)


def np_approx_reciprocal_sqrt(q, x, tb):
    return np_approx_exp2(q, wr(-np_approx_log2(14, x, 0, 32), 32), 32, 15, tb)


def np_approx(fn, q, x, q_x, bits):
    if fn == "approx_log2":
        return np_approx_log2(q, x, q_x, bits)
    if fn == "approx_exp2":
        return np_approx_exp2(q, x, 32, q_x, bits)
    return (np_approx_reciprocal if fn == "approx_reciprocal" else np_approx_reciprocal_sqrt)(q, x, bits)


def np_clamp(v, lo, hi):
    return np.maximum(np.minimum(v, hi), lo)


def np_pool(kind, inp, out_extents, stride, filt, lo=0, hi=255, in_mins=(0, 0, 0, 0), out_mins=(0, 0, 0, 0)):
    inp = i64(inp)
    B, H, W, _ = inp.shape
    c_, ow, oh, ob = out_extents
    (sx, sy), (fw, fh) = stride, filt
    min_x, max_x, min_y, max_y = in_mins[1], in_mins[1] + W - 1, in_mins[2], in_mins[2] + H - 1
    xs, ys = (np.arange(ow) + out_mins[1]) * sx, (np.arange(oh) + out_mins[2]) * sy
    sub = inp[out_mins[3] - in_mins[3]:out_mins[3] - in_mins[3] + ob, :, :, out_mins[0] - in_mins[0]:out_mins[0] - in_mins[0] + c_]
    total, mx = np.zeros((ob, oh, ow, c_), np.int64), np.full((ob, oh, ow, c_), lo, np.int64)
    for ry in range(fh):
        for rx in range(fw):
            xx, yy = xs + rx, ys + ry
            valid = (((yy >= min_y) & (yy <= max_y))[:, None] & ((xx >= min_x) & (xx <= max_x))[None, :])[None, :, :, None]
            tap = sub[:, np.clip(yy - min_y, 0, H - 1)][:, :, np.clip(xx - min_x, 0, W - 1)]
            total = wru(total + np.where(valid, tap, 0), 16)
            mx = np.where(valid, np.maximum(mx, tap), mx)
    if kind == "max":
        return np.minimum(mx, hi).astype(np.uint8)
    count = wr((np.minimum(xs + fw, max_x + 1) - np.maximum(xs, min_x))[None, :] * (np.minimum(ys + fh, max_y + 1) - np.maximum(ys, min_y))[:, None], 32)
    inv = stu(fdiv(wr((2 << 16) + count, 32), wr(2 * count, 32)), 16)[None, :, :, None]
    return np_clamp(stu(stu((total * inv + (1 << 15)) >> 16, 16), 8), lo, hi).astype(np.uint8)


def np_mean(inp, out_extents, rmins, rextents, in_mins=(0, 0, 0, 0), out_mins=(0, 0, 0, 0)):
    inp = i64(inp)
    total = np.zeros(tuple(reversed(out_extents)), np.int64)
    if all(e > 0 for e in rextents):
        for r in np.ndindex(*rextents):
            lo = [out_mins[d] + rmins[d] + r[d] - in_mins[d] for d in range(4)]
            total = wru(total + inp[lo[3]:lo[3] + out_extents[3], lo[2]:lo[2] + out_extents[2], lo[1]:lo[1] + out_extents[1], lo[0]:lo[0] + out_extents[0]], 32)
    extent = 1
    for e in rextents:
        extent = int(wr(extent * e, 32))
    return wru(fdiv(wr(wr(total, 32) + fdiv(extent, 2), 32), extent), 8).astype(np.uint8)


def np_add(a, z1, m1, b, z2, m2, oz, lo, hi):
    i1, i2 = shl(wr(i64(a) - z1, 16), 6, 16), shl(wr(i64(b) - z2, 16), 6, 16)
    v = st(rsr(wr(wr(i1 * m1, 32) + wr(i2 * m2, 32), 32), 16, 32), 16)
    return np_clamp(stu(st(v + oz, 16), 8), lo, hi).astype(np.uint8)


def np_mul(a, z1, b, z2, oz, mult, shift, lo, hi):
    i1, i2 = shl(wr(i64(a) - z1, 16), 6, 16), shl(wr(i64(b) - z2, 16), 6, 16)
    v = st(rsr(m2h(wr(i1 * i2, 32), mult, 32), shift, 32), 16)
    return np_clamp(stu(st(v + oz, 16), 8), lo, hi).astype(np.uint8)


def np_softmax(inp, bm, bs, oz, om, osh):
    """(rows, n) -> (rows, n), the reduction over the whole row"""
    inp = i64(inp)
    diff = shl(wr(inp - inp.max(axis=1, keepdims=True), 16), 6, 16)
    e = np_approx_exp2(15, m2h(diff, bm, 16), 16, bs, 16)
    total = wr(e.sum(axis=1, keepdims=True), 32)
    inv = np_approx_reciprocal(30, total, 16)
    o = rsr(m2h(m2h(e, inv, 16), om, 16), osh, 16)
    return stu(st(o + oz, 16), 8).astype(np.uint8)


def np_l2(inp, zero):
    z = wr(i64(inp) - zero, 16)
    total = wr(wr(z * z, 32).sum(axis=1, keepdims=True), 32)
    inv = np_approx_reciprocal_sqrt(15, total, 32)
    o = st(rsr(wr(z * inv, 32), 8, 32), 16)
    return stu(st(o + 128, 16), 8).astype(np.uint8)


def rng(seed):
    return np.random.default_rng(seed)


def rand_u8(shape, seed):
    return rng(seed).integers(0, 256, shape, dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------------ CPU: second evaluator
APPROX_ARGS = np.concatenate([np.array([0, 1, 2, 3, -1, -2, 32767, 32768, 65535, 65536, (1 << 31) - 1, -(1 << 31), 1 << 30, 12345678], np.int64),
                              rng(1).integers(-(1 << 31), 1 << 31, 4000), rng(2).integers(-70000, 70000, 4000)]).astype(np.int32)


@pytest.mark.parametrize("bits", [16, 32])
def test_checker_approx_helpers_are_the_second_evaluator(bits):
    for q in (0, 1, 8, 13, 14, 15):
        for q_x in (0, 1, 15):
            got, want = hk.approx("approx_log2", q, APPROX_ARGS, q_x, bits), np_approx("approx_log2", q, APPROX_ARGS, q_x, bits)
            assert np.array_equal(got, want), ("approx_log2", q, q_x)
    for q in (0, 3, 15) + ((30,) if bits == 32 else ()):
        for q_x in (0, 1, 7, 14, 15):
            got, want = hk.approx("approx_exp2", q, APPROX_ARGS, q_x, bits), np_approx("approx_exp2", q, APPROX_ARGS, q_x, bits)
            assert np.array_equal(got, want), ("approx_exp2", q, q_x)
    for fn, q in (("approx_reciprocal", 30), ("approx_reciprocal", 15), ("approx_reciprocal_sqrt", 15)):
        assert np.array_equal(hk.approx(fn, q, APPROX_ARGS, 0, bits), np_approx(fn, q, APPROX_ARGS, 0, bits)), (fn, q)


POOL_CASES = {  # c, (W, H), batch, in x/y min, out x/y min and extent, stride, filter
    "edges_3x3_s2": (5, (13, 11), 2, (3, 2), (-1, -1), (11, 9), (2, 2), (3, 3)),
    "edges_2x2_s2": (4, (13, 11), 1, (3, 2), (0, 0), (9, 8), (2, 2), (2, 2)),
    "global_7x7": (9, (7, 7), 2, (0, 0), (0, 0), (1, 1), (1, 1), (7, 7)),
    "wide_17x17": (3, (20, 19), 1, (0, 0), (-1, 0), (4, 3), (1, 1), (17, 17)),
}


def pool_case(name, seed=0, fill=None):
    c, (w, h), b, (ix, iy), (ox, oy), (ow, oh), stride, filt = POOL_CASES[name]
    inp = rand_u8((b, h, w, c), seed) if fill is None else np.full((b, h, w, c), fill, np.uint8)
    return dict(inp=inp, out_extents=(c, ow, oh, b), stride=stride, filt=filt, in_mins=(0, ix, iy, 0), out_mins=(0, ox, oy, 0))


@pytest.mark.parametrize("name", sorted(POOL_CASES))
@pytest.mark.parametrize("kind", ["average", "max"])
def test_checker_pools_are_the_second_evaluator(name, kind):
    for lo, hi in ((0, 255), (40, 200), (200, 40)):
        k = pool_case(name)
        assert np.array_equal(hk.pool(kind, lo=lo, hi=hi, **k), np_pool(kind, lo=lo, hi=hi, **k)), (lo, hi)


MEAN_CASES = {  # input (B, H, W, C), in_mins, out_mins, out_extents, rmins, rextents (Halide order)
    "xy": ((2, 7, 7, 6), (0, 0, 0, 0), (0, 0, 0, 0), (6, 1, 1, 2), (0, 0, 0, 0), (1, 7, 7, 1)),
    "c": ((1, 2, 3, 67), (0, 0, 0, 0), (0, 0, 0, 0), (1, 3, 2, 1), (0, 0, 0, 0), (67, 1, 1, 1)),
    "all": ((2, 2, 3, 5), (0, 0, 0, 0), (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0), (5, 3, 2, 2)),
    "mins": ((3, 6, 7, 9), (2, -1, 3, 1), (1, 0, 0, 0), (4, 3, 2, 2), (2, 0, 4, 1), (2, 3, 2, 2)),
    "stencil": ((1, 6, 9, 4), (0, 0, 0, 0), (0, 0, 0, 0), (4, 7, 5, 1), (0, 0, 0, 0), (1, 3, 2, 1)),
}


@pytest.mark.parametrize("name", sorted(MEAN_CASES))
def test_checker_mean_is_the_second_evaluator_and_the_exact_rounded_mean(name):
    shape, imin, omin, oext, rmin, rext = MEAN_CASES[name]
    inp = rand_u8(shape, 3)
    got = hk.mean(inp, oext, rmin, rext, imin, omin)
    assert np.array_equal(got, np_mean(inp, oext, rmin, rext, imin, omin))
    # (sum + n / 2) / n exactly, by a plain loop over the outputs
    n = int(np.prod(rext))
    for at in np.ndindex(*got.shape):
        o = [omin[d] + at[3 - d] for d in range(4)]
        lo = [o[d] + rmin[d] - imin[d] for d in range(4)]
        s = int(inp[lo[3]:lo[3] + rext[3], lo[2]:lo[2] + rext[2], lo[1]:lo[1] + rext[1], lo[0]:lo[0] + rext[0]].astype(np.int64).sum())
        assert got[at] == (s + n // 2) // n, at


def test_checker_mean_degenerate_regions():
    inp = rand_u8((1, 2, 2, 3), 4)
    for rext in ((1, 0, 1, 1), (1, -1, -1, 1), (1, -2, 1, 1)):   # no taps: the sum is 0; extent 0 divides to 0, a negative one floors
        got = hk.mean(inp, (3, 1, 1, 1), (0, 0, 0, 0), rext)
        assert np.array_equal(got, np_mean(inp, (3, 1, 1, 1), (0, 0, 0, 0), rext)), rext
    assert (hk.mean(inp, (3, 1, 1, 1), (0, 0, 0, 0), (1, 0, 1, 1)) == 0).all()
    assert (hk.mean(inp, (3, 1, 1, 1), (0, 0, 0, 0), (1, -2, 1, 1)) == 0).all()        # (0 + -1) / -2 floors to 0
    assert (hk.mean(inp, (3, 1, 1, 1), (0, 0, 0, 0), (1, -1, 1, 1)) == 1).all()        # (0 + -1) / -1 == 1


EW_ZEROS = (0, 128, 255)


def test_checker_add_mul_are_the_second_evaluator():
    a, b = rand_u8((3, 37), 5), rand_u8((3, 37), 6)
    for z1 in EW_ZEROS:
        for z2 in EW_ZEROS:
            for m1, m2 in ((16384, 16384), (32767, -32768), (-32768, 32767), (1, 0)):
                for oz, lo, hi in ((0, 0, 255), (128, 10, 240), (255, 200, 100)):
                    assert np.array_equal(hk.add(a, z1, m1, b, z2, m2, oz, lo, hi, (37, 3)), np_add(a, z1, m1, b, z2, m2, oz, lo, hi))
            for mult, shift in ((1 << 30, 0), ((1 << 31) - 1, 31), (-(1 << 31), 5), (1518500250, 12), (123456789, 1)):
                for oz, lo, hi in ((0, 0, 255), (128, 10, 240)):
                    assert np.array_equal(hk.mul(a, z1, b, z2, oz, mult, shift, lo, hi, (37, 3)), np_mul(a, z1, b, z2, oz, mult, shift, lo, hi))
    row = np.broadcast_to(rand_u8((3, 1), 7), (3, 37))   # a stride of 0
    assert np.array_equal(hk.add(a, 3, 20000, row, 9, 12000, 7, 0, 255, (37, 3)), np_add(a, 3, 20000, row, 9, 12000, 7, 0, 255))


SOFTMAX_BETA_SCALES = (1 / 64, 1 / 16, 1 / 4)
SOFTMAX_LENGTHS = (1, 2, 5, 10, 64, 65, 1000, 1001)
L2_LENGTHS = (1, 2, 3, 16, 64, 65, 1000, 4097)


def softmax_params(hl, beta_in_scale, out_scale=1 / 256):
    return hl.hannk_softmax_params(beta_in_scale, 1.0, out_scale)


def py_softmax_params(r, out_scale=1 / 256):
    """SoftmaxOp::execute's parameters without the product: IntFloat<int16_t>(log2(e) r) * 2^-6 and IntFloat<int16_t>(out_scale) * 2"""
    import math

    def int_float(x, power):
        m, e = math.frexp(float(np.float32(x)))
        ml = int(math.floor(abs(m) * 32768 + 0.5)) * (1 if m >= 0 else -1)
        if ml == 32768:
            ml, e = ml >> 1, e + 1
        e += power
        return (0 if e < -15 else ml), -max(-15, min(15, e))

    bm, bs = int_float(np.float32(r) * np.float32(np.log2(np.exp(np.float32(1.0)))), -6)
    om, osh = int_float(out_scale, 1)
    return bm, bs, om, osh


def row_contents(kind, n, seed, zero=None):
    r = rng(seed)
    if kind == "uniform":
        return r.integers(0, 256, n, dtype=np.uint8)
    if kind == "band":
        lo = 100 if zero is None else max(0, min(251, zero - 2))
        return r.integers(lo, lo + 5 if zero is not None else 140, n, dtype=np.uint8)
    if kind == "constant":
        return np.full(n, r.integers(0, 256) if zero is None else zero, np.uint8)
    row = r.integers(0, 60, n, dtype=np.uint8)
    row[r.integers(0, n)] = 255
    return row


ROW_KINDS = ("uniform", "band", "constant", "spike")


def test_checker_softmax_l2_are_the_second_evaluator():
    for n in (1, 2, 5, 64, 65, 1001):
        inp = np.stack([row_contents(k, n, 10 + j) for j, k in enumerate(ROW_KINDS)])
        for r in SOFTMAX_BETA_SCALES:
            bm, bs, om, osh = py_softmax_params(r)
            for oz in (0, 3):
                assert np.array_equal(hk.softmax(inp, bm, bs, oz, om, osh), np_softmax(inp, bm, bs, oz, om, osh)), (n, r)
        for bm, bs, om, osh in ((32767, 0, 32767, 0), (-32768, 15, -32768, 15), (1, 7, 16384, 3)):   # the ends of the defined ranges
            assert np.array_equal(hk.softmax(inp, bm, bs, 0, om, osh), np_softmax(inp, bm, bs, 0, om, osh)), (n, bm)
        for zero in (0, 17, 128, 255):
            assert np.array_equal(hk.l2_normalization(inp, zero), np_l2(inp, zero)), (n, zero)


# ------------------------------------------------------------------------------------------------------------------ CPU: the reference's acceptance
def relative_error(x, y):
    with np.errstate(invalid="ignore"):   # an exact result of inf is outside every type: not checked
        return np.abs(x - y) / np.maximum(np.maximum(np.abs(x), np.abs(y)), 1e-6)


PRECISIONS = (0, 1, 2, 3, 8, 15)


@pytest.mark.parametrize("bits", [16, 32])
def test_approx_log2_passes_the_references_own_test(bits):
    """common_halide_test.cpp: test_approx_log2<T>, the whole grid: relative 1e-3 or absolute 2 wherever the exact result fits T"""
    extent = 50000
    scale = (2 ** 31 - 1) // extent
    x = (np.arange(extent, dtype=np.int64) + 1) * scale
    tmin, tmax = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    checked = 0
    for q in PRECISIONS:
        got = hk.approx("approx_log2", q, x.astype(np.int32), 0, bits).astype(np.float64)
        exact = np.round(np.log2(x.astype(np.float64)) * (1 << q))
        fits = (exact >= tmin) & (exact <= tmax)
        bad = fits & (relative_error(exact, got) > 1e-3) & (np.abs(exact - got) > 2)
        assert not bad.any(), (q, int(x[bad][0]), exact[bad][0], got[bad][0])
        checked += int(fits.sum())
    assert checked > 0


@pytest.mark.parametrize("bits", [16, 32])
def test_approx_exp2_passes_the_references_own_test(bits):
    """common_halide_test.cpp: test_approx_exp2<T>, the whole grid (50000 x 15 x 6): relative 1e-3 or absolute 1"""
    extent, offset = 50000, 25000
    tmin, tmax = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    scale = tmax // offset
    x = (np.arange(extent, dtype=np.int64) - offset) * scale   # an i32 expression in the reference's test: it wraps
    x = wr(x, 32)
    checked = 0
    for q in PRECISIONS:
        for y in range(15):
            got = hk.approx("approx_exp2", q, x.astype(np.int32), y, bits).astype(np.float64)
            with np.errstate(over="ignore"):
                exact = np.round(np.exp2(((np.arange(extent, dtype=np.int64) - offset) * scale).astype(np.float64) / (1 << y)) * (1 << q))
            fits = (exact >= tmin) & (exact <= tmax)
            bad = fits & (relative_error(exact, got) > 1e-3) & (np.abs(exact - got) > 1.0)
            assert not bad.any(), (q, y, int(x[bad][0]), exact[bad][0], got[bad][0])
            checked += int(fits.sum())
    assert checked > 0


# ------------------------------------------------------------------------------------------------------------------ CPU: closeness to float64
@pytest.mark.parametrize("r", SOFTMAX_BETA_SCALES, ids=["1/64", "1/16", "1/4"])
def test_softmax_is_within_one_of_float64(r):
    bm, bs, om, osh = py_softmax_params(r)
    worst = 0
    for n in SOFTMAX_LENGTHS:
        for j, kind in enumerate(ROW_KINDS):
            row = row_contents(kind, n, 100 * n + j)
            got = hk.softmax(row[None, :], bm, bs, 0, om, osh)[0].astype(np.int64)
            x = (row.astype(np.float64) - row.max()) * r * np.log2(np.e)
            p = np.exp2(x)
            want = np.clip(np.round(256 * p / p.sum()), 0, 255)
            worst = max(worst, int(np.abs(got - want).max()))
            assert np.abs(got - want).max() <= 1, (n, kind, int(np.abs(got - want).max()))
    print("softmax worst difference", worst)


def test_l2_normalization_is_within_one_of_float64():
    worst = 0
    for n in L2_LENGTHS:
        for j, (kind, zero) in enumerate((("uniform", 0), ("uniform", 128), ("uniform", 255), ("uniform", 17), ("constant", 128), ("band", 128), ("spike", 30))):
            row = row_contents(kind, n, 200 * n + j, zero if kind in ("constant", "band") else None)
            got = hk.l2_normalization(row[None, :], zero)[0].astype(np.int64)
            d = row.astype(np.float64) - zero
            norm = np.sqrt((d * d).sum())
            want = np.clip(np.round(128 * d / norm) + 128, 0, 255) if norm > 0 else np.full(n, 128.0)
            worst = max(worst, int(np.abs(got - want).max()))
            assert np.abs(got - want).max() <= 1, (n, kind, zero, int(np.abs(got - want).max()))
    print("l2_normalization worst difference", worst)


def test_average_pool_is_within_one_of_the_rounded_average():
    for name in ("edges_3x3_s2", "edges_2x2_s2", "global_7x7"):
        k = pool_case(name, seed=8)
        got = hk.pool("average", **k).astype(np.int64)
        # the exact sum and count of the taps inside the input, by a plain loop over the outputs
        c, ow, oh, ob = k["out_extents"]
        inp = k["inp"].astype(np.int64)
        for b in range(ob):
            for y in range(oh):
                for x in range(ow):
                    x0, y0 = (x + k["out_mins"][1]) * k["stride"][0] - k["in_mins"][1], (y + k["out_mins"][2]) * k["stride"][1] - k["in_mins"][2]
                    win = inp[b, max(y0, 0):max(y0 + k["filt"][1], 0), max(x0, 0):max(x0 + k["filt"][0], 0)]
                    n = win.shape[0] * win.shape[1]
                    want = np.floor(win.reshape(n, c).sum(axis=0) / n + 0.5) if n else np.zeros(c)
                    assert np.abs(got[b, y, x] - want).max() <= 1, (name, b, y, x)


# ------------------------------------------------------------------------------------------------------------------ CPU: known answers
def test_pool_windows_half_and_wholly_outside():
    inp = np.full((1, 4, 4, 2), 100, np.uint8)
    inp[0, 0, 0] = (10, 250)
    # output x = -1: taps x in {-2, -1} wholly outside; x = 0 ... ; 2 x 2 windows, stride 2, input x in [1, 4], y in [0, 3]
    k = dict(inp=inp, out_extents=(2, 3, 1, 1), stride=(2, 2), filt=(2, 2), in_mins=(0, 1, 0, 0), out_mins=(0, -1, 0, 0))
    avg, mx = hk.pool("average", **k), hk.pool("max", **k)
    assert avg[0, 0, 0].tolist() == [0, 0] and mx[0, 0, 0].tolist() == [0, 0]                 # wholly outside: the mean of nothing is 0
    assert avg[0, 0, 1].tolist() == [55, 175] and mx[0, 0, 1].tolist() == [100, 250]         # half outside: taps x = 1 only, two rows
    assert avg[0, 0, 2].tolist() == [100, 100]
    assert hk.pool("average", lo=7, hi=200, **k)[0, 0, 0].tolist() == [7, 7] and hk.pool("max", lo=7, hi=200, **k)[0, 0, 0].tolist() == [7, 7]
    # an empty window under crossed bounds: max gives min(output_min, output_max), average clamps 0 with output_min winning
    assert hk.pool("max", lo=200, hi=40, **k)[0, 0, 0].tolist() == [40, 40] and hk.pool("average", lo=200, hi=40, **k)[0, 0, 0].tolist() == [200, 200]
    assert hk.pool("max", lo=200, hi=40, **k)[0, 0, 2].tolist() == [40, 40] and hk.pool("average", lo=200, hi=40, **k)[0, 0, 2].tolist() == [200, 200]


def test_average_pool_u16_sum_wraps():
    """17 x 17 taps of 255: 73695 mod 2^16 = 8159; inv = (2^17 + 289) / 578 = 227; (8159 * 227 + 2^15) >> 16 = 28"""
    inp = np.full((1, 17, 17, 1), 255, np.uint8)
    got = hk.pool("average", inp, (1, 1, 1, 1), (1, 1), (17, 17))
    assert got.item() == 28 and (17 * 17 * 255) % 65536 == 8159 and (131072 + 289) // 578 == 227 and (8159 * 227 + 32768) >> 16 == 28


def test_l2_row_of_zero_points_is_128():
    """approx_log2(14, 0): clz = 32, floor_log2 = -1; the product with the zeroed input is 0 whatever the reciprocal"""
    assert (hk.l2_normalization(np.full((1, 9), 77, np.uint8), 77) == 128).all()
    assert hk.approx("approx_log2", 14, [0], 0, 32)[0] == np_approx_log2(14, [0], 0, 32)[0] == -(1 << 14) + 5


def test_softmax_row_of_one_and_of_equal_elements(hl):
    bm, bs, om, osh = py_softmax_params(1 / 16)
    one = hk.softmax(np.array([[200]], np.uint8), bm, bs, 0, om, osh).item()
    assert one == 255                                                         # round(256 * 1) saturates
    four = hk.softmax(np.full((1, 4), 9, np.uint8), bm, bs, 0, om, osh)[0]
    assert abs(int(four[0]) - 64) <= 1 and (four == four[0]).all()
    assert softmax_params(hl, 1 / 16) == py_softmax_params(1 / 16) == (23637, 9, 16384, 6)


def test_add_at_the_ends_of_its_multipliers():
    a = np.array([[0, 255, 0, 255]], np.uint8)
    b = np.array([[0, 0, 255, 255]], np.uint8)
    # (0 - 255) << 6 = -16320; * 32767 = -534757440; twice = -1069514880 (no i32 wrap); >> 16 rounds to -16320 -> + 0 -> u8_sat 0
    assert hk.add(a, 255, 32767, b, 255, 32767, 0, 0, 255, (4, 1))[0].tolist() == [0, 0, 0, 0]
    # 255 << 6 = 16320; * 32767 * 2 = 1069514880; >> 16 = 16320 -> 255
    assert hk.add(a, 0, 32767, b, 0, 32767, 0, 0, 255, (4, 1))[0].tolist() == [0, 255, 255, 255]
    assert hk.add(a, 0, 32767, b, 0, -32767, 128, 0, 255, (4, 1))[0].tolist() == [128, 255, 0, 128]
    assert hk.add(a, 0, 32767, b, 0, -32767, 128, 100, 140, (4, 1))[0].tolist() == [128, 140, 100, 128]


def test_mul_at_shifts_0_and_31():
    a = np.array([[0, 255, 128, 255]], np.uint8)
    b = np.array([[255, 255, 128, 1]], np.uint8)
    # shift 31 of anything below 2^30 in magnitude rounds to 0
    assert hk.mul(a, 0, b, 0, 5, (1 << 31) - 1, 31, 0, 255, (4, 1))[0].tolist() == [5, 5, 5, 5]
    # shift 0: (255 << 6)^2 = 266342400, multiply_2x_high with 2^30 halves it; i16_sat; + 0; u8_sat
    assert hk.mul(a, 0, b, 0, 0, 1 << 30, 0, 0, 255, (4, 1))[0].tolist() == [0, 255, 255, 255]
    # 1 / 2^12 of the product of the zeroed inputs: multiplier 2^30 is 1/2, shift 11
    assert hk.mul(a, 0, b, 0, 0, 1 << 30, 11, 0, 255, (4, 1))[0].tolist() == [0, 255, 255, 255]
    assert hk.mul(a, 0, b, 0, 0, 1 << 30, 19, 0, 255, (4, 1))[0].tolist() == [0, 254, 64, 1]


# ------------------------------------------------------------------------------------------------------------------ CPU: the entry protocol
def code_of(hl, fn):
    try:
        fn()
    except hl.HalideError as e:
        return e.code
    return 0


def set_dim(buf, d, **fields):
    for k, v in fields.items():
        setattr(buf._dims[d], k, v)


def ok_codes():
    return (0,) if gpu_present() else (-29,)


class PoolArgs:
    def __init__(self, hl, kind="average"):
        self.hl, self.kind = hl, kind
        self.input = hl.Buffer(np.zeros((2, 6, 7, 5), np.uint8))
        self.output = hl.Buffer(np.zeros((2, 3, 4, 5), np.uint8))

    def call(self):
        fn = self.hl.average_pool_uint8 if self.kind == "average" else self.hl.max_pool_uint8
        return code_of(self.hl, lambda: fn(self.input, (2, 2), (3, 3), 0, 255, self.output))


class MeanArgs:
    def __init__(self, hl):
        self.hl = hl
        self.input = hl.Buffer(np.zeros((2, 6, 7, 5), np.uint8))
        self.output = hl.Buffer(np.zeros((2, 1, 1, 5), np.uint8))
        self.mins, self.extents = [0, 0, 0, 0], [1, 7, 6, 1]

    def call(self):
        return code_of(self.hl, lambda: self.hl.mean_uint8(self.input, self.mins, self.extents, self.output))


class EwArgs:
    def __init__(self, hl, op="add"):
        self.hl, self.op = hl, op
        self.input1, self.input2 = hl.Buffer(np.zeros((3, 20), np.uint8)), hl.Buffer(np.zeros((3, 20), np.uint8))
        self.output = hl.Buffer(np.zeros((3, 20), np.uint8))

    def call(self):
        if self.op == "add":
            return code_of(self.hl, lambda: self.hl.add_uint8_uint8(self.input1, 0, 16384, self.input2, 0, 16384, 0, 0, 255, self.output))
        return code_of(self.hl, lambda: self.hl.mul_uint8_uint8_uint8(self.input1, 0, self.input2, 0, 0, 1 << 30, 11, 0, 255, self.output))


class RowArgs:
    def __init__(self, hl, op="softmax"):
        self.hl, self.op = hl, op
        self.input, self.output = hl.Buffer(np.zeros((3, 20), np.uint8)), hl.Buffer(np.zeros((3, 20), np.uint8))

    def call(self):
        if self.op == "softmax":
            return code_of(self.hl, lambda: self.hl.softmax_uint8(self.input, 23637, 9, 0, 16384, 6, self.output))
        return code_of(self.hl, lambda: self.hl.l2_normalization_uint8(self.input, 128, self.output))


ALL_ARGS = [(PoolArgs, "average"), (PoolArgs, "max"), (MeanArgs, None), (EwArgs, "add"), (EwArgs, "mul"), (RowArgs, "softmax"), (RowArgs, "l2")]


def make(hl, cls, op):
    return cls(hl) if op is None else cls(hl, op)


def buffers_of(a):
    return [n for n in ("input", "input1", "input2", "output") if hasattr(a, n)]


@pytest.mark.parametrize("cls,op", ALL_ARGS)
def test_protocol_valid_null_type_dimensions(hl, cls, op):
    assert make(hl, cls, op).call() in ok_codes()
    for which in buffers_of(make(hl, cls, op)):
        a = make(hl, cls, op)
        setattr(a, which, None)
        assert a.call() == -12, which
        a = make(hl, cls, op)
        setattr(a, which, hl.Buffer(np.zeros(getattr(a, which).array.shape, np.int8)))
        assert a.call() == -3, which
        a = make(hl, cls, op)
        setattr(a, which, hl.Buffer(np.zeros(getattr(a, which).array.shape + (1,), np.uint8)))
        assert a.call() == -43, which


@pytest.mark.parametrize("kind", ["average", "max"])
def test_protocol_pool_constraints(hl, kind):
    for d in (0, 3):
        for field, value in (("min", 1), ("extent", 1)):
            a = PoolArgs(hl, kind)
            set_dim(a.output, d, **{field: value})
            assert a.call() == -8, (d, field)
    for which in ("input", "output"):
        a = PoolArgs(hl, kind)
        set_dim(getattr(a, which), 0, stride=2)
        assert a.call() == -8, which
    a = PoolArgs(hl, kind)   # x and y are clamped: no region of either can be out of bounds
    a.input.set_min(0, 100, -50, 0)
    assert a.call() in ok_codes()


def test_protocol_mean_required_region(hl):
    a = MeanArgs(hl)
    a.extents = [1, 8, 6, 1]
    assert a.call() == -4
    a = MeanArgs(hl)
    a.mins = [0, -1, 0, 0]
    assert a.call() == -4
    a = MeanArgs(hl)
    a.mins = [1, 0, 0, 0]          # c + 1 runs past the input's channels
    assert a.call() == -4
    a = MeanArgs(hl)
    a.output = hl.Buffer(np.zeros((2, 1, 1, 4), np.uint8))
    a.mins = [1, 0, 0, 0]
    assert a.call() in ok_codes()
    a = MeanArgs(hl)
    set_dim(a.input, 0, stride=2)
    assert a.call() == -8


@pytest.mark.parametrize("op", ["add", "mul"])
def test_protocol_add_mul_strides_and_regions(hl, op):
    for s1, s2, want in ((1, 1, ok_codes()), (1, 0, ok_codes()), (0, 1, ok_codes()), (0, 0, (-31,) if gpu_present() else (-29,)),
                         (2, 1, (-31,) if gpu_present() else (-29,))):
        a = EwArgs(hl, op)
        if s1 != 1:
            a.input1 = hl.Buffer(np.zeros((3, 40), np.uint8))
            set_dim(a.input1, 0, stride=s1, extent=20)
        if s2 != 1:
            set_dim(a.input2, 0, stride=s2)
        assert a.call() in want, (s1, s2)
    a = EwArgs(hl, op)
    set_dim(a.output, 0, stride=2)
    assert a.call() == -8
    for which in ("input1", "input2"):
        a = EwArgs(hl, op)
        setattr(a, which, hl.Buffer(np.zeros((3, 19), np.uint8)))
        assert a.call() == -4, which
        a = EwArgs(hl, op)
        getattr(a, which).set_min(0, 1)
        assert a.call() == -4, which


@pytest.mark.parametrize("op", ["softmax", "l2"])
def test_protocol_rows_strides_and_regions(hl, op):
    a = RowArgs(hl, op)          # transposed, as ops.cpp passes another axis: any stride of dimension 0 is accepted
    a.input, a.output = hl.Buffer(np.zeros((20, 3), np.uint8).T), hl.Buffer(np.zeros((20, 3), np.uint8).T)
    assert a.call() in ok_codes()
    a = RowArgs(hl, op)
    a.input = hl.Buffer(np.zeros((3, 19), np.uint8))
    assert a.call() == -4
    a = RowArgs(hl, op)
    a.input = hl.Buffer(np.zeros((2, 20), np.uint8))
    assert a.call() == -4
    a = RowArgs(hl, op)          # the input may be larger than the output: the reduction runs over the input's own dimension 0
    a.input = hl.Buffer(np.zeros((4, 25), np.uint8), mins=(-2, -1))
    assert a.call() in ok_codes()


@pytest.mark.parametrize("cls,op", [(EwArgs, "add"), (EwArgs, "mul"), (RowArgs, "softmax"), (RowArgs, "l2")])
def test_protocol_no_bounds_query_ops_take_an_unallocated_buffer_for_an_error(hl, cls, op):
    """built with no_bounds_query: the checks run on the unallocated buffer and the host pointer check ends the call (-34) with its shape
    untouched; a shape that fails a check fails that check"""
    for which in buffers_of(make(hl, cls, op)):
        a = make(hl, cls, op)
        setattr(a, which, hl.Buffer.bounds_query(np.uint8, 2, extents=(20, 3)))
        assert a.call() == -34, which
        assert getattr(a, which).extents == [20, 3]
    a = make(hl, cls, op)
    a.output = hl.Buffer.bounds_query(np.uint8, 2, extents=(21, 3))
    assert a.call() == -4
    a = make(hl, cls, op)
    a.output = hl.Buffer.bounds_query(np.int16, 2, extents=(20, 3))
    assert a.call() == -3 and a.output.raw.type.bits == 16


@pytest.mark.parametrize("kind", ["average", "max"])
def test_pool_bounds_queries(hl, kind):
    a = PoolArgs(hl, kind)
    a.input = hl.Buffer(np.zeros((2, 6, 7, 5), np.uint8), mins=(3, 0, 0, 1))
    a.output = hl.Buffer.bounds_query(np.uint8, 4, mins=(0, -1, 2, 0), extents=(0, 4, 3, 0))
    assert a.call() == 0
    assert a.output.mins == [3, -1, 2, 1] and a.output.extents == [5, 4, 3, 2] and a.output.dim(0).stride == 1
    a = PoolArgs(hl, kind)
    a.output = hl.Buffer(np.zeros((2, 3, 4, 5), np.uint8), mins=(3, 0, 0, 1))
    a.input = hl.Buffer.bounds_query(np.uint8, 4, mins=(0, 9, 8, 0), extents=(1, 7, 6, 1))
    assert a.call() == 0
    assert a.input.mins == [3, 9, 8, 1] and a.input.extents == [5, 7, 6, 2]


def test_mean_bounds_query(hl):
    a = MeanArgs(hl)
    a.output = hl.Buffer(np.zeros((2, 3, 4, 5), np.uint8), mins=(1, 0, -2, 0))
    a.input = hl.Buffer.bounds_query(np.uint8, 4)
    a.mins, a.extents = [2, 0, 1, 0], [3, 7, 1, 1]
    assert a.call() == 0
    assert a.input.mins == [3, 0, -1, 0] and a.input.extents == [5 + 3 - 1, 4 + 7 - 1, 3, 2]


def test_metadata_and_symbols(hl):
    u8, i16, u16, i32, u32 = (1, 8), (0, 16), (1, 16), (0, 32), (1, 32)
    pool = (["input", "stride_x", "stride_y", "filter_width", "filter_height", "output_min", "output_max", "output"], [u8, i32, i32, i32, i32, u8, u8, u8], 4)
    expect = {
        "average_pool_uint8": pool,
        "max_pool_uint8": pool,
        "mean_uint8": (["input", "c_min", "c_extent", "x_min", "x_extent", "y_min", "y_extent", "b_min", "b_extent", "output"], [u8] + [i32] * 8 + [u8], 4),
        "add_uint8_uint8": (["input1", "input1_zero", "input1_multiplier", "input2", "input2_zero", "input2_multiplier", "output_zero", "output_min", "output_max",
                             "output"], [u8, u8, i16, u8, u8, i16, u8, u8, u8, u8], 2),
        "mul_uint8_uint8_uint8": (["input1", "input1_zero", "input2", "input2_zero", "output_zero", "output_multiplier", "output_shift", "output_min", "output_max",
                                   "output"], [u8, u8, u8, u8, u8, i32, u32, u8, u8, u8], 2),
        "softmax_uint8": (["input", "beta_multiplier", "beta_shift", "output_zero", "output_multiplier", "output_shift", "output"], [u8, i16, u16, u8, i16, u16, u8], 2),
        "l2_normalization_uint8": (["input", "input_zero", "output"], [u8, u8, u8], 2),
    }
    assert tuple(expect) == hl.HANNK_NN_OPS == NN_OPS
    assert hl.HANNK_OPS == ("tile_conv_filter_uint8", "conv_u8_u8_u8", "conv_u8_u8_i16", "depthwise_conv_uint8", "depthwise_conv_broadcast_uint8")
    for name, (names, types, rank) in expect.items():
        md = hl.metadata(name)
        args = [md.arguments[k] for k in range(md.num_arguments)]
        assert md.version == 1 and md.name.decode() == name and b"hip" in md.target
        assert [a.name.decode() for a in args] == names
        assert [a.kind for a in args] == [1 if n.startswith("input") and not ("_" in n) else 2 if n == "output" else 0 for n in names]
        assert [(a.type.code, a.type.bits) for a in args] == types and all(a.type.reserved == 1 for a in args)
        assert [a.dimensions for a in args] == [rank if a.kind else 0 for a in args]


def test_mangled_symbols_are_what_the_compiler_makes_of_the_headers(tmp_path):
    """every header is compiled with the host compiler into an object that refers to its three functions; the undefined symbols nm reads
    from it are the ones the library exports"""
    exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "halide_amd", "lib", "libhlmi.so")], capture_output=True, text=True,
                              check=True).stdout.split()
    seen = 0
    for name in NN_OPS:
        src = tmp_path / f"{name}.cpp"
        src.write_text(f'#include "halide/{name}.h"\nvoid *use_{name}[] = {{(void *)&hannk::{name}, (void *)&hannk::{name}_argv, (void *)&hannk::{name}_metadata}};\n')
        obj = tmp_path / f"{name}.o"
        subprocess.run(["g++", "-std=c++17", "-c", "-I", os.path.join(ROOT, "include", "aot"), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(obj)], check=True)
        wanted = [s for s in subprocess.run(["nm", "-u", str(obj)], capture_output=True, text=True, check=True).stdout.split() if s.startswith("_ZN5hannk")]
        assert len(wanted) == 3, (name, wanted)
        for s in wanted:
            assert s in exported, s
            seen += 1
    assert seen == 21


def test_python_symbols_are_the_exported_ones(hl):
    for name in NN_OPS:
        for suffix in ("", "_argv", "_metadata"):
            assert getattr(hl.lib, hl._symbol(name, suffix), None) is not None, (name, suffix)


def _build_consumer():
    import tempfile
    out = os.path.join(tempfile.mkdtemp(prefix="hlmi_hannk_nn_consumer"), "hannk_nn_consumer")
    libdir = os.path.join(ROOT, "halide_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include", "aot"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "hannk_nn_consumer.cpp"), "-o", out, "-L", libdir, "-lhlmi", f"-Wl,-rpath,{libdir}"], check=True)
    return out


def test_consumer_builds_against_the_headers():
    assert os.path.exists(_build_consumer())


# ------------------------------------------------------------------------------------------------------------------ GPU
gpu = pytest.mark.gpu
SWITCHES = ("HLMI_HANNK_POOL_VECTOR", "HLMI_HANNK_POOL_SPLIT", "HLMI_HANNK_MEAN_SPLIT", "HLMI_HANNK_EW_VECTOR", "HLMI_HANNK_ROWS_WAVE", "HLMI_HANNK_ROWS_KEEP")


@pytest.fixture
def switches(monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)

    def set_(**kw):
        for s in SWITCHES:
            monkeypatch.delenv(s, raising=False)
        for k, v in kw.items():
            monkeypatch.setenv("HLMI_HANNK_" + k, str(v))
    return set_


def call_argv(hl, name, args):
    md = hl.metadata(name)
    keep, argv = [], (C.c_void_p * len(args))()
    ctypes_of = {(0, 32): C.c_int32, (1, 8): C.c_uint8, (0, 16): C.c_int16, (1, 16): C.c_uint16, (1, 32): C.c_uint32}
    for j, v in enumerate(args):
        a = md.arguments[j]
        box = v.raw if a.kind else ctypes_of[(a.type.code, a.type.bits)](v)
        keep.append(box)
        argv[j] = C.cast(C.pointer(box), C.c_void_p)
    fn = getattr(hl.lib, hl._symbol(name, "_argv"))
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(C.c_void_p)]
    return hl._check(fn(argv))


def run_paths(hl, name, make_args, want, what="", paths=("direct", "general", "argv")):
    """make_args() -> (args in C order with fresh Buffers, read): every path must give `want`, every byte of it"""
    for path in paths:
        args, read = make_args()
        if path == "direct":
            hl._check(hl._fn[name](*[a.ptr if isinstance(a, hl.Buffer) else a for a in args]))
        elif path == "general":
            hl.debug_hannk_general(name, *args)
        else:
            call_argv(hl, name, args)
        got = read()
        assert got.shape == want.shape and got.dtype == want.dtype, (what, path)
        bad = got != want
        assert not bad.any(), f"{name} {what} {path}: {np.count_nonzero(bad)} of {got.size} differ, first at {tuple(np.argwhere(bad)[0])}"


def pool_args(inb, k, lo, hi, out):
    return [inb, k["stride"][0], k["stride"][1], k["filt"][0], k["filt"][1], lo, hi, out]


GPU_POOL_FILTERS = {"3x3s2": ((2, 2), (3, 3)), "2x2s2": ((2, 2), (2, 2))}


@gpu
@pytest.mark.parametrize("c", [3, 4, 68])
@pytest.mark.parametrize("filt", sorted(GPU_POOL_FILTERS))
@pytest.mark.parametrize("kind", ["average", "max"])
def test_hip_pools_are_the_checker(hl, switches, kind, filt, c):
    """a 13 x 11 input at x in [3, 15], y in [2, 12]; the output's windows cross every edge and leave the input wholly on three sides"""
    stride, f = GPU_POOL_FILTERS[filt]
    inp = rand_u8((2, 11, 13, c), c)
    k = dict(inp=inp, out_extents=(c, 11, 9, 2), stride=stride, filt=f, in_mins=(0, 3, 2, 0), out_mins=(0, -1, -1, 0))
    for lo, hi in ((0, 255), (60, 190)):
        want = hk.pool(kind, lo=lo, hi=hi, **k)

        def make_args():
            out = hl.Buffer(np.full(want.shape, 0x5A, np.uint8), mins=k["out_mins"])
            return pool_args(hl.Buffer(inp.copy(), mins=k["in_mins"]), k, lo, hi, out), lambda: out.numpy().copy()
        for sw in ({}, {"POOL_VECTOR": 0}, {"POOL_SPLIT": 1}, {"POOL_SPLIT": 0, "POOL_VECTOR": 1}):
            switches(**sw)
            run_paths(hl, f"{kind}_pool_uint8", make_args, want, f"{sw} {lo} {hi}", paths=("direct", "general", "argv") if not sw else ("direct",))


@gpu
@pytest.mark.parametrize("kind", ["average", "max"])
def test_hip_pool_partial_quad_in_padded_channels(hl, switches, kind):
    """c = 6 in pixels 8 bytes apart: the dword path with a last quad of two channels; the padding is never part of a result"""
    store = rand_u8((2, 11, 13, 8), 21)
    inp = store[..., :6]
    k = dict(inp=inp, out_extents=(6, 6, 5, 2), stride=(2, 2), filt=(3, 3), in_mins=(0, 0, 0, 0), out_mins=(0, 0, 0, 0))
    want = hk.pool(kind, **k)

    def make_args():
        out = hl.Buffer(np.full(want.shape, 0x5A, np.uint8))
        return pool_args(hl.Buffer(inp), k, 0, 255, out), lambda: out.numpy().copy()
    switches(POOL_SPLIT=0, POOL_VECTOR=1)
    run_paths(hl, f"{kind}_pool_uint8", make_args, want)
    args, _ = make_args()
    assert launches(hl, lambda: hl._check(hl._fn[f"{kind}_pool_uint8"](*[a.ptr if isinstance(a, hl.Buffer) else a for a in args]))) == ["hannk_pool4"]


@gpu
@pytest.mark.parametrize("kind", ["average", "max"])
def test_hip_global_pool_on_both_sides_of_the_split(hl, switches, kind):
    inp = rand_u8((2, 7, 7, 128), 22)
    k = dict(inp=inp, out_extents=(128, 1, 1, 2), stride=(1, 1), filt=(7, 7))
    want = hk.pool(kind, **k)
    assert np.array_equal(want, np_pool(kind, **k))

    def make_args():
        out = hl.Buffer(np.full(want.shape, 0x5A, np.uint8))
        return pool_args(hl.Buffer(inp.copy()), k, 0, 255, out), lambda: out.numpy().copy()
    for sw, kernel in (({}, "hannk_pool_split"), ({"POOL_SPLIT": 0, "POOL_VECTOR": 1}, "hannk_pool4"), ({"POOL_SPLIT": 0}, "hannk_pool_general"),
                       ({"POOL_SPLIT": 1}, "hannk_pool_split"), ({"POOL_VECTOR": 0}, "hannk_pool_general")):
        switches(**sw)
        run_paths(hl, f"{kind}_pool_uint8", make_args, want, str(sw), paths=("direct",))
        args, _ = make_args()
        assert launches(hl, lambda: hl._check(hl._fn[f"{kind}_pool_uint8"](*[a.ptr if isinstance(a, hl.Buffer) else a for a in args]))) == [kernel], sw


@gpu
@pytest.mark.parametrize("kind", ["average", "max"])
def test_hip_pool_cropped_output_and_unaligned_device_input(hl, switches, kind):
    """device buffers of the caller's: an output cropped out of sentinel-padded rows (nothing around it may change), and an input one
    byte off alignment, which the dword kernels may not take"""
    c, w, h, b = 8, 13, 11, 2
    inp = rand_u8((b, h, w, c), 23)
    k = dict(inp=inp, out_extents=(c, 5, 4, b), stride=(2, 2), filt=(3, 3), in_mins=(0, 0, 0, 0), out_mins=(0, 1, 1, 0))
    want = hk.pool(kind, **k)
    for offset, kernel in ((0, "hannk_pool4"), (1, "hannk_pool_general")):
        switches(POOL_SPLIT=0, POOL_VECTOR=1)
        din = DevTensor(hl, (b, h, w, c), offset=offset, fill=inp)
        dout = DevTensor(hl, (b, 4, 5, c), strides=(4 * 9 * 16 + 32, 9 * 16, 16, 1), offset=48, mins=(0, 1, 1, 0))
        names = launches(hl, lambda: hl._check(hl._fn[f"{kind}_pool_uint8"](din.buf.ptr, 2, 2, 3, 3, 0, 255, dout.buf.ptr)))
        got = dout.result()
        assert names == [kernel] and np.array_equal(got, want), (offset, names)
        din.free(), dout.free()


@gpu
def test_hip_pool_plan_threshold(hl, switches):
    """65 536 channel quads (a workgroup for each of 256 compute units): hannk_pool4; one pixel row fewer: one thread per output"""
    w = 64
    rows = 256 * 256 // (w * 16)   # output rows of w pixels x 16 quads
    for oh, kernel in ((rows, "hannk_pool4"), (rows - 1, "hannk_pool_general")):
        inp = hl.Buffer(rand_u8((1, 2 * oh, 2 * w, 64), 24))
        out = hl.Buffer(np.zeros((1, oh, w, 64), np.uint8))
        names = launches(hl, lambda: hl.max_pool_uint8(inp, (2, 2), (2, 2), 0, 255, out))
        assert names == [kernel], (oh, names)
        assert np.array_equal(out.numpy(), inp.array.reshape(1, oh, 2, w, 2, 64).max(axis=(2, 4)))


GPU_MEAN_CASES = {  # input (B, H, W, C), in_mins, out_mins, out_extents, rmins, rextents; the kernel the plan takes
    "xy_7x7x96": ((2, 7, 7, 96), (0, 0, 0, 0), (0, 0, 0, 0), (96, 1, 1, 2), (0, 0, 0, 0), (1, 7, 7, 1), "hannk_mean_wg"),
    "c_67": ((1, 2, 3, 67), (0, 0, 0, 0), (0, 0, 0, 0), (1, 3, 2, 1), (0, 0, 0, 0), (67, 1, 1, 1), "hannk_mean_lanes"),
    "all_5x3x2x2": ((2, 2, 3, 5), (0, 0, 0, 0), (0, 0, 0, 0), (1, 1, 1, 1), (0, 0, 0, 0), (5, 3, 2, 2), "hannk_mean_lanes"),
    "mins": ((3, 6, 7, 9), (2, -1, 3, 1), (1, 0, 0, 0), (4, 3, 2, 2), (2, 0, 4, 1), (2, 3, 2, 2), "hannk_mean_lanes"),
    "taps_300": ((1, 15, 20, 70), (0, 0, 0, 0), (0, 0, 0, 0), (70, 1, 1, 1), (0, 0, 0, 0), (1, 20, 15, 1), "hannk_mean_wg"),
    "small_stencil": ((1, 6, 9, 4), (0, 0, 0, 0), (0, 0, 0, 0), (4, 7, 5, 1), (0, 0, 0, 0), (1, 3, 2, 1), "hannk_mean_general"),
}


@gpu
@pytest.mark.parametrize("name", sorted(GPU_MEAN_CASES))
def test_hip_mean_is_the_checker(hl, switches, name):
    shape, imin, omin, oext, rmin, rext, kernel = GPU_MEAN_CASES[name]
    inp = rand_u8(shape, 31)
    want = hk.mean(inp, oext, rmin, rext, imin, omin)
    scalars = [v for pair in zip(rmin, rext) for v in pair]

    def make_args():
        out = hl.Buffer(np.full(want.shape, 0x5A, np.uint8), mins=omin)
        return [hl.Buffer(inp.copy(), mins=imin)] + scalars + [out], lambda: out.numpy().copy()
    run_paths(hl, "mean_uint8", make_args, want, name)
    args, _ = make_args()
    assert launches(hl, lambda: hl._check(hl._fn["mean_uint8"](*[a.ptr if isinstance(a, hl.Buffer) else a for a in args]))) == [kernel]
    for v in (0, 1):
        switches(MEAN_SPLIT=v)
        run_paths(hl, "mean_uint8", make_args, want, f"{name} split {v}", paths=("direct",))


EW_WIDTHS = (1, 15, 16, 17, 257)


def ew_call_args(op, a, b, out, p):
    if op == "add":
        z1, m1, z2, m2, oz, lo, hi = p
        return "add_uint8_uint8", [a, z1, m1, b, z2, m2, oz, lo, hi, out]
    z1, z2, oz, mult, shift, lo, hi = p
    return "mul_uint8_uint8_uint8", [a, z1, b, z2, oz, mult, shift, lo, hi, out]


def ew_want(op, a, b, p, w, h):
    if op == "add":
        z1, m1, z2, m2, oz, lo, hi = p
        return hk.add(a, z1, m1, b, z2, m2, oz, lo, hi, (w, h))
    z1, z2, oz, mult, shift, lo, hi = p
    return hk.mul(a, z1, b, z2, oz, mult, shift, lo, hi, (w, h))


EW_PARAMS = {"add": (3, 20000, 250, -12000, 100, 5, 250), "mul": (3, 250, 7, 1518500250, 9, 5, 250)}


@gpu
@pytest.mark.parametrize("w", EW_WIDTHS)
@pytest.mark.parametrize("op", ["add", "mul"])
def test_hip_add_mul_are_the_checker(hl, switches, op, w):
    """3 rows of w bytes: dense, with either operand broadcast through a stride of 0, and in padded rows"""
    h, p = 3, EW_PARAMS[op]
    full_a, full_b = rand_u8((h, w + 9), 41)[:, :w], rand_u8((h, w + 5), 42)[:, :w]          # padded rows
    col_a, col_b = np.broadcast_to(rand_u8((h, 1), 43), (h, w)), np.broadcast_to(rand_u8((h, 1), 44), (h, w))
    for what, a, b in (("dense", np.ascontiguousarray(full_a), np.ascontiguousarray(full_b)), ("padded", full_a, full_b), ("b0", full_a, col_b), ("a0", col_a, full_b)):
        want = ew_want(op, a, b, p, w, h)

        def make_args():
            out = hl.Buffer(np.full((h, w), 0x5A, np.uint8))
            return ew_call_args(op, hl.Buffer(a), hl.Buffer(b), out, p)[1], lambda: out.numpy().copy()
        name = ew_call_args(op, None, None, None, p)[0]
        for sw in ({}, {"EW_VECTOR": 1}, {"EW_VECTOR": 0}):
            switches(**sw)
            run_paths(hl, name, make_args, want, f"{what} {sw}", paths=("direct", "general", "argv") if not sw else ("direct",))


@gpu
@pytest.mark.parametrize("op", ["add", "mul"])
def test_hip_add_mul_unaligned_pointers_and_sentinels(hl, switches, op):
    """device buffers 1 and 16 bytes off alignment, the output in sentinel-padded rows: the wide path may only take the chunks whose three
    addresses allow it, and nothing outside the output changes"""
    h, w, p = 3, 257, EW_PARAMS[op]
    a, b = rand_u8((h, w), 45), rand_u8((h, w), 46)
    want = ew_want(op, a, b, p, w, h)
    name = ew_call_args(op, None, None, None, p)[0]
    for oa, ob, oo in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (16, 16, 16), (16, 1, 0), (1, 1, 1)):
        switches(EW_VECTOR=1)
        da, db = DevTensor(hl, (h, w), strides=(272, 1), offset=oa, fill=a), DevTensor(hl, (h, w), strides=(288, 1), offset=ob, fill=b)
        dout = DevTensor(hl, (h, w), strides=(304, 1), offset=oo)
        hl._check(hl._fn[name](*[v.ptr if isinstance(v, hl.Buffer) else v for v in ew_call_args(op, da.buf, db.buf, dout.buf, p)[1]]))
        assert np.array_equal(dout.result(), want), (oa, ob, oo)
        da.free(), db.free(), dout.free()


@gpu
@pytest.mark.parametrize("op", ["add", "mul"])
def test_hip_add_mul_constant_operands_under_every_zero_point(hl, op):
    h, w = 2, 33
    for va in (0, 255):
        for vb in (0, 255):
            a, b = np.full((h, w), va, np.uint8), np.full((h, w), vb, np.uint8)
            for z1 in EW_ZEROS:
                for z2 in EW_ZEROS:
                    p = (z1, 32767, z2, -32768, 128, 0, 255) if op == "add" else (z1, z2, 128, (1 << 31) - 1, 12, 0, 255)
                    want = ew_want(op, a, b, p, w, h)

                    def make_args():
                        out = hl.Buffer(np.full((h, w), 0x5A, np.uint8))
                        return ew_call_args(op, hl.Buffer(a), hl.Buffer(b), out, p)[1], lambda: out.numpy().copy()
                    run_paths(hl, ew_call_args(op, None, None, None, p)[0], make_args, want, f"{va} {vb} {z1} {z2}", paths=("direct", "general"))


ROW_LENGTHS = (1, 2, 63, 64, 65, 1001, 1025)   # 1025: one past the 64 x 16 elements a wave keeps in registers


def rows_input(n, rows, seed):
    return np.stack([row_contents(ROW_KINDS[j % 4], n, seed + j) for j in range(rows)])


def rows_call(hl, op, inb, out):
    if op == "softmax":
        return "softmax_uint8", [inb, 23637, 9, 0, 16384, 6, out]
    return "l2_normalization_uint8", [inb, 131, out]


def rows_want(op, inp, **kw):
    return hk.softmax(inp, 23637, 9, 0, 16384, 6, **kw) if op == "softmax" else hk.l2_normalization(inp, 131, **kw)


@gpu
@pytest.mark.parametrize("n", ROW_LENGTHS)
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("op", ["softmax", "l2"])
def test_hip_rows_are_the_checker(hl, switches, op, rows, n):
    assert hl.lib is not None and ROW_LENGTHS[-1] == 64 * 16 + 1
    inp = rows_input(n, rows, 50 + n)
    want = rows_want(op, inp)

    def make_args():
        out = hl.Buffer(np.full((rows, n), 0x5A, np.uint8))
        return rows_call(hl, op, hl.Buffer(inp.copy()), out)[1], lambda: out.numpy().copy()
    name = rows_call(hl, op, None, None)[0]
    run_paths(hl, name, make_args, want, f"{rows} x {n}")
    switches(ROWS_KEEP=0)
    run_paths(hl, name, make_args, want, f"{rows} x {n} recompute", paths=("direct",))
    switches()
    args, _ = make_args()
    assert launches(hl, lambda: hl._check(hl._fn[name](*[a.ptr if isinstance(a, hl.Buffer) else a for a in args]))) == ["hannk_rows"]


@gpu
@pytest.mark.parametrize("op", ["softmax", "l2"])
def test_hip_rows_transposed_offset_and_sub_region(hl, switches, op):
    name = rows_call(hl, op, None, None)[0]
    # transposed: dimension 0 has the stride of a row, as ops.cpp passes another axis
    store = rand_u8((37, 5), 61)
    want_t = rows_want(op, store.T)

    def make_t():
        dst = np.full((37, 5), 0x5A, np.uint8)
        out = hl.Buffer(dst.T)
        return rows_call(hl, op, hl.Buffer(store.copy().T), out)[1], lambda: np.ascontiguousarray(out.numpy())
    run_paths(hl, name, make_t, want_t, "transposed")
    args, _ = make_t()
    assert launches(hl, lambda: hl._check(hl._fn[name](*[a.ptr if isinstance(a, hl.Buffer) else a for a in args]))) == ["hannk_rows_general"]
    # a sub-region: the input [-3, 70) x [-1, 4), the output [5, 45) x [1, 3): the reduction still runs over all 73 elements of a row
    inp = rows_input(73, 5, 62)
    want = rows_want(op, inp, out_extents=(40, 2), in_mins=(-3, -1), out_mins=(5, 1))
    assert np.array_equal(want, rows_want(op, inp)[2:4, 8:48])

    def make_sub():
        out = hl.Buffer(np.full((2, 40), 0x5A, np.uint8), mins=(5, 1))
        return rows_call(hl, op, hl.Buffer(inp.copy(), mins=(-3, -1)), out)[1], lambda: out.numpy().copy()
    run_paths(hl, name, make_sub, want, "sub-region")
    # rows one byte off alignment on the device, the output inside sentinels
    for offset in (0, 1, 3):
        din, dout = DevTensor(hl, (5, 73), strides=(80, 1), offset=offset, fill=inp), DevTensor(hl, (5, 73), strides=(77, 1), offset=offset + 2)
        hl._check(hl._fn[name](*[v.ptr if isinstance(v, hl.Buffer) else v for v in rows_call(hl, op, din.buf, dout.buf)[1]]))
        assert np.array_equal(dout.result(), rows_want(op, inp)), offset
        din.free(), dout.free()


@gpu
@pytest.mark.parametrize("bits", [16, 32])
def test_hip_approx_helpers_over_random_arguments(hl, bits):
    x = np.concatenate([APPROX_ARGS[:14], rng(70 + bits).integers(-(1 << 31), 1 << 31, (1 << 16) - 14)]).astype(np.int32)
    assert x.size == 1 << 16
    for fn, q, q_x in (("approx_log2", 15, 0), ("approx_log2", 3, 2), ("approx_exp2", 15, 15), ("approx_exp2", 8, 3), ("approx_reciprocal", 30, 0),
                       ("approx_reciprocal_sqrt", 15, 0)):
        got = hl.debug_hannk_approx(fn, q, x, q_x, bits)
        assert np.array_equal(got, hk.approx(fn, q, x, q_x, bits)), (fn, q, q_x)


@gpu
def test_hip_conveniences_against_direct_calls(hl):
    x = rand_u8((2, 11, 13, 8), 81)
    for kind in ("average", "max"):
        # "same" padding at stride 2 under a 3 x 3 filter: 13 -> 7 with padding 1, 11 -> 6 with padding 1 (compute_padding)
        got = hl.hannk_pool2d(kind, x, (3, 3), (2, 2), "same", 10, 240)
        assert np.array_equal(got, hk.pool(kind, x, (8, 7, 6, 2), (2, 2), (3, 3), 10, 240, in_mins=(0, 1, 1, 0)))
        got = hl.hannk_pool2d(kind, x, (2, 2), (2, 2), "valid")
        assert np.array_equal(got, hk.pool(kind, x, (8, 6, 5, 2), (2, 2), (2, 2)))
    assert np.array_equal(hl.hannk_mean(x, (1, 2)), hk.mean(x, (8, 1, 1, 2), (0, 0, 0, 0), (1, 13, 11, 1)))
    assert np.array_equal(hl.hannk_mean(x, -1, keepdims=False), hk.mean(x, (1, 13, 11, 2), (0, 0, 0, 0), (8, 1, 1, 1))[..., 0])
    a, b = rand_u8((2, 5, 7, 24), 82), rand_u8((2, 5, 7, 24), 83)
    q1, q2, qo = (0.05, 120), (0.03, 7), (0.08, 100)
    # add_uint8: lround(s * 2^16 / (so * 2^6)) = lround(640) and lround(384)
    assert np.array_equal(hl.hannk_add(a, q1, b, q2, qo, "relu"), hk.add(a.reshape(-1, 24), 120, 640, b.reshape(-1, 24), 7, 384, 100, 100, 255, (24, 70)).reshape(a.shape))
    col = rand_u8((2, 5, 7, 1), 84)
    want = hk.add(a.reshape(-1, 24), 120, 640, np.broadcast_to(col.reshape(-1, 1), (70, 24)), 7, -384, 100, 0, 255, (24, 70)).reshape(a.shape)
    assert np.array_equal(hl.hannk_add(a, q1, col, q2, qo, None, sign2=-1), want)
    m, e = hl.hannk_int_float(np.float32(0.05) * np.float32(0.03) / np.float32(0.08), 32)
    want = hk.mul(a.reshape(-1, 24), 120, b.reshape(-1, 24), 7, 100, m, 12 - e, 0, 255, (24, 70)).reshape(a.shape)
    assert np.array_equal(hl.hannk_mul(a, q1, b, q2, qo), want)
    rows = rows_input(1001, 3, 85)
    assert np.array_equal(hl.hannk_softmax(rows, 1 / 16), hk.softmax(rows, 23637, 9, 0, 16384, 6))
    assert np.array_equal(hl.hannk_softmax(rows[:, :40], 1 / 16, axis=0), hk.softmax(np.ascontiguousarray(rows[:, :40].T), 23637, 9, 0, 16384, 6).T)
    assert np.array_equal(hl.hannk_l2_normalization(rows, 131), hk.l2_normalization(rows, 131))
    cube = rand_u8((3, 9, 4), 86)
    want = np.moveaxis(hk.l2_normalization(np.ascontiguousarray(np.moveaxis(cube, 1, -1)).reshape(12, 9), 128).reshape(3, 4, 9), -1, 1)
    assert np.array_equal(hl.hannk_l2_normalization(cube, 128, axis=1), want)


@gpu
def test_hip_torch_ops(hl):
    import torch
    import halide_amd.torch_ops  # noqa: F401
    x = rand_u8((2, 11, 13, 8), 91)
    t = torch.from_numpy(x).cuda()
    for kind in ("average", "max"):
        got = torch.ops.hlmi.hannk_pool2d(t, kind, [3, 3], [2, 2], "same", 10, 240)
        assert np.array_equal(got.cpu().numpy(), hk.pool(kind, x, (8, 7, 6, 2), (2, 2), (3, 3), 10, 240, in_mins=(0, 1, 1, 0)))
    assert np.array_equal(torch.ops.hlmi.hannk_mean(t, [1, 2]).cpu().numpy(), hk.mean(x, (8, 1, 1, 2), (0, 0, 0, 0), (1, 13, 11, 1)))
    y = rand_u8((2, 11, 13, 8), 92)
    u = torch.from_numpy(y).cuda()
    want = hk.add(x.reshape(-1, 8), 120, 640, y.reshape(-1, 8), 7, 384, 100, 100, 255, (8, 286)).reshape(x.shape)
    assert np.array_equal(torch.ops.hlmi.hannk_add(t, 0.05, 120, u, 0.03, 7, 0.08, 100, "relu").cpu().numpy(), want)
    m, shift = hl.hannk_mul_params(0.05, 0.03, 0.08)
    want = hk.mul(x.reshape(-1, 8), 120, y.reshape(-1, 8), 7, 100, m, shift, 0, 255, (8, 286)).reshape(x.shape)
    assert np.array_equal(torch.ops.hlmi.hannk_mul(t, 0.05, 120, u, 0.03, 7, 0.08, 100, "none").cpu().numpy(), want)
    rows = rows_input(1001, 3, 93)
    r = torch.from_numpy(rows).cuda()
    assert np.array_equal(torch.ops.hlmi.hannk_softmax(r, 1 / 16, 1.0, 1 / 256, 0, -1).cpu().numpy(), hk.softmax(rows, 23637, 9, 0, 16384, 6))
    assert np.array_equal(torch.ops.hlmi.hannk_softmax(r, 1 / 16, 1.0, 1 / 256, 0, 0).cpu().numpy(),
                          hk.softmax(np.ascontiguousarray(rows.T), 23637, 9, 0, 16384, 6).T)
    assert np.array_equal(torch.ops.hlmi.hannk_l2_normalization(r, 131, 1).cpu().numpy(), hk.l2_normalization(rows, 131))


def test_the_fuzzer_has_the_cases():
    src = open(os.path.join(ROOT, "scripts", "fuzz_parity.py")).read()
    for name in ("hannk_pool", "hannk_elementwise"):
        assert f"def fuzz_{name}(rng):" in src and f'CASES["{name}"] = fuzz_{name}' in src and f"def case_{name}" not in src


@gpu
@pytest.mark.parametrize("name", ["hannk_pool", "hannk_elementwise"])
def test_seeded_fuzz_slice(name):
    """scripts/fuzz_parity.py's cases of these ops, a fixed number from a fixed seed"""
    mod = load_fuzz_parity()
    r = np.random.default_rng(20261020)
    for i in range(60):
        desc, ok = mod.CASES[name](r)
        assert ok, f"case {i}: {desc}"


@gpu
def test_hip_consumer_runs(hl):
    """the C++ consumer: what Pool2DOp::execute, SoftmaxOp::execute and add_uint8 do, through the mangled symbols, checked against its own
    plain loops"""
    r = subprocess.run([_build_consumer()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hannk nn consumer ok" in r.stdout
