"""hannk's elementwise programs, copy, fill, upsample_channels (halide_amd/csrc/hannk_program.hip) and the shallow depthwise variant
(halide_amd/csrc/hannk_conv.hip), DESIGN.md 5.14.

CPU: the plain-C checker against an independent numpy evaluator on every opcode, the reference's own acceptance of approx_log2p1_exp2 /
approx_logistic / approx_tanh on its full grids, the two count widths against each other, closeness to float64, the Python assembler byte
for byte, the entry protocol, metadata and symbols.
GPU (-m gpu): the library on every plan, its general path and _argv byte for byte against the checker."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hannk_program_checker as hp
from parity_helpers import DevTensor, gpu_present, launches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM_OPS = ("elementwise_5xuint8_1xuint8", "elementwise_5xint16_1xuint8int16", "depthwise_conv_shallow_uint8", "copy_uint8_uint8", "fill_uint8",
               "upsample_channels_uint8")
CORNERS = np.array([-32768, -1, 0, 1, 32767], np.int64)


def rng(seed):
    return np.random.default_rng(seed)


# ------------------------------------------------------------------------------------------------------------------ the numpy evaluator
def i64(v):
    return np.asarray(v, np.int64)


def wr(v, bits):
    m = 1 << bits
    v = i64(v) & (m - 1)
    return np.where(v >= (m >> 1), v - m, v)


def st(v, bits):
    return np.clip(i64(v), -(1 << (bits - 1)), (1 << (bits - 1)) - 1)


def shl(a, c, bits):
    """a << c in a signed type of `bits`, c signed; everything is shifted out at |c| >= bits"""
    a, c = np.broadcast_arrays(i64(a), i64(c))
    left = np.where(c >= bits, 0, wr(a << np.clip(c, 0, bits - 1), bits))
    right = np.where(-c >= bits, np.where(a < 0, -1, 0), a >> np.clip(-c, 0, bits - 1))
    return np.where(c >= 0, left, right)


def rsr(a, s, bits):
    """rounding_shift_right: (a >> s) + (s > 0 & (a >> (s - 1)))"""
    a, s = np.broadcast_arrays(i64(a), i64(s))
    pos = shl(a, -s, bits) + (shl(a, -(s - 1), bits) & 1)
    return np.where(s > 0, pos, shl(a, -s, bits))


def m2h(a, b, bits):
    return st((i64(a) * i64(b) + (1 << (bits - 2))) >> (bits - 1), bits)


def floor_log2_u32(x):
    y = (i64(x) & 0xffffffff).copy()
    n = np.zeros(y.shape, np.int64)
    for s in (16, 8, 4, 2, 1):
        big = (y >> s) != 0
        y = np.where(big, y >> s, y)
        n += np.where(big, s, 0)
    return np.where((i64(x) & 0xffffffff) == 0, -1, n)


def np_approx_log2_i16(q, x, q_x):
    """approx_log2(q, x, q_x, Int(16)) of an i32 x; q < 14"""
    x = i64(x)
    fl = floor_log2_u32(x)
    frac1 = wr(shl(x, 15 - fl, 32), 16) & 0x7fff
    frac2 = m2h(frac1, frac1, 16)
    frac3 = m2h(frac2, frac1, 16)
    poly = wr(m2h(2555, frac3, 16) + m2h(-9421, frac2, 16) + m2h(23249, frac1, 16) + 5, 16)
    assert q < 14
    return st(shl(wr(fl - q_x, 16), q, 16) + wr(rsr(poly, 14 - q, 16), 16), 16)


def np_exp2_poly(frac1):
    frac2 = m2h(frac1, frac1, 16)
    frac3 = m2h(frac2, frac1, 16)
    return wr(m2h(2592, frac3, 16) + m2h(7363, frac2, 16) + m2h(22812, frac1, 16), 16)


def np_approx_exp2_i16(q, x, q_x):
    """approx_exp2(q, x, q_x, Int(16)) of an i16 x and a constant count q_x >= 0 (an i32 immediate)"""
    x = i64(x)
    floor_x = wr(x >> q_x, 16)
    e = st(shl(1, wr(floor_x + q, 16), 32), 16)
    frac1 = shl(wr(x - (floor_x << q_x), 16), 15 - q_x, 16)
    return st(e + m2h(e, np_exp2_poly(frac1), 16), 16)


def np_exp2_q16(x, q_x, cw):
    """approx_exp2(16, x, q_x, Int(32)) of an i16 x, a signed count of cw bits"""
    x, q_x = i64(x), i64(q_x)
    floor_x = shl(x, -q_x, max(16, cw))
    e = shl(1, wr(floor_x + 16, 32), 32)
    frac1 = shl(wr(x - shl(floor_x, q_x, 32), 16), wr(15 - wr(q_x, 16), 16), 16)
    poly = shl(np_exp2_poly(frac1), 16, 32)
    return st(e + m2h(e, poly, 32), 32)


def np_log2pm1(q, x, sign, q_x, cw):
    x, q_x = i64(x), i64(q_x)
    raw = np_approx_log2_i16(q, wr(sign * 65536 + np_exp2_q16(x, q_x, cw), 32), 16)
    line = st(rsr(x, wr(wr(q_x, 16) - q, 16), 32), 16)
    return np.where(shl(x, -q_x, max(16, cw)) < 14, raw, line)


def np_logistic(q, x, q_x, cw):
    x2 = m2h(x, -23637, 16)
    return np_approx_exp2_i16(q, wr(-np_log2pm1(11, x2, 1, wr(i64(q_x) - 1, cw), cw), 16), 11)


def np_tanh(q, x, q_x, cw):
    x2 = m2h(x, 23637, 16)
    ax, c = wr(np.abs(x2), 16), wr(i64(q_x) - 2, cw)
    out = np_approx_exp2_i16(q, wr(np_log2pm1(11, ax, -1, c, cw) - np_log2pm1(11, ax, 1, c, cw), 16), 11)
    return np.where(x2 < 0, wr(-out, 16), np.where(x2 == 0, 0, out))


def np_op(code, a, s2, arg3, arg4):
    a, s2, arg3, arg4 = np.broadcast_arrays(i64(a), i64(s2), i64(arg3), i64(arg4))
    b = wr(s2 + arg3, 16)
    if code == 1:
        return st(a + b, 16)
    if code == 2:
        return st(a - b, 16)
    if code == 3:
        return st(m2h(a, b, 16) + arg4, 16)
    if code == 4:
        return st(rsr(a * b, arg4 & 0xffff, 32), 16)
    if code == 5:
        return wr(rsr(a, b, 16), 16)
    if code == 6:
        return np.minimum(a, b)
    if code == 7:
        return np.maximum(a, b)
    if code == 8:
        return np.maximum(np.minimum(a, arg4), arg3)
    if code == 9:
        return wr(rsr(np_logistic(15, a, b, 16), wr(15 - arg4, 16), 16), 16)
    if code == 10:
        return wr(rsr(np_tanh(15, a, b, 16), wr(15 - arg4, 16), 16), 16)
    return np.zeros(a.shape, np.int64)


def np_program(inputs, program, outputs):
    """the interpreter in numpy: inputs five int arrays of one shape -> the last `outputs` slots, saturated as the variant's types"""
    slots = {-k - 1: i64(inputs[k]) for k in range(5)}
    slots[0] = np.zeros(inputs[0].shape, np.int64)
    n = len(program)
    for k, (code, a1, a2, a3, a4) in enumerate(np.asarray(program).tolist()):
        slots[k + 1] = np_op(code, slots[a1], slots[a2], a3, a4) if 1 <= code <= 10 else np.zeros(inputs[0].shape, np.int64)
    if outputs == 1:
        return np.clip(slots[n], 0, 255).astype(np.uint8)
    return np.clip(slots[n - 1], 0, 255).astype(np.uint8), slots[n].astype(np.int16)


def operands(seed, n=4000):
    """random i16 quadruples with every combination of the corners in front"""
    g = np.stack(np.meshgrid(CORNERS, CORNERS, CORNERS, CORNERS, indexing="ij"), -1).reshape(-1, 4)
    r = rng(seed).integers(-32768, 32768, (n, 4))
    return np.concatenate([g, r]).T


# ------------------------------------------------------------------------------------------------------------------ CPU: the checker
@pytest.mark.parametrize("code", [0, 1, 2, 3, 4, 5, 6, 7, 8, 11])
def test_checker_opcodes_are_the_numpy_evaluator(code):
    a, s2, arg3, arg4 = operands(100 + code)
    got = hp.op(code, a, s2, arg3, arg4)
    assert np.array_equal(got, np_op(code, a, s2, arg3, arg4)), code
    if code in (0, 11):
        assert not got.any()


def test_checker_shift_counts_inside_the_type():
    """Shift: every count -15 .. 15 against the definition in exact arithmetic; MulShift: every count 0 .. 31"""
    a = np.concatenate([CORNERS, rng(1).integers(-32768, 32768, 500)])
    for c in range(-15, 16):
        got = hp.op(5, a, c, 0, 0)
        want = wr(a << -c, 16) if c <= 0 else (a + (1 << (c - 1))) >> c
        assert np.array_equal(got, want), c
    b = rng(2).integers(-32768, 32768, a.size)
    for c in range(32):
        want = st((a * b + ((1 << c) >> 1)) >> c, 16)
        assert np.array_equal(hp.op(4, a, b, 0, c), want), c


@pytest.mark.parametrize("code", [9, 10])
def test_checker_logistic_and_tanh_opcodes_are_the_numpy_evaluator(code):
    """a over the corners and random values, q_x = slot + arg3 in 0 .. 15 split both ways, arg4 in 0 .. 15"""
    r = rng(code)
    a = np.concatenate([CORNERS, r.integers(-32768, 32768, 3000)])
    for q_x in range(16):
        s2 = r.integers(-200, 200, a.size)
        arg4 = r.integers(0, 16, a.size)
        got = hp.op(code, a, s2, q_x - s2, arg4)
        assert np.array_equal(got, np_op(code, a, s2, q_x - s2, arg4)), q_x
        assert np.array_equal(got, hp.op(code, a, 0, q_x, arg4)), q_x


@pytest.mark.parametrize("fn", ["approx_log2p1_exp2", "approx_log2m1_exp2", "approx_logistic", "approx_tanh"])
@pytest.mark.parametrize("width", [16, 32])
def test_checker_helpers_are_the_numpy_evaluator(fn, width):
    x = np.concatenate([CORNERS, rng(7).integers(-32768, 32768, 4000)])
    if fn == "approx_log2m1_exp2":
        x = np.maximum(np.abs(x), 1)   # log2(2^x - 1) of a positive x
    for q_x in range(16):
        for q in (7, 8, 11, 13) if "log2" in fn else (7, 8, 15):
            if fn == "approx_logistic":
                want = np_logistic(q, x, q_x, width)
            elif fn == "approx_tanh":
                want = np_tanh(q, x, q_x, width)
            else:
                want = np_log2pm1(q, x, 1 if "p1" in fn else -1, q_x, width)
            assert np.array_equal(hp.approx(fn, x, q, q_x, width), want), (q, q_x)


def relative_error(a, b):
    return np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-6)


def reference_grid():
    """common_halide_test.cpp with T = int16_t: x = (i - 2500) * (32767 / 2500) for i in 0 .. 4999, q_x = 0 .. 15"""
    xs = (np.arange(5000) - 2500) * (32767 // 2500)
    return np.meshgrid(xs, np.arange(16))


def test_reference_acceptance_of_log2p1_exp2():
    x, y = reference_grid()
    with np.errstate(over="ignore"):
        exact = np.clip(np.round(256.0 * np.log2(1.0 + np.exp2(x / 2.0 ** y))), -32768, 32767)
    got = hp.approx("approx_log2p1_exp2", x, 8, y, 32).astype(np.float64)
    bad = (relative_error(exact, got) > 1e-3) & (np.abs(exact - got) > 2.0)
    assert not bad.any(), np.argwhere(bad)[:4]


@pytest.mark.parametrize("q", [8, 15])
def test_reference_acceptance_of_logistic(q):
    x, y = reference_grid()
    exact_x = x / 2.0 ** y
    skip = exact_x > 32767 / 2
    assert np.count_nonzero(skip) == 1239   # the reference's own count: it cannot scale these by log2(e) without losing a bit
    with np.errstate(over="ignore"):
        exact = np.round(2.0 ** q / (1.0 + np.exp(-exact_x)))
    got = hp.approx("approx_logistic", x, q, y, 32).astype(np.float64)
    bad = (relative_error(exact, got) > 1e-1) & (np.abs(exact - got) > 2.0 ** q / 128) & ~skip
    assert not bad.any(), np.argwhere(bad)[:4]


@pytest.mark.parametrize("q", [7, 15])
def test_reference_acceptance_of_tanh(q):
    x, y = reference_grid()
    exact = np.round(2.0 ** q * np.tanh(x / 2.0 ** y))
    got = hp.approx("approx_tanh", x, q, y, 32).astype(np.float64)
    bad = (relative_error(exact, got) > 1e-1) & (np.abs(exact - got) > max(3.0, 2.0 ** q / 512))
    assert not bad.any(), np.argwhere(bad)[:4]


def test_count_widths_agree_except_at_q_x_0():
    """q_x - 1 (logistic) and q_x - 2 (tanh) are the counts: at q_x = 0 the 16-bit left shift of the generator wraps where the 32-bit one of
    the reference's test does not.  The library implements width 16 (DESIGN.md 5.14 records the counts)."""
    x = np.arange(-32768, 32768)
    for fn, differing in (("approx_logistic", 20110), ("approx_tanh", 10)):
        for q_x in range(1, 16):
            assert np.array_equal(hp.approx(fn, x, 15, q_x, 16), hp.approx(fn, x, 15, q_x, 32)), (fn, q_x)
        assert np.count_nonzero(hp.approx(fn, x, 15, 0, 16) != hp.approx(fn, x, 15, 0, 32)) == differing, fn


def test_lstm_helpers_are_close_to_float64():
    """the LSTM program's three instantiations over every i16 argument; the worst differences the checker measures, each inside the
    reference's own tolerance (2^q / 128 for logistic, max(3, 2^q / 512) for tanh)"""
    x = np.arange(-32768, 32768)
    for fn, q, q_x, worst, tolerance in (("approx_logistic", 15, 12, 28, 256), ("approx_tanh", 15, 12, 34, 64), ("approx_tanh", 7, 11, 1, 3)):
        v = x / 2.0 ** q_x
        exact = np.round(2.0 ** q * (1.0 / (1.0 + np.exp(-v)) if fn == "approx_logistic" else np.tanh(v)))
        assert np.abs(hp.approx(fn, x, q, q_x, 16) - exact).max() == worst <= tolerance, (fn, q, q_x)


UNARY_SCALES = (1 / 256, 1 / 128, 1 / 64, 0.03, 1 / 16, 0.1, 1 / 8, 0.2, 1 / 4)
UNARY_ZEROS = (0, 3, 128, 200, 255)


def run_unary(program, x):
    x = np.ascontiguousarray(x, np.uint8).reshape(1, -1)
    return hp.elementwise([x] * 5, program)[0]


@pytest.mark.parametrize("zero", UNARY_ZEROS)
def test_logistic_and_tanh_programs_are_within_one_of_float64(hl, zero):
    x = np.arange(256)
    worst = {"logistic": 0, "tanh": 0}
    for scale in UNARY_SCALES:
        v = (x - zero) * scale
        got = run_unary(hl.hannk_logistic_program(scale, zero), x).astype(np.int64)
        worst["logistic"] = max(worst["logistic"], int(np.abs(got - np.clip(np.round(256.0 / (1.0 + np.exp(-v))), 0, 255)).max()))
        got = run_unary(hl.hannk_tanh_program(scale, zero), x).astype(np.int64)
        worst["tanh"] = max(worst["tanh"], int(np.abs(got - np.clip(np.round(128.0 * np.tanh(v)) + 128, 0, 255)).max()))
    assert worst["logistic"] <= 1 and worst["tanh"] <= 1, worst


# ------------------------------------------------------------------------------------------------------------------ CPU: the assembler
LSTM_PROGRAM = [[9, -1, 0, 12, 15],     # input gate = logistic(15, input 0, 12)
                [10, -2, 0, 12, 15],    # input modulation gate = tanh(15, input 1, 12)
                [9, -3, 0, 12, 15],     # forget gate
                [9, -4, 0, 12, 15],     # output gate
                [4, 1, 2, 0, 19],       # mul_shift(input gate, input modulation gate, 15 + 4)
                [3, 3, -5, 0, 0],       # mul(forget gate, previous state)
                [1, 5, 6, 0, 0],        # state
                [10, 7, 0, 11, 7],      # tanh(7, state, 11)
                [3, 4, 8, 0, 128],      # activation = mul_add(output gate, that, 128)
                [1, 7, 0, 0, 0]]        # state again, behind the activation


def test_assembler_programs_byte_for_byte(hl):
    # IntFloat<int16_t>(1 / 256) = 16384 * 2^-7, times 2^-6: mantissa 16384, exponent -13 (ops.cpp:1801-1812)
    want = np.array([[2, -1, 0, 3, 0], [4, 1, 0, 16384, 9], [9, 2, 0, 13, 8]], np.int16)
    got = hl.hannk_logistic_program(1 / 256, 3)
    assert got.dtype == np.int16 and got.tobytes() == want.tobytes()
    # IntFloat<int16_t>(0.1f) = round(0.8 * 2^15) * 2^-3 = 26214 * 2^-3, times 2^-6: exponent -9 (ops.cpp:1821-1832)
    want = np.array([[2, -1, 0, 128, 0], [4, 1, 0, 26214, 9], [10, 2, 0, 9, 7], [1, 3, 0, 128, 0]], np.int16)
    assert hl.hannk_tanh_program(0.1, 128).tobytes() == want.tobytes()
    assert hl.hannk_lstm_program().tobytes() == np.array(LSTM_PROGRAM, np.int16).tobytes()


def test_assembler_reloads_outputs_that_are_out_of_place(hl):
    p = hl.ElementwiseAssembler()
    a = p.add(p.input(0), p.input(1))
    b = p.sub(p.input(0), 7)
    assert p.assemble([b]).tolist() == [[1, -1, -2, 0, 0], [2, -1, 0, 7, 0]]           # in place: nothing added
    assert p.assemble([b, a]).tolist()[2:] == [[1, 2, 0, 0, 0], [1, 1, 0, 0, 0]]       # out of order: both reloaded by add(x, 0)
    p = hl.ElementwiseAssembler()
    c = p.constant(5)
    assert p.constant(0).index == 0 and c.index == 1 and p.rows == [(1, 0, 0, 5, 0)]
    assert p.clamp(c, -3, 9).index == 2 and p.rows[1] == (8, 1, 1, -3, 9)
    assert p.mul_add(c, 3, 4).index == 3 and p.rows[2] == (3, 1, 0, 3, 4)
    assert p.shift(c, p.input(2), 1).index == 4 and p.rows[3] == (5, 1, -3, 1, 0)
    with pytest.raises(ValueError):
        p.add(c, 40000)


# ------------------------------------------------------------------------------------------------------------------ CPU: copy, upsample
def test_checker_copy_is_numpy():
    inp = rng(11).integers(0, 256, (2, 3, 4, 5), dtype=np.uint8)
    # the output's channels [-2, 9) around the input's [0, 5): padded on either side of dimension 0, pad_value 300 wraps to 44
    got = hp.copy(inp, (11, 4, 3, 2), 300, out_mins=(-2, 0, 0, 0))
    want = np.full((2, 3, 4, 11), 44, np.uint8)
    want[..., 2:7] = inp
    assert np.array_equal(got, want)
    # a window inside the input, offset in x and y
    got = hp.copy(inp, (2, 2, 2, 1), 0, out_mins=(1, 2, 1, 1))
    assert np.array_equal(got, inp[1:2, 1:3, 2:4, 1:3])


@pytest.mark.parametrize("factor", [1, 3, 8, 16, 0])
def test_checker_upsample_is_numpy(factor):
    inp = rng(12).integers(0, 256, (2, 3, 4, 5), dtype=np.uint8)
    oc = 5 * factor if factor else 7
    got = hp.upsample_channels(inp, factor, (oc, 4, 3, 2))
    want = inp[..., (np.arange(oc) // factor) if factor else np.zeros(oc, np.int64)]
    assert np.array_equal(got, want)
    if factor:   # a window that does not start at a multiple of the factor
        got = hp.upsample_channels(inp, factor, (factor + 1, 4, 3, 2), out_mins=(factor - 1, 0, 0, 0))
        assert np.array_equal(got, inp[..., (np.arange(factor - 1, 2 * factor) // factor)])


# ------------------------------------------------------------------------------------------------------------------ CPU: the shallow depthwise variant
SHALLOW_Q = dict(input_zero=7, filter_zero=131, multiplier=1518500250, shift=9, zero=3, lo=1, hi=250)


def shallow_data(seed, d, w, h, fw, fh, b=2):
    r = rng(seed)
    return (r.integers(0, 256, (b, h, w, d), dtype=np.uint8), r.integers(0, 256, (fh, fw, d), dtype=np.uint8), r.integers(-20000, 20000, d).astype(np.int32))


def np_shallow(inp, filt, bias, channels, oh, sy, dil, isx, q):
    """the contract's formula in numpy int64, the epilogue by the conv checker's quantize"""
    import hannk_checker as hc
    b, h, row = inp.shape
    fh, fw, d = filt.shape
    c = np.arange(channels)
    fc = (c % 16) % d
    acc = np.broadcast_to(i64(bias)[fc], (b, oh, channels)).copy()
    for ry in range(fh):
        for rx in range(fw):
            rows = inp[:, ry * dil[1]:ry * dil[1] + (oh - 1) * sy + 1:sy, :]
            a = i64(rows[:, :, c + rx * dil[0] * isx])
            acc += (i64(filt[ry, rx])[fc] - q["filter_zero"]) * (a - q["input_zero"])
    return hc.quantize("u8", wr(acc, 32).astype(np.int32), q["multiplier"], q["shift"], q["zero"], q["lo"], q["hi"])


def test_checker_shallow_d3_is_numpy_and_the_unfused_depthwise_checker():
    """D = 3, 3 x 3, dilation 2: the checker against numpy on the whole fused row, and against the ordinary depthwise checker on the unfused
    layout for the fused indices below 16, where (c % 16) % 3 == c % 3 (16 is no multiple of 3: beyond them the filter repeats out of step)"""
    import hannk_checker as hc
    d, w, h = 3, 11, 9
    inp, filt, bias = shallow_data(1, d, w, h, 3, 3)
    ow, oh = w - 4, h - 4
    got = hp.depthwise_shallow(inp.reshape(2, h, w * d), filt, bias, ow * d, oh, 1, (2, 2), d, **SHALLOW_Q)
    assert np.array_equal(got, np_shallow(inp.reshape(2, h, w * d), filt, bias, ow * d, oh, 1, (2, 2), d, SHALLOW_Q))
    q = SHALLOW_Q
    unfused = hc.depthwise(inp, filt, bias, (d, ow, oh, 2), (1, 1), (2, 2), q["input_zero"], q["filter_zero"], q["multiplier"], q["shift"], q["zero"], q["lo"], q["hi"])
    assert np.array_equal(got[:, :, :16], unfused.reshape(2, oh, ow * d)[:, :, :16])
    assert not np.array_equal(got, unfused.reshape(2, oh, ow * d))


@pytest.mark.parametrize("d", [1, 2, 4, 8, 16])
def test_checker_shallow_is_the_unfused_depthwise_checker_where_d_divides_16(d):
    import hannk_checker as hc
    w, h = 9, 8
    inp, filt, bias = shallow_data(d, d, w, h, 3, 3)
    q = SHALLOW_Q
    got = hp.depthwise_shallow(inp.reshape(2, h, w * d), filt, bias, (w - 2) * d, 2, 2, (1, 2), d, **q)   # stride_y 2, dilation_y 2
    unfused = hc.depthwise(inp, filt, bias, (d, w - 2, 2, 2), (1, 2), (1, 2), q["input_zero"], q["filter_zero"], q["multiplier"], q["shift"], q["zero"], q["lo"], q["hi"])
    assert np.array_equal(got, unfused.reshape(2, 2, (w - 2) * d))


def test_the_general_kernels_slot_array_stays_out_of_scratch_memory(tmp_path):
    """hannk_prog_general indexes a private array with the program's operands; it is the default for every program outside the table plan
    because the compiler keeps that array in registers.  Should a compiler spill it to scratch memory, this fails."""
    csrc = os.path.join(ROOT, "halide_amd", "csrc")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                        "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-slp-vectorize", "-I", os.path.join(ROOT, "include"), "-I", csrc, "-DHLMI_BUILD", "-x", "hip",
                        "--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "hannk_program.hip"), "-o",
                        str(tmp_path / "hannk_program.o")], capture_output=True, text=True, check=True)
    name, scratch = None, {}
    for line in r.stderr.splitlines():
        if "Function Name:" in line:
            name = line.split("Function Name:")[1].split()[0]
        elif "ScratchSize [bytes/lane]:" in line and name:
            scratch[name] = int(line.split("ScratchSize [bytes/lane]:")[1].split()[0])
    prog = {k: v for k, v in scratch.items() if "hannk_prog_" in k}
    assert len(prog) == 7 and sum("hannk_prog_general" in k for k in prog) == 2, sorted(scratch)
    assert not any(prog.values()), prog


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


def body_code(code):
    """an error the entry point raises in its body, after the device has been acquired"""
    return (code,) if gpu_present() else (-29,)


class EwArgs:
    def __init__(self, hl, i16=False, program=None):
        self.hl, self.i16 = hl, i16
        dt = np.int16 if i16 else np.uint8
        self.inputs = [hl.Buffer(np.zeros((3, 20), dt)) for _ in range(5)]
        self.program = hl.Buffer(np.array([[1, -1, -2, 0, 0], [8, 1, 1, 0, 200]] if program is None else program, np.int16).reshape(-1, 5))
        self.output = hl.Buffer(np.zeros((3, 20), np.uint8))
        self.output1 = hl.Buffer(np.zeros((3, 20), np.int16))

    def buffers(self):
        return ["inputs[%d]" % k for k in range(5)] + ["program", "output"] + (["output1"] if self.i16 else [])

    def get(self, which):
        return self.inputs[int(which[7])] if which.startswith("inputs") else getattr(self, which)

    def put(self, which, v):
        if which.startswith("inputs"):
            self.inputs[int(which[7])] = v
        else:
            setattr(self, which, v)

    def call(self):
        if self.i16:
            return code_of(self.hl, lambda: self.hl.elementwise_5xint16_1xuint8int16(*self.inputs, self.program, self.output, self.output1))
        return code_of(self.hl, lambda: self.hl.elementwise_5xuint8_1xuint8(*self.inputs, self.program, self.output))


@pytest.mark.parametrize("i16", [False, True])
def test_protocol_elementwise_null_type_dimensions_unallocated(hl, i16):
    assert EwArgs(hl, i16).call() in ok_codes()
    for which in EwArgs(hl, i16).buffers():
        a = EwArgs(hl, i16)
        have = a.get(which).array
        a.put(which, None)
        assert a.call() == -12, which
        a = EwArgs(hl, i16)
        a.put(which, hl.Buffer(np.zeros(have.shape, np.int8)))
        assert a.call() == -3, which
        a = EwArgs(hl, i16)
        a.put(which, hl.Buffer(np.zeros(have.shape + (1,), have.dtype)))
        assert a.call() == -43, which
        # built with no_bounds_query: an unallocated buffer runs through the checks and ends at the host pointer, its shape untouched
        a = EwArgs(hl, i16)
        a.put(which, hl.Buffer.bounds_query(have.dtype, 2, extents=have.shape[::-1]))
        assert a.call() == -34, which
        assert a.get(which).extents == list(have.shape[::-1])


@pytest.mark.parametrize("i16", [False, True])
def test_protocol_elementwise_constraints_and_regions(hl, i16):
    for d, fields in ((0, dict(min=1)), (0, dict(extent=4)), (0, dict(stride=2)), (1, dict(min=1)), (1, dict(stride=6))):
        a = EwArgs(hl, i16)
        set_dim(a.program, d, **fields)
        assert a.call() == -8, (d, fields)
    a = EwArgs(hl, i16)
    set_dim(a.output, 0, stride=2)
    assert a.call() == -8
    for k in range(5):   # all five inputs are checked whatever the program reads
        a = EwArgs(hl, i16)
        a.inputs[k] = hl.Buffer(np.zeros((3, 19), a.inputs[k].array.dtype))
        assert a.call() == -4, k
        a = EwArgs(hl, i16)
        a.inputs[k].set_min(0, 1)
        assert a.call() == -4, k
    if i16:   # the second output has the first one's mins and extents (src/AddImageChecks.cpp:520-549)
        a = EwArgs(hl, True)
        a.output1 = hl.Buffer(np.zeros((3, 21), np.int16))
        assert a.call() == -8
        a = EwArgs(hl, True)
        a.output1.set_min(0, 1)
        assert a.call() == -8
        a = EwArgs(hl, True)   # its strides are its own
        a.output1 = hl.Buffer(np.zeros((3, 32), np.int16)[:, :20])
        assert a.call() in ok_codes()


@pytest.mark.parametrize("i16", [False, True])
def test_protocol_elementwise_strides(hl, i16):
    dt = np.int16 if i16 else np.uint8
    a = EwArgs(hl, i16)   # every input may broadcast, all five at once
    for k in range(5):
        set_dim(a.inputs[k], 0, stride=0)
    assert a.call() in ok_codes()
    for k in range(5):    # any other stride: specialize_fail, raised in the body
        a = EwArgs(hl, i16)
        a.inputs[k] = hl.Buffer(np.zeros((3, 40), dt))
        set_dim(a.inputs[k], 0, stride=2, extent=20)
        assert a.call() in body_code(-31), k


@pytest.mark.parametrize("i16", [False, True])
def test_protocol_elementwise_program_operands_and_length(hl, i16):
    """this library's own refusal: an operand of a live instruction outside [-5, n] is -8; Noop (0) and unknown opcodes (11) read nothing"""
    for program, want in (([[1, -5, 0, 0, 0]], ok_codes()), ([[1, -6, 0, 0, 0]], (-8,)), ([[1, 0, -6, 0, 0]], (-8,)),
                          ([[1, -1, 0, 0, 0], [1, 1, 1, 0, 0]], ok_codes()),       # operand n: the slot written just before
                          ([[1, -1, 0, 0, 0], [1, 2, 0, 0, 0]], (-8,)),            # operand n + 1: the instruction's own slot
                          ([[1, -1, 0, 0, 0], [1, 0, 2, 0, 0]], (-8,)),
                          ([[0, 99, -99, 0, 0], [11, 77, -77, 0, 0]], ok_codes())):
        assert EwArgs(hl, i16, program).call() in want, program
    twenty = [[1, -1, 0, 1, 0]] + [[1, k, 0, 1, 0] for k in range(1, 20)]
    assert EwArgs(hl, i16, twenty).call() in ok_codes()
    # 21 instructions do not fit scratch.bound_extent(u, 26): halide_error_explicit_bounds_too_small, in the body
    assert EwArgs(hl, i16, twenty + [[1, 20, 0, 1, 0]]).call() in body_code(-2)
    a = EwArgs(hl, i16, np.zeros((0, 5), np.int16))   # the empty program
    assert a.call() in ok_codes()


def test_protocol_copy_fill_upsample(hl):
    def copy(i, o, pad=0):
        return code_of(hl, lambda: hl.copy_uint8_uint8(i, pad, o))

    def up(i, o, f=2):
        return code_of(hl, lambda: hl.upsample_channels_uint8(i, f, o))
    u8 = lambda *shape: hl.Buffer(np.zeros(shape, np.uint8))
    assert copy(u8(2, 3, 4, 3), u8(2, 3, 4, 4)) in ok_codes()
    assert copy(None, u8(2, 3, 4, 4)) == -12 and copy(u8(2, 3, 4, 3), None) == -12
    assert copy(hl.Buffer(np.zeros((2, 3, 4, 3), np.int8)), u8(2, 3, 4, 4)) == -3
    assert copy(u8(3, 4, 3), u8(2, 3, 4, 4)) == -43
    assert copy(u8(2, 3, 3, 3), u8(2, 3, 4, 4)) == -4                    # x
    assert copy(u8(2, 3, 4, 3), hl.Buffer(np.zeros((2, 3, 4, 40), np.uint8), mins=(-20, 0, 0, 0))) in ok_codes()   # dimension 0 is clamped
    assert copy(hl.Buffer.bounds_query(np.uint8, 4, extents=(3, 4, 3, 2)), u8(2, 3, 4, 4)) == -34
    assert copy(u8(2, 3, 4, 3), hl.Buffer.bounds_query(np.uint8, 4, extents=(4, 4, 3, 2))) == -34
    fill = lambda o: code_of(hl, lambda: hl.fill_uint8(7, o))
    assert fill(u8(2, 3, 4, 4)) in ok_codes()
    assert fill(None) == -12 and fill(hl.Buffer(np.zeros((2, 3, 4, 4), np.int8))) == -3 and fill(u8(3, 4, 4)) == -43
    assert fill(hl.Buffer.bounds_query(np.uint8, 4, extents=(4, 4, 3, 2))) == -34
    assert up(u8(2, 3, 4, 3), u8(2, 3, 4, 6)) in ok_codes()
    assert up(u8(2, 3, 4, 3), u8(2, 3, 4, 7)) == -4                      # channel 6 / 2 = 3
    assert up(u8(2, 3, 4, 3), u8(3, 3, 4, 6)) == -8                      # dimension 3 is shared
    assert up(u8(2, 3, 4, 3), u8(2, 3, 4, 9), 0) in ok_codes()           # c / 0 == 0
    q = hl.Buffer.bounds_query(np.uint8, 4)
    assert up(q, hl.Buffer(np.zeros((2, 3, 4, 7), np.uint8), mins=(5, 1, 0, 0)), 3) == 0
    assert q.mins == [1, 1, 0, 0] and q.extents == [3, 4, 3, 2]         # channels 5 .. 11 read 1 .. 3
    q = hl.Buffer.bounds_query(np.uint8, 4, mins=(0, 0, 0, 0), extents=(6, 4, 3, 0))
    assert up(hl.Buffer(np.zeros((2, 3, 4, 3), np.uint8), mins=(0, 0, 0, 4)), q) == 0
    assert q.mins == [0, 0, 0, 4] and q.extents == [6, 4, 3, 2]


class ShallowArgs:
    def __init__(self, hl, d=4, w=8, h=6, fw=3, fh=3):
        self.hl, self.d = hl, d
        self.input = hl.Buffer(np.zeros((2, h, 1, w * d), np.uint8))
        self.filter = hl.Buffer(np.zeros((fh, fw, d), np.uint8))
        self.bias = hl.Buffer(np.zeros(d, np.int32))
        self.output = hl.Buffer(np.zeros((2, h - fh + 1, 1, (w - fw + 1) * d), np.uint8))
        self.stride, self.dilation, self.isx = (1, 1), (1, 1), d

    def call(self):
        return code_of(self.hl, lambda: self.hl.depthwise_conv_shallow_uint8(self.input, 0, self.filter, 0, self.bias, self.stride, self.dilation, self.isx,
                                                                           1 << 30, 0, 0, 0, 255, self.output))


def test_protocol_shallow(hl):
    assert ShallowArgs(hl).call() in ok_codes()
    for which, wrong in (("input", np.int8), ("filter", np.int8), ("bias", np.int16), ("output", np.int8)):
        a = ShallowArgs(hl)
        have = getattr(a, which).array
        setattr(a, which, None)
        assert a.call() == -12, which
        a = ShallowArgs(hl)
        setattr(a, which, hl.Buffer(np.zeros(have.shape, wrong)))
        assert a.call() == -3, which
        a = ShallowArgs(hl)
        setattr(a, which, hl.Buffer(np.zeros(have.shape + (1,), have.dtype)))
        assert a.call() == -43, which
    a = ShallowArgs(hl)   # the output's dimension 1 is {0, 1}
    a.output = hl.Buffer(np.zeros((2, 4, 2, 24), np.uint8))
    assert a.call() == -8
    a = ShallowArgs(hl)
    a.output.set_min(0, 1, 0, 0)
    assert a.call() == -8
    a = ShallowArgs(hl)   # dimension 3 is the input's
    a.output = hl.Buffer(np.zeros((3, 4, 1, 24), np.uint8))
    assert a.call() == -8
    a = ShallowArgs(hl)   # the last tap reads fused index 23 + 2 * 4 = 31: an input row of 31 is one short
    a.input = hl.Buffer(np.zeros((2, 6, 1, 31), np.uint8))
    assert a.call() == -4
    a = ShallowArgs(hl)   # ... and a larger input_stride_x reaches further
    a.isx = 5
    assert a.call() == -4
    a = ShallowArgs(hl)   # y
    a.input = hl.Buffer(np.zeros((2, 5, 1, 32), np.uint8))
    assert a.call() == -4
    a = ShallowArgs(hl)   # no alignment requirement, no require_same_min_extent on filter or bias: D = 4 under 24 fused channels
    a.input = hl.Buffer(np.zeros((2, 6, 1, 35), np.uint8)[:, :, :, 1:33])
    assert a.call() in ok_codes()
    a = ShallowArgs(hl)   # bias shorter than the filter's depth
    a.bias = hl.Buffer(np.zeros(3, np.int32))
    assert a.call() == -4
    # queries: the fused row [0, C + (FW - 1) * dilation_x * input_stride_x), x = {0, 1}, the y span, the output's batches; filter and bias [0, D)
    a = ShallowArgs(hl)
    a.input = hl.Buffer.bounds_query(np.uint8, 4)
    a.bias = hl.Buffer.bounds_query(np.int32, 1)
    a.dilation, a.stride = (2, 1), (1, 2)
    assert a.call() == 0
    assert a.input.mins == [0, 0, 0, 0] and a.input.extents == [24 + 2 * 2 * 4, 1, (4 - 1) * 2 + 3, 2] and a.bias.extents == [4]


def test_metadata_and_symbols(hl):
    u8, i16, i32 = (1, 8), (0, 16), (0, 32)
    ins = ["inputs_%d" % k for k in range(5)]
    expect = {
        "elementwise_5xuint8_1xuint8": (ins + ["program", "output"], [1] * 6 + [2], [u8] * 5 + [i16, u8], 2),
        "elementwise_5xint16_1xuint8int16": (ins + ["program", "output.0", "output.1"], [1] * 6 + [2, 2], [i16] * 6 + [u8, i16], 2),
        "depthwise_conv_shallow_uint8": (["input", "input_zero", "filter", "filter_zero", "bias", "stride_x", "stride_y", "dilation_x", "dilation_y", "input_stride_x",
                                          "output_multiplier", "output_shift", "output_zero", "output_min", "output_max", "output"],
                                         [1, 0, 1, 0, 1] + [0] * 10 + [2], [u8, u8, u8, u8, i32] + [i32] * 7 + [u8, u8, u8, u8], None),
        "copy_uint8_uint8": (["input", "pad_value", "output"], [1, 0, 2], [u8, i32, u8], 4),
        "fill_uint8": (["value", "output"], [0, 2], [u8, u8], 4),
        "upsample_channels_uint8": (["input", "factor", "output"], [1, 0, 2], [u8, i32, u8], 4),
    }
    assert tuple(expect) == hl.HANNK_PROGRAM_OPS == PROGRAM_OPS
    for name, (names, kinds, types, rank) in expect.items():
        md = hl.metadata(name)
        args = [md.arguments[k] for k in range(md.num_arguments)]
        assert md.version == 1 and md.name.decode() == name and b"hip" in md.target
        assert [a.name.decode() for a in args] == names and [a.kind for a in args] == kinds
        assert [(a.type.code, a.type.bits) for a in args] == types and all(a.type.reserved == 1 for a in args)
        if rank is not None:
            assert [a.dimensions for a in args] == [rank if k else 0 for k in kinds]
        else:
            assert [a.dimensions for a in args if a.kind] == [4, 3, 1, 4]
        for suffix in ("", "_argv", "_metadata"):
            assert getattr(hl.lib, hl._symbol(name, suffix), None) is not None, (name, suffix)


def test_mangled_symbols_are_what_the_compiler_makes_of_the_headers(tmp_path):
    """every header is compiled with the host compiler into an object that refers to its three functions; the undefined symbols nm reads
    from it are the ones the library exports"""
    exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "halide_amd", "lib", "libhlmi.so")], capture_output=True, text=True,
                              check=True).stdout.split()
    seen = 0
    for name in PROGRAM_OPS:
        src = tmp_path / f"{name}.cpp"
        src.write_text(f'#include "halide/{name}.h"\nvoid *use_{name}[] = {{(void *)&hannk::{name}, (void *)&hannk::{name}_argv, (void *)&hannk::{name}_metadata}};\n')
        obj = tmp_path / f"{name}.o"
        subprocess.run(["g++", "-std=c++17", "-c", "-I", os.path.join(ROOT, "include", "aot"), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(obj)], check=True)
        wanted = [s for s in subprocess.run(["nm", "-u", str(obj)], capture_output=True, text=True, check=True).stdout.split() if s.startswith("_ZN5hannk")]
        assert len(wanted) == 3, (name, wanted)
        for s in wanted:
            assert s in exported, s
            seen += 1
    assert seen == 18


# ------------------------------------------------------------------------------------------------------------------ GPU
gpu = pytest.mark.gpu
SWITCHES = ("HLMI_HANNK_EW_PLAN", "HLMI_HANNK_MOVE_VECTOR")
PLAN_GENERAL, PLAN_TABLE, PLAN_LDS, PLAN_REG = 0, 1, 2, 3


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
    ctypes_of = {(0, 32): C.c_int32, (1, 8): C.c_uint8}
    for j, v in enumerate(args):
        a = md.arguments[j]
        box = v.raw if a.kind else ctypes_of[(a.type.code, a.type.bits)](v)
        keep.append(box)
        argv[j] = C.cast(C.pointer(box), C.c_void_p)
    fn = getattr(hl.lib, hl._symbol(name, "_argv"))
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(C.c_void_p)]
    return hl._check(fn(argv))


def call(hl, name, args, path="direct"):
    if path == "direct":
        hl._check(hl._fn[name](*[a.ptr if isinstance(a, hl.Buffer) else a for a in args]))
    elif path == "general":
        hl.debug_hannk_general(name, *args)
    else:
        call_argv(hl, name, args)


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = got != want
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} of {got.size} differ, first at {tuple(np.argwhere(bad)[0])}"


EW_WIDTHS = (1, 15, 16, 17, 64, 255, 257, 1000)
ADD_CLAMP = [[1, -1, -2, -100, 0], [8, 1, 1, 10, 200]]
# every opcode once, on five inputs: the result of each instruction feeds a later one
EVERY_OPCODE = [[1, -1, -2, 5, 0], [2, 1, -3, -7, 0], [3, 2, -4, 0, 9], [4, -5, 3, 300, 3], [5, 4, 0, 2, 0], [6, 5, -1, 40, 0], [7, 6, -2, -30, 0],
                [8, 7, 7, 0, 255], [0, 0, 0, 0, 0], [4, 8, 0, 16384, 9], [9, 10, 0, 11, 8], [10, 10, 0, 11, 7], [11, 1, 1, 1, 1], [1, 11, 12, 64, 0]]


def u8_inputs(rows, width, seed, strides0=(1, 1, 1, 1, 1)):
    """five (rows, width) uint8 views; a stride-0 input is one column broadcast along the row"""
    r = rng(seed)
    out = []
    for s in strides0:
        base = r.integers(0, 256, (rows, width if s else 1), dtype=np.uint8)
        out.append(base if s else np.lib.stride_tricks.as_strided(base, shape=(rows, width), strides=(base.strides[0], 0), writeable=False))
    return out


def run_ew_u8(hl, inputs, program, path="direct"):
    prog = hl.Buffer(np.ascontiguousarray(program, np.int16).reshape(-1, 5))
    out = hl.Buffer(np.full(inputs[0].shape, 0x5A, np.uint8))
    call(hl, "elementwise_5xuint8_1xuint8", [hl.Buffer(a) for a in inputs] + [prog, out], path)
    return out.numpy().copy()


@gpu
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("unary", ["logistic", "tanh"])
def test_hip_table_path_is_the_checker(hl, switches, unary, rows):
    program = hl.hannk_logistic_program(0.05, 120) if unary == "logistic" else hl.hannk_tanh_program(0.02, 131)
    for width in EW_WIDTHS:
        x = rng(width).integers(0, 256, (rows, width), dtype=np.uint8)
        if width == 257:
            x[0, :256] = np.arange(256)
        want = hp.elementwise([x] * 5, program)
        assert np.array_equal(want, np_program([x] * 5, program, 1))
        for plan, kernel in ((None, "hannk_prog_general"), (PLAN_TABLE, "hannk_prog_table"), (PLAN_LDS, "hannk_prog_interp"), (PLAN_REG, "hannk_prog_interp"),
                             (PLAN_GENERAL, "hannk_prog_general")):   # (these outputs are below EW_TABLE_MIN_OUTPUTS)
            switches(**({} if plan is None else {"EW_PLAN": plan}))
            names = launches(hl, lambda: same(run_ew_u8(hl, [x] * 5, program), want, (unary, rows, width, plan)))
            assert names == [kernel], (plan, names)
        switches()
        same(run_ew_u8(hl, [x] * 5, program, "general"), want, (unary, rows, width, "general"))
        same(run_ew_u8(hl, [x] * 5, program, "argv"), want, (unary, rows, width, "argv"))


@gpu
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("case", ["add_clamp", "every_opcode", "stride0"])
def test_hip_interpreter_path_is_the_checker(hl, switches, case, rows):
    program = ADD_CLAMP if case == "add_clamp" else EVERY_OPCODE
    for width in EW_WIDTHS:
        inputs = u8_inputs(rows, width, 3 * width + rows, (1, 0, 1, 1, 0) if case == "stride0" else (1,) * 5)
        want = hp.elementwise(inputs, program)
        assert np.array_equal(want, np_program(inputs, program, 1))
        for plan, kernel in ((None, "hannk_prog_general"), (PLAN_TABLE, "hannk_prog_general"), (PLAN_LDS, "hannk_prog_interp"), (PLAN_REG, "hannk_prog_interp"),
                             (PLAN_GENERAL, "hannk_prog_general")):   # (no table of a program that names several inputs)
            switches(**({} if plan is None else {"EW_PLAN": plan}))
            names = launches(hl, lambda: same(run_ew_u8(hl, inputs, program), want, (case, rows, width, plan)))
            assert names == [kernel], (plan, names)
        switches()
        same(run_ew_u8(hl, inputs, program, "general"), want, (case, rows, width, "general"))
        same(run_ew_u8(hl, inputs, program, "argv"), want, (case, rows, width, "argv"))


@gpu
@pytest.mark.parametrize("unary", [True, False])
def test_hip_elementwise_unaligned_pointers_sentinels_and_a_device_program(hl, switches, unary):
    """device buffers 1 - 3 bytes off alignment, the output in sentinel-padded rows, the program held on the device alone"""
    rows, width = 3, 257
    program = np.asarray(hl.hannk_tanh_program(0.03, 100) if unary else ADD_CLAMP, np.int16)
    inputs = u8_inputs(rows, width, 77)
    if unary:
        inputs = [inputs[0]] * 5
    want = hp.elementwise(inputs, program)
    for oi, oo in ((0, 0), (1, 0), (0, 2), (3, 3), (16, 16), (2, 1)):
        for plan in (None, PLAN_TABLE, PLAN_LDS, PLAN_REG):
            switches(**({} if plan is None else {"EW_PLAN": plan}))
            din = [DevTensor(hl, (rows, width), strides=(272, 1), offset=oi, fill=a) for a in (inputs[:1] if unary else inputs)]
            dprog = DevTensor(hl, program.shape, dtype=np.int16, fill=program)
            dout = DevTensor(hl, (rows, width), strides=(304, 1), offset=oo)
            bufs = [d.buf for d in din] * (5 if unary else 1)
            call(hl, "elementwise_5xuint8_1xuint8", bufs + [dprog.buf, dout.buf])
            same(dout.result(), want, (oi, oo, plan))
            for d in din + [dprog, dout]:
                d.free()


def test_python_lstm_program_is_the_numpy_evaluator():
    r = rng(5)
    inputs = [r.integers(-32768, 32768, (2, 300)).astype(np.int16) for _ in range(5)]
    got = hp.elementwise(inputs, LSTM_PROGRAM, outputs=2)
    want = np_program(inputs, LSTM_PROGRAM, 2)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_checker_empty_program():
    """n = 0: the u8 variant returns slot 0 = 0, the i16 variant u8_sat(input 0) and 0, as the generator's output expression gives them"""
    r = rng(6)
    u = [r.integers(0, 256, (2, 9), dtype=np.uint8) for _ in range(5)]
    assert not hp.elementwise(u, np.zeros((0, 5), np.int16)).any()
    s = [r.integers(-32768, 32768, (2, 9)).astype(np.int16) for _ in range(5)]
    o0, o1 = hp.elementwise(s, np.zeros((0, 5), np.int16), outputs=2)
    assert np.array_equal(o0, np.clip(s[0], 0, 255).astype(np.uint8)) and not o1.any()
    with pytest.raises(ValueError):
        hp.elementwise(u, [[1, 1, 0, 0, 0]])


def run_ew_i16(hl, inputs, program, path="direct", out_strides=None):
    prog = hl.Buffer(np.ascontiguousarray(program, np.int16).reshape(-1, 5))
    rows, width = inputs[0].shape
    s0, s1 = out_strides or (width, width)
    o0 = np.full((rows, s0), 0x5A, np.uint8)
    o1 = np.full((rows, s1), 0x5A5A, np.int16)
    b0, b1 = hl.Buffer(o0[:, :width]), hl.Buffer(o1[:, :width])
    call(hl, "elementwise_5xint16_1xuint8int16", [hl.Buffer(a) for a in inputs] + [prog, b0, b1], path)
    b0.numpy(), b1.numpy()
    assert (o0[:, width:] == 0x5A).all() and (o1[:, width:] == 0x5A5A).all()
    return o0[:, :width].copy(), o1[:, :width].copy()


@gpu
@pytest.mark.parametrize("rows", [1, 5])
def test_hip_lstm_program_is_the_checker(hl, switches, rows):
    for width in (1, 7, 8, 9, 64, 130, 1000):
        r = rng(width + rows)
        inputs = [r.integers(-32768, 32768, (rows, width)).astype(np.int16) for _ in range(5)]
        col = r.integers(-32768, 32768, (rows, 1)).astype(np.int16)
        broadcast = inputs[:4] + [np.lib.stride_tricks.as_strided(col, shape=(rows, width), strides=(col.strides[0], 0), writeable=False)]
        for what, ins, strides in (("dense", inputs, None), ("stride0", broadcast, None), ("padded", inputs, (width + 5, width + 3))):
            want = hp.elementwise(ins, LSTM_PROGRAM, outputs=2)
            for plan, kernel in ((None, "hannk_prog_general"), (PLAN_LDS, "hannk_prog_interp"), (PLAN_REG, "hannk_prog_interp"), (PLAN_GENERAL, "hannk_prog_general")):
                switches(**({} if plan is None else {"EW_PLAN": plan}))
                got = [None]
                names = launches(hl, lambda: got.__setitem__(0, run_ew_i16(hl, ins, LSTM_PROGRAM, out_strides=strides)))
                assert names == [kernel], (plan, names)
                same(got[0][0], want[0], (what, rows, width, plan, "activation"))
                same(got[0][1], want[1], (what, rows, width, plan, "state"))
            switches()
            for path in ("general", "argv"):
                got = run_ew_i16(hl, ins, LSTM_PROGRAM, path, strides)
                same(got[0], want[0], (what, path)), same(got[1], want[1], (what, path))


@gpu
def test_hip_elementwise_edges(hl, switches):
    """the empty program, 20 instructions, Noop and an unknown opcode, on every plan"""
    u = u8_inputs(2, 37, 9)
    s = [rng(10 + k).integers(-32768, 32768, (2, 37)).astype(np.int16) for k in range(5)]
    twenty = [[1, -1, 0, 1, 0]] + [[1, k, 0, 1, 0] for k in range(1, 20)]
    for program in (np.zeros((0, 5), np.int16), twenty, [[0, 99, -99, 0, 0], [11, 77, -77, 5, 5]], [[1, -1, -2, 0, 0], [0, 0, 0, 0, 0]]):
        for plan in (None, PLAN_TABLE, PLAN_LDS, PLAN_REG):
            switches(**({} if plan is None else {"EW_PLAN": plan}))
            same(run_ew_u8(hl, u, program), hp.elementwise(u, program), (plan, "u8"))
            got, want = run_ew_i16(hl, s, program), hp.elementwise(s, program, outputs=2)
            same(got[0], want[0], (plan, "i16.0")), same(got[1], want[1], (plan, "i16.1"))
    switches()
    with pytest.raises(hl.HalideError) as e:
        run_ew_u8(hl, u, twenty + [[1, 20, 0, 1, 0]])
    assert e.value.code == -2
    with pytest.raises(hl.HalideError) as e:   # the operand refusal where only the device holds the program
        dprog = DevTensor(hl, (1, 5), dtype=np.int16, fill=np.array([[1, 1, 0, 0, 0]], np.int16))
        call(hl, "elementwise_5xuint8_1xuint8", [hl.Buffer(a) for a in u] + [dprog.buf, hl.Buffer(np.zeros((2, 37), np.uint8))])
    assert e.value.code == -8
    dprog.free()


@gpu
def test_hip_table_plan_threshold(hl, switches):
    """262 144 outputs: the byte table; one fewer, or a program that names two inputs: one thread per output"""
    program = hl.hannk_logistic_program(0.05, 120)
    for n, prog, kernel in ((1 << 18, program, "hannk_prog_table"), ((1 << 18) - 1, program, "hannk_prog_general"), (1 << 18, ADD_CLAMP, "hannk_prog_general")):
        x = rng(n & 7).integers(0, 256, (1, n), dtype=np.uint8)
        got = [None]
        assert launches(hl, lambda: got.__setitem__(0, run_ew_u8(hl, [x] * 5, prog))) == [kernel], n
        same(got[0], hp.elementwise([x] * 5, prog), (n, kernel))


def move_paths(hl, switches, name, make_args, want, what, kernel="hannk_move_general"):
    """the default (`kernel`: the 16-byte kernel where the layout allows one), the forced general kernel, hlmi_hannk_general and _argv"""
    general = "hannk_move_general"
    for path, sw, expect in (("direct", {}, kernel), ("direct", {"MOVE_VECTOR": 1}, kernel), ("direct", {"MOVE_VECTOR": 0}, general), ("general", {}, general),
                             ("argv", {}, kernel)):
        switches(**sw)
        args, read = make_args()
        names = launches(hl, lambda: call(hl, name, args, path))
        same(read(), want, (name, what, path, sw))
        assert names == [expect], (what, path, sw, names)
    switches()


@gpu
def test_hip_copy_is_the_checker(hl, switches):
    r = rng(21)
    # 3 -> 4 channels interleaved (PadOp's special case), odd width: rows of pixels
    inp = r.integers(0, 256, (2, 5, 37, 3), dtype=np.uint8)
    want = hp.copy(inp, (4, 37, 5, 2), 300)
    assert (want[..., 3] == 44).all()

    def make34():
        out = hl.Buffer(np.full((2, 5, 37, 4), 0x5A, np.uint8))
        return [hl.Buffer(inp.copy()), 300, out], lambda: out.numpy().copy()
    move_paths(hl, switches, "copy_uint8_uint8", make34, want, "3 -> 4", "hannk_rows16")
    # equal channels, a window of the input
    inp2 = r.integers(0, 256, (2, 6, 19, 24), dtype=np.uint8)
    want2 = hp.copy(inp2, (24, 19, 4, 2), 9, out_mins=(0, 0, 1, 0))
    assert np.array_equal(want2, inp2[:, 1:5])

    def make_eq():
        out = hl.Buffer(np.full((2, 4, 19, 24), 0x5A, np.uint8), mins=(0, 0, 1, 0))
        return [hl.Buffer(inp2.copy()), 9, out], lambda: out.numpy().copy()
    move_paths(hl, switches, "copy_uint8_uint8", make_eq, want2, "equal", "hannk_rows16")
    # 5 -> 16 channels with a channel min offset: padded on both sides of dimension 0
    inp3 = r.integers(0, 256, (1, 3, 7, 5), dtype=np.uint8)
    want3 = hp.copy(inp3, (16, 7, 3, 1), 200, in_mins=(2, 0, 0, 0), out_mins=(-1, 0, 0, 0))
    assert (want3[..., :3] == 200).all() and np.array_equal(want3[..., 3:8], inp3) and (want3[..., 8:] == 200).all()

    def make516():
        out = hl.Buffer(np.full((1, 3, 7, 16), 0x5A, np.uint8), mins=(-1, 0, 0, 0))
        return [hl.Buffer(inp3.copy(), mins=(2, 0, 0, 0)), 200, out], lambda: out.numpy().copy()
    move_paths(hl, switches, "copy_uint8_uint8", make516, want3, "5 -> 16", "hannk_move_general")
    # an unaligned crop on the device: both buffers off alignment, rows with gaps, sentinels around the output
    for oi, oo in ((0, 0), (1, 3), (16, 16), (5, 0)):
        for sw in ({"MOVE_VECTOR": 1}, {"MOVE_VECTOR": 0}):
            switches(**sw)
            din = DevTensor(hl, (2, 6, 19, 24), strides=(6 * 19 * 24 + 64, 19 * 24 + 16, 24, 1), offset=oi, fill=inp2)
            dout = DevTensor(hl, (2, 4, 19, 24), strides=(4 * 20 * 24 + 48, 20 * 24, 24, 1), offset=oo, mins=(0, 0, 1, 0))
            call(hl, "copy_uint8_uint8", [din.buf, 9, dout.buf])
            same(dout.result(), want2, ("crop", oi, oo, sw))
            din.free(), dout.free()
    switches()


@gpu
@pytest.mark.parametrize("channels", [1, 3, 4, 17, 64])
def test_hip_fill_is_the_value(hl, switches, channels):
    shape = (2, 3, 5, channels)
    want = np.full(shape, 201, np.uint8)

    def make():
        out = hl.Buffer(np.full(shape, 0x5A, np.uint8))
        return [201, out], lambda: out.numpy().copy()
    move_paths(hl, switches, "fill_uint8", make, want, channels, "hannk_rows16")
    for offset in (0, 1, 16):
        for sw in ({"MOVE_VECTOR": 1}, {"MOVE_VECTOR": 0}):
            switches(**sw)
            dout = DevTensor(hl, shape, strides=(3 * 6 * (channels + 3) + 7, 6 * (channels + 3), channels + 3, 1), offset=offset)
            call(hl, "fill_uint8", [201, dout.buf])
            same(dout.result(), want, (channels, offset, sw))
            dout.free()
    switches()


@gpu
@pytest.mark.parametrize("channels", [1, 3, 16, 20])
@pytest.mark.parametrize("factor", [1, 2, 3, 8, 16])
def test_hip_upsample_is_the_checker(hl, switches, factor, channels):
    inp = rng(factor * 100 + channels).integers(0, 256, (2, 3, 5, channels), dtype=np.uint8)
    want = hp.upsample_channels(inp, factor, (channels * factor, 5, 3, 2))
    assert np.array_equal(want, np.repeat(inp, factor, axis=3))

    def make():
        out = hl.Buffer(np.full(want.shape, 0x5A, np.uint8))
        return [hl.Buffer(inp.copy()), factor, out], lambda: out.numpy().copy()
    move_paths(hl, switches, "upsample_channels_uint8", make, want, (factor, channels), "hannk_upsample16")
    # a channel window that starts off a multiple of the factor, on the device, off alignment
    oc = max(channels * factor - 3, 1)
    want = hp.upsample_channels(inp, factor, (oc, 5, 3, 2), out_mins=(1, 0, 0, 0)) if channels * factor > 1 else None
    if want is not None:
        for sw in ({"MOVE_VECTOR": 1}, {"MOVE_VECTOR": 0}):
            switches(**sw)
            din = DevTensor(hl, inp.shape, offset=1, fill=inp)
            dout = DevTensor(hl, want.shape, strides=(3 * 5 * (oc + 2) + 3, 5 * (oc + 2), oc + 2, 1), offset=2, mins=(1, 0, 0, 0))
            call(hl, "upsample_channels_uint8", [din.buf, factor, dout.buf])
            same(dout.result(), want[:, :, :, :oc], (factor, channels, sw))
            din.free(), dout.free()
    switches()


@gpu
def test_hip_upsample_factor_zero(hl, switches):
    inp = rng(3).integers(0, 256, (1, 2, 3, 4), dtype=np.uint8)
    want = hp.upsample_channels(inp, 0, (9, 3, 2, 1))

    def make():
        out = hl.Buffer(np.full(want.shape, 0x5A, np.uint8))
        return [hl.Buffer(inp.copy()), 0, out], lambda: out.numpy().copy()
    move_paths(hl, switches, "upsample_channels_uint8", make, want, "factor 0", "hannk_upsample16")


@gpu
def test_hip_table_takes_several_chunks_per_lane(hl, switches):
    """16 M elements and a ragged tail: each lane of the table kernel takes 4 chunks; the expectation is the checker's table of the 256 bytes"""
    program = hl.hannk_tanh_program(0.02, 131)
    table = hp.elementwise([np.arange(256, dtype=np.uint8).reshape(1, 256)] * 5, program)[0]
    x = rng(16).integers(0, 256, (1, (1 << 24) + 37), dtype=np.uint8)
    got = [None]
    assert launches(hl, lambda: got.__setitem__(0, run_ew_u8(hl, [x] * 5, program))) == ["hannk_prog_table"]
    same(got[0], table[x], "16 M")


SHALLOW_CASES = {"3x3": dict(fw=3, fh=3, sy=1, dil=(1, 1)), "5x5": dict(fw=5, fh=5, sy=1, dil=(1, 1)), "3x3_sy2_dil2": dict(fw=3, fh=3, sy=2, dil=(2, 2))}


@gpu
@pytest.mark.parametrize("case", sorted(SHALLOW_CASES))
@pytest.mark.parametrize("d", [1, 2, 4, 8, 16])
def test_hip_shallow_is_the_checker_and_the_unfused_depthwise(hl, monkeypatch, d, case):
    k, q = SHALLOW_CASES[case], SHALLOW_Q
    for w in (16 // d + (k["fw"] - 1) * k["dil"][0], 21):   # an output whose fused row is exactly 16 wide, and an odd one
        h = 13
        inp, filt, bias = shallow_data(d * 10 + w, d, w, h, k["fw"], k["fh"])
        ow, oh = w - (k["fw"] - 1) * k["dil"][0], (h - 1 - (k["fh"] - 1) * k["dil"][1]) // k["sy"] + 1
        want = hp.depthwise_shallow(inp.reshape(2, h, w * d), filt, bias, ow * d, oh, k["sy"], k["dil"], d, **q)
        unfused = hl.hannk_depthwise_conv2d(inp, filt, bias, q["input_zero"], q["filter_zero"], (1, k["sy"]), k["dil"], 0, q["multiplier"], q["shift"], q["zero"],
                                            q["lo"], q["hi"])
        same(unfused.reshape(2, oh, ow * d), want, (d, case, w, "unfused depthwise_conv_uint8"))
        monkeypatch.delenv("HLMI_HANNK_DW_VECTOR", raising=False)
        same(hl.hannk_depthwise_conv2d_shallow(inp, filt, bias, q["input_zero"], q["filter_zero"], (1, k["sy"]), k["dil"], 0, q["multiplier"], q["shift"], q["zero"],
                                               q["lo"], q["hi"]).reshape(2, oh, ow * d), want, (d, case, w, "convenience"))
        # the dword kernel takes a fused row only where its length, the row strides and every tap offset are multiples of 4
        vector_ok = (ow * d) % 4 == 0 and (k["dil"][0] * d) % 4 == 0 and (w * d) % 4 == 0
        for path, forced, kernel in (("direct", None, "hannk_dw_general"), ("direct", 1, "hannk_dw" if vector_ok else "hannk_dw_general"),
                                     ("direct", 0, "hannk_dw_general"), ("general", 1, "hannk_dw_general"), ("argv", 1, "hannk_dw" if vector_ok else "hannk_dw_general")):
            monkeypatch.delenv("HLMI_HANNK_DW_VECTOR", raising=False)
            if forced is not None:
                monkeypatch.setenv("HLMI_HANNK_DW_VECTOR", str(forced))
            out = hl.Buffer(np.full((2, oh, 1, ow * d), 0x5A, np.uint8))
            args = [hl.Buffer(inp.reshape(2, h, 1, w * d).copy()), q["input_zero"], hl.Buffer(filt), q["filter_zero"], hl.Buffer(bias), 1, k["sy"], k["dil"][0],
                    k["dil"][1], d, q["multiplier"], q["shift"], q["zero"], q["lo"], q["hi"], out]
            names = launches(hl, lambda: call(hl, "depthwise_conv_shallow_uint8", args, path))
            same(out.numpy().reshape(2, oh, ow * d), want, (d, case, w, path, forced))
            assert names == [kernel], (d, case, w, path, forced, names)


@gpu
def test_hip_shallow_unaligned_device_buffers_and_a_filter_off_step(hl, monkeypatch):
    """device buffers 1 - 3 bytes off alignment inside sentinels with padded rows (the dword kernel may not take them), and D = 3, whose
    filter repeats at (c % 16) % 3"""
    q, h = SHALLOW_Q, 9
    for d, w in ((4, 12), (3, 11)):
        inp, filt, bias = shallow_data(d + w, d, w, h, 3, 3)
        ow, oh = w - 2, h - 2
        want = hp.depthwise_shallow(inp.reshape(2, h, w * d), filt, bias, ow * d, oh, 1, (1, 1), d, **q)
        for oi, oo, pad in ((0, 0, 0), (1, 0, 0), (0, 3, 0), (2, 2, 4), (0, 0, 4), (0, 0, 3)):
            for forced in (None, 1):
                monkeypatch.delenv("HLMI_HANNK_DW_VECTOR", raising=False)
                if forced is not None:
                    monkeypatch.setenv("HLMI_HANNK_DW_VECTOR", str(forced))
                row = w * d + pad
                din = DevTensor(hl, (2, h, 1, w * d), strides=(h * row + pad, row, row, 1), offset=oi, fill=inp.reshape(2, h, 1, w * d))
                dout = DevTensor(hl, (2, oh, 1, ow * d), strides=(oh * (ow * d + 5) + 1, ow * d + 5, ow * d + 5, 1), offset=oo)
                call(hl, "depthwise_conv_shallow_uint8", [din.buf, q["input_zero"], hl.Buffer(filt), q["filter_zero"], hl.Buffer(bias), 1, 1, 1, 1, d, q["multiplier"],
                                                         q["shift"], q["zero"], q["lo"], q["hi"], dout.buf])
                same(dout.result().reshape(2, oh, ow * d), want, (d, oi, oo, pad, forced))
                din.free(), dout.free()


@gpu
@pytest.mark.parametrize("width", [16, 32])
def test_hip_program_helpers_over_random_arguments(hl, width):
    r = rng(width)
    n = 1 << 20
    x, q, q_x = r.integers(-32768, 32768, n), r.integers(0, 16, n), r.integers(0, 16, n)
    x[:5] = CORNERS
    for fn in ("approx_log2p1_exp2", "approx_log2m1_exp2", "approx_logistic", "approx_tanh"):
        qq = np.minimum(q, 13) if "log2" in fn else q   # approx_log2 in Int(16) shifts its polynomial right: q < 14
        same(hl.debug_hannk_program_approx(fn, x, qq, q_x, width), hp.approx(fn, x, qq, q_x, width), (fn, width))


@gpu
def test_hip_conveniences_are_the_direct_calls(hl, switches):
    x = rng(31).integers(0, 256, (2, 5, 7, 6), dtype=np.uint8)
    flat = x.reshape(-1, 6)
    same(hl.hannk_logistic(x, 0.04, 99), hp.elementwise([flat] * 5, hl.hannk_logistic_program(0.04, 99)).reshape(x.shape), "logistic")
    same(hl.hannk_tanh(x, 0.04, 99), hp.elementwise([flat] * 5, hl.hannk_tanh_program(0.04, 99)).reshape(x.shape), "tanh")
    a, b = x, x[:, :, :, :1]   # the second operand broadcasts along the innermost axis: passed with a stride of 0
    bb = np.ascontiguousarray(np.broadcast_to(b, a.shape)).reshape(-1, 6)
    same(hl.hannk_elementwise([a, b], ADD_CLAMP), hp.elementwise([flat, bb, bb, bb, bb], ADD_CLAMP).reshape(a.shape), "elementwise")
    s = [rng(40 + k).integers(-32768, 32768, (3, 50)).astype(np.int16) for k in range(5)]
    got, want = hl.hannk_lstm_elementwise(*s), hp.elementwise(s, LSTM_PROGRAM, outputs=2)
    same(got[0], want[0], "lstm activation"), same(got[1], want[1], "lstm state")
    for c_pad in ((0, 1), (2, 3)):   # 3 -> 4 channels through the copy itself, and a general channel pad through fill
        img = rng(50).integers(0, 256, (2, 4, 5, 3), dtype=np.uint8)
        pads = ((0, 0), (1, 2), (2, 0), c_pad)
        same(hl.hannk_pad(img, pads, 77), np.pad(img, pads, constant_values=77), ("pad", c_pad))
    same(hl.hannk_pad(x[0, 0], ((1, 1), (0, 0)), 3), np.pad(x[0, 0], ((1, 1), (0, 0)), constant_values=3), "pad rank 2")
    same(hl.hannk_upsample_channels(x, 4), np.repeat(x, 4, axis=3), "upsample")


@gpu
def test_hip_torch_ops_are_the_direct_calls(hl):
    import torch
    import halide_amd.torch_ops  # noqa: F401
    ops = torch.ops.hlmi
    x = rng(61).integers(0, 256, (2, 5, 7, 6), dtype=np.uint8)
    t = torch.from_numpy(x).cuda()
    same(ops.hannk_logistic(t, 0.04, 99).cpu().numpy(), hl.hannk_logistic(x, 0.04, 99), "logistic")
    same(ops.hannk_tanh(t, 0.04, 99).cpu().numpy(), hl.hannk_tanh(x, 0.04, 99), "tanh")
    got = ops.hannk_elementwise([t, t[:, :, :, :1]], torch.tensor(ADD_CLAMP, dtype=torch.int16))
    assert len(got) == 1
    same(got[0].cpu().numpy(), hl.hannk_elementwise([x, x[:, :, :, :1]], ADD_CLAMP), "elementwise")
    s = [rng(70 + k).integers(-32768, 32768, (3, 50)).astype(np.int16) for k in range(5)]
    got = ops.hannk_elementwise([torch.from_numpy(a).cuda() for a in s], torch.from_numpy(hl.hannk_lstm_program()))
    want = hl.hannk_lstm_elementwise(*s)
    same(got[0].cpu().numpy(), want[0], "lstm activation"), same(got[1].cpu().numpy(), want[1], "lstm state")
    img = torch.from_numpy(x[..., :3].copy()).cuda()
    for pads in ([0, 0, 1, 2, 2, 0, 0, 1], [1, 0, 0, 0, 3, 3, 2, 5]):
        want = np.pad(x[..., :3], [(pads[2 * a], pads[2 * a + 1]) for a in range(4)], constant_values=77)
        same(ops.hannk_pad(img, pads, 77).cpu().numpy(), want, ("pad", pads))
    same(ops.hannk_upsample_channels(t, 3).cpu().numpy(), np.repeat(x, 3, axis=3), "upsample")
