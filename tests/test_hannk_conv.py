"""The quantised convolution ops of apps/hannk's op library: tile_conv_filter_uint8, conv_u8_u8_u8, conv_u8_u8_i16, depthwise_conv_uint8 and
depthwise_conv_broadcast_uint8 (csrc/hannk_conv.hip).

The contract is integer only.  Three evaluators face each other:
  * the checker, tests/cpp/hannk_check.c behind hannk_checker.py: plain C loops over the tiled filter, as the contract is written;
  * a second evaluator written here with numpy int64 / Python integers and explicit wrapping, over the UNTILED filter;
  * the library: its default path (the i8 MFMA implicit GEMM with or without split-K, the four-channels-per-lane depthwise kernel), its
    general path (one thread per output) and the `_argv` form, compared byte for byte.
The CPU part holds the checker to the second evaluator, pins the epilogue's known answers, the two algebraic identities the kernels rest on and
the entry protocol; the GPU part holds the library to the checker on shapes chosen for what can go wrong.  Arrays are NHWC: the Halide
dimensions [c, x, y, b] reversed.

Which shapes those are is itself tested on the CPU: test_the_shapes_reach_every_variant restates the host's predicates and asserts that
the tables reach every instance of hannk_conv_mfma<VEC, SPLIT, I16>, hannk_dw<K3, BCAST> and hannk_dw_general<BCAST> and every class of
tails and split geometry; test_the_seeded_slice_reaches_the_kernels does the same for the 40 + 40 cases of scripts/fuzz_parity.py that
test_seeded_fuzz_slice runs.  The checker itself is held to float64 (test_checker_is_within_one_of_float64).  The layouts of aliased
tensors (an output or input that is a channel slice of wider pixels, filters with gaps, i16 rows off an 8-byte boundary) lie in device
allocations full of sentinels (parity_helpers.DevTensor): every byte outside the array proper must come back unchanged."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hannk_checker as hk
from parity_helpers import DevArray, DevTensor, HostArray, gpu_present, launches, load_fuzz_parity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
ACCS = (0, 1, -1, I32_MIN, I32_MAX)
MULTIPLIERS = (1 << 30, I32_MAX, I32_MIN, -(1 << 30))
SHIFTS = (-31, -1, 0, 1, 31)


# ------------------------------------------------------------------------------------------------------------------ the second evaluator
def wrap32(v):
    """int64 array or Python int -> the int32 it is modulo 2^32"""
    if isinstance(v, (int, np.integer)):
        v = int(v) & 0xffffffff
        return v - (1 << 32) if v >= 1 << 31 else v
    v = np.asarray(v, np.int64) & 0xffffffff
    return np.where(v >= 1 << 31, v - (1 << 32), v)


def py_multiply_2x_high(a, b):
    return min(max((int(a) * int(b) + (1 << 30)) >> 31, I32_MIN), I32_MAX)


def py_rounding_shift_right(a, s):
    a, s = int(a), int(s)
    if s > 0:
        return (a >> s) + ((a >> (s - 1)) & 1)
    return wrap32(a << -s)


def py_quantize_i16(acc, m, s):
    return min(max(py_rounding_shift_right(py_multiply_2x_high(acc, m), s), -32768), 32767)


def py_quantize_u8(acc, m, s, zero, lo, hi):
    v = min(py_quantize_i16(acc, m, s) + zero, 32767)
    v = min(max(v, 0), 255)
    return max(min(v, hi), lo)


def np_quantize(acc, m, s, zero=0, lo=0, hi=255, i16=False):
    """the epilogue over an int32-valued int64 array (every intermediate fits int64)"""
    acc = np.asarray(acc, np.int64)
    p = np.minimum((acc * int(m) + (1 << 30)) >> 31, I32_MAX)
    if s > 0:
        v = (p >> s) + ((p >> (s - 1)) & 1)
    else:
        v = wrap32(p << -s)
    q = np.clip(v, -32768, 32767)
    if i16:
        return q.astype(np.int16)
    u = np.clip(np.minimum(q + zero, 32767), 0, 255)
    return np.maximum(np.minimum(u, hi), lo).astype(np.uint8)


def np_conv_acc(inp, filt, bias, out_whb, stride, dilation, az, fz, origin=(0, 0), wrap=True):
    """inp (B, H, W, CP) with CP >= CI, filt (CO, FH, FW, CI) UNTILED, -> the wrapped int32 accumulators (OB, OH, OW, CO) as int64 (the exact
    sums where `wrap` is off); channels CI .. CP of the input meet filter_zero (the tiler's padding) and add nothing"""
    co, fh, fw, ci = filt.shape
    ow, oh, ob = out_whb
    acc = np.zeros((ob, oh, ow, co), np.int64) + np.asarray(bias, np.int64)[:co]
    f = filt.astype(np.int64) - fz
    for ry in range(fh):
        for rx in range(fw):
            ys = origin[1] + ry * dilation[1] + stride[1] * np.arange(oh)
            xs = origin[0] + rx * dilation[0] + stride[0] * np.arange(ow)
            a = inp[:ob][:, ys][:, :, xs][..., :ci].astype(np.int64) - az
            acc += np.einsum("byxi,oi->byxo", a, f[:, ry, rx, :])
    return wrap32(acc) if wrap else acc


def np_depthwise_acc(inp, filt, bias, out_whb, stride, dilation, az, fz, broadcast=False, wrap=True):
    fh, fw, c = filt.shape
    ow, oh, ob = out_whb
    acc = np.zeros((ob, oh, ow, c), np.int64) + np.asarray(bias, np.int64)[:c]
    for ry in range(fh):
        for rx in range(fw):
            ys = ry * dilation[1] + stride[1] * np.arange(oh)
            xs = rx * dilation[0] + stride[0] * np.arange(ow)
            a = inp[:ob][:, ys][:, :, xs].astype(np.int64) - az
            a = a[..., :1] if broadcast else a[..., :c]
            acc += a * (filt[ry, rx, :].astype(np.int64) - fz)
    return wrap32(acc) if wrap else acc


def in_extent(out, filt, stride, dilation):
    return (out - 1) * stride + (filt - 1) * dilation + 1


class Case:
    """random operands of one convolution; `cp` = the input's channel extent (a multiple of 4, of 16 for depthwise, 1 for the broadcast variant)"""

    def __init__(self, ci, co, fw, fh, stride, dilation, ow, oh, ob, seed, zeros=None, quant=None, depthwise=False, broadcast=False, data="noise",
                 bias="noise"):
        rng = np.random.default_rng(seed)
        self.ci, self.co, self.fw, self.fh, self.stride, self.dilation, self.out_whb = ci, co, fw, fh, stride, dilation, (ow, oh, ob)
        self.depthwise, self.broadcast = depthwise, broadcast
        self.az, self.fz = zeros if zeros is not None else (int(rng.integers(0, 256)), int(rng.integers(0, 256)))
        # multiplier, shift, zero, lo, hi: a scale that keeps most outputs inside the range, a few at its ends
        self.quant = quant if quant is not None else (int(rng.integers(1 << 29, 1 << 31)), int(rng.integers(6, 12)), int(rng.integers(0, 256)), 3, 250)
        iw, ih = in_extent(ow, fw, stride[0], dilation[0]), in_extent(oh, fh, stride[1], dilation[1])
        self.cp = 1 if broadcast else -(-ci // 16) * 16 if depthwise else -(-ci // 4) * 4
        fill = {"noise": None, "zeros": 0, "ones": 255}[data]
        gen = (lambda shape: rng.integers(0, 256, shape, dtype=np.uint8)) if fill is None else (lambda shape: np.full(shape, fill, np.uint8))
        self.inp = np.full((ob, ih, iw, self.cp), self.az, np.uint8)
        self.inp[..., :ci] = gen((ob, ih, iw, ci))
        self.filt = gen((fh, fw, co)) if depthwise else gen((co, fh, fw, ci))
        self.bias = {"noise": rng.integers(-(1 << 20), 1 << 20, co), "min": np.full(co, I32_MIN), "max": np.full(co, I32_MAX)}[bias].astype(np.int32)
        self.tiled = None if depthwise else hk.tile(self.filt, self.fz)

    def want(self, out_dtype=np.uint8):
        m, s, z, lo, hi = self.quant
        ext = [self.co] + list(self.out_whb)
        if self.depthwise:
            return hk.depthwise(self.inp, self.filt, self.bias, ext, self.stride, self.dilation, self.az, self.fz, m, s, z, lo, hi, self.broadcast)
        return hk.conv(self.inp, self.tiled, self.bias, ext, self.stride, self.dilation, self.az, self.fz, m, s, z, lo, hi, out_dtype)

    def second(self, out_dtype=np.uint8):
        m, s, z, lo, hi = self.quant
        if self.depthwise:
            acc = np_depthwise_acc(self.inp, self.filt, self.bias, self.out_whb, self.stride, self.dilation, self.az, self.fz, self.broadcast)
        else:
            acc = np_conv_acc(self.inp, self.filt, self.bias, self.out_whb, self.stride, self.dilation, self.az, self.fz)
        return np_quantize(acc, m, s, z, lo, hi, np.dtype(out_dtype) == np.dtype(np.int16))


CONV_SHAPES = {   # ci, co, fw, fh, stride, dilation, ow, oh, ob
    "one_block": (4, 16, 1, 1, (1, 1), (1, 1), 1, 1, 1),
    "padded_k_and_co": (3, 8, 3, 3, (2, 2), (1, 1), 9, 5, 2),
    "k_tail_2p5_tiles": (68, 40, 3, 3, (2, 1), (2, 1), 19, 3, 1),
    "long_k": (520, 16, 1, 1, (1, 1), (1, 1), 7, 1, 1),
    "vector_k": (32, 48, 3, 1, (1, 1), (1, 1), 37, 2, 1),     # ci % 16 == 0: the 16-byte fragment path, 2 pixel tiles and a tail
    # the rows test_the_shapes_reach_every_variant needs besides (q = fw * fh * ceil(ci / 4) channel quads, kb = ceil(q / 16) k-blocks)
    "vec_k_tail_plan_split": (80, 40, 3, 1, (1, 1), (1, 1), 7, 5, 1),    # 60 q, 4 kb: the plan splits in 2; a lane group of padding; 35 pixels; 3 co tiles
    "vec_c18_two_batches": (64, 18, 5, 1, (1, 1), (1, 1), 8, 4, 2),      # 80 q, 5 kb: forced 3 gives 2, 2, 1; C % 4 == 2; a wave tile per batch
    "c5_two_k_blocks": (6, 5, 3, 3, (1, 1), (1, 1), 10, 5, 1),           # 18 q, 2 kb: split only by force; 50 pixels
    "vec_one_k_block": (16, 32, 2, 2, (1, 1), (1, 1), 8, 4, 1),          # 16 q, exactly one k-block: never split; 32 pixels
}
DW_SHAPES = {     # c, fw, fh, stride, dilation, ow, oh, ob
    "c16_3x3": (16, 3, 3, (1, 1), (1, 1), 5, 5, 1),
    "c24_5x5_s2": (24, 5, 5, (2, 2), (1, 1), 11, 7, 2),
    "c7_1x1": (7, 1, 1, (1, 1), (1, 1), 6, 5, 1),
    "c20_3x3_d2": (20, 3, 3, (1, 1), (2, 2), 7, 6, 1),
    "c33_2x3_s12": (33, 2, 3, (1, 2), (1, 1), 5, 9, 2),       # a filter that is not square, more rows than a thread's four
    # C % 4 and OH % 4 both zero, or both not and two batches, under a 3 x 3 filter and under another
    "c8_3x3_oh4": (8, 3, 3, (1, 1), (1, 1), 5, 4, 1),
    "c7_3x3_oh5_b2": (7, 3, 3, (2, 1), (1, 1), 4, 5, 2),
    "c12_2x3_oh8": (12, 2, 3, (1, 1), (1, 2), 3, 8, 1),
    "c21_1x2_oh6_b2": (21, 1, 2, (1, 2), (1, 1), 5, 6, 2),
}


def conv_case(name, seed=0, **kw):
    ci, co, fw, fh, st, di, ow, oh, ob = CONV_SHAPES[name]
    return Case(ci, co, fw, fh, st, di, ow, oh, ob, seed, **kw)


def dw_case(name, seed=0, broadcast=False, **kw):
    c, fw, fh, st, di, ow, oh, ob = DW_SHAPES[name]
    return Case(1 if broadcast else c, c, fw, fh, st, di, ow, oh, ob, seed, depthwise=True, broadcast=broadcast, **kw)


# ------------------------------------------------------------------------------------------------------------------ the kernel instances
# What runs, as (row of CONV_SHAPES, HLMI_HANNK_SPLIT_K or None for the plan's own choice), and what each run reaches: the host's
# predicates (hannk_conv_plan, conv_stage_main, dw_entry in halide_amd/csrc/hannk_conv.hip) restated; the split count comes from the hook.
CONV_RUNS = [(name, None) for name in sorted(CONV_SHAPES)] + [
    ("vec_k_tail_plan_split", "1"), ("vec_c18_two_batches", "3"), ("c5_two_k_blocks", "2"), ("c5_two_k_blocks", "5"), ("long_k", "1"),
    ("k_tail_2p5_tiles", "3")]
DW_RUNS = [(name, broadcast, vector) for name in sorted(DW_SHAPES) for broadcast in (False, True) for vector in (None, "1")]
KB_QUADS, WAVE_PX, DW_ROWS, DW_MIN_THREADS = 16, 32, 4, 256 * 256


def conv_splits(hl, name, switch, monkeypatch, cus=256):
    """(splits, k-blocks) of the plan for a row under the switch"""
    ci, co, fw, fh, _, _, ow, oh, ob = CONV_SHAPES[name]
    quads = fw * fh * -(-ci // 4)
    monkeypatch.delenv("HLMI_HANNK_SPLIT_K", raising=False)
    if switch is not None:
        monkeypatch.setenv("HLMI_HANNK_SPLIT_K", switch)
    plan = hl.debug_hannk_conv_plan(ow * oh * ob, co, quads, cus)
    assert plan["mfma"]
    return plan["splits"], -(-quads // KB_QUADS)


def conv_classes(hl, name, switch, monkeypatch):
    ci, co, fw, fh, _, _, ow, oh, ob = CONV_SHAPES[name]
    cq, npix = -(-ci // 4), ow * oh * ob
    quads = fw * fh * cq
    splits, nkb = conv_splits(hl, name, switch, monkeypatch)
    vec, split = cq % 4 == 0, splits > 1
    got = {("instance", vec, split, i16) for i16 in (False, True)}
    got.add(("chosen by", "the plan" if switch is None else "the switch", vec, split))
    got.add("C % 16 == 0" if co % 16 == 0 else "C % 4 == 0 != C % 16" if co % 4 == 0 else "C % 4 != 0")
    if co % 4 and split:
        got.add("C % 4 != 0 under SPLIT")
    got.add("an odd count of co tiles" if -(-co // 16) % 2 else "an even count of co tiles")
    tail = npix % WAVE_PX
    got.add("pixel tail 0" if tail == 0 else "pixel tail 1..16" if tail <= 16 else "pixel tail 17..31")
    if ob > 1 and (ow * oh) % WAVE_PX:
        got.add("a wave tile crosses the batch boundary")
    got.add("k tail 0" if quads % KB_QUADS == 0 else "k tail")
    if vec and quads % KB_QUADS:       # CQ % 4 == 0: the tail is 4, 8 or 12 quads, the lane groups past it load nothing
        got.add("VEC, a lane group of padding")
    if split:
        per = -(-nkb // splits)
        assert splits == -(-nkb // per) and 0 < nkb - (splits - 1) * per <= per
        got.add("splits of equal length" if nkb == splits * per else "a shorter last split")
        if switch is not None and int(switch) > nkb:
            got.add("a forced count above the k-blocks")
        if quads % KB_QUADS:           # the last k-block is in the last split: it holds quads % 16 real quads and the padding
            got.add("a last split with real and padded k")
    return got


CONV_CLASSES = ([("instance", vec, split, i16) for vec in (False, True) for split in (False, True) for i16 in (False, True)]
                + [("chosen by", who, vec, split) for who in ("the plan", "the switch") for vec in (False, True) for split in (False, True)]
                + ["C % 16 == 0", "C % 4 == 0 != C % 16", "C % 4 != 0", "C % 4 != 0 under SPLIT", "an odd count of co tiles", "an even count of co tiles",
                   "pixel tail 0", "pixel tail 1..16", "pixel tail 17..31", "a wave tile crosses the batch boundary", "k tail 0", "k tail",
                   "VEC, a lane group of padding", "splits of equal length", "a shorter last split", "a forced count above the k-blocks",
                   "a last split with real and padded k"])


def dw_instance(name, broadcast, vector):
    """the kernel instance dw_entry launches for an aligned input: (launch name, template arguments)"""
    c, fw, fh, _, _, ow, oh, ob = DW_SHAPES[name]
    threads = -(-c // 4) * ow * -(-oh // DW_ROWS) * ob
    if vector != "0" and (vector is not None or threads >= DW_MIN_THREADS):
        return ("hannk_dw", (fw, fh) == (3, 3), broadcast)
    return ("hannk_dw_general", broadcast)


def dw_classes(name, broadcast, vector):
    c, _, _, _, _, _, oh, ob = DW_SHAPES[name]
    inst = dw_instance(name, broadcast, vector)
    return {(inst, "C % 4 == 0" if c % 4 == 0 else "C % 4 != 0"), (inst, "OH % 4 == 0" if oh % DW_ROWS == 0 else "OH % 4 != 0")} | ({(inst, "ob > 1")} if ob > 1 else set())


DW_INSTANCES = [("hannk_dw", k3, bcast) for k3 in (False, True) for bcast in (False, True)] + [("hannk_dw_general", bcast) for bcast in (False, True)]
DW_CLASSES = [(inst, what) for inst in DW_INSTANCES for what in ("C % 4 == 0", "C % 4 != 0", "OH % 4 == 0", "OH % 4 != 0", "ob > 1")]


def test_the_shapes_reach_every_variant(hl, monkeypatch):
    """the counterpart of test_resnet50.py's test of the same name: every instance of hannk_conv_mfma<VEC, SPLIT, I16> and of the
    depthwise kernels, and every class of sizes in which their tails, clamps and split ranges differ, has a run in the tables above"""
    reached = {}
    for name, switch in CONV_RUNS:
        for cls in conv_classes(hl, name, switch, monkeypatch):
            reached.setdefault(cls, []).append((name, switch))
    for name, broadcast, vector in DW_RUNS:
        for cls in dw_classes(name, broadcast, vector):
            reached.setdefault(cls, []).append((name, broadcast, vector))
    missing = [cls for cls in CONV_CLASSES + DW_CLASSES if not reached.get(cls)]
    assert not missing, missing
    assert set(reached) <= set(CONV_CLASSES + DW_CLASSES), set(reached) - set(CONV_CLASSES + DW_CLASSES)
    # the rows the issue names are what it says of them
    assert conv_splits(hl, "vec_k_tail_plan_split", None, monkeypatch) == (2, 4) and conv_splits(hl, "vec_c18_two_batches", "3", monkeypatch) == (3, 5)
    assert conv_splits(hl, "c5_two_k_blocks", "5", monkeypatch) == (2, 2) and conv_splits(hl, "c5_two_k_blocks", None, monkeypatch) == (1, 2)
    assert conv_splits(hl, "vec_one_k_block", None, monkeypatch) == (1, 1)


# ------------------------------------------------------------------------------------------------------------------ CPU: the checker
@pytest.mark.parametrize("name", sorted(CONV_SHAPES))
@pytest.mark.parametrize("out_dtype", [np.uint8, np.int16], ids=["u8", "i16"])
def test_checker_conv_is_the_second_evaluator(name, out_dtype):
    c = conv_case(name, seed=11)
    assert np.array_equal(c.want(out_dtype), c.second(out_dtype))


@pytest.mark.parametrize("name", sorted(DW_SHAPES))
def test_checker_depthwise_is_the_second_evaluator(name):
    c = dw_case(name, seed=12)
    assert np.array_equal(c.want(), c.second())
    b = Case(1, 20, 3, 3, (1, 1), (1, 1), 4, 3, 2, seed=13, depthwise=True, broadcast=True)
    assert np.array_equal(b.want(), b.second())


def test_checker_tiler_is_the_second_evaluator():
    rng = np.random.default_rng(3)
    for ci, co in ((3, 8), (68, 40)):
        f = rng.integers(0, 256, (co, 2, 3, ci), dtype=np.uint8)   # (co, fh, fw, ci)
        iz, oz = 200, 17
        cq, co16 = -(-ci // 4), -(-co // 16)
        got = hk.tile_filter(f, iz, oz, [4, 16, cq, co16, 3, 2])
        want = np.zeros((2, 3, co16, cq, 16, 4), np.uint8)
        for y in range(2):
            for x in range(3):
                full = np.full((co16 * 16, cq * 4), iz, np.int64)
                full[:co, :ci] = f[:, y, x, :]
                want[y, x] = ((full - iz + oz) & 0xff).reshape(co16, 16, cq, 4).transpose(0, 2, 1, 3)
        assert np.array_equal(got, want)
        assert (got[:, :, -1, :, co % 16:, :] == oz).all() and (ci % 4 == 0 or (got[:, :, :, -1, :, ci % 4:] == oz).all())   # the padding is output_zero


def test_checker_quantize_is_the_second_evaluator():
    rng = np.random.default_rng(5)
    acc = np.concatenate([rng.integers(I32_MIN, I32_MAX, 4096), np.array(ACCS)]).astype(np.int32)
    for m in MULTIPLIERS + (1518500250,):
        for s in SHIFTS + (7,):
            assert np.array_equal(hk.quantize("i16", acc, m, s), np_quantize(acc, m, s, i16=True)), (m, s)
            assert np.array_equal(hk.quantize("u8", acc, m, s, 128, 10, 240), np_quantize(acc, m, s, 128, 10, 240)), (m, s)


def test_epilogue_known_answers():
    """every (acc, multiplier, shift) of the issue's list against Python integers, and the values that can be worked out by hand"""
    for a in ACCS:
        for m in MULTIPLIERS:
            assert hk.multiply_2x_high(a, m) == py_multiply_2x_high(a, m)
            for s in SHIFTS:
                assert hk.quantize_i16(a, m, s) == py_quantize_i16(a, m, s), (a, m, s)
                for zero, lo, hi in ((0, 0, 255), (128, 0, 255), (255, 20, 200), (3, 200, 100)):
                    assert hk.quantize_and_relu_u8(a, m, s, zero, lo, hi) == py_quantize_u8(a, m, s, zero, lo, hi), (a, m, s, zero, lo, hi)
    # multiply_2x_high: 2^30 is one half; the one saturating product; the most negative that does not saturate
    assert hk.multiply_2x_high(1, 1 << 30) == 1          # (2^30 + 2^30) >> 31: one half rounds up
    assert hk.multiply_2x_high(-1, 1 << 30) == 0         # (-2^30 + 2^30) >> 31
    assert hk.multiply_2x_high(I32_MIN, I32_MIN) == I32_MAX
    assert hk.multiply_2x_high(I32_MIN, I32_MAX) == -I32_MAX
    assert hk.multiply_2x_high(I32_MAX, I32_MAX) == I32_MAX - 1
    # rounding_shift_right: ties go up, a negative shift is a wrapping left shift
    assert [hk.rounding_shift_right(v, 1) for v in (5, -5, 3, -3, I32_MAX)] == [3, -2, 2, -1, 1 << 30]
    assert hk.rounding_shift_right(I32_MIN, 31) == -1 and hk.rounding_shift_right(I32_MAX, 31) == 1 and hk.rounding_shift_right(1, 31) == 0
    assert hk.rounding_shift_right(3, -31) == I32_MIN and hk.rounding_shift_right(1, -1) == 2 and hk.rounding_shift_right(I32_MAX, -1) == -2
    # the whole epilogue: saturation to int16, the zero point added with saturation, u8, and a crossed min > max where min wins
    assert hk.quantize_i16(I32_MIN, I32_MIN, 0) == 32767 and hk.quantize_i16(I32_MIN, I32_MAX, 0) == -32768
    assert hk.quantize_i16(1000, 1 << 30, 1) == 250 and hk.quantize_i16(-1000, 1 << 30, 2) == -125
    assert hk.quantize_and_relu_u8(I32_MIN, I32_MIN, 0, 255, 0, 255) == 255
    assert hk.quantize_and_relu_u8(-1000, 1 << 30, 0, 10, 0, 255) == 0
    assert hk.quantize_and_relu_u8(100, 1 << 30, 0, 10, 0, 255) == 60
    assert hk.quantize_and_relu_u8(100, 1 << 30, 0, 10, 200, 100) == 200 and hk.quantize_and_relu_u8(1 << 20, 1 << 30, 0, 10, 200, 100) == 200


def test_four_term_expansion_is_the_direct_sum_modulo_2_32():
    """conv_generator.cpp:131-149 computes offset_c - filter_zero * sum_input + sum(input * filter) in int32; the contract states the direct
    sum.  K = 3 * 3 * 2048 of 255 * 255 is 1.2e9 and stays inside int32: the bias pushes the true sum over."""
    K = 3 * 3 * 2048
    a = np.full(K, 255, np.int64)
    f = np.full(K, 255, np.int64)
    rng = np.random.default_rng(9)
    for az, fz, bias in ((0, 0, I32_MAX), (1, 2, I32_MAX - 5), (255, 0, I32_MIN), (128, 128, I32_MAX), (0, 255, I32_MIN + 3)):
        for noise in (False, True):
            if noise:
                a, f = rng.integers(0, 256, K).astype(np.int64), rng.integers(0, 256, K).astype(np.int64)
            direct = bias + int(((a - az) * (f - fz)).sum())
            assert noise or az or fz or not I32_MIN <= direct <= I32_MAX, "the case must overflow"
            # the reference's terms, each wrapped where the generator's int32 wraps
            offset_c = wrap32(bias + wrap32(fz * az * K) - wrap32(int((f * az).sum())))
            convolved = wrap32(wrap32(offset_c - wrap32(fz * int(a.sum()))) + wrap32(int((a * f).sum())))
            assert convolved == wrap32(direct), (az, fz, bias, noise)


def test_recentring_identity():
    """sum (a - az)(f - fz) = sum a'f' - fz' sum a' - az' sum f' + K az' fz' with x' = x - 128 (the signed operands of the i8 MFMA), in
    wrapping 32-bit arithmetic, also where padded k (a' = f' = 0) is summed and only the real K enters the constant"""
    rng = np.random.default_rng(10)
    for K, pad in ((1, 63), (36, 28), (4680, 56)):
        for az, fz in ((0, 0), (255, 255), (128, 128), (1, 254), (int(rng.integers(0, 256)), int(rng.integers(0, 256)))):
            for fill in (None, 0, 255):
                a = rng.integers(0, 256, K).astype(np.int64) if fill is None else np.full(K, fill, np.int64)
                f = rng.integers(0, 256, K).astype(np.int64) if fill is None else np.full(K, 255 - fill, np.int64)
                direct = wrap32(int(((a - az) * (f - fz)).sum()))
                ap, fp = np.concatenate([a - 128, np.zeros(pad, np.int64)]), np.concatenate([f - 128, np.zeros(pad, np.int64)])
                azp, fzp = az - 128, fz - 128
                # as the kernel has them: byte sums of the padded fragments minus 128 per byte
                sa = int((ap + 128).sum()) - 128 * (K + pad)
                sf = int((fp + 128).sum()) - 128 * (K + pad)
                got = wrap32(wrap32(int((ap * fp).sum())) - wrap32(fzp * sa) - wrap32(azp * sf) + wrap32(K * azp * fzp))
                assert got == direct, (K, az, fz, fill)


def test_checker_is_within_one_of_float64(capsys):
    """Both evaluators above were written from one reading of the generator; this one is not.  On every row of CONV_SHAPES and DW_SHAPES,
    under random multipliers and every shift 0 .. 12, the checker's u8 and i16 results are within 1 of
    clip(round(acc * m / 2^(31 + s)) + zero), computed in float64 from the exact int64 sum, wherever that sum fits int32 (beyond it the
    contract wraps and the real quotient is another number).  The bound is derived: multiply_2x_high and the rounding shift each round
    to nearest, so the result is within 1/2 + 2^-(s + 1) <= 1 of the real quotient q (1/2 of it at s = 0, where nothing is shifted);
    round(q) is within 1/2 of q; the two integers are less than 2 apart.  (float64 holds acc * m to 2^-53 of its size, 2^-22 after the
    division: far from moving a rounding by a whole step.)"""
    rng = np.random.default_rng(77)
    worst, inside, compared = 0, {"u8": 0, "i16": 0}, 0
    for depthwise, names in ((False, sorted(CONV_SHAPES)), (True, sorted(DW_SHAPES))):
        for name in names:
            for s in range(13):
                m, zero = int(rng.integers(1 << 26, 1 << 31)), int(rng.integers(0, 256))
                c = (dw_case if depthwise else conv_case)(name, seed=100 + s, quant=(m, s, zero, 0, 255))
                acc = (np_depthwise_acc if depthwise else np_conv_acc)(c.inp, c.filt, c.bias, c.out_whb, c.stride, c.dilation, c.az, c.fz, wrap=False)
                fits = (acc >= I32_MIN) & (acc <= I32_MAX)
                real = np.rint(acc.astype(np.float64) * m / 2.0 ** (31 + s))
                for key, dt, z, lo, hi in (("u8", np.uint8, zero, 0, 255), ("i16", np.int16, 0, -32768, 32767)):
                    if depthwise and key == "i16":
                        continue
                    want = np.clip(real + z, lo, hi)
                    diff = np.abs(c.want(dt).astype(np.float64) - want)[fits]
                    worst = max(worst, int(diff.max()))
                    inside[key] += int(np.count_nonzero((want[fits] > lo) & (want[fits] < hi)))
                    compared += diff.size
    with capsys.disabled():
        print(f"\n  checker against float64: worst difference {worst} over {compared} results, {inside} of them strictly inside their range")
    assert inside["u8"] > 10000 and inside["i16"] > 10000, "the multipliers and shifts must leave results that are not clipped"
    assert worst <= 1


# ------------------------------------------------------------------------------------------------------------------ CPU: the fuzzer's cases
FUZZ_SEED, FUZZ_CASES = 20261021, 40


def test_the_fuzzer_has_the_cases():
    """scripts/fuzz_parity.py keeps the two cases, each as a draw that touches neither the library nor the device and a run"""
    src = open(os.path.join(ROOT, "scripts", "fuzz_parity.py")).read()
    for name in ("hannk_conv", "hannk_depthwise"):
        assert f"def fuzz_{name}(rng):" in src and f'CASES["{name}"] = fuzz_{name}' in src and f"def case_{name}" not in src
        assert f"def draw_{name}(rng):" in src and f"def run_{name}(d):" in src and f"return run_{name}(draw_{name}(rng))" in src
        draw = src.split(f"def draw_{name}(rng):")[1].split("\ndef ")[0]
        assert "hl." not in draw and "hk." not in draw and "import" not in draw, name


def drawn_cases(mod):
    """the parameters of test_seeded_fuzz_slice's cases, in its order"""
    r = np.random.default_rng(FUZZ_SEED)
    return [mod.draw_hannk_conv(r) for _ in range(FUZZ_CASES)], [mod.draw_hannk_depthwise(r) for _ in range(FUZZ_CASES)]


def test_the_seeded_slice_reaches_the_kernels(hl, monkeypatch):
    """conditions on the draw, not measurements: the 40 + 40 cases of the fixed seed hold every MFMA instance twice, the general conv
    four times, a sliced output eight times and each instance of hannk_dw once; and the draw's own restatement of the plan is the hook's"""
    conv, dw = drawn_cases(load_fuzz_parity())
    kernels = [d["kernel"] for d in conv]
    for vec in (False, True):
        for split in (False, True):
            for i16 in (False, True):
                assert kernels.count(("mfma", vec, split, i16)) >= 2, (vec, split, i16, kernels)
    assert kernels.count("general") >= 4
    assert sum(d["sliced_output"] for d in conv + dw) >= 8 and sum(d["sliced_output"] for d in conv) >= 4 and sum(d["sliced_output"] for d in dw) >= 4
    assert sum(d["ci"] % 16 == 0 for d in conv) >= 8 and sum(d["i16"] for d in conv) >= 10
    assert sum(d["in_pixel_stride"] > -(-d["ci"] // 4) * 4 for d in conv) >= 4
    dwk = [d["kernel"] for d in dw]
    for k3 in (False, True):
        for bcast in (False, True):
            assert dwk.count(("dw", k3, bcast)) >= 1, (k3, bcast, dwk)
    for d in conv:
        if not d["general"]:
            monkeypatch.delenv("HLMI_HANNK_SPLIT_K", raising=False)
            if d["split"] is not None:
                monkeypatch.setenv("HLMI_HANNK_SPLIT_K", str(d["split"]))
            ow, oh, ob = d["out"]
            assert hl.debug_hannk_conv_plan(ow * oh * ob, d["co"], d["fw"] * d["fh"] * -(-d["ci"] // 4))["splits"] == d["splits"], d


# ------------------------------------------------------------------------------------------------------------------ CPU: the entry protocol
def code_of(hl, fn):
    try:
        fn()
    except hl.HalideError as e:
        return e.code
    return 0


class ConvArgs:
    """valid host buffers of a small conv (ci 8, co 20, 3 x 2 filter, output 5 x 4 x 2), to be broken one field at a time"""

    def __init__(self, hl, i16=False):
        self.hl, self.i16 = hl, i16
        self.input = hl.Buffer(hl.aligned_array((2, 5, 7, 8), np.uint8, 64, 1))
        self.filter = hl.Buffer(hl.aligned_array((2, 3, 2, 2, 16, 4), np.uint8, 64, 1))
        self.bias = hl.Buffer(np.zeros(20, np.int32))
        self.output = hl.Buffer(np.zeros((2, 4, 5, 20), np.int16 if i16 else np.uint8))
        self.stride, self.dilation = (1, 1), (1, 1)

    def call(self):
        fn = self.hl.conv_u8_u8_i16 if self.i16 else self.hl.conv_u8_u8_u8
        return code_of(self.hl, lambda: fn(self.input, 3, self.filter, 5, self.bias, self.stride, self.dilation, 1 << 30, 1, 0, 0, 255, self.output))


class DwArgs:
    def __init__(self, hl, broadcast=False):
        self.hl, self.broadcast = hl, broadcast
        self.input = hl.Buffer(hl.aligned_array((2, 6, 7, 1 if broadcast else 32), np.uint8, 64, 1))
        self.filter = hl.Buffer(np.zeros((3, 3, 20), np.uint8))
        self.bias = hl.Buffer(np.zeros(20, np.int32))
        self.output = hl.Buffer(np.zeros((2, 4, 5, 20), np.uint8))

    def call(self):
        fn = self.hl.depthwise_conv_broadcast_uint8 if self.broadcast else self.hl.depthwise_conv_uint8
        return code_of(self.hl, lambda: fn(self.input, 3, self.filter, 5, self.bias, (1, 1), (1, 1), 1 << 30, 1, 0, 0, 255, self.output))


def set_dim(buf, d, **fields):
    for k, v in fields.items():
        setattr(buf._dims[d], k, v)


def test_protocol_valid_calls_reach_the_device(hl):
    """the baselines the broken calls below start from are accepted: with a GPU they run, without one they fail at the device (-29)"""
    ok = (0,) if gpu_present() else (-29,)
    assert ConvArgs(hl).call() in ok and ConvArgs(hl, True).call() in ok and DwArgs(hl).call() in ok and DwArgs(hl, True).call() in ok


@pytest.mark.parametrize("i16", [False, True], ids=["u8", "i16"])
def test_protocol_null_type_dimensions(hl, i16):
    for which in ("input", "filter", "bias", "output"):
        a = ConvArgs(hl, i16)
        setattr(a, which, None)
        assert a.call() == -12, which
    a = ConvArgs(hl, i16)
    a.filter = hl.Buffer(hl.aligned_array((2, 3, 2, 2, 16, 4), np.int8, 64, 1))
    assert a.call() == -3
    a = ConvArgs(hl, i16)
    a.output = hl.Buffer(np.zeros((2, 4, 5, 20), np.uint8 if i16 else np.int16))
    assert a.call() == -3
    a = ConvArgs(hl, i16)
    a.filter = hl.Buffer(hl.aligned_array((3, 2, 2, 16, 4), np.uint8, 64, 1))
    assert a.call() == -43
    a = ConvArgs(hl, i16)
    a.input = hl.Buffer(np.zeros((5, 7, 8), np.uint8))
    assert a.call() == -43


CONV_CONSTRAINTS = {
    "input.min.0": lambda a: set_dim(a.input, 0, min=4),
    "input.extent.0": lambda a: set_dim(a.input, 0, extent=4),
    "input.stride.1": lambda a: set_dim(a.input, 1, stride=6),
    "input.stride.2": lambda a: set_dim(a.input, 2, stride=57),
    "input.stride.3": lambda a: set_dim(a.input, 3, stride=282),
    "filter.min.0": lambda a: set_dim(a.filter, 0, min=1),
    "filter.extent.0": lambda a: set_dim(a.filter, 0, extent=2),
    "filter.min.1": lambda a: set_dim(a.filter, 1, min=1),
    "filter.extent.1": lambda a: set_dim(a.filter, 1, extent=8),
    "filter.stride.1": lambda a: set_dim(a.filter, 1, stride=8),
    "filter.min.2": lambda a: set_dim(a.filter, 2, min=1),
    "filter.stride.2": lambda a: set_dim(a.filter, 2, stride=128),
    "filter.min.3": lambda a: set_dim(a.filter, 3, min=-1),
    "filter.stride.3": lambda a: set_dim(a.filter, 3, stride=160),
    "filter.min.4": lambda a: set_dim(a.filter, 4, min=1),
    "filter.stride.4": lambda a: set_dim(a.filter, 4, stride=288),
    "filter.min.5": lambda a: set_dim(a.filter, 5, min=1),
    "filter.stride.5": lambda a: set_dim(a.filter, 5, stride=800),
    "bias.min.0": lambda a: set_dim(a.bias, 0, min=2),            # the output's min 0 is the bias's
    "bias.extent.0": lambda a: setattr(a, "bias", a.hl.Buffer(np.zeros(24, np.int32))),
    "bias.stride.0": lambda a: set_dim(a.bias, 0, stride=2),
    "output.min.0": lambda a: (set_dim(a.output, 0, min=16), set_dim(a.bias, 0, min=16)),   # equal mins, but not 0
    "output.stride.0": lambda a: set_dim(a.output, 0, stride=2),
    "output.min.3": lambda a: set_dim(a.output, 3, min=1),
    "output.extent.3": lambda a: set_dim(a.output, 3, extent=1),
}


@pytest.mark.parametrize("field", sorted(CONV_CONSTRAINTS))
def test_protocol_conv_constraints(hl, field):
    a = ConvArgs(hl, i16=field.startswith("filter"))
    CONV_CONSTRAINTS[field](a)
    assert a.call() == -8, field


def test_protocol_conv_alignment_and_regions(hl):
    a = ConvArgs(hl)
    raw = np.zeros(2 * 3 * 2 * 2 * 64 + 128, np.uint8)
    off = (-raw.ctypes.data) % 64 + 16                                      # 16 off a 64-byte boundary
    a.filter = hl.Buffer(raw[off:off + 2 * 3 * 2 * 2 * 64].reshape(2, 3, 2, 2, 16, 4))
    assert a.call() == -24
    a = ConvArgs(hl)
    raw = np.zeros(2 * 5 * 7 * 8 + 64, np.uint8)
    off = (-raw.ctypes.data) % 64 + 2                                       # the input's host alignment is 4
    a.input = hl.Buffer(raw[off:off + 2 * 5 * 7 * 8].reshape(2, 5, 7, 8))
    assert a.call() == -24
    a = ConvArgs(hl)
    a.input = hl.Buffer(hl.aligned_array((2, 5, 6, 8), np.uint8, 64, 1))    # x: 5 outputs under 3 taps need 7
    assert a.call() == -4
    a = ConvArgs(hl)
    a.input = hl.Buffer(hl.aligned_array((2, 4, 7, 8), np.uint8, 64, 1))    # y: 4 outputs under 2 taps need 5
    assert a.call() == -4
    a = ConvArgs(hl)
    a.stride = (2, 1)                                                       # the same input under stride 2: x up to 10
    assert a.call() == -4
    a = ConvArgs(hl)
    a.filter = hl.Buffer(hl.aligned_array((2, 3, 1, 2, 16, 4), np.uint8, 64, 1))   # 20 output channels need two co tiles
    assert a.call() == -4
    a = ConvArgs(hl)
    set_dim(a.input, 1, min=1)                                              # the input starts one pixel late
    assert a.call() == -4


def test_protocol_depthwise(hl):
    for which in ("input", "filter", "bias", "output"):
        a = DwArgs(hl)
        setattr(a, which, None)
        assert a.call() == -12, which
    a = DwArgs(hl)
    a.bias = hl.Buffer(np.zeros(20, np.float32))
    assert a.call() == -3
    a = DwArgs(hl)
    a.filter = hl.Buffer(np.zeros((3, 3, 1, 20), np.uint8))
    assert a.call() == -43
    broken = {
        "input.min.0": lambda a: set_dim(a.input, 0, min=1),
        "input.stride.1": lambda a: set_dim(a.input, 1, stride=24),
        "input.stride.2": lambda a: set_dim(a.input, 2, stride=232),
        "input.stride.3": lambda a: set_dim(a.input, 3, stride=1352),
        "filter.extent.0": lambda a: setattr(a, "filter", a.hl.Buffer(np.zeros((3, 3, 24), np.uint8))),
        "filter.min.1": lambda a: set_dim(a.filter, 1, min=1),
        "filter.min.2": lambda a: set_dim(a.filter, 2, min=-1),
        "bias.extent.0": lambda a: setattr(a, "bias", a.hl.Buffer(np.zeros(21, np.int32))),
        "output.min.0": lambda a: set_dim(a.output, 0, min=1),
        "output.extent.3": lambda a: set_dim(a.output, 3, extent=1),
    }
    for field, brk in broken.items():
        a = DwArgs(hl)
        brk(a)
        assert a.call() == -8, field
    a = DwArgs(hl, broadcast=True)
    a.input = hl.Buffer(hl.aligned_array((2, 6, 7, 2), np.uint8, 64, 1))
    assert a.call() == -8                                                   # the broadcast variant takes ONE input channel
    a = DwArgs(hl)
    a.input = hl.Buffer(hl.aligned_array((2, 6, 7, 16), np.uint8, 64, 1))    # 20 channels need the input to cover 32
    assert a.call() == -4
    a = DwArgs(hl)
    a.input = hl.Buffer(hl.aligned_array((2, 5, 7, 32), np.uint8, 64, 1))
    assert a.call() == -4
    a = DwArgs(hl)
    raw = np.zeros(2 * 6 * 7 * 32 + 64, np.uint8)
    off = (-raw.ctypes.data) % 64 + 4
    a.input = hl.Buffer(raw[off:off + 2 * 6 * 7 * 32].reshape(2, 6, 7, 32))
    assert a.call() == -24


def test_protocol_tile_filter(hl):
    def call(inp, out):
        return code_of(hl, lambda: hl.tile_conv_filter_uint8(inp, 1, 2, out))
    inp = lambda: hl.Buffer(np.zeros((20, 2, 3, 8), np.uint8))
    out = lambda: hl.Buffer(hl.aligned_array((2, 3, 2, 2, 16, 4), np.uint8, 64, 1))
    assert call(inp(), out()) in ((0,) if gpu_present() else (-29,))
    assert call(None, out()) == -12 and call(inp(), None) == -12
    assert call(hl.Buffer(np.zeros((20, 2, 3, 8), np.int8)), out()) == -3
    assert call(inp(), hl.Buffer(np.zeros((3, 2, 2, 16, 4), np.uint8))) == -43
    for d, fields in ((0, dict(min=1)), (0, dict(extent=2)), (1, dict(min=1)), (1, dict(extent=8)), (1, dict(stride=8)), (2, dict(min=1)),
                      (2, dict(stride=128))):
        o = out()
        set_dim(o, d, **fields)
        assert call(inp(), o) == -8, (d, fields)


def test_all_ones_queries_tell_the_tiling(hl):
    """what ConvOp::prepare and DepthwiseConv2DOp::prepare ask: every buffer unallocated, every extent 1"""
    q = lambda dt, nd: hl.Buffer.bounds_query(dt, nd, extents=[1] * nd)
    for fn, odt in ((hl.conv_u8_u8_u8, np.uint8), (hl.conv_u8_u8_i16, np.int16)):
        i, f, b, o = q(np.uint8, 4), q(np.uint8, 6), q(np.int32, 1), q(odt, 4)
        assert fn(i, 0, f, 0, b, (1, 1), (1, 1), 0, 0, 0, 0, 0, o) == 0
        assert f.extents[:2] == [hk.VECTOR_REDUCTION, hk.ACCUM_VECTOR_SIZE] == [4, 16] and f.dim(1).stride == 4 and f.dim(2).stride == 64
        assert i.extents[0] == 4
    i, f, b, o = q(np.uint8, 4), q(np.uint8, 3), q(np.int32, 1), q(np.uint8, 4)
    assert hl.depthwise_conv_uint8(i, 0, f, 0, b, (1, 1), (1, 1), 0, 0, 0, 0, 0, o) == 0
    assert i.extents[0] == hk.DEPTHWISE_VECTOR == 16
    i, f, b, o = q(np.uint8, 4), q(np.uint8, 3), q(np.int32, 1), q(np.uint8, 4)
    assert hl.depthwise_conv_broadcast_uint8(i, 0, f, 0, b, (1, 1), (1, 1), 0, 0, 0, 0, 0, o) == 0
    assert i.extents[0] == 1


def test_shaped_query_answers_input_and_bias(hl):
    """a shaped (unallocated) output and a real filter: the input and the bias get the regions the call would read"""
    f = hl.Buffer(hl.aligned_array((2, 3, 3, 17, 16, 4), np.uint8, 64, 1))           # fh 2, fw 3, 3 co tiles, 17 quads
    o = hl.Buffer.bounds_query(np.uint8, 4, mins=[0, 2, -1, 3], extents=[40, 19, 3, 2])
    i, b = hl.Buffer.bounds_query(np.uint8, 4), hl.Buffer.bounds_query(np.int32, 1)
    assert hl.conv_u8_u8_u8(i, 0, f, 0, b, (2, 1), (2, 3), 0, 0, 0, 0, 0, o) == 0
    assert i.mins == [0, 4, -1, 3] and i.extents == [68, 18 * 2 + 2 * 2 + 1, 2 + 3 + 1, 2]
    assert b.mins == [0] and b.extents == [40]
    assert all(i.dim(d).stride % 4 == 0 for d in (1, 2, 3))


def test_metadata(hl):
    conv_names = ["input", "input_zero", "filter", "filter_zero", "bias", "stride_x", "stride_y", "dilation_x", "dilation_y", "output_multiplier",
                  "output_shift", "output_zero", "output_min", "output_max", "output"]
    dw_names = conv_names[:9] + ["input_stride_x"] + conv_names[9:]
    u8, i32 = (1, 8), (0, 32)
    conv_types = [u8, u8, u8, u8, i32, i32, i32, i32, i32, i32, i32, u8, u8, u8, u8]
    conv_kinds = [1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2]
    expect = {
        "tile_conv_filter_uint8": (["input", "input_zero", "output_zero", "output"], [1, 0, 0, 2], [u8] * 4, [4, 0, 0, 6]),
        "conv_u8_u8_u8": (conv_names, conv_kinds, conv_types, None),
        "conv_u8_u8_i16": (conv_names, conv_kinds, conv_types[:-1] + [(0, 16)], None),
        "depthwise_conv_uint8": (dw_names, conv_kinds[:9] + [0] + conv_kinds[9:], conv_types[:9] + [i32] + conv_types[9:], None),
        "depthwise_conv_broadcast_uint8": (dw_names, conv_kinds[:9] + [0] + conv_kinds[9:], conv_types[:9] + [i32] + conv_types[9:], None),
    }
    assert tuple(expect) == hl.HANNK_OPS
    for name, (names, kinds, types, dims) in expect.items():
        md = hl.metadata(name)
        args = [md.arguments[k] for k in range(md.num_arguments)]
        assert md.version == 1 and md.name.decode() == name and b"hip" in md.target
        assert [a.name.decode() for a in args] == names and [a.kind for a in args] == kinds
        assert [(a.type.code, a.type.bits) for a in args] == types and all(a.type.reserved == 1 for a in args)
        if dims is None:
            dims = [{"input": 4, "filter": 3 if "depthwise" in name else 6, "bias": 1, "output": 4}.get(n, 0) for n in names]
        assert [a.dimensions for a in args] == dims
    for name in ("conv_u8_u8_u8", "conv_u8_u8_i16"):   # what ConvOp::filter_type reads
        t = hl.metadata(name).arguments[2].type
        assert (t.code, t.bits, t.reserved) == (1, 8, 1)


def test_plan_has_a_split_k_threshold(hl, monkeypatch):
    """few wave tiles (32 co x 32 pixels each) and a long k: k is split; enough tiles for every SIMD of 256 compute units, or a short
    k: it is not.  The switch forces either."""
    monkeypatch.delenv("HLMI_HANNK_SPLIT_K", raising=False)
    assert hl.debug_hannk_conv_plan(7, 16, 130) == {"mfma": True, "splits": 3, "wave_tiles": 1}
    assert hl.debug_hannk_conv_plan(7, 16, 16)["splits"] == 1                       # one k-block
    assert hl.debug_hannk_conv_plan(32 * 1023, 16, 130)["splits"] > 1 and hl.debug_hannk_conv_plan(32 * 1024, 16, 130)["splits"] == 1
    assert hl.debug_hannk_conv_plan(49, 1024, 256)["splits"] == 8                   # MobileNet's last pointwise layer at batch 1
    monkeypatch.setenv("HLMI_HANNK_SPLIT_K", "1")
    assert hl.debug_hannk_conv_plan(7, 16, 130)["splits"] == 1
    monkeypatch.setenv("HLMI_HANNK_SPLIT_K", "9")
    assert hl.debug_hannk_conv_plan(7, 16, 130)["splits"] == 9 and hl.debug_hannk_conv_plan(7, 16, 16)["splits"] == 1
    for setting, splits in (("0", 1), ("-3", 1), ("1000000", 9)):   # no split below 1; never more splits than the 9 k-blocks of 130 quads
        monkeypatch.setenv("HLMI_HANNK_SPLIT_K", setting)
        assert hl.debug_hannk_conv_plan(7, 16, 130)["splits"] == splits, setting


def test_consumer_builds_against_the_headers():
    """tests/cpp/hannk_consumer.cpp, written against halide/<name>.h, compiles and links with the host compiler against libhlmi.so"""
    exe = _build_consumer()
    assert os.path.exists(exe)


def _build_consumer():
    import tempfile
    out = os.path.join(tempfile.mkdtemp(prefix="hlmi_hannk_consumer"), "hannk_consumer")
    libdir = os.path.join(ROOT, "halide_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include", "aot"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "hannk_consumer.cpp"), "-o", out, "-L", libdir, "-lhlmi", f"-Wl,-rpath,{libdir}"], check=True)
    return out


# ------------------------------------------------------------------------------------------------------------------ GPU
gpu = pytest.mark.gpu


def conv_args(hl, c, inp, tiled, bias, out):
    m, s, z, lo, hi = c.quant
    return [inp, c.az, tiled, c.fz, bias, c.stride[0], c.stride[1], c.dilation[0], c.dilation[1]] + ([0] if c.depthwise else []) + [m, s, z, lo, hi, out]


def entry_name(c, out_dtype=np.uint8):
    if c.depthwise:
        return "depthwise_conv_broadcast_uint8" if c.broadcast else "depthwise_conv_uint8"
    return "conv_u8_u8_i16" if np.dtype(out_dtype) == np.dtype(np.int16) else "conv_u8_u8_u8"


def call_argv(hl, name, args):
    md = hl.metadata(name)
    keep, argv = [], (C.c_void_p * len(args))()
    for j, v in enumerate(args):
        a = md.arguments[j]
        box = v.raw if a.kind else (C.c_uint8(v) if a.type.bits == 8 else C.c_int32(v))
        keep.append(box)
        argv[j] = C.cast(C.pointer(box), C.c_void_p)
    fn = getattr(hl.lib, hl._symbol(name, "_argv"))
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(C.c_void_p)]
    return hl._check(fn(argv))


def run_all_paths(hl, c, out_dtype=np.uint8):
    """the direct call, the general path and `_argv` on fresh buffers: three dense arrays (OB, OH, OW, C)"""
    name = entry_name(c, out_dtype)
    ow, oh, ob = c.out_whb
    got = []
    for path in ("direct", "general", "argv"):
        inp = hl.Buffer(hl.aligned_array(c.inp.shape, np.uint8, 64, 1))
        inp.array[...] = c.inp
        if c.depthwise:
            filt = hl.Buffer(c.filt.copy())
        else:
            filt = hl.Buffer(hl.aligned_array(c.tiled.shape, np.uint8, 64, 1))
            filt.array[...] = c.tiled
        out = hl.Buffer(np.full((ob, oh, ow, c.co), 0x5A, out_dtype))
        args = conv_args(hl, c, inp, filt, hl.Buffer(c.bias.copy()), out)
        if path == "direct":
            hl._check(hl._fn[name](*[a.ptr if isinstance(a, hl.Buffer) else a for a in args]))
        elif path == "general":
            hl.debug_hannk_general(name, *args)
        else:
            call_argv(hl, name, args)
        got.append(out.numpy().copy())
    return got


def assert_all_paths(hl, c, out_dtype=np.uint8, what=""):
    want = c.want(out_dtype)
    for path, got in zip(("direct", "general", "argv"), run_all_paths(hl, c, out_dtype)):
        bad = got != want
        assert not bad.any(), f"{what} {path}: {np.count_nonzero(bad)} of {got.size} differ, first at {tuple(np.argwhere(bad)[0])}"


@gpu
@pytest.mark.parametrize("name", sorted(CONV_SHAPES))
@pytest.mark.parametrize("out_dtype", [np.uint8, np.int16], ids=["u8", "i16"])
def test_hip_conv_is_the_checker(hl, name, out_dtype, monkeypatch):
    monkeypatch.delenv("HLMI_HANNK_SPLIT_K", raising=False)
    assert_all_paths(hl, conv_case(name, seed=21), out_dtype, name)


@gpu
def test_hip_conv_runs_the_mfma_kernel_and_splits_k(hl, monkeypatch):
    """the default path is the MFMA kernel; on both sides of the plan's split-K threshold (the plan's own choice for the long k, the
    switch for the other side and for more splits than the plan would take) the bytes are the checker's"""
    c = conv_case("long_k", seed=22)
    want = c.want()
    monkeypatch.delenv("HLMI_HANNK_SPLIT_K", raising=False)
    assert hl.debug_hannk_conv_plan(7, 16, 130)["splits"] > 1
    for setting, names in ((None, ["hannk_conv_finish", "hannk_conv_mfma"]), ("1", ["hannk_conv_mfma"]), ("2", ["hannk_conv_finish", "hannk_conv_mfma"]),
                           ("9", ["hannk_conv_finish", "hannk_conv_mfma"])):
        if setting is not None:
            monkeypatch.setenv("HLMI_HANNK_SPLIT_K", setting)
        inp, filt = hl.Buffer(hl.aligned_array(c.inp.shape, np.uint8, 64, 1)), hl.Buffer(hl.aligned_array(c.tiled.shape, np.uint8, 64, 1))
        inp.array[...], filt.array[...] = c.inp, c.tiled
        out = hl.Buffer(np.zeros((1, 1, 7, 16), np.uint8))
        args = conv_args(hl, c, inp, filt, hl.Buffer(c.bias.copy()), out)
        ran = launches(hl, lambda: hl._check(hl._fn["conv_u8_u8_u8"](*[a.ptr if isinstance(a, hl.Buffer) else a for a in args])))
        assert ran == names, (setting, ran)
        assert np.array_equal(out.numpy(), want), setting
    monkeypatch.delenv("HLMI_HANNK_SPLIT_K")
    c = conv_case("k_tail_2p5_tiles", seed=23)     # a k tail inside the last split
    want = c.want(np.int16)
    for setting in ("3", "5"):
        monkeypatch.setenv("HLMI_HANNK_SPLIT_K", setting)
        assert np.array_equal(run_all_paths(hl, c, np.int16)[0], want), setting


ZERO_POINTS = (0, 1, 128, 255)


@gpu
@pytest.mark.parametrize("data", ["zeros", "ones"])
def test_hip_conv_constant_operands_and_zero_points(hl, data):
    """all-0 and all-255 operands under every pair of zero points of {0, 1, 128, 255}: filter_zero == 0 and input_zero == 0 are the
    reference's specialisations, 128 makes a re-centred zero point 0, 255 * 255 * K is the largest sum"""
    for az in ZERO_POINTS:
        for fz in ZERO_POINTS:
            c = conv_case("padded_k_and_co", seed=30, zeros=(az, fz), data=data, quant=(1 << 30, 4, 7, 0, 255))
            want = c.want()
            got = run_all_paths(hl, c)[0]
            assert np.array_equal(got, want), (data, az, fz)
    c = conv_case("k_tail_2p5_tiles", seed=31, zeros=(0, 0), data=data, quant=(1 << 30, 9, 0, 0, 255))
    assert_all_paths(hl, c, np.int16, data)


@gpu
@pytest.mark.parametrize("bias", ["min", "max"])
def test_hip_conv_bias_at_the_ends_wraps(hl, bias):
    for name in ("padded_k_and_co", "long_k"):
        c = conv_case(name, seed=32, bias=bias, zeros=(3, 250) if bias == "min" else (250, 250), quant=(I32_MAX, 3, 100, 0, 255))
        assert_all_paths(hl, c, np.uint8, name)
        assert_all_paths(hl, c, np.int16, name)
    c = dw_case("c24_5x5_s2", seed=33, bias=bias, zeros=(255, 0) if bias == "min" else (0, 0), quant=(I32_MAX, 2, 100, 0, 255))
    assert_all_paths(hl, c, np.uint8, "depthwise")


@gpu
def test_hip_conv_cropped_output_and_padded_rows(hl):
    """an output box with non-zero mins in x, y and b, inside host arrays whose rows and planes are padded with sentinels: the result
    is the checker's for that box and no byte outside it is written; then the same from device allocations of the test's own, their
    first element 16 bytes off the allocation (the MFMA kernel still applies), then the input 17 and the output 1 byte off it (a
    misaligned input: the general kernel runs)"""
    c = conv_case("k_tail_2p5_tiles", seed=40)
    ow, oh, ob = c.out_whb
    B, IH, IW, CP = c.inp.shape
    omins, imins = [0, 3, -2, 5], [0, 6, -2, 5]             # x: output min 3 under stride 2 reads from 6 on; y under stride 1 from -2
    want = c.want()
    for kind, in_off, out_off, kernel in ((HostArray, 0, 0, "hannk_conv_mfma"), (DevArray, 16, 16, "hannk_conv_mfma"), (DevArray, 17, 1, "hannk_conv_general")):
        rs, ps = IW * CP + 12, (IW * CP + 12) * IH + 40      # multiples of 4
        src = kind(hl, (B, IH, IW * CP), np.uint8, rs, ps, offset=in_off, fill=c.inp.reshape(B, IH, IW * CP))
        ors, ops_ = ow * c.co + 5, (ow * c.co + 5) * oh + 3
        dst = kind(hl, (ob, oh, ow * c.co), np.uint8, ors, ops_, offset=out_off)
        if kind is HostArray:
            v = np.lib.stride_tricks.as_strided
            ibuf = hl.Buffer(v(src.host, (B, IH, IW, CP), (ps, rs, CP, 1)), mins=imins)
            obuf = hl.Buffer(v(dst.host, (ob, oh, ow, c.co), (ops_, ors, c.co, 1)), mins=omins)
            assert ibuf.raw.host % 4 == 0, "numpy's allocations are at least 16-byte aligned"
        else:
            ibuf = hl.Buffer.wrap_device(src.p.value + in_off, np.uint8, [CP, IW, IH, B], [1, CP, rs, ps], imins)
            obuf = hl.Buffer.wrap_device(dst.p.value + out_off, np.uint8, [c.co, ow, oh, ob], [1, c.co, ors, ops_], omins)
        filt = hl.Buffer(hl.aligned_array(c.tiled.shape, np.uint8, 64, 1))
        filt.array[...] = c.tiled
        args = conv_args(hl, c, ibuf, filt, hl.Buffer(c.bias.copy()), obuf)
        ran = launches(hl, lambda: hl._check(hl._fn["conv_u8_u8_u8"](*[a.ptr if isinstance(a, hl.Buffer) else a for a in args])))
        assert kernel in ran, (kind.__name__, in_off, ran)
        if kind is HostArray:
            obuf.numpy()
            got = dst._checked(dst.flat.copy(), dst.before)
        else:
            obuf.device_sync()
            got = dst.result()
            ibuf.device_detach(), obuf.device_detach()
        assert np.array_equal(got.reshape(ob, oh, ow, c.co), want), (kind.__name__, in_off)
        src.free(), dst.free()


@gpu
@pytest.mark.parametrize("name", sorted(DW_SHAPES))
@pytest.mark.parametrize("vector", [None, "1"], ids=["plan", "vector"])
def test_hip_depthwise_is_the_checker(hl, name, vector, monkeypatch):
    """the plan's own choice (at these sizes the one-thread-per-output kernel) and the four-channels-per-lane kernel, forced"""
    monkeypatch.delenv("HLMI_HANNK_DW_VECTOR", raising=False)
    if vector is not None:
        monkeypatch.setenv("HLMI_HANNK_DW_VECTOR", vector)
    c = dw_case(name, seed=50)
    assert_all_paths(hl, c, np.uint8, name)
    inp, out = hl.Buffer(hl.aligned_array(c.inp.shape, np.uint8, 64, 1)), hl.Buffer(np.zeros(tuple(reversed([c.co] + list(c.out_whb))), np.uint8))
    inp.array[...] = c.inp
    args = conv_args(hl, c, inp, hl.Buffer(c.filt.copy()), hl.Buffer(c.bias.copy()), out)
    ran = launches(hl, lambda: hl._check(hl._fn["depthwise_conv_uint8"](*[a.ptr if isinstance(a, hl.Buffer) else a for a in args])))
    assert ran == (["hannk_dw"] if vector else ["hannk_dw_general"])


@gpu
def test_hip_depthwise_plan_threshold(hl, monkeypatch):
    """hannk_dw runs where its threads (4 channels x 4 rows each) give each of 256 compute units a workgroup: 512 channels, 16 x 32
    pixels, batch 4 is exactly that many; batch 3 is below it"""
    monkeypatch.delenv("HLMI_HANNK_DW_VECTOR", raising=False)
    for ob, kernel in ((4, "hannk_dw"), (3, "hannk_dw_general")):
        c = Case(512, 512, 3, 3, (1, 1), (1, 1), 16, 32, ob, seed=55, depthwise=True)
        inp, out = hl.Buffer(hl.aligned_array(c.inp.shape, np.uint8, 64, 1)), hl.Buffer(np.zeros((ob, 32, 16, 512), np.uint8))
        inp.array[...] = c.inp
        args = conv_args(hl, c, inp, hl.Buffer(c.filt.copy()), hl.Buffer(c.bias.copy()), out)
        ran = launches(hl, lambda: hl._check(hl._fn["depthwise_conv_uint8"](*[a.ptr if isinstance(a, hl.Buffer) else a for a in args])))
        assert ran == [kernel], (ob, ran)
        assert np.array_equal(out.numpy(), c.want()), ob


@gpu
def test_hip_depthwise_broadcast_and_constants(hl, monkeypatch):
    monkeypatch.setenv("HLMI_HANNK_DW_VECTOR", "1")
    b = Case(1, 20, 3, 3, (1, 1), (1, 1), 6, 5, 2, seed=51, depthwise=True, broadcast=True)
    assert_all_paths(hl, b, np.uint8, "broadcast 3x3")
    b = Case(1, 20, 2, 4, (2, 1), (1, 2), 5, 3, 1, seed=52, depthwise=True, broadcast=True)
    assert_all_paths(hl, b, np.uint8, "broadcast 2x4")
    for data in ("zeros", "ones"):
        for az in ZERO_POINTS:
            for fz in ZERO_POINTS:
                c = dw_case("c20_3x3_d2", seed=53, zeros=(az, fz), data=data, quant=(1 << 30, 2, 9, 0, 255))
                assert np.array_equal(run_all_paths(hl, c)[0], c.want()), (data, az, fz)


@gpu
def test_hip_depthwise_unaligned_device_input_takes_the_general_kernel(hl, monkeypatch):
    """even where the switch asks for hannk_dw: its dword loads need a dword-aligned input"""
    monkeypatch.setenv("HLMI_HANNK_DW_VECTOR", "1")
    c = dw_case("c24_5x5_s2", seed=54)
    ow, oh, ob = c.out_whb
    B, IH, IW, CP = c.inp.shape
    want = c.want()
    for offset, kernel in ((16, "hannk_dw"), (2, "hannk_dw_general")):
        src = DevArray(hl, (B, IH, IW * CP), np.uint8, offset=offset, fill=c.inp.reshape(B, IH, IW * CP))
        ibuf = hl.Buffer.wrap_device(src.p.value + offset, np.uint8, [CP, IW, IH, B], [1, CP, IW * CP, IW * CP * IH])
        out = hl.Buffer(np.zeros((ob, oh, ow, c.co), np.uint8))
        args = conv_args(hl, c, ibuf, hl.Buffer(c.filt.copy()), hl.Buffer(c.bias.copy()), out)
        ran = launches(hl, lambda: hl._check(hl._fn["depthwise_conv_uint8"](*[a.ptr if isinstance(a, hl.Buffer) else a for a in args])))
        assert ran == [kernel], (offset, ran)
        assert np.array_equal(out.numpy(), want), offset
        ibuf.device_detach()
        src.free()


@gpu
def test_hip_epilogue_sweep(hl):
    """the device's epilogue alone: 2^16 random accumulators and the edge values under every (multiplier, shift) of the known-answer list"""
    rng = np.random.default_rng(60)
    acc = np.concatenate([rng.integers(I32_MIN, I32_MAX, 1 << 16), np.array(ACCS), np.array([I32_MIN + 1, I32_MAX - 1, 1 << 30, -(1 << 30)])]).astype(np.int32)
    for m in MULTIPLIERS:
        for s in SHIFTS:
            assert np.array_equal(hl.debug_hannk_quantize("i16", acc, m, s), hk.quantize("i16", acc, m, s)), (m, s)
            assert np.array_equal(hl.debug_hannk_quantize("u8", acc, m, s, 128, 0, 255), hk.quantize("u8", acc, m, s, 128, 0, 255)), (m, s)
    assert np.array_equal(hl.debug_hannk_quantize("u8", acc, 1 << 30, 20, 3, 200, 100), np.full(acc.shape, 200, np.uint8))   # a crossed min > max


@gpu
@pytest.mark.parametrize("ci,co", [(3, 8), (68, 40)])
def test_hip_tile_filter_and_its_output_fed_to_conv(hl, ci, co):
    rng = np.random.default_rng(70)
    filt = rng.integers(0, 256, (co, 3, 3, ci), dtype=np.uint8)
    fz = 77
    tiled = hl.hannk_tile_filter(filt, fz)
    want = hk.tile(filt, fz)
    assert np.array_equal(tiled.numpy(), want)
    # a different input_zero and output_zero, a cropped box of tiles with non-zero mins in co / 16, x and y, through the general hook too
    cq, co16 = -(-ci // 4), -(-co // 16)
    for path in ("direct", "general"):
        o = hl.Buffer(hl.aligned_array((2, 2, co16, cq, 16, 4), np.uint8, 64, 1), mins=[0, 0, 0, 0 if co16 == 1 else 1, 1, 1])
        if path == "direct":
            hl.tile_conv_filter_uint8(hl.Buffer(filt), 200, 9, o)
        else:
            hl.debug_hannk_general("tile_conv_filter_uint8", hl.Buffer(filt), 200, 9, o)
        assert np.array_equal(o.numpy(), hk.tile_filter(filt, 200, 9, [4, 16, cq, co16, 2, 2], out_mins=o.mins)), path
    # the tiled filter as the library made it, fed to conv
    c = Case(ci, co, 3, 3, (1, 1), (1, 1), 6, 4, 1, seed=71, zeros=(5, fz))
    c.filt, c.tiled = filt, want
    inp = hl.Buffer(hl.aligned_array(c.inp.shape, np.uint8, 64, 1))
    inp.array[...] = c.inp
    out = hl.Buffer(np.zeros((1, 4, 6, co), np.uint8))
    m, s, z, lo, hi = c.quant
    hl.conv_u8_u8_u8(inp, c.az, tiled, c.fz, hl.Buffer(c.bias), c.stride, c.dilation, m, s, z, lo, hi, out)
    assert np.array_equal(out.numpy(), c.want()) and np.array_equal(out.numpy(), c.second())


# ---- every kernel instance (the tables beside CONV_SHAPES and DW_SHAPES)
def host_operands(hl, c):
    """input, filter and bias of a Case in fresh host buffers, aligned as the interpreter allocates"""
    inp = hl.Buffer(hl.aligned_array(c.inp.shape, np.uint8, 64, 1))
    inp.array[...] = c.inp
    if c.depthwise:
        return inp, hl.Buffer(c.filt.copy()), hl.Buffer(c.bias.copy())
    filt = hl.Buffer(hl.aligned_array(c.tiled.shape, np.uint8, 64, 1))
    filt.array[...] = c.tiled
    return inp, filt, hl.Buffer(c.bias.copy())


def call_entry(hl, name, args, general=False):
    if general:
        return hl.debug_hannk_general(name, *args)
    return hl._check(hl._fn[name](*[a.ptr if isinstance(a, hl.Buffer) else a for a in args]))


def direct_launches(hl, c, out_dtype=np.uint8):
    ow, oh, ob = c.out_whb
    out = hl.Buffer(np.zeros((ob, oh, ow, c.co), out_dtype))
    args = conv_args(hl, c, *host_operands(hl, c), out)
    ran = launches(hl, lambda: call_entry(hl, entry_name(c, out_dtype), args))
    assert np.array_equal(out.numpy(), c.want(out_dtype))
    return ran


@gpu
@pytest.mark.parametrize("out_dtype", [np.uint8, np.int16], ids=["u8", "i16"])
@pytest.mark.parametrize("name,switch", CONV_RUNS, ids=[f"{n}-{'plan' if s is None else 'split' + s}" for n, s in CONV_RUNS])
def test_hip_conv_every_instance(hl, on_stream, monkeypatch, name, switch, out_dtype):
    """every run of CONV_RUNS, all paths, both output types, on both kinds of stream; hannk_conv_finish runs where the row's class says
    SPLIT.  A frame queue's plan sees a quarter of the compute units: where that changes the plan's own choice the launch list is
    held to the class on the device-wide stream only."""
    splits, _ = conv_splits(hl, name, switch, monkeypatch)
    on_a_quarter, _ = conv_splits(hl, name, switch, monkeypatch, cus=64)
    c = conv_case(name, seed=24)
    assert_all_paths(hl, c, out_dtype, f"{name} {switch}")
    ran = direct_launches(hl, c, out_dtype)
    assert "hannk_conv_mfma" in ran
    if on_stream == "device" or (splits > 1) == (on_a_quarter > 1):
        assert ("hannk_conv_finish" in ran) == (splits > 1), (ran, splits)


@gpu
@pytest.mark.parametrize("name,broadcast,vector", DW_RUNS, ids=[f"{n}-{'broadcast' if b else 'plain'}-{'vector' if v else 'plan'}" for n, b, v in DW_RUNS])
def test_hip_depthwise_every_instance(hl, on_stream, monkeypatch, name, broadcast, vector):
    monkeypatch.delenv("HLMI_HANNK_DW_VECTOR", raising=False)
    if vector is not None:
        monkeypatch.setenv("HLMI_HANNK_DW_VECTOR", vector)
    c = dw_case(name, seed=56, broadcast=broadcast)
    assert_all_paths(hl, c, np.uint8, f"{name} {broadcast} {vector}")
    assert direct_launches(hl, c) == [dw_instance(name, broadcast, vector)[0]]


# ---- the layouts an aliased tensor has: the reference's interpreter turns ConcatenationOp, SplitOp and PadOp into offset aliases, so a conv
# writes (and reads) channels [k, k + C) of pixels that hold P > C
OUT_SLICES = [(8, 24, 0), (8, 24, 8), (10, 24, 3), (12, 13, 0)]   # (C, P, k); P = 13: the packed store's alignment rotates from pixel to pixel
SLICE_IDS = [f"c{nc}_of_{p}_at_{k}" for nc, p, k in OUT_SLICES]
CONV_SLICE_PATHS = {   # HLMI_HANNK_SPLIT_K, the general hook, the launches
    "mfma": ("1", False, ["hannk_conv_mfma"]),
    "split": ("2", False, ["hannk_conv_finish", "hannk_conv_mfma"]),
    "general": (None, True, ["hannk_conv_general"]),
}


def out_slice(hl, c, pixel_stride, channel, out_dtype=np.uint8):
    """a device tensor of the Case's output extents: channels [channel, channel + C) of pixels `pixel_stride` elements apart"""
    ow, oh, ob = c.out_whb
    return DevTensor(hl, (ob, oh, ow, c.co), (oh * ow * pixel_stride, ow * pixel_stride, pixel_stride, 1), offset=channel * np.dtype(out_dtype).itemsize,
                     dtype=out_dtype)


@gpu
@pytest.mark.parametrize("path", sorted(CONV_SLICE_PATHS))
@pytest.mark.parametrize("out_dtype", [np.uint8, np.int16], ids=["u8", "i16"])
@pytest.mark.parametrize("nc,pixel_stride,channel", OUT_SLICES, ids=SLICE_IDS)
def test_hip_conv_output_is_a_channel_slice(hl, monkeypatch, nc, pixel_stride, channel, out_dtype, path):
    """store4 picks its packed store from the address: the bytes are the checker's and those between one pixel's channels and the next
    (and before the first, after the last) come back untouched, from the MFMA kernel, from hannk_conv_finish and from the general kernel"""
    switch, general, names = CONV_SLICE_PATHS[path]
    monkeypatch.delenv("HLMI_HANNK_SPLIT_K", raising=False)
    if switch is not None:
        monkeypatch.setenv("HLMI_HANNK_SPLIT_K", switch)
    c = Case(8, nc, 3, 3, (1, 1), (1, 1), 8, 5, 1, seed=41)
    dst = out_slice(hl, c, pixel_stride, channel, out_dtype)
    try:
        args = conv_args(hl, c, *host_operands(hl, c), dst.buf)
        ran = launches(hl, lambda: call_entry(hl, entry_name(c, out_dtype), args, general))
        assert ran == names
        assert np.array_equal(dst.result(), c.want(out_dtype))
    finally:
        dst.free()


@gpu
@pytest.mark.parametrize("broadcast", [False, True], ids=["plain", "broadcast"])
@pytest.mark.parametrize("nc,pixel_stride,channel", OUT_SLICES, ids=SLICE_IDS)
def test_hip_depthwise_output_is_a_channel_slice(hl, monkeypatch, nc, pixel_stride, channel, broadcast):
    monkeypatch.setenv("HLMI_HANNK_DW_VECTOR", "1")
    c = Case(1 if broadcast else nc, nc, 3, 3, (1, 1), (1, 1), 8, 5, 1, seed=42, depthwise=True, broadcast=broadcast)
    dst = out_slice(hl, c, pixel_stride, channel)
    try:
        args = conv_args(hl, c, *host_operands(hl, c), dst.buf)
        ran = launches(hl, lambda: call_entry(hl, entry_name(c), args))
        assert ran == ["hannk_dw"]
        assert np.array_equal(dst.result(), c.want())
    finally:
        dst.free()


CONV_INPUT_SLICES = {   # ci, the pixel stride above CP, the first channel (= byte) inside the wider pixel, the kernel
    "vec_fragments_4_byte_aligned": (16, 4, 4, "hannk_conv_mfma"),     # ci % 16 == 0: the 16-byte fragments lie at 4 + 20 n
    "pixels_20_wider": (6, 20, 4, "hannk_conv_mfma"),
    "first_channel_2": (6, 4, 2, "hannk_conv_general"),                # not a dword boundary: the MFMA kernel's loads may not take it
}


@gpu
@pytest.mark.parametrize("out_dtype", [np.uint8, np.int16], ids=["u8", "i16"])
@pytest.mark.parametrize("name", sorted(CONV_INPUT_SLICES))
def test_hip_conv_input_is_a_channel_slice(hl, monkeypatch, name, out_dtype):
    """the input as CP channels of wider pixels in a device allocation: pixel, row and plane strides above the dense ones, sentinels
    in every gap (a gap byte read as a channel changes the sum)"""
    monkeypatch.delenv("HLMI_HANNK_SPLIT_K", raising=False)
    ci, wider, first, kernel = CONV_INPUT_SLICES[name]
    c = Case(ci, 20, 3, 3, (1, 1), (1, 1), 6, 4, 2, seed=43)
    B, IH, IW, CP = c.inp.shape
    P = CP + wider
    src = DevTensor(hl, c.inp.shape, ((IW * P + 4) * IH + 8, IW * P + 4, P, 1), offset=first, fill=c.inp)
    try:
        ow, oh, ob = c.out_whb
        out = hl.Buffer(np.zeros((ob, oh, ow, c.co), out_dtype))
        _, filt, bias = host_operands(hl, c)
        ran = launches(hl, lambda: call_entry(hl, entry_name(c, out_dtype), conv_args(hl, c, src.buf, filt, bias, out)))
        assert kernel in ran and (kernel == "hannk_conv_mfma" or ran == [kernel]), ran
        assert np.array_equal(out.numpy(), c.want(out_dtype))
    finally:
        src.free()


@gpu
@pytest.mark.parametrize("first,kernel", [(16, "hannk_dw"), (2, "hannk_dw_general")])
def test_hip_depthwise_input_is_a_channel_slice(hl, monkeypatch, first, kernel):
    """20 channels (32 with the padding) of pixels 48 bytes apart, from channel 16 on (hannk_dw) and from byte 2 on (no dword loads)"""
    monkeypatch.setenv("HLMI_HANNK_DW_VECTOR", "1")
    c = Case(20, 20, 3, 3, (1, 1), (1, 1), 6, 5, 2, seed=44, depthwise=True)
    B, IH, IW, CP = c.inp.shape
    P = CP + 16
    src = DevTensor(hl, c.inp.shape, ((IW * P + 16) * IH + 32, IW * P + 16, P, 1), offset=first, fill=c.inp)
    try:
        out = hl.Buffer(np.zeros((2, 5, 6, 20), np.uint8))
        _, filt, bias = host_operands(hl, c)
        ran = launches(hl, lambda: call_entry(hl, entry_name(c), conv_args(hl, c, src.buf, filt, bias, out)))
        assert ran == [kernel]
        assert np.array_equal(out.numpy(), c.want())
    finally:
        src.free()


@gpu
@pytest.mark.parametrize("general", [False, True], ids=["default", "general"])
def test_hip_filters_with_gaps(hl, monkeypatch, general):
    """the tiled filter with dim(3), dim(4) and dim(5) strides above the dense ones by multiples of 64 and sentinels between the tiles;
    the depthwise filter with padded dim(1) and dim(2) strides"""
    monkeypatch.delenv("HLMI_HANNK_SPLIT_K", raising=False)
    monkeypatch.setenv("HLMI_HANNK_DW_VECTOR", "1")
    c = Case(20, 40, 3, 2, (1, 1), (1, 1), 7, 5, 1, seed=45)
    FH, FW, CO16, CQ = c.tiled.shape[:4]
    s3 = CQ * 64 + 64
    s4 = CO16 * s3 + 128
    s5 = FW * s4 + 64
    filt = DevTensor(hl, c.tiled.shape, (s5, s4, s3, 64, 4, 1), offset=64, fill=c.tiled)
    try:
        for out_dtype in (np.uint8, np.int16):
            out = hl.Buffer(np.zeros((1, 5, 7, 40), out_dtype))
            inp, _, bias = host_operands(hl, c)
            ran = launches(hl, lambda: call_entry(hl, entry_name(c, out_dtype), conv_args(hl, c, inp, filt.buf, bias, out), general))
            assert ("hannk_conv_general" if general else "hannk_conv_mfma") in ran
            assert np.array_equal(out.numpy(), c.want(out_dtype)), out_dtype
    finally:
        filt.free()
    for broadcast in (False, True):
        c = Case(1 if broadcast else 21, 21, 3, 3, (1, 1), (1, 1), 5, 6, 1, seed=46, depthwise=True, broadcast=broadcast)
        filt = DevTensor(hl, c.filt.shape, (3 * (21 + 3) + 5, 21 + 3, 1), offset=3, fill=c.filt)
        try:
            out = hl.Buffer(np.zeros((1, 6, 5, 21), np.uint8))
            inp, _, bias = host_operands(hl, c)
            ran = launches(hl, lambda: call_entry(hl, entry_name(c), conv_args(hl, c, inp, filt.buf, bias, out), general))
            assert ran == ["hannk_dw_general" if general else "hannk_dw"]
            assert np.array_equal(out.numpy(), c.want()), broadcast
        finally:
            filt.free()


@gpu
@pytest.mark.parametrize("split", ["1", None], ids=["unsplit", "plan"])    # the stores of hannk_conv_mfma; of hannk_conv_finish (the plan splits in 5)
@pytest.mark.parametrize("off", [2, 4, 6])
def test_hip_conv_i16_cropped_output_and_padded_rows(hl, monkeypatch, off, split):
    """test_hip_conv_cropped_output_and_padded_rows for conv_u8_u8_i16: the output box at non-zero mins inside rows an odd count of
    elements long (the 8-byte store's predicate changes from row to row) and planes padded further, its first element 2, 4 and 6 bytes
    off an 8-byte boundary; every byte around it is a sentinel that must come back"""
    monkeypatch.delenv("HLMI_HANNK_SPLIT_K", raising=False)
    if split is not None:
        monkeypatch.setenv("HLMI_HANNK_SPLIT_K", split)
    c = conv_case("k_tail_2p5_tiles", seed=47)
    ow, oh, ob = c.out_whb
    B, IH, IW, CP = c.inp.shape
    omins, imins = [0, 3, -2, 5], [0, 6, -2, 5]
    rs = ow * c.co + 5
    dst = DevTensor(hl, (ob, oh, ow, c.co), (rs * oh + 3, rs, c.co, 1), offset=off, mins=omins, dtype=np.int16)
    try:
        inp, filt, bias = host_operands(hl, c)
        inp = hl.Buffer(inp.array, mins=imins)
        ran = launches(hl, lambda: call_entry(hl, "conv_u8_u8_i16", conv_args(hl, c, inp, filt, bias, dst.buf)))
        assert ran == (["hannk_conv_mfma"] if split else ["hannk_conv_finish", "hannk_conv_mfma"]), ran
        assert np.array_equal(dst.result(), c.want(np.int16))
    finally:
        dst.free()


@gpu
def test_seeded_fuzz_slice():
    """scripts/fuzz_parity.py's cases of conv and depthwise, 40 of each from the seed test_the_seeded_slice_reaches_the_kernels draws from"""
    mod = load_fuzz_parity()
    r = np.random.default_rng(FUZZ_SEED)
    for name in ("hannk_conv", "hannk_depthwise"):
        for i in range(FUZZ_CASES):
            desc, ok = mod.CASES[name](r)
            assert ok, f"{name} case {i}: {desc}"


def explicit_pad(x, zero, channel_multiple, px, py):
    b, h, w, c = x.shape
    cp = -(-c // channel_multiple) * channel_multiple
    return np.pad(x, ((0, 0), (py, py), (px, px), (0, cp - c)), constant_values=zero)


@gpu
def test_hip_conveniences_pad_like_numpy(hl):
    """hl.hannk_conv2d and hl.hannk_depthwise_conv2d: channel padding to 4 / 16 and spatial padding with input_zero, against the checker on
    an explicitly padded copy"""
    rng = np.random.default_rng(80)
    x = rng.integers(0, 256, (2, 6, 9, 7), dtype=np.uint8)
    assert np.array_equal(hl.hannk_pad_input(x, 99, 4, (2, 1)), explicit_pad(x, 99, 4, 2, 1))
    filt = rng.integers(0, 256, (10, 3, 3, 7), dtype=np.uint8)
    bias = rng.integers(-1000, 1000, 10).astype(np.int32)
    for out_dtype in (np.uint8, np.int16):
        got = hl.hannk_conv2d(x, filt, bias, 99, 130, (2, 1), (1, 2), (2, 1), 1 << 30, 8, 20, 5, 240, out_dtype)
        ow, oh = hk.out_extent(9, 3, 2, 1, 2), hk.out_extent(6, 3, 1, 2, 1)
        assert got.shape == (2, oh, ow, 10) and got.dtype == out_dtype
        want = hk.conv(explicit_pad(x, 99, 4, 2, 1), hk.tile(filt, 130), bias, [10, ow, oh, 2], (2, 1), (1, 2), 99, 130, 1 << 30, 8, 20, 5, 240, out_dtype)
        assert np.array_equal(got, want)
    dfilt = rng.integers(0, 256, (3, 3, 7), dtype=np.uint8)
    got = hl.hannk_depthwise_conv2d(x, dfilt, bias[:7], 99, 130, 1, 1, 1, 1 << 30, 3, 20, 5, 240)
    want = hk.depthwise(explicit_pad(x, 99, 16, 1, 1), dfilt, bias[:7], [7, 9, 6, 2], (1, 1), (1, 1), 99, 130, 1 << 30, 3, 20, 5, 240)
    assert got.shape == (2, 6, 9, 7) and np.array_equal(got, want)
    got = hl.hannk_depthwise_conv2d(x[..., :1], dfilt, bias[:7], 99, 130, 1, 1, 0, 1 << 30, 3, 20, 5, 240)   # one channel under seven: broadcast
    want = hk.depthwise(np.ascontiguousarray(x[..., :1]), dfilt, bias[:7], [7, 7, 4, 2], (1, 1), (1, 1), 99, 130, 1 << 30, 3, 20, 5, 240, broadcast=True)
    assert np.array_equal(got, want)


@gpu
def test_hip_torch_ops(hl):
    import torch
    import halide_amd.torch_ops  # noqa: F401
    rng = np.random.default_rng(90)
    x = rng.integers(0, 256, (2, 6, 9, 7), dtype=np.uint8)
    filt = rng.integers(0, 256, (10, 3, 3, 7), dtype=np.uint8)
    bias = rng.integers(-1000, 1000, 10).astype(np.int32)
    dev = lambda a: torch.from_numpy(a).cuda()
    got = torch.ops.hlmi.hannk_conv2d(dev(x), dev(filt), dev(bias), 99, 130, [2, 1], [1, 2], [2, 1], 1 << 30, 8, 20, 5, 240, False)
    ow, oh = hk.out_extent(9, 3, 2, 1, 2), hk.out_extent(6, 3, 1, 2, 1)
    want = hk.conv(explicit_pad(x, 99, 4, 2, 1), hk.tile(filt, 130), bias, [10, ow, oh, 2], (2, 1), (1, 2), 99, 130, 1 << 30, 8, 20, 5, 240)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    got = torch.ops.hlmi.hannk_conv2d(dev(x), dev(filt), dev(bias), 99, 130, [2, 1], [1, 2], [2, 1], 1 << 30, 8, 20, 5, 240, True)
    want = hk.conv(explicit_pad(x, 99, 4, 2, 1), hk.tile(filt, 130), bias, [10, ow, oh, 2], (2, 1), (1, 2), 99, 130, 1 << 30, 8, 20, 5, 240, np.int16)
    assert got.dtype == torch.int16 and np.array_equal(got.cpu().numpy(), want)
    dfilt = rng.integers(0, 256, (3, 3, 7), dtype=np.uint8)
    got = torch.ops.hlmi.hannk_depthwise_conv2d(dev(x), dev(dfilt), dev(bias[:7]), 99, 130, [1, 1], [1, 1], [1, 1], 1 << 30, 3, 20, 5, 240)
    want = hk.depthwise(explicit_pad(x, 99, 16, 1, 1), dfilt, bias[:7], [7, 9, 6, 2], (1, 1), (1, 1), 99, 130, 1 << 30, 3, 20, 5, 240)
    assert np.array_equal(got.cpu().numpy(), want)
    with pytest.raises((RuntimeError, TypeError)):
        torch.ops.hlmi.hannk_conv2d(dev(x).float(), dev(filt), dev(bias), 99, 130, [2, 1], [1, 2], [2, 1], 1 << 30, 8, 20, 5, 240, False)


@gpu
def test_hip_consumer_runs(hl):
    """the C++ consumer: the tiling learnt from the all-ones queries, the filter type from the metadata, one filter tiled and one
    convolution run through the mangled symbols, checked in the program against loops of its own"""
    r = subprocess.run([_build_consumer()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hannk consumer ok" in r.stdout
