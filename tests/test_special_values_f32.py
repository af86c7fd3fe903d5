"""The float-input pipelines that tests/test_special_values.py does not reach (gaussian_blur_direct and the resampled
gaussian_blur variants, the eight resize_*_float32_* entry points, bgu, conv_layer, conv_layer_bf16, depthwise_separable_conv) on
their usual inputs with single elements replaced by the values where a device expression and its C restatement part ways: both
zeros, denormals, FLT_MIN, magnitudes whose products and sums overflow, the infinities, NaN.  Same shape as that file: one table,
bit patterns compared, a NaN of the reference answered by any NaN.

A row names its inputs (`base`), which input gets which values and where (`puts`: values at `fixed` positions are put there
explicitly, the others by a generator seeded with the row's name), its reference (`want`) and the ways to run it (`paths`).  Which
values a row gets is decided by what its reference defines, not by what passes; every exclusion stands at its row.  Three CPU tests
hold the table itself: the inputs hold exactly the multiset of bit patterns the row names; the special elements sit where the
kernels compute and do not store (the last pixel, a halo column, the last row and column); and, on the reference alone in both
canonical forms, the all-noise output is finite, at most a quarter of the special output is NaN, and some output that is no NaN
differs from the all-noise one.

What the kernels do at those places (halide_amd/csrc): resize.hip's fused kernels compute rows past ny and columns past the span
from stale LDS or re-read columns and do not store them, and st_out's clampf maps NaN to 1 and -0 to +0; gaussian_blur.hip's taps<N,
false> computes edge taps with a clamped weight and drops them with a select, and every path runs mad over every tap, a zero weight
included (0 * inf is NaN in the contract); conv_layer.hip's loader clamps pixels past npix to the last pixel; the three main kernels
of conv_layer_bf16.hip compute input-linear positions that are no output pixel; depthwise_separable_conv.hip's zero padding is
fma(f, 0, acc), so an infinite tap over the border gives NaN and the ReLU 0, and its templated kernel loads clamped addresses and
masks afterwards."""
import functools
import os
import re
import zlib
from typing import Callable, NamedTuple

import numpy as np
import pytest

import checker_lib
import parity_helpers as ph
from test_bgu import _run as _bgu_run, _scene
from test_conv_layer import _data as _conv_data, _run as _conv_run
from test_depthwise_separable_conv import _data as _dsc_data, _run as _dsc_run
from test_gaussian_blur import GENERAL as GB_GENERAL, TILED as GB_TILED, _gpu_direct, _gpu_resampled
from test_resize import GENERAL as RS_GENERAL, _gpu as _gpu_resize
from test_special_values import COMMON, INF, MAX_NAN_SHARE, NAN

f32, f64 = np.float32, np.float64
_bits = lambda *b: np.array(b, np.uint32).view(f32)
_cat = lambda *a: np.concatenate([np.asarray(v, f32).ravel() for v in a])
NEG0, DENORMAL, PLUS_INF = _bits(0x80000000), _bits(0x00012345), INF[:1]
FIRST8 = COMMON[:8]   # the zeros, the denormals, FLT_MIN, 1e-30, -0.25, 4: nothing above 4


class Put(NamedTuple):
    values: np.ndarray    # each replaces one element of the input
    fixed: tuple = ()     # ((index into values, position), ...): put there explicitly, whatever the seed
    ok: Callable = None   # (position, value) -> may the generator put it there


class Path(NamedTuple):
    env: dict             # switches of the library, set for the call
    run: Callable         # (hl, *inputs) -> output
    launches: set = None  # the kernels the call must launch, where the path is forced or the row is about the path


def _same(got, want, what):
    ph.same_bits_or_nan(np.ascontiguousarray(got), want, what)


class Row(NamedTuple):
    base: Callable             # () -> the all-noise inputs
    puts: dict                 # index of the input -> Put
    want: Callable             # (oracle, *inputs) -> what `compare` takes as the reference
    paths: dict                # name -> Path
    compare: Callable = _same  # (got, want, what)
    out: Callable = lambda w: w   # the reference's output array out of what `want` returns


def _fix(values, *pairs):
    """((index, position), ...) for (value, position) pairs; a value named twice takes its second occurrence the second time"""
    out, used = [], set()
    for v, pos in pairs:
        idx = [i for i in np.flatnonzero(values.view(np.uint32) == np.asarray(v, f32).reshape(1).view(np.uint32)[0]) if int(i) not in used]
        used.add(int(idx[0]))
        out.append((int(idx[0]), tuple(pos)))
    return tuple(out)


ROWS = {}

# ---------------------------------------------------------------------------------------------------- gaussian_blur
# 45 x 70 (h x w): test_gaussian_blur.py's test_the_paths_launch_what_they_say shows that the tiled kernels run at this size under
# HLMI_GB_TILE.  The last row and the last column each hold a special element: the tiled kernels re-read the last column for lanes
# past the source and repeat the last row for rows past the output, and store neither.
GB_H, GB_W = 45, 70
GB_PATHS = {"by_size": ({}, False, None), "general": ({}, True, GB_GENERAL), "tile16": ({"HLMI_GB_TILE": "16"}, False, GB_TILED),
            "tile4": ({"HLMI_GB_TILE": "4"}, False, GB_TILED)}


def _gb_direct_row(sigma, trunc, values, last_row, last_col, ok=None):
    fixed = _fix(values, (last_row, (GB_H - 1, GB_W // 3)), (last_col, (GB_H // 3, GB_W - 1)))
    return Row(lambda: [ph.noise((GB_H, GB_W), seed=GB_H * GB_W + trunc)], {0: Put(values, fixed, ok)},
               lambda oracle, img: checker_lib.gaussian_blur.direct(img, sigma, trunc),
               {p: Path(env, functools.partial(_gpu_direct, sigma=sigma, trunc=trunc, general=g), names) for p, (env, g, names) in GB_PATHS.items()})


def _inside16(pos, v):
    """+inf at least 16 pixels from every edge: its 31 x 31 footprint (R = 15) lies inside the image, 232 NaN of 3150"""
    return not np.isinf(v) or (16 <= pos[0] <= GB_H - 17 and 16 <= pos[1] <= GB_W - 17)


# all: R = 5; every value twice, NaN in the last row, +inf in the last column
ROWS["gaussian_blur_direct_all"] = _gb_direct_row(1.5, 3, _cat(COMMON, COMMON, INF, INF, NAN, NAN), NAN, PLUS_INF)
# zero_weights: sigma 1.0, trunc 15 gives R = 15 and a table whose four outermost weights are exactly 0 (halide_exp underflows below
# about 8e-38).  One +inf: 0 * inf is NaN in the contract, a path that skipped zero taps would give inf.  No -inf and no NaN: with one
# infinity every NaN of the output is the zero weights' doing.
ROWS["gaussian_blur_direct_zero_weights"] = _gb_direct_row(1.0, 15, _cat(COMMON, COMMON, PLUS_INF), COMMON[10], COMMON[9], _inside16)
# zero_weights_finite: trunc 14, two zero weights; 1e37 and +-3e18 against table entries down to 8e-38.  Finite values only: the row is
# about the last place of the small weights, which a NaN or an infinity would hide.
ROWS["gaussian_blur_direct_zero_weights_finite"] = _gb_direct_row(1.0, 14, _cat(COMMON, COMMON), COMMON[10], COMMON[9])

RS_H, RS_W = 96, 128
GBR_PATHS = {"by_size": ({}, False, None), "general": ({}, True, GB_GENERAL | {"gb_down", "gb_up"}),
             "tile4": ({"HLMI_GB_TILE": "4"}, False, GB_TILED | {"gb_down", "gb_up"})}


def _gb_resampled_row(udf, sigma, values, last_row, last_col):
    fixed = _fix(values, (last_row, (RS_H - 1, RS_W // 3)), (last_col, (RS_H // 3, RS_W - 1)))
    return Row(lambda: [ph.noise((RS_H, RS_W), seed=RS_H * RS_W + udf[2])], {0: Put(values, fixed)},
               lambda oracle, img: checker_lib.gaussian_blur.resampled(udf, img, sigma, 3),
               {p: Path(env, lambda hl, img, g=g: _gpu_resampled(hl, udf, img, sigma, 3, general=g), names) for p, (env, g, names) in GBR_PATHS.items()})


ROWS["gaussian_blur_2_1_2"] = _gb_resampled_row((2, 1, 2), 4.0, _cat(COMMON, COMMON, PLUS_INF, NAN), NAN, PLUS_INF)
# factors 8 and 16: finite values only.  One non-finite low-resolution sample reaches (2 R + 1 + U) F output pixels per axis, and one inf
# plus one NaN made 33 % to 88 % of the checker's output NaN: past the quarter at which the comparison still compares.
for _udf, _sigma in (((3, 2, 8), 10.0), ((4, 3, 16), 20.0), ((2, 3, 16), 20.0)):
    ROWS["gaussian_blur_%d_%d_%d" % _udf] = _gb_resampled_row(_udf, _sigma, _cat(COMMON, COMMON), COMMON[10], COMMON[9])

# ---------------------------------------------------------------------------------------------------- resize, float32
# The checker's output holds no NaN and no infinity: the final clamp `m = v < 1 ? v : 1; m > 0 ? m : 0` maps NaN and +inf to 1, -inf,
# -0.25 and -0 to +0.  These rows therefore compare plain bits, and what they pin is that clamp.  NaN in the last row and -inf in the
# last column: next to the rows past ny and the columns past the span that the fused kernels compute and do not store.
RESIZE_VALUES = _cat(COMMON, COMMON, INF, INF, NAN, NAN)


def _resize_row(kernel, up, scale, shape, paths, read_only=False):
    c, h, w = shape
    fixed = _fix(RESIZE_VALUES, (NAN, (c - 1, h - 1, w // 3)), (INF[1:], (0, h // 3, w - 1)))
    run = lambda general: lambda hl, img: _gpu_resize(hl, kernel, img, scale, up, general=general)   # noqa: E731

    @functools.lru_cache(maxsize=None)
    def read(extent):
        """the input coordinates along an axis of `extent` that some output's window holds (begin is the same in both forms)"""
        n = checker_lib.resize_out_size(extent, extent, scale)[0]
        begin, weights, _ = checker_lib.resize.tables(kernel, up, scale, 0, n, 0, extent)
        return {int(b) + k for b in begin for k in range(weights.shape[0])}
    ok = (lambda pos, v: pos[1] in read(h) and pos[2] in read(w)) if read_only else None
    return Row(lambda: [ph.noise(shape, seed=h * w + len(kernel))], {0: Put(RESIZE_VALUES, fixed, ok)},
               lambda oracle, img: checker_lib.resize.resize(kernel, img, scale, up),
               {p: Path({}, run(p == "general"), names) for p, names in paths.items()})


for _kernel in checker_lib.RESIZE_KERNELS:
    for _up, _scale in ((True, 1.5), (False, 0.5)):
        ROWS[f"resize_{_kernel}_float32_{'up' if _up else 'down'}"] = _resize_row(_kernel, _up, _scale, (3, 48, 64), {"by_size": None, "general": RS_GENERAL})
# Shapes whose fused tile does not fit (test_resize.py, PATH_CASES: the footprint is past 12288 floats whatever the image's size), so
# that the general kernels run by size: the smallest of each direction, where rs_pass_x stages its spans in LDS, and 2100 wide, where
# a workgroup's span is past the 2048 floats it can stage and rs_pass_x gathers from global memory (RESIZE_GATHER, asserted below).
RESIZE_GENERAL_ONLY = {"resize_linear_float32_up_0.15": ("linear", True, 0.15, (1, 40, 400)), "resize_box_float32_down_0.07": ("box", False, 0.07, (1, 30, 400)),
                       "resize_linear_float32_up_0.1_gather": ("linear", True, 0.1, (1, 20, 2100)), "resize_box_float32_down_0.07_gather": ("box", False, 0.07, (1, 30, 2100))}
RESIZE_GATHER = [n for n in RESIZE_GENERAL_ONLY if n.endswith("_gather")]
# Far below 1 an _up kernel's two or so taps read a fraction of the input: the generator puts the values where some window reads them.
for _name, _case in RESIZE_GENERAL_ONLY.items():
    ROWS[_name] = _resize_row(*_case, {"by_size": RS_GENERAL}, read_only=True)
RESIZE_ROWS = [n for n in ROWS if n.startswith("resize_")]

# ---------------------------------------------------------------------------------------------------- bgu
# One row per input, so that a failure names it.  No NaN in splat_loc and slice_loc: their gray value becomes a bin index through a
# float-to-int conversion, which is undefined for NaN (test_special_values.py's bilateral_grid row carries the same exclusion);
# nothing above 4 and no infinity in splat_loc and in the plain `values` row: they enter the 4 x 4 normal equations of every cell
# within three cells, and the fitted transforms then saturate the whole output.  values_big has them all: 94 % of its outputs
# change and 95 % of those are saturated at 0 or 1, so it is a check of the final clamp and little else.
BGU_W, BGU_H = 192, 128


def _bgu_row(which, values):
    def base():
        hi, lo, val = _scene(BGU_W, BGU_H, seed=len(which))
        return [lo, val, hi]   # splat_loc, values, slice_loc
    return Row(base, {("splat_loc", "values", "slice_loc").index(which): Put(values)},
               lambda oracle, lo, val, hi: oracle.bgu(1 / 8, 16, lo, val, hi),
               {"by_size": Path({}, lambda hl, lo, val, hi: _bgu_run(hl, 1 / 8, 16, lo, val, hi))})


ROWS["bgu_splat_loc"] = _bgu_row("splat_loc", FIRST8)
ROWS["bgu_values"] = _bgu_row("values", FIRST8)
ROWS["bgu_slice_loc"] = _bgu_row("slice_loc", _cat(COMMON, COMMON, INF, INF))
ROWS["bgu_values_big"] = Row(ROWS["bgu_values"].base, {1: Put(_cat(COMMON, INF, NAN))}, ROWS["bgu_values"].want, ROWS["bgu_values"].paths)

# ---------------------------------------------------------------------------------------------------- conv_layer (exact f32)
# (3, 5, 13, 64, 128): 195 pixels are two workgroups, the second partial, and two chunks of input channels; (1, 3, 9, 32, 256) has a
# second workgroup column.  The NaN sits in the input's last pixel, to which the loader clamps the pixels past npix that it computes
# and never stores; +inf in a halo column.  The reference is an exact fma chain, overflow included, and its ReLU `v > 0 ? v : 0` turns
# NaN and -0 into +0: bit for bit, no NaN.
CONV_IN, CONV_BIAS = _cat(COMMON, INF, NAN), _cat(NEG0, DENORMAL, PLUS_INF, NAN)
C_LO, C_HI = 4, 36    # input channels of the explicitly placed elements: two 32-channel chunks where there are two


def _conv_fixed(values, n, h, w, ci):
    hi = C_HI if ci > 32 else C_LO + 1
    return _fix(values, (NAN, (n - 1, h + 1, w + 1, hi)), (PLUS_INF, (n - 1, 1, w + 1, C_LO)))   # the last pixel; a halo column


def _conv_row(n, h, w, ci, co):
    return Row(lambda: list(_conv_data(n, h, w, ci, co, seed=n + h + w + ci)),
               {0: Put(CONV_IN, _conv_fixed(CONV_IN, n, h, w, ci)), 1: Put(CONV_IN), 2: Put(CONV_BIAS)},
               lambda oracle, inp, filt, bias: oracle.conv_layer(inp, filt, bias),
               {"by_size": Path({}, lambda hl, inp, filt, bias: _conv_run(hl, hl.conv_layer, inp, filt, bias), {"conv3x3_f32_mfma"})})


CONV_SHAPES = [(3, 5, 13, 64, 128), (1, 3, 9, 32, 256)]
for _s in CONV_SHAPES:
    ROWS["conv_layer_%dx%dx%dx%dx%d" % _s] = _conv_row(*_s)

# ---------------------------------------------------------------------------------------------------- conv_layer_bf16
# W = 13, 70 and 126 take conv3x3_bf16_p<6>, conv3x3_bf16_p<8> and the fallback conv3x3_bf16_mfma (conv_bf16_plan).  All three launch
# under the one name conv3x3_bf16_mfma, which tests/golden/launch_plans.json and the benchmark's kernel selection hold in place, so
# the launch record cannot tell them apart: test_conv_bf16_shapes_take_the_three_kernels restates the plan from the source's constants.
#
# Input: COMMON, the infinities, NaN twice (the last pixel and a halo column: both are input-linear positions that are no output
# pixel's centre), and 0x7f7fffff (rounds up to the bf16 infinity), 0x7f7f7fff (stays the largest bf16), 0x3f808000 and 0x3f818000 (ties
# at an even and at an odd bf16).  Filter: magnitudes of at most 4 only (the zeros, the denormals, FLT_MIN, 1e-30, -0.25, 4) plus the
# infinities and NaN.  The oracle forms products and sums in double and the device in f32, so every product of two finite operands and
# every finite `mag` must stay below 2^127 for the two to agree on what overflows: 1e37 stands once, and the input channel C_BIG that
# holds 0x7f7f7fff (3.4e38) has its filter taps scaled by 2^-4 and takes no special filter element.
#
# Whether the matrix core keeps bf16 subnormal operands has a row of its own below; here an operand that rounds to a bf16 subnormal
# never shares its input channel with a non-finite operand of the other tensor (channels by ci % 4: 0 non-finite input, 1 denormal
# input, 2 non-finite filter, 3 denormal filter), so that a failure of these rows names something else.
#
# Comparison: where `mag` is finite the existing rule |got - want| <= 2e-6 mag + 1e-6; where it is not, the output has a non-finite or
# bf16-rounded-to-infinity operand, the order of accumulation cannot change an infinity of one sign or the 0 the ReLU makes of a NaN,
# and got must equal want bit for bit.
BF16_BITS = _bits(0x7f7fffff, 0x7f7f7fff, 0x3f808000, 0x3f818000)
BF16_IN = _cat(COMMON, INF, NAN, NAN, BF16_BITS)
BF16_FILT = _cat(FIRST8, INF, NAN)
C_BIG = 21
BF16_SHAPES = {(1, 3, 13, 64, 128): "conv3x3_bf16_p<6>", (1, 3, 70, 64, 128): "conv3x3_bf16_p<8>", (1, 3, 126, 64, 128): "conv3x3_bf16_mfma"}
BF16_LAUNCHES = {"conv_filter_bf16", "conv3x3_bf16_mfma"}


def _denormal(v):
    return v != 0 and abs(float(v)) < 2.0 ** -126


def _bf16_in_ok(pos, v):
    if v.view(np.uint32) == 0x7f7f7fff:
        return pos[3] == C_BIG
    return pos[3] != C_BIG and (pos[3] % 4 == 0 if not np.isfinite(v) or v.view(np.uint32) == 0x7f7fffff else pos[3] % 4 == 1 if _denormal(v) else True)


def _bf16_filt_ok(pos, v):
    return pos[0] != C_BIG and (pos[0] % 4 == 2 if not np.isfinite(v) else pos[0] % 4 == 3 if _denormal(v) else True)


def _bf16_compare(got, want, what):
    ref, mag = want
    assert got.shape == ref.shape and got.dtype == f32, what
    fin = np.isfinite(mag)
    with np.errstate(invalid="ignore"):
        err, tol = np.abs(got.astype(f64) - ref.astype(f64)), 2e-6 * mag.astype(f64) + 1e-6
    bad = fin & ~(err <= tol)   # a NaN or an infinity of the library where mag is finite is beyond every tolerance
    print(f"{what}: mag finite at {fin.mean():.1%}, worst |got - want| / tolerance there {np.max(np.where(fin & np.isfinite(err), err / tol, 0)):.3f}")
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} of {np.count_nonzero(fin)} beyond tolerance, first at {tuple(np.argwhere(bad)[0])}"
    odd = ~fin & (got.view(np.uint32) != ref.view(np.uint32))
    assert not odd.any(), f"{what}: {np.count_nonzero(odd)} of {np.count_nonzero(~fin)} outputs with a non-finite mag differ in bits, first at {tuple(np.argwhere(odd)[0])}"


def _bf16_base(n, h, w, ci, co):
    inp, filt, bias = _conv_data(n, h, w, ci, co, seed=3 * n + h + w)
    filt[C_BIG] *= f32(2.0 ** -4)
    return [inp, filt, bias]


def _bf16_row(base, puts):
    return Row(base, puts, lambda oracle, inp, filt, bias: oracle.conv_layer_bf16(inp, filt, bias),
               {"by_size": Path({}, lambda hl, inp, filt, bias: _conv_run(hl, hl.conv_layer_bf16, inp, filt, bias), BF16_LAUNCHES)},
               _bf16_compare, lambda w: w[0])


for _s in BF16_SHAPES:
    _n, _h, _w, _ci, _co = _s
    _fixed = _fix(BF16_IN, (NAN, (_n - 1, _h + 1, _w + 1, C_HI)), (NAN, (_n - 1, 1, _w + 1, C_LO)))   # the last pixel; a halo column
    ROWS["conv_layer_bf16_%dx%dx%dx%dx%d" % _s] = _bf16_row(functools.partial(_bf16_base, *_s), {0: Put(BF16_IN, _fixed, _bf16_in_ok), 1: Put(BF16_FILT, (), _bf16_filt_ok)})

# bf16 subnormal operands: the input elements 0x00012345 and 0x80012345 round to the bf16 subnormals +-2^-133 and meet filter elements
# 2^120 at tap SUB_TAP of their input channels, one channel in each 32-channel chunk; everything else of those two channels is zero,
# in the input and in the filter.  Each product is +-2^-13 (1.2e-4) in every output channel of one pixel.  Everything else is noise
# scaled by 2^-6 under a positive bias, so that `mag` is about 0.05 and the tolerance about 1.1e-6, a hundredth of the product, and the
# ReLU clips nothing.  Measured on an MI355X: v_cvt_pk_bf16_f32 and v_mfma_f32_32x32x16_bf16 keep the subnormals, all three kernels are
# within 0.02 of the tolerance on these rows; a matrix core that read them as zero would be 100 tolerances off.
SUB_TAP, SUB_PIXELS = (1, 2), {C_LO: (2, 5), C_HI: (1, 9)}   # (ky, kx); channel -> (y, x) of the input element
SUB_VALUES = _bits(0x00012345, 0x80012345)


def _sub_base(n, h, w, ci, co):
    rng = np.random.default_rng(h + w + ci)
    inp = (rng.uniform(-1, 1, (n, h + 2, w + 2, ci)) * 2.0 ** -6).astype(f32)
    filt = (rng.uniform(-1, 1, (ci, 3, 3, co)) * 2.0 ** -6).astype(f32)
    bias = (rng.uniform(0.5, 1, co) * 2.0 ** -6).astype(f32)
    for c in SUB_PIXELS:
        inp[..., c], filt[c] = 0, 0
        filt[(c,) + SUB_TAP] = f32(2.0 ** 120)
    return [inp, filt, bias]


for _s in BF16_SHAPES:
    _fixed = tuple((i, (0,) + SUB_PIXELS[c] + (c,)) for i, c in enumerate(SUB_PIXELS))
    ROWS["conv_layer_bf16_subnormal_%dx%dx%dx%dx%d" % _s] = _bf16_row(functools.partial(_sub_base, *_s), {0: Put(SUB_VALUES, _fixed)})
SUB_ROWS = [n for n in ROWS if n.startswith("conv_layer_bf16_subnormal")]
BF16_ROWS = [n for n in ROWS if n.startswith("conv_layer_bf16") and n not in SUB_ROWS]

# ---------------------------------------------------------------------------------------------------- depthwise_separable_conv
# (1, 4, 59, 32, 16, 1, 3, 3) is the templated kernel: its tile is 56 pixels, so the row has a full tile and a partial one; by default
# and under HLMI_DSC_NO_A32=1.  The other two run the generic kernel.  Both kernels launch as dsc_fused.  Depthwise filter: +inf at the
# corner tap (0, 0) of one channel and a denormal at tap (fh - 1, fw - 1) of another.  Zero padding is fma(f, 0, acc), so the infinite
# tap over the border gives NaN and the ReLU 0, where a path that skipped out-of-bounds taps would give a number or inf.  Pointwise
# filter: one NaN and one -0; bias: -0 and a denormal.  Bit for bit; the ReLU leaves no NaN.
DSC_SHAPES = [(1, 4, 59, 32, 16, 1, 3, 3), (2, 7, 45, 8, 5, 1, 3, 3), (1, 9, 33, 16, 24, 1, 5, 3)]
DSC_IN, DSC_DW, DSC_PW, DSC_BIAS = _cat(COMMON, INF, NAN), _cat(PLUS_INF, DENORMAL), _cat(NAN, NEG0), _cat(NEG0, DENORMAL)
DSC_INF_CHANNEL, DSC_DENORMAL_CHANNEL = 3, 6


def _dsc_row(n, h, w, ci, co, cm, fw, fh, paths):
    dw_fixed = ((0, (0, 0, DSC_INF_CHANNEL, 0)), (1, (fh - 1, fw - 1, DSC_DENORMAL_CHANNEL, 0)))
    return Row(lambda: list(_dsc_data(n, h, w, ci, co, cm, fw, fh, seed=n + h + w + 1)),
               {0: Put(DSC_IN), 1: Put(DSC_DW, dw_fixed), 2: Put(DSC_PW), 3: Put(DSC_BIAS)},
               lambda oracle, inp, dw, pw, bias: oracle.depthwise_separable_conv(inp, dw, pw, bias),
               {p: Path(env, lambda hl, *a: _dsc_run(hl, *a), {"dsc_fused"}) for p, env in paths.items()})


for _i, _s in enumerate(DSC_SHAPES):
    ROWS["depthwise_separable_conv_" + "x".join(map(str, _s))] = _dsc_row(*_s, {"by_size": {}, "no_a32": {"HLMI_DSC_NO_A32": "1"}} if _i == 0 else {"by_size": {}})
DSC_ROWS = [n for n in ROWS if n.startswith("depthwise")]


# ---------------------------------------------------------------------------------------------------- the inputs and the references
@functools.lru_cache(maxsize=None)
def _inputs(name):
    """(the all-noise inputs, the same with the special values in, [(input, position), ...] of the replaced elements)"""
    row = ROWS[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    base = [np.ascontiguousarray(a, f32) for a in row.base()]
    special, at = [a.copy() for a in base], []
    for i, put in sorted(row.puts.items()):
        fixed, taken = dict(put.fixed), set()
        for j in sorted(range(len(put.values)), key=lambda j: j not in fixed):   # the explicit positions first
            v = put.values[j]
            while True:
                pos = fixed[j] if j in fixed else tuple(int(rng.integers(0, n)) for n in base[i].shape)
                if pos not in taken and (j in fixed or put.ok is None or put.ok(pos, v)):
                    break
                assert j not in fixed, (name, pos)
            taken.add(pos)
            special[i][pos] = v
            at.append((i, pos))
    for a in base + special:
        a.setflags(write=False)
    return base, special, sorted(at)


@functools.lru_cache(maxsize=None)
def _want(name, canon, special=True):
    """what the row's reference makes of its inputs in canonical form `canon` (the oracle's and the checkers' switches both)"""
    import oracle_lib
    with oracle_lib.canon(canon), checker_lib.canon(canon):
        w = ROWS[name].want(oracle_lib, *_inputs(name)[1 if special else 0])
    for a in (w if isinstance(w, tuple) else (w,)):
        a.setflags(write=False)
    return w


def _out(name, canon, special=True):
    return ROWS[name].out(_want(name, canon, special))


def test_table_names_the_pipelines_in_scope():
    pipelines = {re.match(r"gaussian_blur_direct|gaussian_blur|resize|bgu|conv_layer_bf16|conv_layer|depthwise_separable_conv", n).group() for n in ROWS}
    assert pipelines == {"gaussian_blur_direct", "gaussian_blur", "resize", "bgu", "conv_layer", "conv_layer_bf16", "depthwise_separable_conv"}
    assert sorted(n for n in ROWS if n.startswith("resize") and n not in RESIZE_GENERAL_ONLY) == sorted(
        f"resize_{k}_float32_{d}" for k in checker_lib.RESIZE_KERNELS for d in ("up", "down"))
    assert len(ROWS) == 3 + 4 + 8 + 4 + 4 + 2 + 3 + 3 + 3


@pytest.mark.parametrize("name", ROWS)
def test_inputs_hold_what_their_row_says(name):
    row = ROWS[name]
    base, special, at = _inputs(name)
    for i, (b, s) in enumerate(zip(base, special)):
        mine = [pos for j, pos in at if j == i]
        want = row.puts[i].values if i in row.puts else np.array([], f32)
        assert sorted(np.array([s[p] for p in mine], f32).view(np.uint32).tolist()) == sorted(want.view(np.uint32).tolist()), i
        assert sorted(map(tuple, np.argwhere(s.view(np.uint32) != b.view(np.uint32)).tolist())) == mine, i
        assert np.isfinite(b).all()
    for i, put in row.puts.items():
        for j, pos in put.fixed:
            assert special[i][pos].view(np.uint32) == put.values[j].view(np.uint32), (i, pos)


@pytest.mark.parametrize("name", ROWS)
def test_special_elements_sit_where_the_kernels_compute_and_do_not_store(name):
    """Explicitly, not by luck of the seed: the positions below are `fixed` in the table."""
    _, special, at = _inputs(name)
    odd = lambda a: ~np.isfinite(a) | (a == 0) | (np.abs(a) < f32(2.0 ** -126)) | (np.abs(a) > 2)   # noqa: E731  (no noise element is any of these)
    if name.startswith(("gaussian_blur", "resize")):
        img = special[0]
        assert odd(img[..., -1, :]).any() and odd(img[..., :, -1]).any()
        if name in ("gaussian_blur_direct_all", "gaussian_blur_2_1_2") or name.startswith("resize"):
            assert np.isnan(img[..., -1, :]).any() and np.isinf(img[..., :, -1]).any()
        elif name != "gaussian_blur_direct_zero_weights":
            assert np.isfinite(img).all()
    if name == "gaussian_blur_direct_zero_weights":
        (y, x), = np.argwhere(~np.isfinite(special[0]))
        assert special[0][y, x] == np.inf and min(y, GB_H - 1 - y, x, GB_W - 1 - x) >= 16
    if name.startswith("conv_layer"):
        inp = special[0]
        n, hp, wp, ci = inp.shape
        mine = [pos for i, pos in at if i == 0]
        assert len({pos[3] // 32 for pos in mine}) >= min(2, ci // 32)                      # input channels in two 32-channel chunks
        if name not in SUB_ROWS:   # (those are about two products in the middle of the image)
            assert np.isnan(inp[n - 1, hp - 1, wp - 1]).any()                               # the last pixel
            assert not np.isfinite(inp[:, 1:-1, [0, wp - 1]]).all()                         # a halo column, off the corners


@pytest.mark.parametrize("name", ROWS)
def test_reference_output_is_mostly_numbers_and_the_special_values_reach_it(each_canon, name):
    want, plain = _out(name, each_canon), _out(name, each_canon, special=False)
    assert want.shape == plain.shape and want.dtype == plain.dtype == f32 and np.isfinite(plain).all()
    nan = np.isnan(want)
    changed = (want.view(np.uint32) != plain.view(np.uint32)) & ~nan
    print(f"{name} canon {each_canon}: NaN {nan.mean():.1%}, inf {np.isinf(want).mean():.1%}, other differences from noise {changed.mean():.1%}")
    assert nan.mean() <= MAX_NAN_SHARE
    assert changed.any(), "no special element survives to a comparable output"


# ---------------------------------------------------------------------------------------------------- CPU: what single rows are about
def test_zero_weights_row_keeps_meaning_what_it_says(each_canon):
    gc = checker_lib.gaussian_blur
    with checker_lib.canon(each_canon):
        assert gc.radius(1.5, 3) == 5 and gc.radius(1.0, 15) == 15 and gc.radius(1.0, 14) == 14
        kn15, kn14 = gc.kernel_table(1.0, 15)[0], gc.kernel_table(1.0, 14)[0]
    assert np.flatnonzero(kn15 == 0).tolist() == [0, 1, 29, 30] and np.flatnonzero(kn14 == 0).tolist() == [0, 28]
    for kn in (kn15, kn14):   # exact zeros and normal numbers, no denormal
        assert (np.abs(kn[kn != 0]) >= f32(2.0 ** -126)).all() and kn[kn != 0].min() < 1e-36
    # one +inf whose 31 x 31 footprint lies inside the image: the rows at distance 14 and 15 are NaN whole (4 x 31), the 27 others at
    # column distance 14 and 15 (27 x 4); nothing else makes a NaN
    want = _out("gaussian_blur_direct_zero_weights", each_canon)
    (y, x), = np.argwhere(np.isinf(_inputs("gaussian_blur_direct_zero_weights")[1][0]))
    nan = np.zeros(want.shape, bool)
    nan[y - 15:y + 16, x - 15:x + 16] = True
    nan[y - 13:y + 14, x - 13:x + 14] = False
    assert nan.sum() == 232 and np.array_equal(np.isnan(want), nan)
    assert (want[y - 13:y + 14, x - 13:x + 14] == np.inf).all()
    assert np.isfinite(_out("gaussian_blur_direct_zero_weights_finite", each_canon)).all()


@pytest.mark.parametrize("name", RESIZE_ROWS)
def test_resize_rows_hit_both_arms_of_the_clamp(each_canon, name):
    want, plain = _out(name, each_canon), _out(name, each_canon, special=False)
    assert np.isfinite(want).all() and want.min() >= 0 and want.max() <= 1 and not (want.view(np.uint32) == 0x80000000).any()
    for arm in (0x00000000, 0x3f800000):
        assert ((want.view(np.uint32) == arm) & (plain.view(np.uint32) != 0x00000000) & (plain.view(np.uint32) != 0x3f800000)).any(), hex(arm)


@pytest.mark.parametrize("name", RESIZE_GENERAL_ONLY)
def test_resize_general_only_shapes(name):
    """resize.hip: fused_fits and rs_pass_x's `staged`, restated from the source's constants"""
    kernel, up, scale, (c, h, w) = RESIZE_GENERAL_ONLY[name]
    k = lambda const: ph.kernel_const("resize.hip", const)   # noqa: E731
    ow, oh = checker_lib.resize_out_size(w, h, scale)
    inv = f32(1) / f32(scale)
    taps = checker_lib.RESIZE_TAPS[kernel] if up else int(np.ceil(f32(checker_lib.RESIZE_TAPS[kernel]) * inv))
    foot = int(np.ceil(f32(k("FU_Y") if up else k("FT_X")) * inv)) + taps + 3
    assert foot * (k("FT_X") if up else k("FD_Y")) > k("FUSED_LDS")
    begin = checker_lib.resize.tables(kernel, up, scale, 0, ow, 0, w)[0]
    spans = [int(begin[min(x0 + 255, ow - 1)]) + taps - int(begin[x0]) for x0 in range(0, ow, 256)]
    limit = k("PX_LDS") // k("PX_ROWS")
    assert all(s > limit for s in spans) if name in RESIZE_GATHER else all(taps <= s <= limit for s in spans), spans


def test_conv_bf16_shapes_take_the_three_kernels():
    """conv_bf16_plan (halide_amd/csrc/conv_layer_bf16.hip) restated: the window of a 256-position tile is ARp = TQ + 2 (W + 2) + 2 rows;
    conv3x3_bf16_p runs while ARp <= 64 * 8, with 6 staging passes while ARp <= 64 * 6; past it the fallback, since AR <= 32 * 12 fails too."""
    src = open(os.path.join(ph.ROOT, "halide_amd", "csrc", "conv_layer_bf16.hip")).read()
    for text in ("pl.AR = TP + 2 * (g.W + 2) + 2, pl.ARp = TQ + 2 * (g.W + 2) + 2;", "pl.AR <= 32 * 12 &&", "lin && pl.ARp <= 64 * 8 &&", "pers ? pl.ARp > 64 * 6 :",
                 "run(conv3x3_bf16_p<8>, PT, pl.sh_p, pl.ARp, pl.d_img, pl.d_row) : run(conv3x3_bf16_p<6>,", "return run(conv3x3_bf16_mfma, 256, pl.sh_mfma);"):
        assert text in src, text
    tp, tq = ph.kernel_const("conv_layer_bf16.hip", "TP"), ph.kernel_const("conv_layer_bf16.hip", "TQ")
    got = {}
    for (n, h, w, ci, co), kernel in BF16_SHAPES.items():
        ar, arp = tp + 2 * (w + 2) + 2, tq + 2 * (w + 2) + 2
        lin = ar <= 32 * 12
        pers = lin and arp <= 64 * 8 and co % 128 == 0 and ci % 64 == 0
        got[kernel] = "conv3x3_bf16_p<8>" if pers and arp > 64 * 6 else "conv3x3_bf16_p<6>" if pers else "conv3x3_bf16_lin" if lin else "conv3x3_bf16_mfma"
    assert got == {k: k for k in BF16_SHAPES.values()}


@pytest.mark.parametrize("name", BF16_ROWS)
def test_conv_bf16_rows_keep_f32_and_double_agreed_on_what_overflows(each_canon, name):
    base, special, _ = _inputs(name)
    inp, filt, _ = special
    ref, mag = _want(name, each_canon)
    fin = np.isfinite(mag)
    print(f"{name}: mag not finite at {1 - fin.mean():.1%}, largest finite mag {mag[fin].max():.3g}")
    assert mag[fin].max() < 1e38 and 0.02 < 1 - fin.mean() < 0.9      # both comparison rules bite
    assert np.count_nonzero(inp == f32(1e37)) <= 2 and np.abs(filt[np.isfinite(filt)]).max() <= 4
    # no operand that rounds to a bf16 subnormal shares its input channel with a non-finite operand of the other tensor
    sub = lambda a: (a != 0) & (np.abs(a) < f32(2.0 ** -126))            # noqa: E731
    wild = lambda a: ~np.isfinite(a) | (a.view(np.uint32) == 0x7f7fffff)  # noqa: E731
    ci = lambda mask, axis: set(np.argwhere(mask)[:, axis].tolist())      # noqa: E731
    assert not ci(sub(inp), 3) & ci(wild(filt), 0) and not ci(sub(filt), 0) & ci(wild(inp), 3)


@pytest.mark.parametrize("name", SUB_ROWS)
def test_conv_bf16_subnormal_rows_are_two_products_far_above_the_tolerance(each_canon, name):
    (ref, mag), (plain, _) = _want(name, each_canon), _want(name, each_canon, special=False)
    assert np.isfinite(mag).all() and (plain > 0).all() and (ref > 0).all()
    tol = 2e-6 * mag.astype(f64) + 1e-6
    d = ref.astype(f64) - plain.astype(f64)
    for sign, (c, (y, x)) in zip((1, -1), SUB_PIXELS.items()):
        oy, ox = y - SUB_TAP[0], x - SUB_TAP[1]
        assert np.allclose(d[0, oy, ox], sign * 2.0 ** -13, rtol=0, atol=1e-8) and (tol[0, oy, ox] < 2.0 ** -13 / 50).all()
        d[0, oy, ox] = 0
    assert not d.any()


@pytest.mark.parametrize("name", DSC_ROWS)
def test_dsc_infinite_corner_tap_gives_zero_over_the_border(each_canon, name):
    """Tap (0, 0) reads (y - fh / 2, x - fw / 2): over the top rows and left columns it is 0 * inf = NaN in the channel's depthwise sum,
    which every output channel then carries into the ReLU: 0.  Inside it is +-inf, which the pointwise weight's sign and the ReLU make
    inf or 0.  A path that skipped out-of-bounds taps would leave numbers over the border: the same inputs with that tap set to 0 do."""
    import oracle_lib
    _, (inp, dw, pw, bias), _ = _inputs(name)
    fh, fw = dw.shape[:2]
    want = _out(name, each_canon)
    border = np.zeros(want.shape[1:3], bool)
    border[:fh // 2], border[:, :fw // 2] = True, True
    assert (want[:, border].view(np.uint32) == 0).all()
    inside = want[:, ~border]
    assert (np.isinf(inside) | (inside == 0)).all() and np.isinf(inside).mean() > 0.25
    skipped = dw.copy()
    skipped[0, 0, DSC_INF_CHANNEL, 0] = 0
    with oracle_lib.canon(each_canon):
        assert np.count_nonzero(oracle_lib.depthwise_separable_conv(inp, skipped, pw, bias)[:, border]) > 0.25 * want[:, border].size


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name,path", [(n, p) for n, r in ROWS.items() for p in r.paths], ids=lambda v: v)
def test_hip_special_values(hl, oracle, monkeypatch, name, path):
    """Against the reference in the library's canonical form: bit for bit, NaN for NaN; conv_layer_bf16 by its own rule
    (_bf16_compare).  Where the path is forced, or the row is about the path, the launch record must name its kernels."""
    row = ROWS[name]
    p = row.paths[path]
    for k, v in p.env.items():
        monkeypatch.setenv(k, v)
    inputs, got = [a.copy() for a in _inputs(name)[1]], {}
    names = set(ph.launches(hl, lambda: got.update(out=p.run(hl, *inputs))))
    if p.launches is not None:
        assert names == p.launches
    row.compare(np.ascontiguousarray(got["out"]), _want(name, oracle.get_canon()), f"{name} {path}")
