"""ctypes bindings to tests/cpp/hannk_check.c, the plain-C checker of the hannk convolution ops — TEST INFRASTRUCTURE ONLY.  Declares the one checker_lib.Checker of
the three hannk checkers (hannk_check.c and hannk_program_check.c, which includes hannk_nn_check.c: hk_*, hkn_* and hkp_* in one object,
integer throughout, no canonical-form switch) with all its signatures; hannk_nn_checker.py and hannk_program_checker.py take `lib` and the
argument helpers from here.  Imports neither the product nor torch.

Arrays are the Halide dimensions reversed, the innermost axis dense, the outer ones possibly padded (strides are read from the array): an
activation [c, x, y, b] is an array of shape (B, H, W, C), the tiled filter [4, 16, ci / 4, co / 16, fx, fy] one of shape
(FH, FW, CO16, CQ, 16, 4), a depthwise filter [c, fx, fy] one of shape (FH, FW, C).  `mins` are Halide-ordered (dimension 0 first)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from checker_lib import Checker

VECTOR_REDUCTION, ACCUM_VECTOR_SIZE, DEPTHWISE_VECTOR = 4, 16, 16


def _bind(L):
    I, P, N, U = C.c_int32, C.c_void_p, C.c_long, C.c_uint8                 # hannk_check.c
    L.hk_multiply_2x_high.restype, L.hk_multiply_2x_high.argtypes = I, [I, I]
    L.hk_rounding_shift_right.restype, L.hk_rounding_shift_right.argtypes = I, [I, I]
    L.hk_quantize_i16.restype, L.hk_quantize_i16.argtypes = C.c_int16, [I, I, I]
    L.hk_quantize_and_relu_u8.restype, L.hk_quantize_and_relu_u8.argtypes = U, [I, I, I, U, U, U]
    L.hk_quantize.restype, L.hk_quantize.argtypes = None, [C.c_int, P, N, I, I, U, U, U, P]
    L.hk_tile_filter.restype, L.hk_tile_filter.argtypes = None, [P, P, P, P, U, U, P, P, P, P]
    L.hk_conv.restype = None
    L.hk_conv.argtypes = [P, P, P, P, P, C.c_int, C.c_int, C.c_int, P, P, P, P, P] + [C.c_int] * 5 + [U, U, I, I, U, U, U]
    L.hk_depthwise.restype = None
    L.hk_depthwise.argtypes = [P, P, P, P, P, C.c_int, C.c_int, P, P, P, P, P] + [C.c_int] * 5 + [U, U, I, I, U, U, U]
    I = C.c_int                                                               # hannk_nn_check.c
    L.hkn_approx.restype, L.hkn_approx.argtypes = None, [I, I, P, N, I, I, P]
    L.hkn_pool.restype, L.hkn_pool.argtypes = None, [I, P, P, P, P, P, P, P, P, I, I, I, I, I, I]
    L.hkn_mean.restype, L.hkn_mean.argtypes = None, [P] * 9
    L.hkn_add.restype, L.hkn_add.argtypes = None, [P, P, P, I, I, P, P, P, I, I, I, I, I, P, P, P, P]
    L.hkn_mul.restype, L.hkn_mul.argtypes = None, [P, P, P, I, P, P, P, I, I, C.c_int32, C.c_uint32, I, I, P, P, P, P]
    L.hkn_softmax.restype, L.hkn_softmax.argtypes = None, [P, P, P, P, I, C.c_uint, I, I, C.c_uint, P, P, P, P]
    L.hkn_l2_normalization.restype, L.hkn_l2_normalization.argtypes = None, [P, P, P, P, I, P, P, P, P]
    L.hkp_approx.restype, L.hkp_approx.argtypes = None, [I, P, P, P, N, I, P]   # hannk_program_check.c
    L.hkp_op.restype, L.hkp_op.argtypes = None, [I, P, P, P, P, N, P]
    L.hkp_elementwise.restype, L.hkp_elementwise.argtypes = I, [I, P, P, P, P, I, P, N, P, N, I, I]
    L.hkp_copy.restype, L.hkp_copy.argtypes = None, [P, P, P, P, I, P, P, P, P]
    L.hkp_upsample_channels.restype, L.hkp_upsample_channels.argtypes = None, [P, P, P, I, P, P, P, P]
    L.hkp_depthwise_shallow.restype, L.hkp_depthwise_shallow.argtypes = None, [P, I, I, P, I, I, I, P, P, I, I, I] + [I] * 6 + [C.c_int32, C.c_int32, I, I, I]


lib = Checker("hannk", ("hannk_check.c", "hannk_program_check.c"), _bind).lib


def _ints(v):
    return (C.c_int * len(v))(*[int(x) for x in v])


def _longs(v):
    return (C.c_long * len(v))(*[int(x) for x in v])


def _estrides(a):
    """element strides, Halide order (innermost first)"""
    return [s // a.itemsize for s in a.strides[::-1]]


def _extents(a):
    return list(a.shape[::-1])


def multiply_2x_high(a, b):
    return int(lib().hk_multiply_2x_high(int(a), int(b)))


def rounding_shift_right(a, s):
    return int(lib().hk_rounding_shift_right(int(a), int(s)))


def quantize_i16(acc, multiplier, shift):
    return int(lib().hk_quantize_i16(int(acc), int(multiplier), int(shift)))


def quantize_and_relu_u8(acc, multiplier, shift, zero, lo, hi):
    return int(lib().hk_quantize_and_relu_u8(int(acc), int(multiplier), int(shift), int(zero), int(lo), int(hi)))


def quantize(fn, acc, multiplier, shift, zero=0, lo=0, hi=255):
    """fn 0 / "i16": quantize_i16 -> int16; fn 1 / "u8": quantize_and_relu_u8 -> uint8; over an int32 array"""
    fn = {"i16": 0, "u8": 1}.get(fn, fn)
    acc = np.ascontiguousarray(acc, np.int32)
    out = np.zeros(acc.shape, np.int16 if fn == 0 else np.uint8)
    lib().hk_quantize(fn, acc.ctypes.data, acc.size, int(multiplier), int(shift), int(zero), int(lo), int(hi), out.ctypes.data)
    return out


def tile_filter(inp, input_zero, output_zero, out_extents, in_mins=(0, 0, 0, 0), out_mins=(0, 0, 0, 0, 0, 0)):
    """inp (CO, FH, FW, CI) u8 (Halide [ci, x, y, co]) -> the tiled array of Halide extents `out_extents` = [4, 16, cq, co16, fw, fh]"""
    inp = np.asarray(inp)
    assert inp.dtype == np.uint8 and inp.ndim == 4 and len(out_extents) == 6
    out = np.zeros(tuple(reversed([int(e) for e in out_extents])), np.uint8)
    lib().hk_tile_filter(inp.ctypes.data, _ints(in_mins), _ints(_extents(inp)), _longs(_estrides(inp)), int(input_zero), int(output_zero),
                         out.ctypes.data, _ints(out_mins), _ints(_extents(out)), _longs(_estrides(out)))
    return out


def tile(filter, filter_zero):
    """the whole filter (CO, FH, FW, CI) tiled for conv, padded entries filter_zero: shape (FH, FW, CO16, CQ, 16, 4)"""
    co, fh, fw, ci = np.asarray(filter).shape
    return tile_filter(filter, filter_zero, filter_zero, [4, 16, -(-ci // 4), -(-co // 16), fw, fh])


def out_extent(size, filt, stride, dilation, padding=0):
    return (int(size) + 2 * int(padding) - (int(filt) - 1) * int(dilation) - 1) // int(stride) + 1


def conv(inp, tiled, bias, out_extents, stride=(1, 1), dilation=(1, 1), input_zero=0, filter_zero=0, multiplier=1 << 30, shift=0, zero=0, lo=0, hi=255,
         out_dtype=np.uint8, in_mins=(0, 0, 0, 0), out_mins=(0, 0, 0, 0)):
    """inp (B, H, W, 4 CQ) u8, tiled (FH, FW, CO16, CQ, 16, 4) u8, bias int32 (C,), out_extents Halide [C, OW, OH, OB] -> dense (OB, OH, OW, C)"""
    inp, tiled = np.asarray(inp), np.asarray(tiled)
    bias = np.ascontiguousarray(bias, np.int32)
    assert inp.dtype == np.uint8 and tiled.dtype == np.uint8 and tiled.ndim == 6 and tiled.shape[4:] == (16, 4)
    fh, fw, co16, cq = tiled.shape[:4]
    assert inp.shape[3] == 4 * cq and co16 * 16 >= out_extents[0] and bias.size >= out_extents[0]
    i16 = np.dtype(out_dtype) == np.dtype(np.int16)
    out = np.zeros(tuple(reversed([int(e) for e in out_extents])), np.int16 if i16 else np.uint8)
    lib().hk_conv(inp.ctypes.data, _ints(in_mins), _longs(_estrides(inp)), tiled.ctypes.data, _longs(_estrides(tiled)), cq, fw, fh, bias.ctypes.data,
                  out.ctypes.data, _ints(out_mins), _ints(_extents(out)), _longs(_estrides(out)), int(i16), int(stride[0]), int(stride[1]),
                  int(dilation[0]), int(dilation[1]), int(input_zero), int(filter_zero), int(multiplier), int(shift), int(zero), int(lo), int(hi))
    return out


def depthwise(inp, filt, bias, out_extents, stride=(1, 1), dilation=(1, 1), input_zero=0, filter_zero=0, multiplier=1 << 30, shift=0, zero=0, lo=0,
              hi=255, broadcast=False, in_mins=(0, 0, 0, 0), out_mins=(0, 0, 0, 0)):
    """inp (B, H, W, CIN) u8, filt (FH, FW, C) u8, bias int32 (C,), out_extents Halide [C, OW, OH, OB] -> dense (OB, OH, OW, C) u8"""
    inp, filt = np.asarray(inp), np.asarray(filt)
    bias = np.ascontiguousarray(bias, np.int32)
    assert inp.dtype == np.uint8 and filt.dtype == np.uint8 and filt.ndim == 3
    fh, fw, c = filt.shape
    assert c >= out_extents[0] and bias.size >= out_extents[0] and (broadcast or inp.shape[3] >= out_extents[0])
    out = np.zeros(tuple(reversed([int(e) for e in out_extents])), np.uint8)
    lib().hk_depthwise(inp.ctypes.data, _ints(in_mins), _longs(_estrides(inp)), filt.ctypes.data, _longs(_estrides(filt)), fw, fh, bias.ctypes.data,
                       out.ctypes.data, _ints(out_mins), _ints(_extents(out)), _longs(_estrides(out)), 0 if broadcast else 1, int(stride[0]),
                       int(stride[1]), int(dilation[0]), int(dilation[1]), int(input_zero), int(filter_zero), int(multiplier), int(shift), int(zero),
                       int(lo), int(hi))
    return out
