"""ctypes bindings to tests/cpp/hannk_program_check.c, the plain-C checker of hannk's Elementwise interpreter, its approx_logistic / approx_tanh
helpers, copy, upsample_channels and the shallow depthwise variant — TEST INFRASTRUCTURE ONLY.  The hkp_* half of hannk_checker.py's one object.
Imports neither the product nor torch.

Arrays are the Halide dimensions reversed: a rank-2 operand [x, y] is an array of shape (rows, n), an activation [c, x, y, b] one of shape
(B, H, W, C).  Strides are read from the arrays (a broadcast view is passed as it is); `mins` are Halide-ordered."""
from __future__ import annotations

import ctypes as C

import numpy as np

from hannk_checker import _estrides, _ints, _longs, lib

FNS = {"approx_log2p1_exp2": 0, "approx_log2m1_exp2": 1, "approx_logistic": 2, "approx_tanh": 3}


def _i32(v, shape):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.int32), shape))


def approx(fn, x, q, q_x, width=16):
    """fn: a name of FNS or its number; x, q, q_x broadcast against each other -> int32.  x is the i16 argument, q the precision of the
    result (Int(16)), q_x that of the argument, `width` the width of the count q_x (16: the generator, 32: the reference's own test)"""
    shape = np.broadcast_shapes(np.shape(x), np.shape(q), np.shape(q_x))
    x, q, q_x = _i32(x, shape), _i32(q, shape), _i32(q_x, shape)
    out = np.zeros(shape, np.int32)
    lib().hkp_approx(FNS.get(fn, fn), x.ctypes.data, q.ctypes.data, q_x.ctypes.data, x.size, int(width), out.ctypes.data)
    return out


def op(code, a, s2, arg3, arg4):
    """one instruction of the interpreter over arrays of its four i16 operands (a = slot[arg1], s2 = slot[arg2]) -> int32"""
    shape = np.broadcast_shapes(np.shape(a), np.shape(s2), np.shape(arg3), np.shape(arg4))
    a, s2, arg3, arg4 = _i32(a, shape), _i32(s2, shape), _i32(arg3, shape), _i32(arg4, shape)
    out = np.zeros(shape, np.int32)
    lib().hkp_op(int(code), a.ctypes.data, s2.ctypes.data, arg3.ctypes.data, arg4.ctypes.data, a.size, out.ctypes.data)
    return out


def elementwise(inputs, program, outputs=1):
    """inputs: five arrays (rows, n) of one dtype, uint8 or int16, any strides with the innermost 0 or one element (views are passed as
    they are); program: (count, 5) int16.  outputs = 1 -> the u8 result; outputs = 2 (int16 inputs) -> (u8, i16).  Raises ValueError
    where an operand is out of range or the program has more than 20 instructions."""
    assert len(inputs) == 5
    dt = inputs[0].dtype
    assert dt in (np.dtype(np.uint8), np.dtype(np.int16)) and all(a.dtype == dt and a.shape == inputs[0].shape for a in inputs)
    program = np.ascontiguousarray(program, np.int16).reshape(-1, 5)
    rows, n = inputs[0].shape
    out0 = np.zeros((rows, n), np.uint8)
    out1 = np.zeros((rows, n), np.int16) if outputs == 2 else None
    ptrs = (C.c_void_p * 5)(*[a.ctypes.data for a in inputs])
    rc = lib().hkp_elementwise(1 if dt == np.dtype(np.int16) else 0, ptrs, _longs([_estrides(a)[0] for a in inputs]), _longs([_estrides(a)[1] for a in inputs]),
                               program.ctypes.data, program.shape[0], out0.ctypes.data, n, None if out1 is None else out1.ctypes.data, n, n, rows)
    if rc:
        raise ValueError(f"program refused ({rc})")
    return out0 if out1 is None else (out0, out1)


def copy(inp, out_extents, pad_value, in_mins=(0, 0, 0, 0), out_mins=(0, 0, 0, 0)):
    """inp (B, H, W, C) u8 -> dense (OB, OH, OW, OC) of Halide extents `out_extents`"""
    inp = np.asarray(inp)
    assert inp.dtype == np.uint8
    out = np.zeros(tuple(reversed([int(e) for e in out_extents])), np.uint8)
    lib().hkp_copy(inp.ctypes.data, _ints(in_mins), _ints(inp.shape[::-1]), _longs(_estrides(inp)), int(pad_value), out.ctypes.data, _ints(out_mins),
                   _ints(out.shape[::-1]), _longs(_estrides(out)))
    return out


def upsample_channels(inp, factor, out_extents, in_mins=(0, 0, 0, 0), out_mins=(0, 0, 0, 0)):
    inp = np.asarray(inp)
    assert inp.dtype == np.uint8
    out = np.zeros(tuple(reversed([int(e) for e in out_extents])), np.uint8)
    lib().hkp_upsample_channels(inp.ctypes.data, _ints(in_mins), _longs(_estrides(inp)), int(factor), out.ctypes.data, _ints(out_mins), _ints(out.shape[::-1]),
                                _longs(_estrides(out)))
    return out


def depthwise_shallow(inp, filt, bias, channels, out_height, stride_y=1, dilation=(1, 1), input_stride_x=1, input_zero=0, filter_zero=0, multiplier=1 << 30,
                      shift=0, zero=0, lo=0, hi=255):
    """inp (B, H, L) u8, the fused c-x row innermost; filt (FH, FW, D) u8; bias int32 (D,) -> dense (B, out_height, channels) u8 (the output's
    dimension 1, of extent 1, left out)"""
    inp, filt = np.ascontiguousarray(inp, np.uint8), np.ascontiguousarray(filt, np.uint8)
    bias = np.ascontiguousarray(bias, np.int32)
    b, h, row = inp.shape
    fh, fw, d = filt.shape
    assert bias.shape == (d,)
    assert channels - 1 + (fw - 1) * dilation[0] * input_stride_x < row and (out_height - 1) * stride_y + (fh - 1) * dilation[1] < h
    out = np.zeros((b, out_height, channels), np.uint8)
    lib().hkp_depthwise_shallow(inp.ctypes.data, row, h, filt.ctypes.data, d, fw, fh, bias.ctypes.data, out.ctypes.data, channels, out_height, b, int(stride_y),
                                int(dilation[0]), int(dilation[1]), int(input_stride_x), int(input_zero), int(filter_zero), int(multiplier), int(shift), int(zero),
                                int(lo), int(hi))
    return out
