"""ctypes bindings to tests/cpp/hannk_nn_check.c, the plain-C checker of hannk's pooling, mean, add, mul, softmax and l2_normalization ops
and of the approx_* helpers — TEST INFRASTRUCTURE ONLY.  The hkn_* half of hannk_checker.py's one object.  Imports neither the product
nor torch.

Arrays are the Halide dimensions reversed: an activation [c, x, y, b] is an array of shape (B, H, W, C), a rank-2 operand [x, y] one of
shape (rows, n).  Strides are read from the arrays (a transposed or broadcast view is passed as it is); `mins` are Halide-ordered."""
from __future__ import annotations

import numpy as np

from hannk_checker import _estrides, _extents, _ints, _longs, lib

FNS = {"approx_log2": 0, "approx_exp2": 1, "approx_reciprocal": 2, "approx_reciprocal_sqrt": 3}


def _u8(a):
    a = np.asarray(a)
    assert a.dtype == np.uint8
    return a


def _out(extents):
    return np.zeros(tuple(reversed([int(e) for e in extents])), np.uint8)


def approx(fn, q, x, q_x=0, bits=32):
    """fn: a name of FNS or its number; x int32 array (approx_exp2's argument is an i32 here, as in the reference's own test) -> int32"""
    x = np.ascontiguousarray(x, np.int32)
    out = np.zeros(x.shape, np.int32)
    lib().hkn_approx(FNS.get(fn, fn), int(q), x.ctypes.data, x.size, int(q_x), int(bits), out.ctypes.data)
    return out


def pool(kind, inp, out_extents, stride, filt, lo=0, hi=255, in_mins=(0, 0, 0, 0), out_mins=(0, 0, 0, 0)):
    """inp (B, H, W, C) u8 -> dense (OB, OH, OW, C) of Halide extents `out_extents`; kind "average" or "max"; stride, filt: (x, y)"""
    inp = _u8(inp)
    out = _out(out_extents)
    lib().hkn_pool(1 if kind == "average" else 0, inp.ctypes.data, _ints(in_mins), _ints(_extents(inp)), _longs(_estrides(inp)), out.ctypes.data,
                   _ints(out_mins), _ints(_extents(out)), _longs(_estrides(out)), int(stride[0]), int(stride[1]), int(filt[0]), int(filt[1]), int(lo), int(hi))
    return out


def mean(inp, out_extents, rmins, rextents, in_mins=(0, 0, 0, 0), out_mins=(0, 0, 0, 0)):
    inp = _u8(inp)
    out = _out(out_extents)
    lib().hkn_mean(inp.ctypes.data, _ints(in_mins), _longs(_estrides(inp)), _ints(rmins), _ints(rextents), out.ctypes.data, _ints(out_mins),
                   _ints(_extents(out)), _longs(_estrides(out)))
    return out


def add(a, zero1, mul1, b, zero2, mul2, out_zero, lo, hi, out_extents, a_mins=(0, 0), b_mins=(0, 0), out_mins=(0, 0)):
    a, b = _u8(a), _u8(b)
    out = _out(out_extents)
    lib().hkn_add(a.ctypes.data, _ints(a_mins), _longs(_estrides(a)), int(zero1), int(mul1), b.ctypes.data, _ints(b_mins), _longs(_estrides(b)), int(zero2),
                  int(mul2), int(out_zero), int(lo), int(hi), out.ctypes.data, _ints(out_mins), _ints(_extents(out)), _longs(_estrides(out)))
    return out


def mul(a, zero1, b, zero2, out_zero, multiplier, shift, lo, hi, out_extents, a_mins=(0, 0), b_mins=(0, 0), out_mins=(0, 0)):
    a, b = _u8(a), _u8(b)
    out = _out(out_extents)
    lib().hkn_mul(a.ctypes.data, _ints(a_mins), _longs(_estrides(a)), int(zero1), b.ctypes.data, _ints(b_mins), _longs(_estrides(b)), int(zero2),
                  int(out_zero), int(multiplier), int(shift), int(lo), int(hi), out.ctypes.data, _ints(out_mins), _ints(_extents(out)), _longs(_estrides(out)))
    return out


def softmax(inp, beta_multiplier, beta_shift, out_zero, out_multiplier, out_shift, out_extents=None, in_mins=(0, 0), out_mins=(0, 0)):
    """inp (rows, n) u8 (any strides) -> dense (rows', n') of Halide extents `out_extents` (default: the input's)"""
    inp = _u8(inp)
    out = _out(_extents(inp) if out_extents is None else out_extents)
    lib().hkn_softmax(inp.ctypes.data, _ints(in_mins), _ints(_extents(inp)), _longs(_estrides(inp)), int(beta_multiplier), int(beta_shift), int(out_zero),
                      int(out_multiplier), int(out_shift), out.ctypes.data, _ints(out_mins), _ints(_extents(out)), _longs(_estrides(out)))
    return out


def l2_normalization(inp, zero, out_extents=None, in_mins=(0, 0), out_mins=(0, 0)):
    inp = _u8(inp)
    out = _out(_extents(inp) if out_extents is None else out_extents)
    lib().hkn_l2_normalization(inp.ctypes.data, _ints(in_mins), _ints(_extents(inp)), _longs(_estrides(inp)), int(zero), out.ctypes.data, _ints(out_mins),
                               _ints(_extents(out)), _longs(_estrides(out)))
    return out
