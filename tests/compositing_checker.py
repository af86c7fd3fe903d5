"""ctypes bindings to tests/cpp/compositing_check.c, the plain-C checker of compositing — TEST INFRASTRUCTURE ONLY.

The checker is one file of integer arithmetic: a checker_lib.Checker without float forms, so without a canonical-form switch.
tests/test_compositing.py and scripts/fuzz_parity.py both come here.  Imports neither the product nor torch."""
from __future__ import annotations

import ctypes as C

import numpy as np

from checker_lib import Checker

OPS = ("over", "atop", "xor", "in", "out")   # op code = index
LAYERS, NOPS = 6, 5
u8, u16 = np.uint8, np.uint16


def _bind(L):
    P = C.c_void_p
    L.cc_scale16.restype, L.cc_scale16.argtypes = C.c_uint16, [C.c_uint16, C.c_uint8]
    L.cc_scale16_div255.restype, L.cc_scale16_div255.argtypes = C.c_uint16, [C.c_uint16, C.c_uint8]
    L.cc_scale8.restype, L.cc_scale8.argtypes = C.c_uint8, [C.c_uint8, C.c_uint8]
    L.cc_divide.restype, L.cc_divide.argtypes = C.c_uint16, [C.c_uint16, C.c_uint8]
    L.cc_scale16_sweep.restype, L.cc_scale16_sweep.argtypes = None, [P, P, P, P, C.c_size_t]
    L.cc_compositing.restype, L.cc_compositing.argtypes = None, [C.POINTER(P), P, P, C.c_int, C.c_int]


lib = Checker("compositing", ("compositing_check.c",), _bind).lib


def scale16(a, s) -> int:
    return int(lib().cc_scale16(int(a), int(s)))


def scale8(a, s) -> int:
    return int(lib().cc_scale8(int(a), int(s)))


def divide(n, d) -> int:
    return int(lib().cc_divide(int(n), int(d)))


def scale16_sweep(a, s):
    """(the two-shift scale16, the generator comment's (c + 127) / 255) of the pairs (a[i], s[i])"""
    a, s = np.ascontiguousarray(a, u16), np.ascontiguousarray(s, u8)
    assert a.shape == s.shape
    two, div = np.zeros(a.shape, u16), np.zeros(a.shape, u16)
    lib().cc_scale16_sweep(a.ctypes.data, s.ctypes.data, two.ctypes.data, div.ctypes.data, a.size)
    return two, div


def run(layers, ops):
    """layers: six (4, H, W) uint8 arrays, each already cropped to the output's box; ops: five int32 codes.  Returns (4, H, W) uint8."""
    assert len(layers) == LAYERS
    layers = [np.ascontiguousarray(l, u8) for l in layers]
    shape = layers[0].shape
    assert len(shape) == 3 and shape[0] == 4 and all(l.shape == shape for l in layers)
    ops = np.ascontiguousarray(ops, np.int32)
    assert ops.shape == (NOPS,)
    out = np.zeros(shape, u8)
    ptrs = (C.c_void_p * LAYERS)(*[l.ctypes.data for l in layers])
    lib().cc_compositing(ptrs, ops.ctypes.data, out.ctypes.data, shape[2], shape[1])
    return out
