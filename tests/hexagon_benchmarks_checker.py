"""ctypes bindings to tests/cpp/hexagon_benchmarks_check.c, the plain-C checker of the six filters of apps/hexagon_benchmarks — TEST
INFRASTRUCTURE ONLY.

The checker is one file of integer arithmetic: a checker_lib.Checker without float forms, so without a canonical-form switch.
tests/test_hexagon_benchmarks.py and scripts/fuzz_parity.py both come here.  Imports neither the product nor torch."""
from __future__ import annotations

import ctypes as C

import numpy as np

from checker_lib import Checker
from parity_helpers import DevArray

NAMES = ("conv3x3a16", "conv3x3a32", "dilate3x3", "median3x3", "gaussian5x5", "sobel")
MASKED = ("conv3x3a16", "conv3x3a32")
HALO = {n: (2 if n == "gaussian5x5" else 1) for n in NAMES}
DRIVER_MASK = np.array([[1, -4, 7], [2, -5, 8], [3, -6, 9]], np.int8)   # [i][j] = mask(j, i), as process.h fills it


def _bind(L):
    P, I, G = C.c_void_p, C.c_int, C.c_long
    for n in NAMES:
        for f in (getattr(L, "hb_" + n), getattr(L, "hb_" + n + "_verify")):
            f.restype = None
            f.argtypes = [P, I, I, G] + ([P] if n in MASKED else []) + [P, I, I, I, I]
    L.hb_conv3x3_sum.restype, L.hb_conv3x3_sum.argtypes = None, [P, I, I, G, P, P, I, I, I, I]


lib = Checker("hexagon_benchmarks", ("hexagon_benchmarks_check.c",), _bind).lib


def _plane(image):
    image = np.asarray(image)
    assert image.ndim == 2 and image.dtype == np.uint8 and image.strides[1] == 1 and image.shape[0] > 0 and image.shape[1] > 0
    return image, image.strides[0] if image.shape[0] > 1 else image.shape[1]


def _mask(name, mask):
    if name not in MASKED:
        assert mask is None
        return []
    m = np.ascontiguousarray(mask, np.int8)
    assert m.shape == (3, 3)
    return [m]


def run(name, image, mask=None, region=None, verify=False):
    """The filter `name` of the (H, W) uint8 `image` (sample (0, 0) its first element) over the output region (ox, oy, ow, oh), by
    default the image's own box; mask: (3, 3) int8, [i][j] = mask(j, i), for the two conv3x3 filters.  verify: the restatement of
    process.h's verifier instead of the generator's.  Returns (oh, ow) uint8."""
    image, stride = _plane(image)
    ox, oy, ow, oh = region if region is not None else (0, 0, image.shape[1], image.shape[0])
    out = np.zeros((oh, ow), np.uint8)
    m = _mask(name, mask)
    f = getattr(lib(), "hb_" + name + ("_verify" if verify else ""))
    f(image.ctypes.data, image.shape[1], image.shape[0], stride, *[a.ctypes.data for a in m], out.ctypes.data, ox, oy, ow, oh)
    return out


def conv_sum(image, mask, region=None):
    """the int32 sum of the 3x3 window before the shift, (oh, ow) int32"""
    image, stride = _plane(image)
    ox, oy, ow, oh = region if region is not None else (0, 0, image.shape[1], image.shape[0])
    out = np.zeros((oh, ow), np.int32)
    m = np.ascontiguousarray(mask, np.int8)
    lib().hb_conv3x3_sum(image.ctypes.data, image.shape[1], image.shape[0], stride, m.ctypes.data, out.ctypes.data, ox, oy, ow, oh)
    return out


class DevPlane(DevArray):
    """An (H, W) uint8 plane inside a flat device allocation of its own, wrapped as a device-only buffer: the row stride and the
    byte offset of the first element from the allocation's start (which is 256-byte aligned) are the caller's.  `hl` is the product
    module.  parity_helpers.DevArray for one uint8 plane: `result()` returns the plane as the device holds it and asserts that
    every byte outside it (a sentinel) is as it was."""

    def __init__(self, hl, h, w, row_stride=None, offset=0, mins=None, fill=None):
        super().__init__(hl, (h, w), np.uint8, row_stride, offset=offset, mins=mins, fill=fill)
