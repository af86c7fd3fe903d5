"""ctypes bindings to tests/cpp/resnet50_check.c, the plain-C checker of apps/resnet_50 — TEST INFRASTRUCTURE ONLY.

A checker_lib.Checker with float forms (a shared object and a canonical-form switch of its own), built with OpenMP; where the host
has the FMA instruction the compiler may emit it for fmaf (-mfma).  Imports neither the product nor torch.

Arrays are the Halide dimensions reversed, float32, the innermost axis dense, rows and planes possibly padded: an activation (c, x, y) is
an array of shape (H, W, C), convolution weights (co, kx, ky, ci) one of shape (CI, KH, KW, CO), fc weights (n, c) one of shape (C, N)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from checker_lib import Checker, host_has_fma

MODES = ("raw", "scaled", "scaled_relu", "residual_relu")
NCONV = 53
f32 = np.float32


def _bind(L):
    I, P, N = C.c_int, C.c_void_p, C.c_long
    L.rn_out_extent.restype, L.rn_out_extent.argtypes = I, [I, I, I, I]
    L.rn_conv.restype, L.rn_conv.argtypes = None, [P, N, N, P, N, N, N, P, P, P, P, P, N, N, P, N, N] + [I] * 9
    L.rn_maxpool.restype, L.rn_maxpool.argtypes = None, [P, N, N, P, N, N] + [I] * 6
    L.rn_tail.restype, L.rn_tail.argtypes = None, [P, N, N, I, I, I, P, N, P, I, P, P, P, P]
    L.rn_network.restype, L.rn_network.argtypes = None, [P, P, P, P, P, P, P]


checker = Checker("resnet50", ("resnet50_check.c",), _bind, float_forms=True,
                  flags=["-ftree-vectorize", "-fopenmp"] + (["-mfma"] if host_has_fma() else []))
lib, set_canon, get_canon, canon = checker.lib, checker.set_canon, checker.get_canon, checker.canon


def out_extent(size, k, stride, pad):
    """compute_shape (Resnet50Generator.cpp:245-251), truncating"""
    return (pad * 2 + size - k + 1 + stride - 1) // stride


def _arr(a, ndim):
    a = np.asarray(a)
    assert a.ndim == ndim and a.dtype == f32 and (a.shape[-1] <= 1 or a.strides[-1] == 4), (a.shape, a.dtype, a.strides)
    return a


def _strides(a):
    """element strides of every axis but the innermost, innermost first (Halide dimensions 1, 2, ...)"""
    return [s // 4 for s in a.strides[-2::-1]]


def _p(a):
    return None if a is None else a.ctypes.data


def conv(inp, weights, gamma=None, beta=None, mu=None, sig=None, residual=None, stride=1, pad=0, mode="raw"):
    """one convolution layer: inp (H, W, CI), weights (CI, KH, KW, CO), the four vectors (CO,), residual (OH, OW, CO) in the last mode;
    returns a dense (OH, OW, CO) array"""
    inp, weights = _arr(inp, 3), _arr(weights, 4)
    mode = MODES.index(mode) if isinstance(mode, str) else int(mode)
    H, W, CI = inp.shape
    ci2, KH, KW, CO = weights.shape
    assert ci2 == CI
    OW, OH = out_extent(W, KW, stride, pad), out_extent(H, KH, stride, pad)
    assert OW > 0 and OH > 0
    vec = [None] * 4
    if mode:
        vec = [np.ascontiguousarray(_arr(v, 1)) for v in (gamma, beta, mu, sig)]
        assert all(v.shape == (CO,) for v in vec)
    rs = [0, 0]
    if mode == 3:
        residual = _arr(residual, 3)
        assert residual.shape == (OH, OW, CO)
        rs = _strides(residual)
    out = np.empty((OH, OW, CO), f32)
    (isx, isy), (wkx, wky, wci) = _strides(inp), _strides(weights)
    lib().rn_conv(_p(inp), isx, isy, _p(weights), wkx, wky, wci, *[_p(v) for v in vec], _p(residual) if mode == 3 else None, rs[0], rs[1],
                  _p(out), CO, CO * OW, CI, W, H, CO, KW, KH, stride, pad, mode)
    return out


def maxpool(inp, k, stride, pad):
    """inp (H, W, C) -> dense (OH, OW, C)"""
    inp = _arr(inp, 3)
    H, W, Cn = inp.shape
    OW, OH = out_extent(W, k, stride, pad), out_extent(H, k, stride, pad)
    out = np.empty((OH, OW, Cn), f32)
    isx, isy = _strides(inp)
    lib().rn_maxpool(_p(inp), isx, isy, _p(out), Cn, Cn * OW, Cn, W, H, k, stride, pad)
    return out


def tail(inp, fc_weights, fc_bias):
    """inp (H, W, C), fc_weights (C, N), fc_bias (N,) -> dict(pool (C,), fc (N,), e (N,), out (N,))"""
    inp, fw, fb = _arr(inp, 3), _arr(fc_weights, 2), np.ascontiguousarray(_arr(fc_bias, 1))
    H, W, Cn = inp.shape
    N = fb.size
    assert fw.shape == (Cn, N)
    r = dict(pool=np.empty(Cn, f32), fc=np.empty(N, f32), e=np.empty(N, f32), out=np.empty(N, f32))
    isx, isy = _strides(inp)
    lib().rn_tail(_p(inp), isx, isy, Cn, W, H, _p(fw), _strides(fw)[0], _p(fb), N, _p(r["pool"]), _p(r["fc"]), _p(r["e"]), _p(r["out"]))
    return r


def network(inp, params):
    """the whole network: inp (224, 224, 3) and the 267 parameters in signature order -> dict(pool (2048,), fc (1000,), out (1000,))"""
    inp = np.ascontiguousarray(_arr(inp, 3))
    assert inp.shape == (224, 224, 3) and len(params) == 5 * NCONV + 2
    params = [np.ascontiguousarray(p, f32) for p in params]
    ptrs = (C.c_void_p * (5 * NCONV))(*[p.ctypes.data for p in params[:5 * NCONV]])
    assert params[-2].shape == (2048, 1000) and params[-1].shape == (1000,)
    r = dict(pool=np.empty(2048, f32), fc=np.empty(1000, f32), out=np.empty(1000, f32))
    lib().rn_network(_p(inp), ptrs, _p(params[-2]), _p(params[-1]), _p(r["pool"]), _p(r["fc"]), _p(r["out"]))
    return r
