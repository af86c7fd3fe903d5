#!/usr/bin/env python3
"""Randomised parity sweep: every pipeline on random shapes / origins / parameters, GPU result vs oracle, bit for bit.

    python scripts/fuzz_parity.py [--seed S] [--seconds T] [--only a,b]

Not part of the pytest suite (the suite pins fixed cases); this is the tool that looks for cases the suite does not have.
Prints one line per pipeline (cases run, failures) and the parameters of every failure.  Uses oracle/ as the checker
only (tests/oracle_lib.py) and, for the pipelines oracle/ does not restate, the plain-C checkers (tests/checker_lib.py)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import halide_amd as hl  # noqa: E402
import oracle_lib as oracle  # noqa: E402

oracle.set_canon(hl.canon_fma())   # the oracle evaluates the canonical form the loaded library was built for


def checkers():
    """tests/checker_lib.py in the same form.  Loaded (and its object built) by the three cases that use it, not at import: the
    other pipelines' cases need oracle/ only.  Every thread sets the same value, so the call is safe from any of them."""
    import checker_lib
    checker_lib.set_canon(hl.canon_fma())
    return checker_lib

f32 = np.float32


def image_u16(rng, w, h, kind):
    if kind == 0:
        return rng.integers(0, 65536, (3, h, w), dtype=np.uint16)
    yy, xx = np.mgrid[0:h, 0:w].astype(f32)
    base = (np.sin(xx / 31.0 + rng.random() * 6) + np.cos(yy / 17.0) + 2.2) / 4.4
    img = np.stack([base * 65535.0, np.roll(base, 5, 1) * 52000.0, base[::-1] * 46000.0]) + rng.normal(0, 900, (3, h, w))
    if kind == 2:
        img[:, : h // 2] = rng.integers(0, 2) * 65535          # flat saturated / black half
    return np.clip(img, 0, 65535).astype(np.uint16)


def image_f32(rng, c, w, h):
    yy, xx = np.mgrid[0:h, 0:w].astype(f32)
    return np.stack([(np.sin(xx / (7.0 + i) + rng.random() * 6) + np.cos(yy / (11.0 - i))) * 0.23 + 0.5 + rng.random((h, w)) * 0.1
                     for i in range(c)]).astype(f32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def rdim(rng, lo, hi):
    """Sizes with a bias to the small and to tile multiples +-1."""
    r = rng.random()
    if r < 0.3:
        return int(rng.integers(lo, min(hi, lo + 20) + 1))
    if r < 0.6:
        base = int(rng.choice([32, 64, 128, 256])) * int(rng.integers(1, 4)) + int(rng.integers(-1, 2))
        return int(min(max(base, lo), hi))
    return int(rng.integers(lo, hi + 1))


# ---- one random case per call; each returns (description, ok)
def case_local_laplacian(rng):
    w, h = rdim(rng, 1, 700), rdim(rng, 1, 500)
    # the fast path (ll_down01e / ll_up0h: levels == 8, width a multiple of 4, even output origin and width) gets most of the draws
    levels = 8 if rng.random() < 0.6 else int(rng.integers(2, 9))
    if rng.random() < 0.6:
        w = max(4, (w + 3) & ~3)
    alpha, beta = f32(rng.choice([1.0 / 7.0, 0.5, 1.0, 0.05]) / max(levels - 1, 1)), f32(rng.choice([1.0, 0.5, 2.0, 0.0]))
    ox, oy = (int(rng.integers(-40, 40)), int(rng.integers(-40, 40))) if rng.random() < 0.5 else (0, 0)
    inp = image_u16(rng, w, h, int(rng.integers(0, 3)))
    a = hl.Buffer(inp).set_min(ox, oy, 0)
    want = oracle.local_laplacian(inp, levels, alpha, beta, origin=(ox, oy))
    crop = ""
    if rng.random() < 0.25 and w >= 8 and h >= 4:
        # the output region strictly inside the input (taps clamp at the INPUT's edges: the crop of the full result is expected)
        x0, y0 = int(rng.integers(0, w // 2)) & ~1, int(rng.integers(0, h // 2))
        cw, ch = max(2, int(rng.integers(1, w - x0 + 1)) & ~1), int(rng.integers(1, h - y0 + 1))
        o = hl.Buffer(np.zeros((3, ch, cw), np.uint16)).set_min(ox + x0, oy + y0, 0)
        want = want[:, y0:y0 + ch, x0:x0 + cw]
        crop = f" crop=({x0},{y0},{cw},{ch})"
    else:
        o = hl.Buffer(np.zeros_like(inp)).set_min(ox, oy, 0)
    hl.local_laplacian(a, levels, alpha, beta, o)
    return f"{w}x{h} levels={levels} alpha={alpha} beta={beta} origin=({ox},{oy}){crop}", same(o.numpy(), want)


def case_bilateral_grid(rng):
    w, h = rdim(rng, 1, 600), rdim(rng, 1, 400)
    r_sigma = f32(rng.choice([0.1, 0.05, 0.25, 0.5]))
    inp = image_f32(rng, 1, w, h)[0]
    a, o = hl.Buffer(inp), hl.Buffer(np.zeros_like(inp))
    hl.bilateral_grid(a, r_sigma, o)
    return f"{w}x{h} r_sigma={r_sigma}", same(o.numpy(), oracle.bilateral_grid(inp, r_sigma))


def case_nl_means(rng):
    w, h = rdim(rng, 1, 300), rdim(rng, 1, 200)
    fast = rng.random() < 0.7
    patch, search = (7, 7) if fast else (int(rng.choice([1, 3, 5])), int(rng.choice([1, 3, 5, 9])))
    if not fast:
        w, h = min(w, 64), min(h, 48)
    sigma = f32(rng.choice([0.12, 0.05, 0.5]))
    inp = image_f32(rng, 3, w, h)
    a, o = hl.Buffer(inp), hl.Buffer(np.zeros_like(inp))
    hl.nl_means(a, patch, search, sigma, o)
    return f"{w}x{h} patch={patch} search={search} sigma={sigma}", same(o.numpy(), oracle.nl_means(inp, patch, search, sigma))


def case_stencil_chain(rng):
    w, h = rdim(rng, 1, 500), rdim(rng, 1, 400)
    inp = rng.integers(0, 65536, (h, w), dtype=np.uint16)
    a, o = hl.Buffer(inp), hl.Buffer(np.zeros_like(inp))
    hl.stencil_chain(a, o)
    return f"{w}x{h}", same(o.numpy(), oracle.stencil_chain(inp))


def case_halide_blur(rng):
    w, h = rdim(rng, 1, 600), rdim(rng, 1, 400)
    inp = rng.integers(0, 65536, (h + 2, w + 2), dtype=np.uint16)
    a, o = hl.Buffer(inp), hl.Buffer(np.zeros((h, w), np.uint16))
    hl.halide_blur(a, o)
    return f"{w}x{h}", same(o.numpy(), oracle.blur(inp))


def case_unsharp(rng):
    w, h = rdim(rng, 1, 500), rdim(rng, 1, 400)
    inp = image_f32(rng, 3, w + 6, h + 6)
    a, o = hl.Buffer(inp).set_min(-3, -3, 0), hl.Buffer(np.zeros((3, h, w), f32))
    hl.unsharp(a, o)
    return f"{w}x{h}", same(o.numpy(), oracle.unsharp(inp, (0, 0), (w, h), (-3, -3)))


def case_harris(rng):
    w, h = rdim(rng, 1, 500), rdim(rng, 1, 400)
    inp = image_f32(rng, 3, w + 4, h + 4)
    a, o = hl.Buffer(inp).set_min(1, 1, 0), hl.Buffer(np.zeros((h, w), f32)).set_min(3, 3)
    hl.harris(a, o)
    return f"{w}x{h}", same(o.numpy(), oracle.harris(inp, (3, 3), (w, h), (1, 1)))


def case_max_filter(rng):
    w, h = rdim(rng, 1, 300), rdim(rng, 1, 200)
    inp = image_f32(rng, 3, w, h)
    a, o = hl.Buffer(inp), hl.Buffer(np.zeros_like(inp))
    hl.max_filter(a, o)
    return f"{w}x{h}", same(o.numpy(), oracle.max_filter(inp))


def case_hist(rng):
    w, h = rdim(rng, 1, 600), rdim(rng, 1, 400)
    inp = rng.integers(0, 256, (3, h, w), dtype=np.uint8) if rng.random() < 0.5 else (image_f32(rng, 3, w, h) * 255).astype(np.uint8)
    a, o = hl.Buffer(inp), hl.Buffer(np.zeros_like(inp))
    hl.hist(a, o)
    return f"{w}x{h}", same(o.numpy(), oracle.hist(inp))


def case_interpolate(rng):
    w, h = rdim(rng, 1, 500), rdim(rng, 1, 400)
    inp = image_f32(rng, 4, w, h)
    inp[3] = (rng.random((h, w)) > rng.random()).astype(f32) * inp[3]
    a, o = hl.Buffer(inp), hl.Buffer(np.zeros((3, h, w), f32))
    hl.interpolate(a, o)
    return f"{w}x{h}", same(o.numpy(), oracle.interpolate(inp))


def case_iir_blur(rng):
    w, h, c = rdim(rng, 1, 400), rdim(rng, 1, 400), int(rng.integers(1, 4))
    alpha = f32(rng.choice([0.1, 0.5, 0.9, 1.0]))
    inp = image_f32(rng, c, w, h)
    a, o = hl.Buffer(inp), hl.Buffer(np.zeros_like(inp))
    hl.iir_blur(a, alpha, o)
    return f"{w}x{h}x{c} alpha={alpha}", same(o.numpy(), oracle.iir_blur(inp, alpha))


def case_bgu(rng):
    W, H = rdim(rng, 8, 500), rdim(rng, 8, 400)
    factor = int(rng.choice([1, 2, 4, 8]))
    lw, lh = max(1, W // factor), max(1, H // factor)
    hi = image_f32(rng, 3, W, H)
    lo = image_f32(rng, 3, lw, lh)
    val = np.clip(lo * lo * (3 - 2 * lo) + rng.normal(0, 0.02, lo.shape), 0, 1).astype(f32)
    r_sigma, s_sigma = f32(rng.choice([1 / 8, 1 / 4, 1 / 16, 0.3])), int(rng.choice([16, 8, 5, 3, 2]))
    x0, y0 = int(rng.integers(0, W)), int(rng.integers(0, H))
    reg = (x0, y0, int(rng.integers(1, W - x0 + 1)), int(rng.integers(1, H - y0 + 1))) if rng.random() < 0.4 else (0, 0, W, H)
    bo = hl.Buffer(np.zeros((3, reg[3], reg[2]), f32)).set_min(reg[0], reg[1], 0)
    hl.bgu(r_sigma, s_sigma, hl.Buffer(lo), hl.Buffer(val), hl.Buffer(hi), bo)
    want = oracle.bgu(r_sigma, s_sigma, lo, val, hi, region=reg)
    return f"{W}x{H} /{factor} r={r_sigma} s={s_sigma} region={reg}", same(bo.numpy(), want)


def case_lens_blur(rng):
    w, h = rdim(rng, 1, 160), rdim(rng, 1, 120)
    slices = int(rng.integers(1, 33))
    focus = int(rng.integers(1, min(slices, 32) + 1))
    scale, samples = f32(rng.choice([0.5, 1.0, 0.2, 0.0])), int(rng.integers(1, 40))
    left = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
    right = np.roll(left, int(rng.integers(0, 9)), 2)
    o = hl.Buffer(np.zeros((3, h, w), f32))
    hl.lens_blur(hl.Buffer(left), hl.Buffer(right), slices, focus, scale, samples, o)
    return f"{w}x{h} slices={slices} focus={focus} scale={scale} samples={samples}", same(o.numpy(), oracle.lens_blur(left, right, slices, focus, scale, samples))


def case_camera_pipe(rng):
    ow, oh = 2 * rdim(rng, 1, 160), 2 * rdim(rng, 1, 120)   # even output sizes, like the reference's 2x2 demosaic tiles
    raw = rng.integers(0, 1024, (oh + 32, ow + 40), dtype=np.uint16)   # the generator's footprint: 40 x 32 more than the output
    if rng.random() < 0.3:
        raw[rng.integers(0, raw.shape[0], 20), rng.integers(0, raw.shape[1], 20)] = 65535   # hot pixels
    m3 = np.array([[1.6697, -0.2693, -0.4004, -42.4346], [-0.3576, 1.0615, 1.5949, -37.1158], [-0.2175, -1.8751, 6.9640, -26.6970]], f32)
    m7 = np.array([[2.2997, -0.4478, 0.1706, -39.0923], [-0.3826, 1.5906, -0.2080, -25.4311], [-0.0888, -0.7344, 2.2832, -20.0826]], f32)
    ct, gamma, contrast, sharpen = f32(rng.choice([3700.0, 3200.0, 7000.0, 5000.0])), f32(rng.choice([2.0, 1.0, 2.2])), f32(rng.choice([50.0, 0.0, 100.0])), f32(rng.choice([1.0, 0.0, 2.5]))
    black, white = int(rng.choice([25, 0, 64])), int(rng.choice([1023, 900, 4095]))
    o = hl.Buffer(np.zeros((3, oh, ow), np.uint8))
    hl.camera_pipe(hl.Buffer(raw), hl.Buffer(m3), hl.Buffer(m7), ct, gamma, contrast, sharpen, black, white, o)
    want = oracle.camera_pipe(raw, m3, m7, ct, gamma, contrast, sharpen, black, white, ow, oh)
    return f"{ow}x{oh} ct={ct} gamma={gamma} contrast={contrast} sharpen={sharpen} black={black} white={white}", same(o.numpy(), want)


def case_depthwise_separable_conv(rng):
    n, hh, ww = int(rng.integers(1, 4)), rdim(rng, 1, 40), rdim(rng, 1, 40)
    ci, co = int(rng.choice([32, 16, 8, 3])), int(rng.choice([16, 8, 32, 5]))
    inp = rng.uniform(-1, 1, (n, hh, ww, ci)).astype(f32)   # same box as the output: the generator pads with zeros
    dw, pw, bias = rng.uniform(-1, 1, (3, 3, ci, 1)).astype(f32), rng.uniform(-1, 1, (ci, co)).astype(f32), rng.uniform(-1, 1, (co,)).astype(f32)
    o = hl.Buffer(np.zeros((n, hh, ww, co), f32))
    hl.depthwise_separable_conv(hl.Buffer(inp), hl.Buffer(dw), hl.Buffer(pw), hl.Buffer(bias), o)
    return f"n={n} {ww}x{hh} ci={ci} co={co}", same(o.numpy(), oracle.depthwise_separable_conv(inp, dw, pw, bias))


def _conv_data(rng, ci_choices=(32, 64, 128, 192)):
    n, hh, ww = int(rng.integers(1, 4)), rdim(rng, 1, 60), rdim(rng, 1, 130)     # W <= 125: input-linear kernel, wider: im2col kernel
    ci, co = int(rng.choice(ci_choices)), int(rng.choice([128, 256]))
    inp = rng.uniform(-1, 1, (n, hh + 2, ww + 2, ci)).astype(f32)
    filt, bias = rng.uniform(-1, 1, (ci, 3, 3, co)).astype(f32), rng.uniform(-1, 1, (co,)).astype(f32)
    return n, hh, ww, ci, co, inp, filt, bias


def case_conv_layer(rng):
    n, hh, ww, ci, co, inp, filt, bias = _conv_data(rng)
    o = hl.Buffer(np.zeros((n, hh, ww, co), f32))
    hl.conv_layer(hl.Buffer(inp), hl.Buffer(filt), hl.Buffer(bias), o)
    return f"n={n} {ww}x{hh} ci={ci} co={co}", same(o.numpy(), oracle.conv_layer(inp, filt, bias))


def case_conv_layer_bf16(rng):
    """tolerance, not bit-exactness: bf16 operands, f32 accumulation in hardware order (tests/test_conv_layer.py); the bf16
    entry point wants input channels in multiples of 64"""
    n, hh, ww, ci, co, inp, filt, bias = _conv_data(rng, (64, 128, 192))
    o = hl.Buffer(np.zeros((n, hh, ww, co), f32))
    hl.conv_layer_bf16(hl.Buffer(inp), hl.Buffer(filt), hl.Buffer(bias), o)
    want, mag = oracle.conv_layer_bf16(inp, filt, bias)
    err = np.abs(o.numpy().astype(np.float64) - want.astype(np.float64))
    return f"n={n} {ww}x{hh} ci={ci} co={co}", bool((err <= 2e-6 * mag.astype(np.float64) + 1e-6).all())


def fuzz_resize(rng):
    """resize: random type, kernel, direction, factor in [0.05, 8], sizes, origins and crops, against tests/cpp/resize_check.c"""
    checker = checkers()
    kernel = str(rng.choice(checker.RESIZE_KERNELS))
    tname = str(rng.choice(list(checker.RESIZE_TYPE_INDEX)))
    up = bool(rng.integers(0, 2))
    scale = float(f32(np.exp(rng.uniform(np.log(0.05), np.log(8.0)))))
    taps = checker.RESIZE_TAPS[kernel]
    need = taps if up else int(np.ceil(f32(taps) * (f32(1) / f32(scale))))
    w, h, c = max(rdim(rng, 1, 700), need), max(rdim(rng, 1, 500), need), int(rng.integers(1, 5))
    dt = np.dtype(tname)
    inp = rng.random((c, h, w), dtype=f32) if tname == "float32" else rng.integers(0, np.iinfo(dt).max + 1, (c, h, w)).astype(dt)
    in_min = [int(v) for v in rng.integers(-40, 41, 3)] if rng.random() < 0.5 else [0, 0, 0]
    # the full output of the driver's size, or a crop of it / a region around it (windows are clamped, any region is legal)
    fw, fh = max(1, min(int(f32(w) * f32(scale)), 1500)), max(1, min(int(f32(h) * f32(scale)), 1200))
    x0, y0 = int(np.floor(in_min[0] * scale)), int(np.floor(in_min[1] * scale))
    if rng.random() < 0.5:
        ox, oy = x0 + int(rng.integers(-3, fw)), y0 + int(rng.integers(-3, fh))
        ow, oh = int(rng.integers(1, fw + 1)), int(rng.integers(1, fh + 1))
    else:
        ox, oy, ow, oh = x0, y0, fw, fh
    c0 = int(rng.integers(0, c))
    oc = int(rng.integers(1, c - c0 + 1))
    out_min = [ox, oy, in_min[2] + c0]
    a, o = hl.Buffer(inp, mins=in_min), hl.Buffer(np.zeros((oc, oh, ow), dt), mins=out_min)
    hl.resize(a, scale, o, kernel, upsample=up)
    want = np.zeros((oc, oh, ow), dt)
    r = checker.lib().rc_resize(checker.RESIZE_KERNELS.index(kernel), checker.RESIZE_TYPE_INDEX[tname], int(up), scale, inp.ctypes.data,
                                checker.i3(in_min), checker.i3((w, h, c)), want.ctypes.data, checker.i3(out_min), checker.i3((ow, oh, oc)))
    desc = f"{kernel} {tname} {'up' if up else 'down'} x{scale!r} in {w}x{h}x{c} min {in_min} out {ow}x{oh}x{oc} min {out_min}"
    return desc, r == 0 and same(o.numpy(), want)


def fuzz_gaussian_blur(rng):
    """gaussian_blur: the direct blur (any output region) or a random one of the 36 variants, random sigma in [0.3, 12], trunc in 0..5,
    sizes and input origins, on either path, against tests/cpp/gaussian_blur_check.c"""
    check = checkers().lib()
    w, h = rdim(rng, 1, 300), rdim(rng, 1, 200)
    sigma = float(f32(np.exp(rng.uniform(np.log(0.3), np.log(12.0)))))
    trunc = int(rng.integers(0, 6))
    inp = rng.random((h, w), dtype=f32)
    in_min = [int(v) for v in rng.integers(-40, 41, 2)] if rng.random() < 0.5 else [0, 0]
    general = bool(rng.integers(0, 2))
    a = hl.Buffer(inp, mins=in_min)
    if rng.random() < 0.4:
        name = "gaussian_blur_direct"
        ow, oh = rdim(rng, 1, 300), rdim(rng, 1, 200)
        out_min = [in_min[0] + int(rng.integers(-60, w + 60)), in_min[1] + int(rng.integers(-60, h + 60))] if rng.random() < 0.5 else list(in_min)
        o = hl.Buffer(np.zeros((oh, ow), f32), mins=out_min)
        want = np.zeros((oh, ow), f32)
        r = check.gc_direct(inp.ctypes.data, in_min[0], in_min[1], w, h, sigma, trunc, want.ctypes.data, out_min[0], out_min[1], ow, oh)
    else:
        u, d, f = int(rng.integers(2, 5)), int(rng.integers(1, 4)), int(rng.choice([2, 4, 8, 16]))
        name = hl.gaussian_blur_variant(u, d, f)
        ow, oh = (w, h) if rng.random() < 0.7 else (rdim(rng, 1, 300), rdim(rng, 1, 200))
        out_min = [0, 0]
        o = hl.Buffer(hl.aligned_array((oh, ow)))
        want = np.zeros((oh, ow), f32)
        r = check.gc_resampled(u, d, f, inp.ctypes.data, in_min[0], in_min[1], w, h, sigma, trunc, want.ctypes.data, ow, oh)
    if general:
        hl.debug_gaussian_blur_general(name, a, sigma, trunc, o)
    else:
        hl._check(hl._fn[name](a.ptr, sigma, trunc, o.ptr))
    desc = f"{name}{' general' if general else ''} sigma {sigma!r} trunc {trunc} in {w}x{h} min {in_min} out {ow}x{oh} min {out_min}"
    return desc, r == 0 and same(np.ascontiguousarray(o.numpy()), want)


def _strided(rng, shape):
    """a zeroed (C, H, W) array, dense or inside a larger allocation with padded rows and planes"""
    c, h, w = shape
    if rng.random() < 0.5:
        return np.zeros(shape, f32)
    py, px = int(rng.integers(0, 4)), int(rng.integers(0, 9))
    return np.zeros((c, h + py, w + px), f32)[:, :h, px // 2:px // 2 + w]


def fuzz_linear_blur(rng):
    """linear_blur or simple_blur on a random output region, channel range, mins and strides, on either path, against
    tests/cpp/linear_blur_check.c.  simple_blur: random width and height around the region, the input placed over the box they
    require, now and then one cell short of it; linear_blur: a random region around an input with mins that are 0 or not.  Where
    the checker finds the input short (-4) the entry point must say the same."""
    linear = bool(rng.integers(0, 2))
    general = bool(rng.integers(0, 2))
    on, oc = int(rng.integers(1, 5)), int(rng.integers(-2, 3))
    ow, oh = rdim(rng, 1, 200), rdim(rng, 1, 120)
    clamp = lambda v, n: max(min(v, n - 1), 0)
    if linear:
        w, h = rdim(rng, 1, 200), rdim(rng, 1, 120)
        width, height = w, h
        ix0, iy0 = (0, 0) if rng.random() < 0.6 else (int(rng.integers(-4, 12)), int(rng.integers(-4, 12)))
        ox, oy = int(rng.integers(min(ix0, 0) - 30, w + 30)), int(rng.integers(min(iy0, 0) - 30, h + 30))
        if ix0 > 0 and rng.random() < 0.8:   # mostly regions such an input covers
            ox, oy = max(ox, ix0), max(oy, iy0)
        if ix0 < 0 and rng.random() < 0.8:
            ow, oh = max(1, min(ow, ix0 + w - 2 - ox)), max(1, min(oh, iy0 + h - 2 - oy))
    else:
        ox, oy = int(rng.integers(-60, 200)), int(rng.integers(-60, 120))
        width = int(rng.integers(-3, max(ox + ow, 0) + 40)) if rng.random() < 0.8 else 1
        height = int(rng.integers(-3, max(oy + oh, 0) + 40)) if rng.random() < 0.8 else 1
        bx0, bx1, by0, by1 = clamp(ox, width), clamp(ox + ow + 1, width), clamp(oy, height), clamp(oy + oh + 1, height)
        m = [int(v) for v in rng.integers(0, 4, 4)]
        if rng.random() < 0.1:
            m[int(rng.integers(0, 4))] = -1
        ix0, iy0, w, h = bx0 - m[0], by0 - m[1], bx1 - bx0 + 1 + m[0] + m[2], by1 - by0 + 1 + m[1] + m[3]
        if w < 1 or h < 1:
            ix0, iy0, w, h = bx0, by0, max(w, 1), max(h, 1)
    c_lo, c_hi = int(rng.integers(0, 3)), int(rng.integers(0, 3))   # input channels beside the output's
    vals = rng.random((on + c_lo + c_hi, h, w), dtype=f32) * f32(1.2) - f32(0.05)
    src = _strided(rng, vals.shape)
    src[...] = vals
    a = hl.Buffer(src, mins=(ix0, iy0, oc - c_lo))
    o = hl.Buffer(_strided(rng, (on, oh, ow)), mins=(ox, oy, oc))
    mine = np.ascontiguousarray(vals[c_lo:c_lo + on])
    want = np.zeros((on, oh, ow), f32)
    rc = checkers().lib().lc_blur(int(linear), mine.ctypes.data, ix0, iy0, w, h, on, width, height, want.ctypes.data, ox, oy, ow, oh)
    name = "linear_blur" if linear else "simple_blur"
    fn = hl.lib.hlmi_linear_blur_general
    fn.restype, fn.argtypes = hl.C.c_int, [hl.C.c_char_p, hl._BP, hl.C.c_int32, hl.C.c_int32, hl._BP]
    if general:
        r = fn(name.encode(), a.ptr, width, height, o.ptr)
    elif linear:
        r = hl._fn[name](a.ptr, o.ptr)
    else:
        r = hl._fn[name](a.ptr, width, height, o.ptr)
    desc = (f"{name}{' general' if general else ''} in {w}x{h}x{vals.shape[0]} min {(ix0, iy0, oc - c_lo)} strides {[a.dim(i).stride for i in range(3)]} "
            f"width {width} height {height} out {ow}x{oh}x{on} min {(ox, oy, oc)} strides {[o.dim(i).stride for i in range(3)]} -> {r} (checker {rc})")
    return desc, r == rc and (rc != 0 or same(np.ascontiguousarray(o.numpy()), want))


def _strided_rows(rng, shape):
    """a zeroed (H, W) or (C, H, W) array, dense or inside a larger allocation: padded rows (an odd row stride among them), padded
    planes and a first element that is not the allocation's"""
    lead, (h, w) = tuple(shape[:-2]), shape[-2:]
    if rng.random() < 0.4:
        return np.zeros(shape, f32)
    py, px, x0 = int(rng.integers(0, 3)), int(rng.integers(0, 8)), int(rng.integers(0, 4))
    return np.zeros(lead + (h + py, w + px + x0), f32)[..., :h, x0:x0 + w]


def fuzz_wavelet(rng):
    """One of haar_x, inverse_haar_x, daubechies_x and inverse_daubechies_x on a random output region (mins negative, odd, past the
    input on either side), channel range, input mins and strides, on either path, against tests/cpp/wavelet_check.c
    (tests/wavelet_checker.py).  Widths reach several 128-pair waves, so that the wide and the per-tap paths both run."""
    import wavelet_checker as wc
    wc.set_canon(hl.canon_fma())
    name = wc.NAMES[int(rng.integers(0, 4))]
    general = bool(rng.integers(0, 2))
    w, h = rdim(rng, 1, 700), rdim(rng, 1, 24)
    ix0, iy0 = (0, 0) if rng.random() < 0.5 else (int(rng.integers(-9, 10)), int(rng.integers(-5, 6)))
    oh, oy = rdim(rng, 1, 24), iy0 + int(rng.integers(-4, h + 4))
    if wc.is_inverse(name):
        ic0 = int(rng.choice([0, 0, 0, 1, -1, -2, 2]))
        nc = int(rng.integers(1, 4))
        vals = rng.random((nc, h, w), dtype=f32) * f32(2) - f32(1)
        in_min = (ix0, iy0, ic0)
        ow = rdim(rng, 1, 1400)
        ox = int(rng.integers(2 * ix0 - 40, 2 * (ix0 + w) + 40)) if rng.random() < 0.6 else 2 * ix0
        out_shape, out_min = (oh, ow), (ox, oy)
    else:
        vals = rng.random((h, w), dtype=f32) * f32(2) - f32(1)
        in_min = (ix0, iy0)
        ow = rdim(rng, 1, 400)
        ox = int(rng.integers((ix0 - 40) // 2, (ix0 + w + 40) // 2)) if rng.random() < 0.6 else ix0 // 2
        oc, on = [(0, 2), (0, 2), (1, 1), (0, 1), (-1, 3), (0, 3), (5, 1)][int(rng.integers(0, 7))]
        out_shape, out_min = (on, oh, ow), (ox, oy, oc)
    src = _strided_rows(rng, vals.shape)
    src[...] = vals
    a, o = hl.Buffer(src, mins=in_min), hl.Buffer(_strided_rows(rng, out_shape), mins=out_min)
    want = wc.run(name, vals, out_shape=out_shape, out_min=out_min, in_min=in_min)
    if general:
        fn = hl.lib.hlmi_wavelet_general
        fn.restype, fn.argtypes = hl.C.c_int, [hl.C.c_char_p, hl._BP, hl._BP]
        r = fn(name.encode(), a.ptr, o.ptr)
    else:
        r = hl._fn[name](a.ptr, o.ptr)
    nd = len(in_min)
    desc = (f"{name}{' general' if general else ''} in {vals.shape[::-1]} min {in_min} strides {[a.dim(i).stride for i in range(nd)]} "
            f"out {out_shape[::-1]} min {out_min} strides {[o.dim(i).stride for i in range(len(out_min))]} -> {r}")
    return desc, r == 0 and same(np.ascontiguousarray(o.numpy()), want)


def fuzz_reaction_diffusion(rng):
    """One of reaction_diffusion_init, reaction_diffusion_update, reaction_diffusion_render and hlmi_reaction_diffusion_run on a random
    frame (mins, strides, mouse inside, on the border or far outside, frame numbers up to the int32 wrap), on either path and, for run,
    under a random HLMI_RD_STEPS_PER_LAUNCH, against tests/cpp/reaction_diffusion_check.c (tests/reaction_diffusion_checker.py).
    Frames reach several 64 x 32 tiles; update also takes outputs larger than the frame."""
    import reaction_diffusion_checker as rdc
    rdc.set_canon(hl.canon_fma())
    what = ("init", "update", "render", "run")[int(rng.integers(0, 4))]
    general = bool(rng.integers(0, 2))
    w, h = rdim(rng, 1, 200), rdim(rng, 1, 100)
    mins = (0, 0) if rng.random() < 0.5 else (int(rng.integers(-9, 1)), int(rng.integers(-5, 1)))
    fn = hl.lib.hlmi_reaction_diffusion_general
    fn.restype, fn.argtypes = hl.C.c_int, [hl.C.c_char_p, hl._BP, hl.C.c_int32, hl.C.c_int32, hl.C.c_int32, hl.C.c_int32, hl._BP, hl._BP]
    if what == "init":
        nc, oc = int(rng.integers(1, 5)), int(rng.integers(-2, 3))
        o = hl.Buffer(_strided_rows(rng, (nc, h, w)), mins=mins + (oc,))
        r = fn(b"reaction_diffusion_init", None, 0, 0, 0, 0, o.ptr, None) if general else hl._fn["reaction_diffusion_init"](o.ptr)
        return f"init{' general' if general else ''} {(w, h, nc)} min {mins + (oc,)} -> {r}", r == 0 and same(np.ascontiguousarray(o.numpy()), rdc.init((nc, h, w), mins + (oc,)))
    vals = rng.random((3, h, w), dtype=f32) * f32(2) - f32(0.5)
    src = _strided_rows(rng, vals.shape)
    src[...] = vals
    a = hl.Buffer(src, mins=mins + (0,))
    if what == "render":
        vals = np.clip(vals, 0, 1)
        src[...] = vals
        o = hl.Buffer(np.ascontiguousarray(_strided_rows(rng, (h, w))).astype(np.uint32), mins=mins)
        r = fn(b"reaction_diffusion_render", a.ptr, 0, 0, 0, 0, None, o.ptr) if general else hl._fn["reaction_diffusion_render"](a.ptr, o.ptr)
        return f"render{' general' if general else ''} {(w, h)} min {mins} -> {r}", r == 0 and np.array_equal(np.ascontiguousarray(o.numpy()), rdc.render(vals))
    # a mouse whose clobber box the frame holds: the box is in extent coordinates, the frame starts at mins <= 0
    far = rng.random() < 0.3
    mouse = (int(rng.integers(-10, w + mins[0] - 10)) if w + mins[0] > 0 else -1000, int(rng.integers(-10, h + mins[1] - 10)) if h + mins[1] > 0 else -1000)
    if far:
        mouse = (-1000 - int(rng.integers(0, 2 ** 30)), mouse[1])
    box = rdc.clobber_box(w, h, *mouse)
    if box[1] > mins[0] + w - 1 or box[3] > mins[1] + h - 1:
        mouse = (-1000, -1000)   # the degenerate box at (0, 0): held, mins <= 0
        if mins[0] + w - 1 < 0 or mins[1] + h - 1 < 0:
            mins = (0, 0)
            a = hl.Buffer(src, mins=(0, 0, 0))
    frame = int(rng.choice([0, 1, 77, 2 ** 31 - 2, -2 ** 31, -5]))
    if what == "update":
        grow = (0, 0, 0, 0) if rng.random() < 0.6 else tuple(int(v) for v in rng.integers(0, 6, 4))
        out_shape, out_min = (3, h + grow[1] + grow[3], w + grow[0] + grow[2]), (mins[0] - grow[0], mins[1] - grow[1])
        o = hl.Buffer(_strided_rows(rng, out_shape), mins=out_min + (0,))
        want = rdc.update(vals, *mouse, frame, state_min=mins, out_shape=out_shape, out_min=out_min)
        r = (fn(b"reaction_diffusion_update", a.ptr, mouse[0], mouse[1], frame, 0, o.ptr, None) if general
             else hl._fn["reaction_diffusion_update"](a.ptr, mouse[0], mouse[1], frame, o.ptr))
        return (f"update{' general' if general else ''} {(w, h)} min {mins} mouse {mouse} frame {frame} out {out_shape[::-1]} min {out_min} -> {r}",
                r == 0 and same(np.ascontiguousarray(o.numpy()), want))
    steps, S = int(rng.integers(1, 10)), int(rng.choice([0, 1, 2, 4]))   # 0: the switch unset, the plan's choice
    with_render = bool(rng.integers(0, 2))
    o = hl.Buffer(_strided_rows(rng, vals.shape), mins=mins + (0,))
    p = hl.Buffer(np.zeros((h, w), np.uint32), mins=mins) if with_render else None
    want = rdc.run(vals, *mouse, frame, steps, state_min=mins)
    before = os.environ.get("HLMI_RD_STEPS_PER_LAUNCH")
    os.environ.pop("HLMI_RD_STEPS_PER_LAUNCH", None)
    if S:
        os.environ["HLMI_RD_STEPS_PER_LAUNCH"] = str(S)
    try:
        if general:
            r = fn(b"run", a.ptr, mouse[0], mouse[1], frame, steps, o.ptr, p.ptr if p else None)
        else:
            run = hl.lib.hlmi_reaction_diffusion_run
            run.restype, run.argtypes = hl.C.c_int, [hl._BP, hl.C.c_int32, hl.C.c_int32, hl.C.c_int32, hl.C.c_int32, hl._BP, hl._BP]
            r = run(a.ptr, mouse[0], mouse[1], frame, steps, o.ptr, p.ptr if p else None)
    finally:
        os.environ.pop("HLMI_RD_STEPS_PER_LAUNCH", None)
        if before is not None:
            os.environ["HLMI_RD_STEPS_PER_LAUNCH"] = before
    ok = r == 0 and same(np.ascontiguousarray(o.numpy()), want) and (p is None or np.array_equal(np.ascontiguousarray(p.numpy()), rdc.render(want)))
    return f"run{' general' if general else ''} S {S} steps {steps} {(w, h)} min {mins} mouse {mouse} frame0 {frame} render {with_render} -> {r}", ok


def _u8_view(rng, shape):
    """a zeroed uint8 (C, H, W) view inside one allocation: dense, or with longer rows, planes further apart (channel strides that
    are no multiple of 4 among them) and a first element that is not the allocation's"""
    c, h, w = shape
    if rng.random() < 0.35:
        return np.zeros(shape, np.uint8)
    rs = w + int(rng.integers(0, 10))
    cs = rs * h + int(rng.integers(0, 10))
    x0 = int(rng.integers(0, 9))
    return np.lib.stride_tricks.as_strided(np.zeros(x0 + c * cs + 8, np.uint8)[x0:], shape, (cs, rs, 1))


def fuzz_compositing(rng):
    """compositing on a random output box (a non-zero min among them), every layer larger than it or exactly it with mins, extents and
    strides of its own (sometimes one buffer for several layers), random op codes with out-of-range ones, on either path, against
    tests/cpp/compositing_check.c (tests/compositing_checker.py).  Widths reach several 512-pixel waves, so that the 8-byte and the
    per-byte paths both run."""
    import compositing_checker as cc
    general = bool(rng.integers(0, 2))
    w, h = rdim(rng, 1, 1300), rdim(rng, 1, 12)
    ox, oy = (0, 0) if rng.random() < 0.4 else (int(rng.integers(-20, 21)), int(rng.integers(-9, 10)))
    bufs, crops = [], []
    for k in range(6):
        if k and rng.random() < 0.15:   # the same buffer again
            j = int(rng.integers(0, k))
            bufs.append(bufs[j]), crops.append(crops[j])
            continue
        lx, ly, lc = (int(v) for v in rng.integers(0, 9, 3)) if rng.random() < 0.6 else (0, 0, 0)   # what the layer holds before the box
        shape = (4 + lc + int(rng.integers(0, 2)), h + ly + int(rng.integers(0, 3)), w + lx + int(rng.integers(0, 9)))
        a = _u8_view(rng, shape)
        a[...] = rng.integers(0, 256, shape, dtype=np.uint8)
        if rng.random() < 0.5:   # alphas 0, 1 and 255 often
            pick = rng.integers(0, 6, shape[1:])
            a[lc + 3] = np.where(pick == 0, 0, np.where(pick == 1, 255, np.where(pick == 2, 1, a[lc + 3])))
        bufs.append(hl.Buffer(a, mins=(ox - lx, oy - ly, -lc)))
        crops.append(a[lc:lc + 4, ly:ly + h, lx:lx + w].copy())
    codes = rng.integers(-1, 6, 5).astype(np.int32)
    if rng.random() < 0.2:
        codes[int(rng.integers(0, 5))] = int(rng.choice([-2 ** 31, 2 ** 31 - 1, 255, 256, -128, 1 << 16]))
    pre = int(rng.integers(0, 4))
    opsa = np.concatenate([rng.integers(-9, 9, pre), codes, rng.integers(-9, 9, int(rng.integers(0, 3)))]).astype(np.int32)
    ops = hl.Buffer(opsa, mins=(-pre,))
    o = hl.Buffer(_u8_view(rng, (4, h, w)), mins=(ox, oy, 0))
    want = cc.run(crops, codes)
    (hl.debug_compositing_general if general else hl.compositing)(bufs, ops, o)
    desc = (f"compositing{' general' if general else ''} {w}x{h} at ({ox}, {oy}) ops {codes.tolist()} layer mins {[b.mins for b in bufs]} "
            f"strides {[[b.dim(i).stride for i in (1, 2)] for b in bufs]} out strides {[o.dim(i).stride for i in (1, 2)]}")
    return desc, same(np.ascontiguousarray(o.numpy()), want)


def _u8_plane(rng, h, w):
    """(row stride, byte offset of the first element) of a uint8 (H, W) plane: dense and on the 8-byte grid, or with longer rows
    (multiples of 8 and not) and a first element 0 .. 8 bytes into its allocation"""
    if rng.random() < 0.35:
        return w, 0
    return w + int(rng.choice([0, 8, 16, 1, 3, 5, 11])), int(rng.integers(0, 9))


def fuzz_hexagon_benchmarks(rng):
    """one of the six filters of apps/hexagon_benchmarks on a random input and an output of its own size (smaller, equal, larger; for
    sobel at any origin, negative and past the input included), random row strides and pointer offsets for both, for the conv3x3
    pair a random mask (with +-127 and -128) inside a mask buffer with mins, extents and a row stride of its own, on either path,
    against tests/cpp/hexagon_benchmarks_check.c (tests/hexagon_benchmarks_checker.py).  Widths reach several 496-pixel waves, so
    that the 8-byte and the per-byte paths both run."""
    import hexagon_benchmarks_checker as hb
    name = hb.NAMES[int(rng.integers(0, len(hb.NAMES)))]
    general = bool(rng.integers(0, 2))
    iw, ih = rdim(rng, 1, 1100), rdim(rng, 1, 40)
    if rng.random() < 0.5:   # sizes on the 8-byte grid: the 8-byte path
        iw = max(8, iw // 8 * 8)
    r = rng.random()
    ow, oh = (iw, ih) if r < 0.5 else (rdim(rng, 1, 1100), rdim(rng, 1, 40))
    if r < 0.7 and iw % 8 == 0:
        ow = max(8, ow // 8 * 8)
    ox, oy = 0, 0
    if name == "sobel" and rng.random() < 0.6:
        ox, oy = int(rng.choice([-16, -8, 8, 24, -3, 5, iw, iw + 8, -ow - 8])), int(rng.integers(-12, ih + 6))
    data = rng.integers(0, 256, (ih, iw), dtype=np.uint8) if rng.random() < 0.7 else rng.choice(np.array([0, 1, 127, 128, 254, 255], np.uint8), (ih, iw))
    a, o = hb.DevPlane(hl, ih, iw, *_u8_plane(rng, ih, iw), fill=data), hb.DevPlane(hl, oh, ow, *_u8_plane(rng, oh, ow), mins=(ox, oy))
    mask = mb = None
    if name in hb.MASKED:
        pick = rng.random()
        mask = (rng.integers(-128, 128, (3, 3)) if pick < 0.5 else rng.choice(np.array([-128, -127, 127, 16, 0, 1, -1]), (3, 3))).astype(np.int8)
        if pick > 0.9:
            mask = hb.DRIVER_MASK.copy()
        mx, my, ex, ey = int(rng.integers(0, 3)), int(rng.integers(0, 3)), int(rng.integers(0, 3)), int(rng.integers(0, 3))
        rs = 3 + mx + ex + int(rng.integers(0, 6))
        box = np.lib.stride_tricks.as_strided(rng.integers(-128, 128, (3 + my + ey) * rs + 8).astype(np.int8), (3 + my + ey, 3 + mx + ex), (rs, 1))
        box[my:my + 3, mx:mx + 3] = mask
        mb = hl.Buffer(box, mins=(-mx, -my))
    want = hb.run(name, data, mask, (ox, oy, ow, oh))
    try:
        if general:
            hl.debug_hexagon_benchmarks_general(name, a.buf, mb, o.buf)
        else:
            getattr(hl, name)(*([a.buf, mb, o.buf] if mb is not None else [a.buf, o.buf]))
        got = o.result()
    finally:
        a.free(), o.free()
    desc = (f"{name}{' general' if general else ''} input {iw}x{ih} stride {a.buf.dim(1).stride} at byte {a.host.ctypes.data - a.flat.ctypes.data}, "
            f"output {ow}x{oh} at ({ox}, {oy}) stride {o.buf.dim(1).stride} at byte {o.host.ctypes.data - o.flat.ctypes.data}"
            + (f", mask {mask.tolist()} mins {mb.mins} stride {mb.dim(1).stride}" if mb else ""))
    return desc, same(got, want)


def _f32_square(rng, n):
    """(row stride in elements, byte offset of the first element) of an (n, n) float32 matrix: dense on 16 bytes, or with longer rows
    (multiples of 4 elements and not) and a first element 0 .. 3 elements into its allocation"""
    if rng.random() < 0.35:
        return n, 0
    return n + int(rng.choice([0, 4, 8, 1, 3, 5])), 4 * int(rng.integers(0, 4))


def fuzz_mat_mul(rng):
    """mat_mul at a random size 1 .. 200 (hlmi_mat_mul_sized) or on the one-thread-per-output path, A, B and out each with a row stride
    and a pointer offset of their own, noise in [-1, 1) and in a third of the cases a handful of +-0, subnormals, +-Inf, NaN and
    magnitudes whose products overflow, against tests/cpp/mat_mul_check.c (tests/mat_mul_checker.py).  Compared bit for bit, NaN for
    NaN (sign and payload of a produced NaN belong to the processor); the bytes around `out` must come back unchanged."""
    import mat_mul_checker as mm
    from parity_helpers import DevArray
    n = rdim(rng, 1, 200)
    general = rng.random() < 0.3
    A, B = (rng.random((n, n), dtype=f32) * 2 - 1 for _ in range(2))
    special = rng.random() < 0.33
    if special:
        pool = np.array([0.0, -0.0, 1e-40, -3e-39, np.inf, -np.inf, np.nan, 3e38, -2e38, 2.0 ** 100, 2.0 ** -100], f32)
        for m in (A, B):
            k = int(rng.integers(1, 6))
            m[rng.integers(0, n, k), rng.integers(0, n, k)] = rng.choice(pool, k)
    la, lb, lo = (_f32_square(rng, n) for _ in range(3))
    a, b, o = (DevArray(hl, (n, n), f32, lay[0], offset=lay[1], fill=m) for lay, m in ((la, A), (lb, B), (lo, None)))
    want = mm.run(A, B)
    try:
        (hl.debug_mat_mul_general if general else hl.mat_mul_sized)(n, a.buf, b.buf, o.buf)
        got = o.result()
    finally:
        a.free(), b.free(), o.free()
    nan = np.isnan(want)
    ok = got.shape == want.shape and bool(np.isnan(got[nan]).all()) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    desc = (f"mat_mul{' general' if general else ''} n {n}{' special values' if special else ''}, (row stride, byte offset) A {la} B {lb} out {lo}")
    return desc, ok


def fuzz_linear_algebra(rng):
    """One of the twelve f32 pipelines of apps/linear_algebra at random sizes (vectors 0 .. 3000, matrix extents 1 .. 200 within the
    variant's squareness rule), on the default or the one-thread-per-output path, every buffer in a device allocation with a column
    stride and a pointer offset of its own, in a third of the cases with the output being the wrapper's y / C input, noise in [-1, 1)
    with random a and b and in a third of the cases a handful of special values, against tests/cpp/linear_algebra_check.c
    (tests/linear_algebra_checker.py) in the library's canonical form.  Bit for bit, NaN for NaN; the bytes around every buffer must
    come back unchanged."""
    from linear_algebra_checker import f32 as la
    la.set_canon(hl.canon_fma())
    name = la.NAMES[int(rng.integers(0, len(la.NAMES)))]
    general = rng.random() < 0.3
    a, b = (float(f32(rng.random() * 4 - 2)) for _ in range(2))
    mk = lambda *s: (rng.random(s, dtype=f32) * 2 - 1).astype(f32)
    gemm = name in la.GEMM_FLAGS
    if gemm:
        ta, tb = la.GEMM_FLAGS[name]
        M, N, K = (rdim(rng, 1, 200) for _ in range(3))
        K = M if ta else K
        N = K if tb else N
        ins = {"A_": mk(K, M), "B_": mk(N, K), "C_": mk(N, M)}
        order, out, alias_of = ("A_", "B_", "C_", "result"), "result", "C_"
        want = lambda: la.sgemm(ta, tb, a, ins["A_"], ins["B_"], b, ins["C_"])
    elif name.startswith("halide_sgemv"):
        t = name.endswith("_trans")
        w, h = rdim(rng, 1, 200), rdim(rng, 1, 200)
        ins = {"A": mk(h, w), "x": mk(w if t else h), "y": mk(h if t else w)}
        order, out, alias_of = ("A", "x", "y", "output"), "output", "y"
        want = lambda: la.sgemv(t, a, ins["A"], ins["x"], b, ins["y"])
    elif name == "halide_sger_impl":
        w, h = rdim(rng, 1, 200), rdim(rng, 1, 200)
        ins = {"x": mk(w), "y": mk(h), "result": mk(h, w)}
        order, out, alias_of = ("x", "y", "result"), "result", None
        want = lambda: la.sger(a, ins["x"], ins["y"], ins["result"])
    else:
        n = int(rng.integers(0, 3001))
        ins = {"x": mk(n)}
        if name in ("halide_saxpy_impl", "halide_sdot"):
            ins["y"] = mk(n)
        order = ("x", "result") if name == "halide_sasum" else ("x", "y", "result")
        out, alias_of = "result", {"halide_sscal_impl": "x", "halide_saxpy_impl": "y"}.get(name)
        want = {"halide_scopy_impl": lambda: la.scopy(ins["x"]), "halide_sscal_impl": lambda: la.sscal(a, ins["x"]),
                "halide_saxpy_impl": lambda: la.saxpy(a, ins["x"], ins["y"]), "halide_sdot": lambda: la.sdot(ins["x"], ins["y"]),
                "halide_sasum": lambda: la.sasum(ins["x"])}[name]
    special = rng.random() < 0.33
    if special:
        pool = np.array([0.0, -0.0, 1e-40, -3e-39, np.inf, -np.inf, np.nan, 3e38, -2e38, 2.0 ** 100, 2.0 ** -100], f32)
        for m in ins.values():
            if m.size:
                k = int(rng.integers(1, 4))
                m.reshape(-1)[rng.integers(0, m.size, k)] = rng.choice(pool, k)
    expect = want()
    alias = alias_of is not None and rng.random() < 0.33
    shapes = {k: v.shape for k, v in ins.items()}
    shapes.setdefault(out, expect.shape)
    lays, arrs = {}, {}
    try:
        for k in order:
            if k == "y" and k not in ins:
                arrs[k] = None
                continue
            if k == out and alias:
                arrs[k] = arrs[alias_of]
                continue
            s = shapes[k]
            lays[k] = ((s[1] + int(rng.choice([0, 4, 1, 3]))) if len(s) == 2 else None, 4 * int(rng.integers(0, 4)))
            arrs[k] = la.Arr(hl, "dev", s, lays[k][0], lays[k][1], fill=ins.get(k))
        bufs = [None if arrs[k] is None else arrs[k].buf for k in order]
        if name in ("halide_sdot", "halide_sasum"):
            args = bufs
        elif gemm or name.startswith("halide_sgemv"):
            args = [a, bufs[0], bufs[1], b, bufs[2], bufs[3]]
        else:
            args = [a] + bufs
        if general:
            hl.debug_linear_algebra_general(name, *args)
        else:
            hl._check(hl._fn[name](*[v.ptr if isinstance(v, hl.Buffer) else v for v in args]))
        got = np.asarray(arrs[out].result()).reshape(expect.shape)
        for k, v in arrs.items():
            if v is not None and v is not arrs[out]:
                v.result()   # the inputs and the bytes around them are as they were
    finally:
        for v in {id(v): v for v in arrs.values() if v is not None}.values():
            v.free()
    nan = np.isnan(expect)
    ok = bool(np.isnan(got[nan]).all()) and np.array_equal(got.view(np.uint32)[~nan], expect.view(np.uint32)[~nan])
    desc = (f"{name}{' general' if general else ''} shapes {shapes} a {a} b {b}{' special values' if special else ''}{' in place' if alias else ''}, "
            f"(column stride, byte offset) {lays}")
    return desc, ok


def fuzz_linear_algebra_f64(rng):
    """One of the twelve f64 pipelines of apps/linear_algebra, drawn as fuzz_linear_algebra draws the f32 ones (vectors 0 .. 3000, matrix
    extents 1 .. 200 within the variant's squareness rule, either path, device allocations with a column stride and a pointer offset
    of 0 or 8 bytes, a third of the cases in place, a third with special values), against the ld_* half of tests/cpp/linear_algebra_check.c
    (tests/linear_algebra_checker.py) in the library's canonical form.  Bit for bit, NaN for NaN; the bytes around every buffer
    must come back unchanged."""
    from linear_algebra_checker import f64 as ld
    f64 = np.float64
    ld.set_canon(hl.canon_fma())
    name = ld.NAMES[int(rng.integers(0, len(ld.NAMES)))]
    general = rng.random() < 0.3
    a, b = (float(rng.random() * 4 - 2) for _ in range(2))
    mk = lambda *s: rng.random(s) * 2 - 1
    gemm = name in ld.GEMM_FLAGS
    if gemm:
        ta, tb = ld.GEMM_FLAGS[name]
        M, N, K = (rdim(rng, 1, 200) for _ in range(3))
        K = M if ta else K
        N = K if tb else N
        ins = {"A_": mk(K, M), "B_": mk(N, K), "C_": mk(N, M)}
        order, out, alias_of = ("A_", "B_", "C_", "result"), "result", "C_"
        want = lambda: ld.dgemm(ta, tb, a, ins["A_"], ins["B_"], b, ins["C_"])
    elif name.startswith("halide_dgemv"):
        t = name.endswith("_trans")
        w, h = rdim(rng, 1, 200), rdim(rng, 1, 200)
        ins = {"A": mk(h, w), "x": mk(w if t else h), "y": mk(h if t else w)}
        order, out, alias_of = ("A", "x", "y", "output"), "output", "y"
        want = lambda: ld.dgemv(t, a, ins["A"], ins["x"], b, ins["y"])
    elif name == "halide_dger_impl":
        w, h = rdim(rng, 1, 200), rdim(rng, 1, 200)
        ins = {"x": mk(w), "y": mk(h), "result": mk(h, w)}
        order, out, alias_of = ("x", "y", "result"), "result", None
        want = lambda: ld.dger(a, ins["x"], ins["y"], ins["result"])
    else:
        n = int(rng.integers(0, 3001))
        ins = {"x": mk(n)}
        if name in ("halide_daxpy_impl", "halide_ddot"):
            ins["y"] = mk(n)
        order = ("x", "result") if name == "halide_dasum" else ("x", "y", "result")
        out, alias_of = "result", {"halide_dscal_impl": "x", "halide_daxpy_impl": "y"}.get(name)
        want = {"halide_dcopy_impl": lambda: ld.dcopy(ins["x"]), "halide_dscal_impl": lambda: ld.dscal(a, ins["x"]),
                "halide_daxpy_impl": lambda: ld.daxpy(a, ins["x"], ins["y"]), "halide_ddot": lambda: ld.ddot(ins["x"], ins["y"]),
                "halide_dasum": lambda: ld.dasum(ins["x"])}[name]
    special = rng.random() < 0.33
    if special:
        pool = np.array([0.0, -0.0, 1e-310, -3e-309, np.inf, -np.inf, np.nan, 1.5e308, -1e308, 2.0 ** 600, 2.0 ** -600], f64)
        for m in ins.values():
            if m.size:
                k = int(rng.integers(1, 4))
                m.reshape(-1)[rng.integers(0, m.size, k)] = rng.choice(pool, k)
    expect = want()
    alias = alias_of is not None and rng.random() < 0.33
    shapes = {k: v.shape for k, v in ins.items()}
    shapes.setdefault(out, expect.shape)
    lays, arrs = {}, {}
    try:
        for k in order:
            if k == "y" and k not in ins:
                arrs[k] = None
                continue
            if k == out and alias:
                arrs[k] = arrs[alias_of]
                continue
            s = shapes[k]
            lays[k] = ((s[1] + int(rng.choice([0, 2, 1, 3]))) if len(s) == 2 else None, 8 * int(rng.integers(0, 2)))
            arrs[k] = ld.Arr(hl, "dev", s, lays[k][0], lays[k][1], fill=ins.get(k))
        bufs = [None if arrs[k] is None else arrs[k].buf for k in order]
        if name in ("halide_ddot", "halide_dasum"):
            args = bufs
        elif gemm or name.startswith("halide_dgemv"):
            args = [a, bufs[0], bufs[1], b, bufs[2], bufs[3]]
        else:
            args = [a] + bufs
        if general:
            hl.debug_linear_algebra_general_f64(name, *args)
        else:
            hl._check(hl._fn[name](*[v.ptr if isinstance(v, hl.Buffer) else v for v in args]))
        got = np.asarray(arrs[out].result()).reshape(expect.shape)
        for k, v in arrs.items():
            if v is not None and v is not arrs[out]:
                v.result()   # the inputs and the bytes around them are as they were
    finally:
        for v in {id(v): v for v in arrs.values() if v is not None}.values():
            v.free()
    nan = np.isnan(expect)
    ok = bool(np.isnan(got[nan]).all()) and np.array_equal(got.view(np.uint64)[~nan], expect.view(np.uint64)[~nan])
    desc = (f"{name}{' general' if general else ''} shapes {shapes} a {a} b {b}{' special values' if special else ''}{' in place' if alias else ''}, "
            f"(column stride, byte offset) {lays}")
    return desc, ok


FFT_SIZES = [n for n in range(2, 4097) if n <= 256 or n in (384, 512, 768, 1024, 2048, 4096)]


def fuzz_fft(rng):
    """One of the four 2-D transforms of apps/fft (c2c forward and inverse, r2c, c2r) at random allowed sizes (each dimension 2 .. 256
    or one of a few larger ones, at most 2^16 points, both even for r2c and c2r), a random gain (1, 0, -1, a power of two or any
    float), on the default or the one-thread-per-line path, input and output in device allocations with a row stride and a pointer
    offset of their own (a c2r input sometimes taller than it is read, the rest NaN), noise in [-1, 1) and in a quarter of the cases a
    few signed zeros, subnormals and large magnitudes, against tests/cpp/fft_check.c (tests/fft_checker.py) in the library's
    canonical form with the library's table function.  Bit for bit, NaN for NaN; the bytes around both buffers must come back
    unchanged."""
    import fft_checker as fc
    from parity_helpers import DevArray
    fc.set_canon(hl.canon_fma())
    fc.use_twiddles(hl.fft_twiddles_address())
    kind = fc.KINDS[int(rng.integers(0, 4))]
    real = kind in ("r2c", "c2r")
    ok_sizes = [n for n in FFT_SIZES if hl.fft_size_ok(n) and not (real and n % 2)]
    while True:
        n0, n1 = (int(rng.choice(ok_sizes)) for _ in range(2))
        if n0 * n1 <= 1 << 16:
            break
    general = rng.random() < 0.3
    gain = float(f32([1.0, 0.0, -1.0, 1.0 / (n0 * n1), rng.random() * 4 - 2][int(rng.integers(0, 5))]))
    ishape, oshape = fc.in_shape(kind, n0, n1), fc.out_shape(kind, n0, n1)
    extra = int(rng.integers(0, 3)) if kind == "c2r" else 0
    x = (rng.random((ishape[0] + extra,) + ishape[1:], dtype=f32) * 2 - 1).astype(f32)
    special = rng.random() < 0.25
    if special:
        pool = np.array([0.0, -0.0, 1e-40, -3e-39, 2.0 ** -100, 1e30, -1e30], f32)
        k = int(rng.integers(1, 6))
        flat = x.reshape(-1)
        flat[rng.integers(0, flat.size, k)] = rng.choice(pool, k)
    if extra:
        x[ishape[0]:] = np.nan
    want = fc.run(kind, x, n1=n1, gain=gain)

    def lay(comps):
        if rng.random() < 0.35:
            return 0, 0
        return int(rng.choice([0, 2, 4, 1, 3])), 4 * int(rng.integers(0, 4))

    def dev(shape, fill, pad, off):
        rows, w, comps = shape if len(shape) == 3 else shape + (1,)
        rs = w * comps + pad
        a = DevArray(hl, (rows, w * comps), f32, row_stride=rs, offset=off, fill=None if fill is None else fill.reshape(rows, w * comps))
        a.buf.device_detach()
        a.buf = hl.Buffer.wrap_device(a.p.value + off, f32, [w, rows, comps], [comps, rs, 1])
        return a

    li, lo = lay(ishape[-1]), lay(oshape[-1])
    i, o = dev(x.shape, x, *li), dev(oshape, None, *lo)
    try:
        (hl.debug_fft2d_general if general else hl.fft2d)(kind, i.buf, o.buf, gain, sizes=(n0, n1))
        got = o.result().reshape(oshape)
        i.result()
    finally:
        i.free(), o.free()
    nan = np.isnan(want)
    ok = bool(np.isnan(got[nan]).all()) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    desc = (f"fft {kind}{' general' if general else ''} {n0} x {n1} gain {gain}{' special values' if special else ''}{f' +{extra} NaN rows' if extra else ''}, "
            f"(row pad, byte offset) input {li} output {lo}")
    return desc, ok


def _nhwc(shape, pixel_stride, row_pad, plane_pad, fill):
    """a (B, H, W, C) uint8 view holding `fill` inside an allocation of its own: pixels `pixel_stride` bytes apart (C = dense), rows and
    planes longer by `row_pad` and `plane_pad`, the first element on a 64-byte boundary as the interpreter allocates; every other byte 0xA5"""
    b, h, w, c = shape
    rs = w * pixel_stride + row_pad
    ps = rs * h + plane_pad
    raw = np.full(ps * b + 64, 0xA5, np.uint8)
    off = -raw.ctypes.data % 64
    v = np.lib.stride_tricks.as_strided(raw[off:], (b, h, w, c), (ps, rs, pixel_stride, 1))
    v[...] = fill
    return v, raw


def _hannk_quant(rng):
    return int(rng.integers(1 << 29, 1 << 31)), int(rng.integers(4, 13)), int(rng.integers(0, 256)), int(rng.integers(0, 40)), int(rng.integers(200, 256))


def _hannk_conv_splits(npix, co, quads, forced, cus=256):
    """hannk_conv_plan's split count (halide_amd/csrc/hannk_conv.hip), restated: the draw may not ask the library"""
    nkb = -(-quads // 16)
    wave_tiles = -(-npix // 32) * -(-(-(-co // 16)) // 2)
    want = forced if forced is not None else min(-(-4 * cus // wave_tiles), 16) if wave_tiles < 4 * cus else 1
    splits = max(1, min(want, nkb if forced is not None else nkb // 2))
    return -(-nkb // -(-nkb // splits))


def _slice_of_wider(rng, c, probability):
    """(pixel stride, first channel): c channels of pixels that hold more, as a ConcatenationOp's or a PadOp's alias has them"""
    if rng.random() >= probability:
        return c, 0
    extra = int(rng.integers(1, 10))
    return c + extra, int(rng.integers(0, extra + 1))


def draw_hannk_conv(rng):
    """the parameters of one fuzz_hannk_conv case and the classes they fall in; no array, no library, no device"""
    ci = 16 * int(rng.integers(1, 9)) if rng.random() < 0.25 else rdim(rng, 1, 150)
    co = rdim(rng, 1, 70)
    fw, fh = int(rng.integers(1, 5)), int(rng.integers(1, 5))
    (sx, sy), (dx, dy) = (int(v) for v in rng.integers(1, 4, 2)), (int(v) for v in rng.integers(1, 4, 2))
    ow, oh, ob = rdim(rng, 1, 40), rdim(rng, 1, 12), int(rng.integers(1, 4))
    d = dict(ci=ci, co=co, fw=fw, fh=fh, stride=(sx, sy), dilation=(dx, dy), out=(ow, oh, ob), omin=[0] + [int(v) for v in rng.integers(-3, 4, 3)])
    d["i16"], d["general"] = bool(rng.random() < 0.34), bool(rng.random() < 0.2)
    d["split"] = None if d["general"] or rng.random() < 0.55 else int(rng.integers(1, 7))
    d["az"], d["fz"] = int(rng.integers(0, 256)), int(rng.integers(0, 256))
    d["margin"] = (int(rng.integers(0, 3)), int(rng.integers(0, 3)))
    cp = -(-ci // 4) * 4
    d["in_pixel_stride"] = cp + (4 * int(rng.integers(1, 6)) if rng.random() < 0.3 else 0)
    d["in_pads"] = tuple(4 * int(rng.integers(1, 4)) if rng.random() < 0.5 else 0 for _ in range(2))
    d["out_pixel_stride"], d["out_channel"] = _slice_of_wider(rng, co, 0.4)
    d["out_pads"] = (3, int(rng.integers(0, 6)))
    d["quant"] = _hannk_quant(rng)
    d["seed"] = int(rng.integers(0, 1 << 32))
    # classes
    d["vec"] = (cp // 4) % 4 == 0
    d["splits"] = 1 if d["general"] else _hannk_conv_splits(ow * oh * ob, co, fw * fh * (cp // 4), d["split"])
    d["kernel"] = "general" if d["general"] else ("mfma", d["vec"], d["splits"] > 1, d["i16"])
    d["sliced_output"] = d["out_pixel_stride"] > co
    return d


def _with_env(name, value, fn):
    prev = os.environ.pop(name, None)
    try:
        if value is not None:
            os.environ[name] = str(value)
        return fn()
    finally:
        os.environ.pop(name, None)
        if prev is not None:
            os.environ[name] = prev


def run_hannk_conv(d):
    """one drawn case on the device against tests/cpp/hannk_check.c.  The output lies in a device allocation of the case's own
    (parity_helpers.DevTensor): every byte of it outside the output's elements must come back unchanged, those between two pixels'
    channels included; and the kernels launched must be the ones the draw's classes name."""
    import hannk_checker as hk
    from parity_helpers import DevTensor, launches
    rng = np.random.default_rng(d["seed"])
    ci, co, fw, fh, (sx, sy), (dx, dy), (ow, oh, ob), omin, (mx, my) = d["ci"], d["co"], d["fw"], d["fh"], d["stride"], d["dilation"], d["out"], d["omin"], d["margin"]
    az, fz, q, odt = d["az"], d["fz"], d["quant"], np.int16 if d["i16"] else np.uint8
    cp = -(-ci // 4) * 4
    # the input: the region the box reads plus a margin on every side
    ext = lambda o, s, f, dil: (o - 1) * s + (f - 1) * dil + 1
    imin = [0, omin[1] * sx - mx, omin[2] * sy - my, omin[3]]
    noise = rng.integers(0, 256, (ob, ext(oh, sy, fh, dy) + 2 * my, ext(ow, sx, fw, dx) + 2 * mx, cp), dtype=np.uint8)
    noise[..., ci:] = az
    inp, _keep_i = _nhwc(noise.shape, d["in_pixel_stride"], *d["in_pads"], noise)
    filt = rng.integers(0, 256, (co, fh, fw, ci), dtype=np.uint8)
    tiled = hk.tile(filt, fz)
    bias = rng.integers(-(1 << 24), 1 << 24, co).astype(np.int32)
    want = hk.conv(inp, tiled, bias, [co, ow, oh, ob], (sx, sy), (dx, dy), az, fz, *q, odt, in_mins=imin, out_mins=omin)
    P, k = d["out_pixel_stride"], d["out_channel"]
    rs = ow * P + d["out_pads"][0]
    o = DevTensor(hl, (ob, oh, ow, co), (rs * oh + d["out_pads"][1], rs, P, 1), offset=k * np.dtype(odt).itemsize, mins=omin, dtype=odt)
    try:
        tb = hl.Buffer(hl.aligned_array(tiled.shape, np.uint8, 64, 1))
        tb.array[...] = tiled
        name = "conv_u8_u8_i16" if d["i16"] else "conv_u8_u8_u8"
        args = [hl.Buffer(inp, mins=imin), az, tb, fz, hl.Buffer(bias), sx, sy, dx, dy, *q, o.buf]
        if d["general"]:
            call = lambda: hl.debug_hannk_general(name, *args)
        else:
            call = lambda: hl._check(hl._fn[name](*[a.ptr if isinstance(a, hl.Buffer) else a for a in args]))
        ran = _with_env("HLMI_HANNK_SPLIT_K", d["split"], lambda: launches(hl, call))
        try:
            ok = np.array_equal(o.result(), want)
        except AssertionError:      # bytes outside the output were written
            ok = False
        expect = ["hannk_conv_general"] if d["general"] else ["hannk_conv_finish", "hannk_conv_mfma"] if d["splits"] > 1 else ["hannk_conv_mfma"]
        ok = ok and ran == expect
    finally:
        o.free()
    desc = (f"{name}{' general' if d['general'] else ''} {ci}->{co} filter {fw}x{fh} stride ({sx},{sy}) dilation ({dx},{dy}) out {ow}x{oh}x{ob} at {omin[1:]} "
            f"zeros ({az},{fz}) quant {q} split {d['split']} ({d['splits']} planned, ran {ran}) input strides {[v for v in inp.strides]} "
            f"output channels {k}..{k + co} of {P}")
    return desc, ok


def fuzz_hannk_conv(rng):
    """conv_u8_u8_u8 or conv_u8_u8_i16 (a third) on random channels (1 .. 150 in, a multiple of 16 in a quarter of the cases; 1 .. 70 out),
    filter 1 .. 4 square or not, strides and dilations 1 .. 3, zero points, an output box with mins of its own cropped out of a larger input,
    padded pixels, rows and planes on the input, an output that is a channel slice of wider pixels, the default path (any split-K the
    plan takes, or one forced by HLMI_HANNK_SPLIT_K) or the general one, against tests/cpp/hannk_check.c.  Compared byte for byte; the
    bytes around and between the output's pixels must come back unchanged."""
    return run_hannk_conv(draw_hannk_conv(rng))


def draw_hannk_depthwise(rng):
    """the parameters of one fuzz_hannk_depthwise case and the classes they fall in; no array, no library, no device"""
    c = rdim(rng, 1, 70)
    fw, fh = (3, 3) if rng.random() < 0.4 else (int(rng.integers(1, 6)), int(rng.integers(1, 6)))
    (sx, sy), (dx, dy) = (int(v) for v in rng.integers(1, 4, 2)), (int(v) for v in rng.integers(1, 4, 2))
    d = dict(c=c, fw=fw, fh=fh, stride=(sx, sy), dilation=(dx, dy), out=(rdim(rng, 1, 30), rdim(rng, 1, 14), int(rng.integers(1, 4))),
             omin=[0] + [int(v) for v in rng.integers(-3, 4, 3)])
    d["broadcast"], d["general"] = bool(rng.random() < 0.3), bool(rng.random() < 0.25)
    d["az"], d["fz"] = int(rng.integers(0, 256)), int(rng.integers(0, 256))
    cp = 1 if d["broadcast"] else -(-c // 16) * 16
    d["in_pixel_stride"] = cp + (16 * int(rng.integers(1, 3)) if not d["broadcast"] and rng.random() < 0.3 else 0)
    d["in_pads"] = tuple(16 * int(rng.integers(1, 4)) if not d["broadcast"] and rng.random() < 0.5 else 0 for _ in range(2))
    d["out_pixel_stride"], d["out_channel"] = _slice_of_wider(rng, c, 0.4)
    d["out_pads"] = (int(rng.integers(0, 6)), int(rng.integers(0, 6)))
    q = _hannk_quant(rng)
    d["quant"] = (q[0], int(rng.integers(0, 8)), *q[2:])
    d["vector"] = None if d["general"] or rng.random() < 0.3 else 1   # these outputs are below the plan's threshold: force its kernel
    d["seed"] = int(rng.integers(0, 1 << 32))
    # classes
    d["kernel"] = ("general", d["broadcast"]) if d["vector"] is None else ("dw", (fw, fh) == (3, 3), d["broadcast"])
    d["sliced_output"] = d["out_pixel_stride"] > c
    return d


def run_hannk_depthwise(d):
    """one drawn case on the device against tests/cpp/hannk_check.c, the output in a device allocation of the case's own as in run_hannk_conv"""
    import hannk_checker as hk
    from parity_helpers import DevTensor, launches
    rng = np.random.default_rng(d["seed"])
    c, fw, fh, (sx, sy), (dx, dy), (ow, oh, ob), omin = d["c"], d["fw"], d["fh"], d["stride"], d["dilation"], d["out"], d["omin"]
    az, fz, q, broadcast = d["az"], d["fz"], d["quant"], d["broadcast"]
    cp = 1 if broadcast else -(-c // 16) * 16
    ext = lambda o, s, f, dil: (o - 1) * s + (f - 1) * dil + 1
    imin = [0, omin[1] * sx, omin[2] * sy, omin[3]]
    noise = rng.integers(0, 256, (ob, ext(oh, sy, fh, dy), ext(ow, sx, fw, dx), cp), dtype=np.uint8)
    inp, _keep_i = _nhwc(noise.shape, d["in_pixel_stride"], *d["in_pads"], noise) if not broadcast else (noise, None)
    filt = rng.integers(0, 256, (fh, fw, c), dtype=np.uint8)
    bias = rng.integers(-(1 << 16), 1 << 16, c).astype(np.int32)
    want = hk.depthwise(inp, filt, bias, [c, ow, oh, ob], (sx, sy), (dx, dy), az, fz, *q, broadcast, in_mins=imin, out_mins=omin)
    P, k = d["out_pixel_stride"], d["out_channel"]
    rs = ow * P + d["out_pads"][0]
    o = DevTensor(hl, (ob, oh, ow, c), (rs * oh + d["out_pads"][1], rs, P, 1), offset=k, mins=omin)
    try:
        name = "depthwise_conv_broadcast_uint8" if broadcast else "depthwise_conv_uint8"
        args = [hl.Buffer(inp, mins=imin), az, hl.Buffer(filt), fz, hl.Buffer(bias), sx, sy, dx, dy, 0, *q, o.buf]
        if d["general"]:
            call = lambda: hl.debug_hannk_general(name, *args)
        else:
            call = lambda: hl._check(hl._fn[name](*[a.ptr if isinstance(a, hl.Buffer) else a for a in args]))
        ran = _with_env("HLMI_HANNK_DW_VECTOR", d["vector"], lambda: launches(hl, call))
        try:
            ok = np.array_equal(o.result(), want)
        except AssertionError:      # bytes outside the output were written
            ok = False
        ok = ok and ran == (["hannk_dw_general"] if d["kernel"][0] == "general" else ["hannk_dw"])
    finally:
        o.free()
    desc = (f"{name}{' general' if d['general'] else ''} c {c} filter {fw}x{fh} stride ({sx},{sy}) dilation ({dx},{dy}) out {ow}x{oh}x{ob} at {omin[1:]} "
            f"zeros ({az},{fz}) quant {q} vector {d['vector']} (ran {ran}) input strides {[v for v in inp.strides]} output channels {k}..{k + c} of {P}")
    return desc, ok


def fuzz_hannk_depthwise(rng):
    """depthwise_conv_uint8 or its broadcast variant on random channels (1 .. 70), filter 1 .. 5 (3 x 3 in two fifths of the cases), strides
    and dilations 1 .. 3, zero points, a cropped output box that may be a channel slice of wider pixels, padded input pixels, rows and
    planes (multiples of 16), either path, against tests/cpp/hannk_check.c, byte for byte, the bytes between the output's pixels included."""
    return run_hannk_depthwise(draw_hannk_depthwise(rng))


def _hannk_nn_call(name, args, general, env):
    """the entry point (or its general path) under the given HLMI_HANNK_* switches, restored afterwards"""
    keys = ["HLMI_HANNK_" + k for k in ("POOL_VECTOR", "POOL_SPLIT", "MEAN_SPLIT", "EW_VECTOR", "ROWS_WAVE", "ROWS_KEEP")]
    prev = {k: os.environ.pop(k, None) for k in keys}
    try:
        for k, v in env.items():
            os.environ["HLMI_HANNK_" + k] = str(v)
        if general:
            hl.debug_hannk_general(name, *args)
        else:
            hl._check(hl._fn[name](*[a.ptr if isinstance(a, hl.Buffer) else a for a in args]))
    finally:
        for k in keys:
            os.environ.pop(k, None)
            if prev[k] is not None:
                os.environ[k] = prev[k]


def fuzz_hannk_pool(rng):
    """average_pool_uint8, max_pool_uint8 or mean_uint8: random channels (1 .. 70), filters 1 .. 8, strides 1 .. 3, an input translated so
    that windows cross its edges or miss it, clamps that may cross; mean over a random region of a random subset of the dimensions; the
    plan's kernel, a forced one or the general path, against tests/cpp/hannk_nn_check.c, byte for byte."""
    import hannk_nn_checker as hk
    general = rng.random() < 0.25
    c, ob = rdim(rng, 1, 70), int(rng.integers(1, 3))
    if rng.random() < 0.3:
        rext = [int(rng.integers(2, 9)) if rng.random() < 0.5 else 1 for _ in range(4)]
        oext = [c if rext[0] == 1 else 1, rdim(rng, 1, 6), rdim(rng, 1, 5), ob]
        omin, rmin = [int(v) for v in rng.integers(-2, 3, 4)], [int(v) for v in rng.integers(-2, 3, 4)]
        imin = [omin[d] + rmin[d] - int(rng.integers(0, 2)) for d in range(4)]
        iext = [omin[d] + rmin[d] - imin[d] + oext[d] + rext[d] - 1 + int(rng.integers(0, 2)) for d in range(4)]
        inp = rng.integers(0, 256, tuple(reversed(iext)), dtype=np.uint8)
        want = hk.mean(inp, oext, rmin, rext, imin, omin)
        o = hl.Buffer(np.full(want.shape, 0x5A, np.uint8), mins=omin)
        env = {} if general or rng.random() < 0.5 else {"MEAN_SPLIT": int(rng.integers(0, 2))}
        _hannk_nn_call("mean_uint8", [hl.Buffer(inp, mins=imin)] + [v for pair in zip(rmin, rext) for v in pair] + [o], general, env)
        return f"mean_uint8{' general' if general else ''} in {iext} at {imin} out {oext} at {omin} region {rext} at {rmin} {env}", np.array_equal(o.numpy(), want)
    kind = "average" if rng.random() < 0.5 else "max"
    w, h = rdim(rng, 1, 20), rdim(rng, 1, 14)
    (fw, fh), (sx, sy) = rng.integers(1, 9, 2), rng.integers(1, 4, 2)
    ow, oh = rdim(rng, 1, 12), rdim(rng, 1, 8)
    imin = [0, int(rng.integers(-3, 4)), int(rng.integers(-3, 4)), 0]
    omin = [0, int(rng.integers(-2, 2)), int(rng.integers(-2, 2)), 0]
    lo, hi = (int(rng.integers(0, 60)), int(rng.integers(190, 256))) if rng.random() < 0.8 else (int(rng.integers(0, 256)), int(rng.integers(0, 256)))
    cp = c if rng.random() < 0.5 else -(-c // 4) * 4 + 4 * int(rng.integers(0, 2))   # pixels padded to quads: the dword kernels
    store = rng.integers(0, 256, (ob, h, w, cp), dtype=np.uint8)
    inp = store[..., :c]
    want = hk.pool(kind, inp, (c, ow, oh, ob), (sx, sy), (fw, fh), lo, hi, imin, omin)
    o = hl.Buffer(np.full(want.shape, 0x5A, np.uint8), mins=omin)
    env = {} if general or rng.random() < 0.4 else {"POOL_SPLIT": int(rng.integers(0, 2))} if rng.random() < 0.7 else {"POOL_VECTOR": 0}
    _hannk_nn_call(f"{kind}_pool_uint8", [hl.Buffer(inp, mins=imin), int(sx), int(sy), int(fw), int(fh), lo, hi, o], general, env)
    desc = (f"{kind}_pool_uint8{' general' if general else ''} c {c} (pixel stride {cp}) in {w}x{h} at {imin[1:3]} out {ow}x{oh}x{ob} at {omin[1:3]} "
            f"filter {fw}x{fh} stride ({sx},{sy}) clamp ({lo},{hi}) {env}")
    return desc, np.array_equal(o.numpy(), want)


def fuzz_hannk_elementwise(rng):
    """add_uint8_uint8, mul_uint8_uint8_uint8, softmax_uint8 or l2_normalization_uint8 on 1 .. 6 rows of 1 .. 1500 bytes in padded rows:
    either operand of add / mul broadcast through a stride of 0, multipliers and shifts over their whole ranges; softmax and
    l2_normalization on dense or transposed buffers; the plan's kernel, a forced one or the general path, against
    tests/cpp/hannk_nn_check.c, byte for byte."""
    import hannk_nn_checker as hk
    general = rng.random() < 0.25
    h = int(rng.integers(1, 7))
    op = ("add", "mul", "softmax", "l2")[int(rng.integers(0, 4))]
    if op in ("add", "mul"):
        w = rdim(rng, 1, 300)
        ops = []
        for k in range(2):
            if rng.random() < 0.2 and (k == 0 or ops[0].strides[1] != 0):
                ops.append(np.broadcast_to(rng.integers(0, 256, (h, 1), dtype=np.uint8), (h, w)))
            else:
                ops.append(rng.integers(0, 256, (h, w + int(rng.integers(0, 20))), dtype=np.uint8)[:, :w])
        z1, z2, oz = (int(v) for v in rng.integers(0, 256, 3))
        lo, hi = int(rng.integers(0, 60)), int(rng.integers(190, 256))
        o = hl.Buffer(np.full((h, w), 0x5A, np.uint8))
        if op == "add":
            m1, m2 = (int(v) for v in rng.integers(-32768, 32768, 2))
            want = hk.add(ops[0], z1, m1, ops[1], z2, m2, oz, lo, hi, (w, h))
            name, args = "add_uint8_uint8", [hl.Buffer(ops[0]), z1, m1, hl.Buffer(ops[1]), z2, m2, oz, lo, hi, o]
        else:
            mult, shift = int(rng.integers(-(1 << 31), 1 << 31)), int(rng.integers(0, 32))
            want = hk.mul(ops[0], z1, ops[1], z2, oz, mult, shift, lo, hi, (w, h))
            name, args = "mul_uint8_uint8_uint8", [hl.Buffer(ops[0]), z1, hl.Buffer(ops[1]), z2, oz, mult, shift, lo, hi, o]
        env = {} if general or rng.random() < 0.5 else {"EW_VECTOR": int(rng.integers(0, 2))}
        _hannk_nn_call(name, args, general, env)
        return f"{name}{' general' if general else ''} {w}x{h} strides {[a.strides for a in ops]} {args[1:-1]} {env}", np.array_equal(o.numpy(), want)
    n = rdim(rng, 1, 1500)
    transposed = rng.random() < 0.2
    store = rng.integers(0, 256, (n, h) if transposed else (h, n), dtype=np.uint8)
    if rng.random() < 0.3:
        store[...] = rng.integers(0, 60, store.shape, dtype=np.uint8)
    inp = store.T if transposed else store
    dst = np.full(store.shape, 0x5A, np.uint8)
    o = hl.Buffer(dst.T if transposed else dst)
    if op == "softmax":
        bm, bs, oz = int(rng.integers(1, 32768)), int(rng.integers(0, 16)), int(rng.integers(0, 8))
        om, osh = int(rng.integers(1, 32768)), int(rng.integers(0, 16))
        want = hk.softmax(inp, bm, bs, oz, om, osh)
        name, args = "softmax_uint8", [hl.Buffer(inp), bm, bs, oz, om, osh, o]
    else:
        zero = int(rng.integers(0, 256))
        want = hk.l2_normalization(inp, zero)
        name, args = "l2_normalization_uint8", [hl.Buffer(inp), zero, o]
    env = {} if general or rng.random() < 0.5 else {"ROWS_KEEP": 0} if rng.random() < 0.6 else {"ROWS_WAVE": 0}
    _hannk_nn_call(name, args, general, env)
    return f"{name}{' general' if general else ''} {h} rows of {n}{' transposed' if transposed else ''} {args[1:-1]} {env}", np.array_equal(np.ascontiguousarray(o.numpy()), want)


CASES = {k[5:]: v for k, v in list(globals().items()) if k.startswith("case_")}
CASES["resize"] = fuzz_resize   # these three: their checkers are not oracle/'s (tests/checker_lib.py)
CASES["gaussian_blur"] = fuzz_gaussian_blur
CASES["linear_blur"] = fuzz_linear_blur   # both entry points
CASES["reaction_diffusion"] = fuzz_reaction_diffusion   # init, update, render and run; its checker has a module of its own
CASES["wavelet"] = fuzz_wavelet   # all four entry points; its checker has a module of its own (tests/wavelet_checker.py)
CASES["compositing"] = fuzz_compositing   # integer throughout: its checker (tests/compositing_checker.py) has no canonical form
CASES["hexagon_benchmarks"] = fuzz_hexagon_benchmarks   # all six entry points; integer throughout (tests/hexagon_benchmarks_checker.py)
CASES["mat_mul"] = fuzz_mat_mul   # sized and general paths; one chain in both canonical forms (tests/mat_mul_checker.py)
CASES["linear_algebra"] = fuzz_linear_algebra   # all twelve entry points, both paths (tests/linear_algebra_checker.py)
CASES["linear_algebra_f64"] = fuzz_linear_algebra_f64   # the f64 half, both paths (tests/linear_algebra_checker.py)
CASES["fft"] = fuzz_fft   # all four kinds, both paths (tests/fft_checker.py)
CASES["hannk_conv"] = fuzz_hannk_conv   # both output types, both paths, split-K; integer throughout (tests/hannk_checker.py)
CASES["hannk_depthwise"] = fuzz_hannk_depthwise   # both variants, both paths
CASES["hannk_pool"] = fuzz_hannk_pool   # both pools and mean, every kernel of their plans (tests/hannk_nn_checker.py)
CASES["hannk_elementwise"] = fuzz_hannk_elementwise   # add, mul, softmax, l2_normalization, every kernel of their plans


def stress(args, only):
    """Host threads calling different pipelines at once: the caches (remap tables, filter images, camera set-up), the
    allocation cache and the per-stream arenas under contention.  Results must still be the oracle's."""
    import threading
    names = [n for n in CASES if not only or n in only]
    hip = hl.hip_runtime()
    log, lock = [], threading.Lock()
    counts = {n: [0, 0, 0] for n in names}
    t_end = time.time() + args.seconds

    def worker(i):
        rng = np.random.default_rng(args.seed * 7919 + i)
        stream = None
        if i % 2 == 1:
            import ctypes
            stream = ctypes.c_void_p()
            assert hip.hipStreamCreateWithFlags(ctypes.byref(stream), 1) == 0
            hl.set_stream(stream.value)
        while time.time() < t_end:
            name = names[int(rng.integers(0, len(names)))]
            try:
                desc, ok = CASES[name](rng)
                with lock:
                    counts[name][0] += 1
                    if not ok:
                        counts[name][1] += 1
                        log.append(f"thread {i}: {name}: MISMATCH {desc}")
            except Exception as e:  # noqa: BLE001
                with lock:
                    counts[name][0] += 1
                    counts[name][2] += 1
                    log.append(f"thread {i}: {name}: EXCEPTION {type(e).__name__}: {str(e)[:200]}")
        if stream is not None:
            hl.set_stream(None)
            hip.hipStreamSynchronize(stream)

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(args.threads)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for line in log[:20]:
        print("  " + line)
    bad = 0
    for n in names:
        c = counts[n]
        bad += c[1] + c[2]
        print(f"{n}: {c[0]} cases, {c[1]} mismatches, {c[2]} exceptions")
    print(f"STRESS ({args.threads} threads) " + ("CLEAN" if bad == 0 else f"FOUND {bad}"))
    return 0 if bad == 0 else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--seconds", type=float, default=20.0, help="time budget per pipeline")
    ap.add_argument("--only", default="")
    ap.add_argument("--threads", type=int, default=1, help="> 1: concurrency stress — that many host threads draw random cases of ALL "
                    "pipelines for --seconds in total, every second thread on a stream of its own")
    ap.add_argument("--frame-queue", action="store_true", help="run the cases with the calling thread on a frame-queue stream "
                    "(halide_hip_partition_stream(1, 4)): local_laplacian takes its throughput geometry there — one ll_down01e "
                    "workgroup per CU, fewer and taller units, taller ll_up0h tiles, non-temporal frame accesses")
    args = ap.parse_args()
    only = [s for s in args.only.split(",") if s]
    if args.threads > 1:
        return stress(args, only)
    if args.frame_queue:
        q = hl.partition_stream(1, 4)
        assert q, "the device refused a frame-queue stream"
        hl.set_stream(q)
    bad = 0
    for name, fn in CASES.items():
        if only and name not in only:
            continue
        rng = np.random.default_rng(args.seed * 1000 + sum(map(ord, name)))
        n = fails = errors = 0
        t0 = time.time()
        while time.time() - t0 < args.seconds:
            try:
                desc, ok = fn(rng)
            except Exception as e:  # a case the entry point rejects is a finding too: print it
                errors += 1
                if errors <= 5:
                    print(f"  {name}: EXCEPTION {type(e).__name__}: {str(e)[:200]}", flush=True)
                n += 1
                continue
            n += 1
            if not ok:
                fails += 1
                if fails <= 8:
                    print(f"  {name}: MISMATCH {desc}", flush=True)
        bad += fails + errors
        print(f"{name}: {n} cases, {fails} mismatches, {errors} exceptions", flush=True)
    print("FUZZ " + ("CLEAN" if bad == 0 else f"FOUND {bad}"))
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
