"""resnet50: the f32 ResNet-50 forward pass of apps/resnet_50 as exact k-ordered chains.

The contract is in include/hlmi_pipelines.h and DESIGN.md 5.11.  The checker is tests/cpp/resnet50_check.c, plain C, built and bound by
tests/resnet50_checker.py.  The CPU tests hold each layer function of the checker to a float64 evaluation within a bound derived here,
the whole checker to a float64 plain-torch ResNet-50 by the reference's own acceptance (validate_resnet50_output.py: equal argmax,
probabilities equal to 2 decimals), show that the inputs used on the GPU tell a wrong summation order from the right one, state the
-0 trap in numbers, and hold the entry point to its protocol, its metadata and its loaders.  The GPU tests hold the layer hook (every
variant of the plan, default and general path), the pool and tail hooks and the whole network to the checker bit for bit, NaN for
NaN, in the canonical form the loaded library reports."""
import ctypes as C
import functools
import os
import struct
import subprocess
import threading

import numpy as np
import pytest

import resnet50_checker as rn
from parity_helpers import ROOT, DevArray, HostArray, call_argv, call_direct, kernel_const
from parity_helpers import gpu_present as _gpu_present, launches as _launches, same_bits as _same, same_bits_or_nan as _same_or_nan

f32, f64, u32 = np.float32, np.float64, np.uint32
U = 2.0 ** -24   # unit roundoff of binary32

# the plan's constants, read from the source: a kernel without them fails here
KC, TILE, SHORT_K = (kernel_const("resnet50.hip", n) for n in ("KC", "TILE", "SHORT_K"))
MFMA, GENERAL = "resnet50_conv_mfma", "resnet50_conv_general"
PAD_OF = {1: 0, 3: 1, 7: 3}


@pytest.fixture(autouse=True)
def _checker_follows_the_library(hl):
    rn.set_canon(hl.canon_fma())
    yield


def _expected_launch(hl, co, K, general):
    """conv_plan() of resnet50.hip restated; K = KW KH CI"""
    if general or not hl.canon_fma():
        return GENERAL
    return GENERAL if K <= SHORT_K and co <= TILE else MFMA


# ---------------------------------------------------------------------------------------------------- the network's shape, restated
def _convs():
    """(ci, co, k, stride, pad, input size) of the 53 convolutions in argument order: conv1, br1 x 4, br2a x 16, br2b x 16, br2c x 16"""
    br1, a, b, c = [], [], [], []
    cin, size = 64, 56
    for mid, blocks, stride in ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)):
        for i in range(blocks):
            st = stride if i == 0 else 1
            osize = rn.out_extent(size, 1, st, 0)
            if i == 0:
                br1.append((cin, 4 * mid, 1, st, 0, size))
            a.append((cin, mid, 1, 1, 0, size))
            b.append((mid, mid, 3, st, 1, size))
            c.append((mid, 4 * mid, 1, 1, 0, osize))
            cin, size = 4 * mid, osize
    return [(3, 64, 7, 2, 3, 224)] + br1 + a + b + c


CONVS = _convs()


def _state_dict(seed):
    """a torchvision-layout ResNet-50 state dict of float32 arrays with the issue's seeded initialisation"""
    rng = np.random.default_rng(seed)
    sd = {}

    def layer(prefix_conv, prefix_bn, ci, co, k, small_gamma):
        sd[prefix_conv + ".weight"] = (rng.standard_normal((co, ci, k, k)) * np.sqrt(2.0 / (k * k * ci))).astype(f32)
        sd[prefix_bn + ".weight"] = (rng.random(co) * (0.25 if small_gamma else 1.0) + (0.125 if small_gamma else 0.5)).astype(f32)
        sd[prefix_bn + ".bias"] = (0.1 * rng.standard_normal(co)).astype(f32)
        sd[prefix_bn + ".running_mean"] = (0.1 * rng.standard_normal(co)).astype(f32)
        sd[prefix_bn + ".running_var"] = (rng.random(co) + 0.5).astype(f32)
        sd[prefix_bn + ".num_batches_tracked"] = np.array(0, np.int64)

    layer("conv1", "bn1", 3, 64, 7, False)
    cin = 64
    for s, (mid, blocks) in enumerate(((64, 3), (128, 4), (256, 6), (512, 3))):
        for i in range(blocks):
            p = f"layer{s + 1}.{i}"
            layer(p + ".conv1", p + ".bn1", cin, mid, 1, False)
            layer(p + ".conv2", p + ".bn2", mid, mid, 3, False)
            layer(p + ".conv3", p + ".bn3", mid, 4 * mid, 1, True)
            if i == 0:
                layer(p + ".downsample.0", p + ".downsample.1", cin, 4 * mid, 1, False)
            cin = 4 * mid
    sd["fc.weight"] = (rng.standard_normal((1000, 2048)) * np.sqrt(4.0 / 2048)).astype(f32)
    sd["fc.bias"] = (0.1 * rng.standard_normal(1000)).astype(f32)
    return sd


@functools.lru_cache(maxsize=None)
def _net_case(seed):
    """(state dict, image (224, 224, 3), parameter list, the checker's result in the library's form), computed once per module"""
    import halide_amd as hl
    sd = _state_dict(seed)
    named = hl.resnet50_params_from_state_dict(sd)
    params = [named[n] for n in hl.RESNET50_PARAM_NAMES]
    image = np.random.default_rng(seed + 1000).random((224, 224, 3), dtype=f32)
    rn.set_canon(hl.canon_fma())
    want = rn.network(image, params)
    for a in [image] + params + list(want.values()):
        a.setflags(write=False)
    # a degenerate input cannot pass silently: the conditions the issue states, on the checker's output
    assert np.isfinite(want["out"]).all() and np.isfinite(want["fc"]).all()
    assert want["fc"].max() < 80
    top = np.sort(want["out"])[::-1]
    assert top[0] - top[1] >= 1e-3, (top[0], top[1])
    return sd, image, params, want


SEEDS = (1,)


# ---------------------------------------------------------------------------------------------------- layer inputs
def _noise(shape, seed):
    return (np.random.default_rng(seed).random(shape, dtype=f32) * 2 - 1).astype(f32)


def _vectors(co, seed):
    rng = np.random.default_rng(seed)
    gamma = (rng.random(co) + 0.5).astype(f32) * np.where(rng.random(co) < 0.3, f32(-1), f32(1))
    return gamma.astype(f32), (0.1 * rng.standard_normal(co)).astype(f32), (0.1 * rng.standard_normal(co)).astype(f32), (rng.random(co) + 0.5).astype(f32)


@functools.lru_cache(maxsize=None)
def _layer_case(ci, co, w, h, k, stride, kind="noise", seed=0):
    """(input (H, W, CI), weights (CI, K, K, CO), (gamma, beta, mu, sig), residual (OH, OW, CO)), never written to"""
    pad = PAD_OF[k]
    ow, oh = rn.out_extent(w, k, stride, pad), rn.out_extent(h, k, stride, pad)
    x, wt = _noise((h, w, ci), 11 + seed), _noise((ci, k, k, co), 12 + seed)
    rng = np.random.default_rng(13 + seed)
    if kind == "order":
        pool = np.array([2.0 ** 24, -2.0 ** 24, 1.0, -1.0, 2.0 ** -24, -2.0 ** -24], f32)
        big = rng.choice(pool, wt.shape).astype(f32)
        big[..., co // 2:] = rng.choice(pool[2:], big[..., co // 2:].shape)   # no 2^24 in the upper half of co: noise x noise roundings show there
        pick = rng.random(wt.shape) < 0.7
        wt[pick] = big[pick]
        sign = np.where(rng.random(x.shape) < 0.5, f32(1), f32(-1)).astype(f32)
        pick = rng.random(x.shape) < 0.7
        x[pick] = sign[pick]
    elif kind == "special":
        specials = np.array([0.0, -0.0, 1e-40, -3e-39, np.inf, -np.inf, np.nan, 3e38, -2e38, 2.0 ** 100, -2.0 ** 100], f32)
        chans = rng.choice(co, max(1, co // 16), replace=False)
        for c in chans:
            for _ in range(3):
                wt[rng.integers(ci), rng.integers(k), rng.integers(k), c] = rng.choice(specials)
        wt[0, 0, 0, chans[0]] = np.inf
        wt[ci - 1, k - 1, k - 1, chans[-1]] = np.nan if len(chans) > 1 else np.inf
    vec = _vectors(co, 14 + seed)
    res = _noise((oh, ow, co), 15 + seed)
    for a in (x, wt, res) + vec:
        a.setflags(write=False)
    return x, wt, vec, res


@functools.lru_cache(maxsize=None)
def _layer_want(canon, ci, co, w, h, k, stride, mode, kind="noise", seed=0):
    x, wt, vec, res = _layer_case(ci, co, w, h, k, stride, kind, seed)
    with rn.canon(canon):
        out = rn.conv(x, wt, *vec, residual=res, stride=stride, pad=PAD_OF[k], mode=mode)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------- float64 evaluations
def _taps64(x, wt, stride, pad):
    """(sum over k of w x, sum over k of |w x|) in float64, shapes (OH, OW, CO)"""
    h, w, ci = x.shape
    _, kh, kw, co = wt.shape
    ow, oh = rn.out_extent(w, kw, stride, pad), rn.out_extent(h, kh, stride, pad)
    xp = np.zeros((h + 2 * pad + stride, w + 2 * pad + stride, ci), f64)
    xp[pad:pad + h, pad:pad + w] = x
    s, a = np.zeros((oh, ow, co), f64), np.zeros((oh, ow, co), f64)
    for ky in range(kh):
        for kx in range(kw):
            patch = xp[ky:ky + stride * oh:stride, kx:kx + stride * ow:stride]   # (OH, OW, CI)
            s += patch @ wt[:, ky, kx, :].astype(f64)
            a += np.abs(patch) @ np.abs(wt[:, ky, kx, :].astype(f64))
    return s, a


LAYER_SHAPES = [(1, 1, 1, 1, 1, 1), (3, 8, 5, 7, 3, 1), (5, 63, 9, 8, 3, 2), (64, 64, 9, 8, 1, 1), (3, 65, 17, 15, 7, 2), (64, 130, 17, 15, 3, 1),
                (5, 130, 17, 15, 1, 2), (1, 64, 5, 7, 7, 1), (5, 8, 9, 8, 7, 2)]
# the same sets of CI, CO and image where the plan's predicate sends the default path to the MFMA kernel (K above SHORT_K, or CO above
# TILE), and images of several rows of tiles
BIG_SHAPES = [(3, 1, 5, 7, 7, 1), (3, 63, 9, 8, 7, 1), (64, 64, 9, 8, 3, 1), (1, 130, 5, 7, 7, 1), (64, 64, 17, 15, 3, 2), (1, 65, 1, 1, 1, 1),
              (5, 130, 40, 36, 1, 1), (3, 130, 40, 36, 3, 1), (64, 65, 90, 92, 1, 2)]


# ---------------------------------------------------------------------------------------------------- CPU 1: the checker's layers
@pytest.mark.parametrize("canon", [0, 1])
@pytest.mark.parametrize("shape", LAYER_SHAPES)
def test_the_checkers_convolution_against_float64(shape, canon):
    """A chain of K steps from +0 carries at most K roundings (fused) or 2 K (multiply, then add), each at most U times a partial sum
    that |w x| summed bounds: |chain - exact| <= (K + 2) U sum|w x| fused and twice that unfused, to first order; what follows the
    chain is five more operations (subtract, divide by a rounded sqrt of a rounded sum, mad, add), each within 2 U of its own result,
    and scales the chain's error by |gamma| / sd.  ReLU is 1-Lipschitz."""
    ci, co, w, h, k, stride = shape
    x, wt, (gamma, beta, mu, sig), res = _layer_case(*shape)
    s, a = _taps64(x, wt, stride, PAD_OF[k])
    K = k * k * ci
    e_chain = (K + 2) * U * a * (1 if canon else 2)
    raw = _layer_want(canon, *shape, "raw")
    assert (np.abs(raw - s) <= e_chain).all(), np.abs(raw - s).max()
    sd = np.sqrt(sig.astype(f64) + f64(f32(1e-5)))
    t = (s - mu) / sd
    scaled = t * gamma + beta
    mag = np.abs(t * gamma) + np.abs(beta) + np.abs(mu / sd * gamma)
    e_scaled = e_chain * np.abs(gamma) / sd * (1 + 8 * U) + 12 * U * mag
    got = _layer_want(canon, *shape, "scaled")
    assert (np.abs(got - scaled) <= e_scaled).all(), np.abs(got - scaled).max()
    got = _layer_want(canon, *shape, "scaled_relu")
    assert (np.abs(got - np.maximum(scaled, 0)) <= e_scaled).all()
    got = _layer_want(canon, *shape, "residual_relu")
    assert (np.abs(got - np.maximum(scaled + res, 0)) <= e_scaled + 2 * U * (np.abs(res) + np.abs(scaled))).all()


def test_the_checkers_convolution_is_exact_where_every_partial_sum_is():
    rng = np.random.default_rng(3)
    for ci, co, w, h, k, stride in LAYER_SHAPES[:6]:
        x = rng.integers(-8, 9, (h, w, ci)).astype(f32)
        wt = rng.integers(-8, 9, (ci, k, k, co)).astype(f32)
        s, a = _taps64(x, wt, stride, PAD_OF[k])
        assert a.max() < 2 ** 24
        for canon in (0, 1):
            with rn.canon(canon):
                _same(rn.conv(x, wt, stride=stride, pad=PAD_OF[k]), s.astype(f32), f"integers {ci, co, w, h, k, stride} canon {canon}")


def test_the_checker_reads_padded_strides():
    shape = (5, 63, 9, 8, 3, 2)
    x, wt, vec, res = _layer_case(*shape)
    wide = np.full((8, 9 + 2, 5 + 3), 9e9, f32)
    wide[:, :9, :5] = x
    wres = np.full(res.shape[:1] + (res.shape[1] + 1, res.shape[2] + 2), 9e9, f32)
    wres[:, :res.shape[1], :res.shape[2]] = res
    wwt = np.full((5, 3 + 1, 3, 63 + 1), 9e9, f32)
    wwt[:, :3, :, :63] = wt
    got = rn.conv(wide[:, :9, :5], wwt[:, :3, :, :63], *vec, residual=wres[:, :res.shape[1], :res.shape[2]], stride=2, pad=1, mode="residual_relu")
    _same(got, rn.conv(x, wt, *vec, residual=res, stride=2, pad=1, mode="residual_relu"), "padded strides")


def _maxpool_numpy(x, k, stride, pad):
    h, w, c = x.shape
    ow, oh = rn.out_extent(w, k, stride, pad), rn.out_extent(h, k, stride, pad)
    xp = np.zeros((h + 2 * pad + stride, w + 2 * pad + stride, c), f32)
    xp[pad:pad + h, pad:pad + w] = x
    out = np.full((oh, ow, c), -np.inf, f32)
    for ry in range(k):
        for rx in range(k):
            out = np.maximum(out, xp[ry:ry + stride * oh:stride, rx:rx + stride * ow:stride])
    return out


POOL_SHAPES = [(1, 1, 1, 3, 2, 1), (5, 9, 8, 3, 2, 1), (64, 17, 15, 3, 2, 1), (3, 6, 7, 2, 1, 0), (65, 5, 7, 3, 1, 1)]


@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_the_checkers_max_pool_is_numpys_maximum_over_the_zero_padded_image(shape):
    c, w, h, k, stride, pad = shape
    for lo in (0.0, -3.0):   # all negative: the +0 exterior wins at the border
        x = (_noise((h, w, c), 5) + f32(lo)).astype(f32)
        _same(rn.maxpool(x, k, stride, pad), _maxpool_numpy(x, k, stride, pad), f"{shape} {lo}")
    if pad:
        assert (rn.maxpool((_noise((h, w, c), 5) - f32(3)).astype(f32), k, stride, pad)[0, 0] == 0).all()


TAIL_SHAPES = [(1, 1, 1, 1), (5, 3, 2, 7), (64, 7, 7, 10), (130, 2, 3, 65)]


def _tail_case(shape, seed=0, scale=1.0):
    c, w, h, n = shape
    rng = np.random.default_rng(40 + seed)
    x = rng.random((h, w, c), dtype=f32)
    fw = (rng.standard_normal((c, n)) * np.sqrt(4.0 / c) * scale).astype(f32)
    fb = (0.1 * rng.standard_normal(n)).astype(f32)
    return x, fw, fb


@pytest.mark.parametrize("canon", [0, 1])
@pytest.mark.parametrize("shape", TAIL_SHAPES)
def test_the_checkers_tail_against_float64_stage_by_stage(shape, canon):
    """Each stage is held to float64 on the checker's own previous stage, so the bounds do not compound: the mean and the fc are chains
    as above; halide_exp is within 2^-20 relative of exp on this range (tests/test_device_math.py sweeps it); the sum of N positive
    terms is within N U of itself, the quotient within U."""
    c, w, h, n = shape
    x, fw, fb = _tail_case(shape)
    with rn.canon(canon):
        r = rn.tail(x, fw, fb)
    m = 1 if canon else 2
    nn = f64(f32(1.0) / f32(w * h))
    pool = (x.astype(f64) * nn).sum(axis=(0, 1))
    assert (np.abs(r["pool"] - pool) <= (w * h + 2) * U * m * pool).all()
    p = r["pool"].astype(f64)
    fc = fb + p @ fw.astype(f64)
    assert (np.abs(r["fc"] - fc) <= (c + 3) * U * m * (np.abs(fb) + np.abs(p) @ np.abs(fw.astype(f64)))).all()
    e = np.exp(r["fc"].astype(f64))
    assert (np.abs(r["e"] - e) <= 2.0 ** -20 * e).all()
    S = r["e"].astype(f64).sum()
    assert (np.abs(r["out"] - r["e"] / S) <= (n + 2) * U * r["e"] / S).all()
    assert abs(r["out"].astype(f64).sum() - 1) < (n + 4) * U


def test_the_tail_overflows_to_nan_as_the_contract_says():
    x, fw, fb = _tail_case((5, 3, 2, 7))
    fb = fb.copy()
    fb[3] = 200.0   # exp overflows: inf / inf for that class, x / inf = 0 for the others
    r = rn.tail(x, fw, fb)
    assert np.isinf(r["e"][3]) and np.isnan(r["out"][3]) and (np.delete(r["out"], 3) == 0).all()


# ---------------------------------------------------------------------------------------------------- CPU 2: the whole checker
def _torch_forward(sd, image, dtype):
    """plain torch.nn.functional ResNet-50 (eval-mode batch norm, eps 1e-5) from the state dict; returns (pooled, logits, probabilities)"""
    import torch
    import torch.nn.functional as F
    t = lambda k: torch.from_numpy(np.asarray(sd[k])).to(dtype)
    bn = lambda x, p: F.batch_norm(x, t(p + ".running_mean"), t(p + ".running_var"), t(p + ".weight"), t(p + ".bias"), False, 0.0, 1e-5)
    x = torch.from_numpy(np.ascontiguousarray(image.transpose(2, 0, 1))).to(dtype)[None]   # (1, 3, H, W)
    x = F.relu(bn(F.conv2d(x, t("conv1.weight"), stride=2, padding=3), "bn1"))
    x = F.max_pool2d(x, 3, 2, 1)
    for s, blocks in enumerate((3, 4, 6, 3)):
        for i in range(blocks):
            p = f"layer{s + 1}.{i}"
            st = 2 if (i == 0 and s > 0) else 1
            y = F.relu(bn(F.conv2d(x, t(p + ".conv1.weight")), p + ".bn1"))
            y = F.relu(bn(F.conv2d(y, t(p + ".conv2.weight"), stride=st, padding=1), p + ".bn2"))
            y = bn(F.conv2d(y, t(p + ".conv3.weight")), p + ".bn3")
            if i == 0:
                x = bn(F.conv2d(x, t(p + ".downsample.0.weight"), stride=st), p + ".downsample.1")
            x = F.relu(x + y)
    pooled = x.mean(dim=(2, 3))[0]
    logits = pooled @ t("fc.weight").T + t("fc.bias")
    return pooled.numpy(), logits.numpy(), torch.softmax(logits, 0).numpy()


@pytest.mark.parametrize("seed", SEEDS)
def test_the_whole_checker_against_a_float64_torch_resnet50(hl, seed):
    sd, image, params, want = _net_case(seed)
    pooled, logits, prob = _torch_forward(sd, image, __import__("torch").float64)
    print(f"seed {seed}: max |pool| {np.abs(pooled).max():.3f}, logits [{logits.min():.2f}, {logits.max():.2f}], "
          f"max |checker - f64|: logits {np.abs(want['fc'] - logits).max():.3g}, probabilities {np.abs(want['out'] - prob).max():.3g}")
    # the reference's own acceptance (validate_resnet50_output.py)
    assert np.argmax(want["out"]) == np.argmax(prob)
    np.testing.assert_almost_equal(want["out"], prob, decimal=2)
    # max pooling with a -inf exterior (torch) and with a +0 exterior (the generator) agree behind a ReLU; the stem's 112 -> 56 and the
    # strided stages' extents are compute_shape's
    assert pooled.shape == (2048,) and np.abs(pooled).max() < 100


# ---------------------------------------------------------------------------------------------------- CPU 3: the tests can tell
ORDER_SHAPES = [(64, 65, 9, 8, 1, 1), (5, 63, 9, 8, 3, 2)]   # the MFMA kernel's side of the plan and the general kernel's


@pytest.mark.parametrize("shape", ORDER_SHAPES)
def test_the_order_sensitive_input_tells_every_wrong_association(shape):
    ci, co, w, h, k, stride = shape
    x, wt, _, _ = _layer_case(*shape, kind="order")
    want = _layer_want(1, *shape, "raw", "order")
    assert np.isfinite(want).all()
    differs = lambda other: np.count_nonzero(other.view(u32) != want.view(u32))
    with rn.canon(1):
        reversed_k = rn.conv(np.ascontiguousarray(x[:, :, ::-1]), np.ascontiguousarray(wt[::-1]), stride=stride, pad=PAD_OF[k])   # ci downward inside each tap
        assert differs(reversed_k) > 0, "a chain with ci running downward"
        flipped = rn.conv(np.ascontiguousarray(x[::-1, ::-1]), np.ascontiguousarray(wt[:, ::-1, ::-1]), stride=1, pad=PAD_OF[k])[::-1, ::-1] if stride == 1 and k > 1 else None
        if flipped is not None:
            assert differs(np.ascontiguousarray(flipped)) > 0, "taps running downward"
    with rn.canon(0):
        assert differs(rn.conv(x, wt, stride=stride, pad=PAD_OF[k])) > 0, "a multiply-then-add chain"
    s, _ = _taps64(x, wt, stride, PAD_OF[k])
    assert differs(s.astype(f32)) > 0, "a float64 sum rounded once"
    if k == 1:   # pairwise: products rounded to f32, then a balanced tree
        with np.errstate(all="ignore"):
            t = (x[::stride, ::stride].astype(f64)[..., :, None] * wt[:, 0, 0, :].astype(f64)).astype(f32)   # (OH, OW, CI, CO)
            t = np.moveaxis(t, 2, 0)
            while t.shape[0] > 1:
                if t.shape[0] % 2:
                    t = np.concatenate([t, np.zeros((1,) + t.shape[1:], f32)])
                t = (t[0::2] + t[1::2]).astype(f32)
        assert differs(t[0]) > 0, "a pairwise sum"


def _minus_zero_trap(ci, co, w, h, k, co0, i0, j0):
    """all zero except the LAST step of output (co0, i0, j0): w = -2^-100 at (co0, k - 1, k - 1, ci - 1), x = 2^-100 at the pixel that tap
    reads (stride 1): the chain is +0 until its last product underflows to -0"""
    pad = PAD_OF[k]
    x, wt = np.zeros((h, w, ci), f32), np.zeros((ci, k, k, co), f32)
    wt[ci - 1, k - 1, k - 1, co0] = -2.0 ** -100
    x[j0 + k - 1 - pad, i0 + k - 1 - pad, ci - 1] = 2.0 ** -100
    return x, wt


TRAPS = [(1, 1, 1, 1, 1, 0, 0, 0), (3, 8, 5, 7, 3, 5, 2, 3), (5, 65, 9, 8, 1, 64, 8, 7), (3, 65, 17, 15, 7, 33, 4, 5)]   # K = 1, 27, 5, 147: all odd


@pytest.mark.parametrize("trap", TRAPS)
def test_the_minus_zero_trap_in_numbers(trap):
    ci, co, w, h, k, co0, i0, j0 = trap
    assert (k * k * ci) % 2 == 1
    x, wt = _minus_zero_trap(*trap)
    for canon in (0, 1):
        with rn.canon(canon):
            got = rn.conv(x, wt, stride=1, pad=PAD_OF[k]).view(u32).copy()
        # fused, the last step is the tiny negative product plus +0, which rounds to -0; unfused, the product is -0 and -0 + +0 is +0
        assert got[j0, i0, co0] == (0x80000000 if canon else 0)
        got[j0, i0, co0] = 0
        assert not got.any()   # every other output is +0: one further, zero-padded step would have made this one +0 as well
    assert np.array([np.float32(-0.0) + np.float32(0.0) * np.float32(0.0)], f32).view(u32)[0] == 0


SPECIAL_SHAPES = [(5, 130, 17, 15, 3, 1), (64, 65, 9, 8, 1, 1)]


@pytest.mark.parametrize("mode", ["raw", "scaled"])
@pytest.mark.parametrize("shape", SPECIAL_SHAPES)
def test_the_special_values_leave_most_outputs_numbers(hl, shape, mode):
    x, wt, _, _ = _layer_case(*shape, kind="special")
    assert np.isfinite(x).all() and np.isinf(wt).any()
    want = _layer_want(hl.canon_fma(), *shape, mode, "special")
    bad = np.count_nonzero(~np.isfinite(want))
    assert 0 < bad <= want.size / 8, (bad, want.size)


# ---------------------------------------------------------------------------------------------------- CPU 4: the library's surface
def test_the_entry_point_is_exported_with_argv_and_metadata(hl):
    lib = C.CDLL(hl.LIB_PATH)
    for sym in ("resnet50", "resnet50_argv", "resnet50_metadata", "hlmi_resnet50_general", "hlmi_debug_resnet50_layer", "hlmi_debug_resnet50_maxpool",
                "hlmi_debug_resnet50_tail"):
        assert hasattr(lib, sym), sym
    assert not hasattr(lib, "resnet50_auto_schedule")
    assert hl._fn["resnet50"] is not None and len(hl._fn["resnet50"].argtypes) == 269


def test_metadata_states_269_f32_buffers_in_signature_order(hl):
    md = hl.metadata("resnet50")
    assert md.version == 1 and md.num_arguments == 269 and md.name.decode() == "resnet50" and b"hip" in md.target
    a = [md.arguments[i] for i in range(269)]
    assert [x.name.decode() for x in a] == ["input"] + list(hl.RESNET50_PARAM_NAMES) + ["final_output"]
    assert [x.kind for x in a] == [1] * 268 + [2]
    assert all((x.type.code, x.type.bits) == (2, 32) for x in a)
    assert [x.dimensions for x in a] == [3] + [1] * 212 + [4] * 53 + [2, 1, 1]
    assert not any(x.buffer_estimates for x in a)
    # the generator's declaration order (:31-66), a hand-listed sample
    names = [x.name.decode() for x in a]
    for i, n in ((0, "input"), (1, "conv1_gamma"), (2, "br1_gamma_0"), (6, "br2a_gamma_0"), (21, "br2a_gamma_15"), (22, "br2b_gamma_0"), (53, "br2c_gamma_15"),
                 (54, "conv1_beta"), (107, "conv1_mu"), (160, "conv1_sig"), (212, "br2c_sig_15"), (213, "conv1_weights"), (214, "br1_conv_weights_0"),
                 (218, "br2a_conv_weights_0"), (265, "br2c_conv_weights_15"), (266, "fc1000_weights"), (267, "fc1000_bias"), (268, "final_output")):
        assert names[i] == n, (i, names[i], n)


def test_the_aot_header_compiles_as_c(tmp_path):
    src = tmp_path / "c.c"
    ptrs = ", ".join(["struct halide_buffer_t *"] * 269)
    src.write_text(f'#include "aot/resnet50.h"\nint (*const f)({ptrs}) = resnet50;\n'
                   "int (*const a)(void **) = resnet50_argv;\nconst struct halide_filter_metadata_t *(*const m)(void) = resnet50_metadata;\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "c.o")], check=True)


def _box(i):
    """numpy shape of argument i's fixed box"""
    if i == 0:
        return (224, 224, 3)
    if i <= 212:
        return (CONVS[(i - 1) % 53][1],)
    if i <= 265:
        ci, co, k = CONVS[i - 213][:3]
        return (ci, k, k, co)
    return {266: (2048, 1000), 267: (1000,), 268: (1000,)}[i]


@functools.lru_cache(maxsize=None)
def _zero_args():
    """269 buffers over untouched zero pages, shared by the protocol tests (which replace single entries)"""
    import halide_amd as hl
    return tuple(hl.Buffer(np.zeros(_box(i), f32)) for i in range(269))


def _call(hl, how, over=None):
    args = list(_zero_args())
    for i, v in (over or {}).items():
        args[i] = v
    return how(hl, "resnet50", *args)


def _ok():
    return 0 if _gpu_present() else -29   # with everything in order only the device can be missing


HOW = pytest.mark.parametrize("how", [call_direct, call_argv], ids=["direct_call", "argv"])
SAMPLE = [0, 1, 5, 60, 130, 212, 213, 214, 240, 265, 266, 267, 268]


@HOW
def test_a_call_in_order_reaches_the_device(hl, how):
    assert _call(hl, how) == _ok()


@HOW
@pytest.mark.parametrize("i", SAMPLE)
def test_a_null_argument_is_refused(hl, how, i):
    name = (["input"] + list(hl.RESNET50_PARAM_NAMES) + ["final_output"])[i]
    assert _call(hl, how, {i: None}) == -12 and name in hl.last_error()


@HOW
@pytest.mark.parametrize("i", SAMPLE)
def test_a_wrong_type_and_a_wrong_dimension_count_are_refused(hl, how, i):
    assert _call(hl, how, {i: hl.Buffer(np.zeros(_box(i), np.float64))}) == -3
    assert _call(hl, how, {i: hl.Buffer(np.zeros(_box(i), np.int32))}) == -3
    assert _call(hl, how, {i: hl.Buffer(np.zeros((1,) + _box(i), f32))}) == -43
    assert _call(hl, how, {7: None, i: hl.Buffer(np.zeros(_box(i), np.uint16))}) == -12   # null before type
    assert _call(hl, how, {i: hl.Buffer(np.zeros((1,) + _box(i), np.uint16))}) == -3    # type before dimension count


@HOW
@pytest.mark.parametrize("i", SAMPLE[:-1])
def test_an_input_one_short_of_its_box_is_refused_and_a_larger_one_is_not(hl, how, i):
    name = (["input"] + list(hl.RESNET50_PARAM_NAMES))[i]
    box = _box(i)
    for axis in range(len(box)):
        if box[axis] == 1:
            continue   # (one short of a 1 x 1 kernel is an empty buffer, which has no layout to speak of)
        short = tuple(e - (a == axis) for a, e in enumerate(box))
        assert _call(hl, how, {i: hl.Buffer(np.zeros(short, f32))}) == -4 and name in hl.last_error(), (i, axis)
    shifted = hl.Buffer(np.zeros(box, f32), mins=[1] + [0] * (len(box) - 1))   # [1, n + 1) does not cover 0
    assert _call(hl, how, {i: shifted}) == -4
    larger = tuple(e + 1 for e in box)
    assert _call(hl, how, {i: hl.Buffer(np.zeros(larger, f32), mins=[-1] * len(box))}) == _ok()
    padded = np.zeros(box[:-2] + (box[-2] + 1, box[-1] + 3) if len(box) > 1 else (box[0],), f32)
    view = padded[..., :box[-2], :box[-1]] if len(box) > 1 else padded
    assert _call(hl, how, {i: hl.Buffer(view)}) == _ok()


@HOW
def test_an_output_box_inside_the_classes_is_taken_and_one_outside_is_refused(hl, how):
    assert _call(hl, how, {268: hl.Buffer(np.zeros(10, f32), mins=[10])}) == _ok()
    assert _call(hl, how, {268: hl.Buffer(np.zeros(1, f32), mins=[999])}) == _ok()
    for mins, n in (([991], 10), ([-1], 5), ([0], 1001), ([1000], 1)):
        assert _call(hl, how, {268: hl.Buffer(np.zeros(n, f32), mins=mins)}) == -4 and "fc1000_bias" in hl.last_error(), (mins, n)
    b = hl.Buffer(np.zeros((1000, 2), f32)[:, 0])
    assert b.dim(0).stride == 2
    assert _call(hl, how, {268: b}) == -8 and "final_output.stride.0" in hl.last_error()


@HOW
def test_a_bounds_query_answers_every_fixed_box(hl, how):
    dims = lambda b: [(b.raw.dim[d].min, b.raw.dim[d].extent) for d in range(b.raw.dimensions)]
    nd = lambda i: len(_box(i))
    q = [hl.Buffer.bounds_query(f32, nd(i)) for i in range(269)]
    assert how(hl, "resnet50", *q) == 0
    for i in range(269):
        assert dims(q[i]) == [(0, e) for e in reversed(_box(i))], i
        assert q[i].raw.dim[0].stride == 1
    # one query buffer among real ones; a real buffer stays as it is; a query of the wrong type is rewritten, of the wrong rank refused
    for i in SAMPLE[:-1]:
        qi, small = hl.Buffer.bounds_query(np.uint16, nd(i)), hl.Buffer(np.zeros(3, f32))
        assert _call(hl, how, {i: qi, 267 if i != 267 else 1: small}) == 0
        assert dims(qi) == [(0, e) for e in reversed(_box(i))] and (qi.raw.type.code, qi.raw.type.bits) == (2, 32) and dims(small) == [(0, 3)]
        assert _call(hl, how, {i: hl.Buffer.bounds_query(f32, nd(i) + 1)}) == -43
    # an output with a shape keeps it
    qo = hl.Buffer.bounds_query(f32, 1, mins=[10], extents=[10])
    assert _call(hl, how, {268: qo}) == 0 and dims(qo) == [(10, 10)]


def test_without_a_gpu_the_python_calls_refuse_to_run(hl):
    if _gpu_present():
        return   # the statement is about a machine without one
    args = _zero_args()
    for fn in (lambda: hl.resnet50(args[0], args[1:-1], args[-1]), lambda: hl.debug_resnet50_general(args[0], args[1:-1], args[-1]),
               lambda: hl.resnet50(args[0], dict(zip(hl.RESNET50_PARAM_NAMES, args[1:-1])), args[-1])):
        with pytest.raises(hl.HalideError) as e:
            fn()
        assert e.value.code == -29
    x, wt, vec, res = _layer_case(3, 8, 5, 7, 3, 1)
    o = hl.Buffer(np.zeros((7, 5, 8), f32))
    with pytest.raises(hl.HalideError) as e:
        hl.debug_resnet50_layer(hl.Buffer(x.copy()), hl.Buffer(wt.copy()), *[hl.Buffer(v.copy()) for v in vec], None, 1, 1, "scaled", o)
    assert e.value.code == -29


def test_the_python_call_counts_and_names_its_parameters(hl):
    args = _zero_args()
    with pytest.raises(ValueError):
        hl.resnet50(args[0], args[1:-2], args[-1])
    named = dict(zip(hl.RESNET50_PARAM_NAMES, args[1:-1]))
    named.pop("br2b_mu_7")
    with pytest.raises(ValueError, match="br2b_mu_7"):
        hl.resnet50(args[0], named, args[-1])
    assert len(hl.RESNET50_PARAM_NAMES) == 267 == len(set(hl.RESNET50_PARAM_NAMES))


def test_the_layer_hook_refuses_what_does_not_fit(hl):
    x, wt, vec, res = _layer_case(3, 8, 5, 7, 3, 1)
    B = lambda a: hl.Buffer(np.array(a))
    fn = hl.lib.hlmi_debug_resnet50_layer
    fn.restype, fn.argtypes = C.c_int, [hl._BP] * 7 + [C.c_int32] * 4 + [hl._BP]
    good = dict(input=B(x), weights=B(wt), gamma=B(vec[0]), beta=B(vec[1]), mu=B(vec[2]), sig=B(vec[3]), residual=None, output=B(np.zeros((7, 5, 8), f32)))

    def run(stride=1, pad=1, mode=1, **over):
        a = dict(good, **over)
        return fn(*[None if a[k] is None else a[k].ptr for k in ("input", "weights", "gamma", "beta", "mu", "sig", "residual")], stride, pad, mode, 0, a["output"].ptr)

    assert run() == _ok()
    assert run(gamma=None) == -12 and run(output=B(np.zeros((7, 5, 9), f32))) == -8 and run(mu=B(np.zeros(7, f32))) == -8
    assert run(weights=B(np.zeros((4, 3, 3, 8), f32))) == -8 and "weights.extent.3" in hl.last_error()
    assert run(mode=4) == -8 and run(stride=0) == -8 and run(pad=-1) == -8
    assert run(mode=3) == -12 and run(mode=3, residual=B(res)) == _ok() and run(mode=3, residual=B(res[:, :, :7])) == -8
    assert run(input=B(x.astype(np.float64))) == -3


# ---- the loaders
def test_the_state_dict_mapping_is_total_and_one_to_one(hl):
    keys = hl.RESNET50_STATE_DICT_KEYS
    assert sorted(keys) == sorted(hl.RESNET50_PARAM_NAMES) and len(set(keys.values())) == 267
    sd = _state_dict(5)
    assert set(keys.values()) == {k for k in sd if not k.endswith("num_batches_tracked")}
    # process.cpp:143-239, by hand (its file names with dots for underscores)
    for arg, key in (("conv1_weights", "conv1.weight"), ("conv1_mu", "bn1.running_mean"), ("conv1_sig", "bn1.running_var"), ("conv1_gamma", "bn1.weight"),
                     ("conv1_beta", "bn1.bias"), ("br1_conv_weights_0", "layer1.0.downsample.0.weight"), ("br1_mu_1", "layer2.0.downsample.1.running_mean"),
                     ("br1_gamma_3", "layer4.0.downsample.1.weight"), ("br2a_conv_weights_0", "layer1.0.conv1.weight"), ("br2b_conv_weights_3", "layer2.0.conv2.weight"),
                     ("br2c_sig_6", "layer2.3.bn3.running_var"), ("br2a_beta_7", "layer3.0.bn1.bias"), ("br2b_mu_12", "layer3.5.bn2.running_mean"),
                     ("br2c_conv_weights_13", "layer4.0.conv3.weight"), ("br2c_gamma_15", "layer4.2.bn3.weight"), ("fc1000_weights", "fc.weight"), ("fc1000_bias", "fc.bias")):
        assert keys[arg] == key, arg


def test_params_from_a_state_dict_are_transposed_to_the_halide_layout(hl):
    import torch
    sd = _state_dict(6)
    p = hl.resnet50_params_from_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    assert list(p) == list(hl.RESNET50_PARAM_NAMES)
    for i, name in enumerate(hl.RESNET50_PARAM_NAMES):
        assert p[name].shape == _box(i + 1) and p[name].dtype == f32 and p[name].flags.c_contiguous, name
    w = sd["layer2.0.conv2.weight"]   # torch (co, ci, h, w) -> array (ci, h, w, co)
    assert p["br2b_conv_weights_3"][5, 2, 1, 7] == w[7, 5, 2, 1]
    assert p["fc1000_weights"][11, 3] == sd["fc.weight"][3, 11]
    assert np.array_equal(p["br2c_sig_6"], sd["layer2.3.bn3.running_var"])


def test_the_weight_directory_loader_reads_the_references_files(hl, tmp_path, monkeypatch):
    """a handful of small files in load_weights.py's format: `<key>.data` is the transposed array's bytes, `<key>_shape.data` an int32
    count and the REVERSED numpy shape (the Halide extents, innermost first).  The full 102 MB set is not written: the loader is pointed
    at five arguments."""
    names = ("conv1_gamma", "br1_conv_weights_2", "br2b_conv_weights_4", "fc1000_weights", "fc1000_bias")
    monkeypatch.setattr(hl, "RESNET50_PARAM_NAMES", names)
    rng = np.random.default_rng(7)
    torch_shapes = {"conv1_gamma": (64,), "br1_conv_weights_2": (16, 8, 1, 1), "br2b_conv_weights_4": (6, 5, 3, 3), "fc1000_weights": (10, 7), "fc1000_bias": (10,)}
    written = {}
    for n in names:
        t = rng.standard_normal(torch_shapes[n]).astype(f32)
        a = t.transpose(1, 2, 3, 0) if t.ndim == 4 else t.transpose(1, 0) if t.ndim == 2 else t
        base = tmp_path / hl.RESNET50_STATE_DICT_KEYS[n].replace(".", "_")
        (base.parent / (base.name + ".data")).write_bytes(np.ascontiguousarray(a).tobytes())
        (base.parent / (base.name + "_shape.data")).write_bytes(struct.pack("i", a.ndim) + b"".join(struct.pack("i", a.shape[i]) for i in reversed(range(a.ndim))))
        written[n] = (t, a)
    got = hl.resnet50_load_weight_dir(str(tmp_path))
    assert list(got) == list(names)
    for n in names:
        t, a = written[n]
        assert got[n].shape == a.shape and np.array_equal(got[n], a), n
    assert got["br2b_conv_weights_4"][4, 2, 1, 5] == written["br2b_conv_weights_4"][0][5, 4, 2, 1]
    assert (tmp_path / "layer3_0_downsample_0_weight.data").exists() and (tmp_path / "layer2_1_conv2_weight_shape.data").exists()
    (tmp_path / "fc_bias.data").write_bytes(b"\0" * 36)
    with pytest.raises(ValueError):
        hl.resnet50_load_weight_dir(str(tmp_path))


def test_torch_shape_function_and_refusals(hl):
    import torch
    import halide_amd.torch_ops  # noqa: F401
    op = torch.ops.hlmi.resnet50
    meta = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device="meta")
    params = [meta(_box(i + 1)) for i in range(267)]
    out = op(meta((224, 224, 3)), params)
    assert out.shape == (1000,) and out.dtype == torch.float32
    cpu = [torch.zeros(_box(i + 1)) for i in range(267)]
    with pytest.raises(RuntimeError, match="GPU"):
        op(torch.zeros((224, 224, 3)), cpu)
    with pytest.raises(TypeError):
        op(torch.zeros((224, 224, 3), dtype=torch.float64), cpu)
    with pytest.raises(TypeError):
        op(torch.zeros((224, 224, 3)), cpu[:5] + [cpu[5].double()] + cpu[6:])
    with pytest.raises(TypeError):
        op(torch.zeros((224, 224, 3)), cpu[:-1])
    with pytest.raises(TypeError):
        op(torch.zeros((3, 224, 224)), cpu)


# ---------------------------------------------------------------------------------------------------- GPU: the layer hook
def _layer_gpu(hl, shape, mode, general, kind="noise", layout=0, sentinels=True):
    """one call of the layer hook; layout 0: dense host buffers; 1 .. 3: input, residual and output in device allocations of the test's own
    with padded rows and planes and a first element `layout` floats off the 16-byte grid.  Asserts the launch name; returns the output."""
    ci, co, w, h, k, stride = shape
    pad = PAD_OF[k]
    x, wt, vec, res = _layer_case(*shape, kind=kind)
    oh, ow = res.shape[:2]
    if layout:
        mk = lambda a, fill, d: DevArray(hl, a.shape, f32, row_stride=a.shape[2] + d, plane_stride=(a.shape[2] + d) * a.shape[1] + 2 * d + 1, offset=4 * layout, fill=fill)
        xi, ri, oo = mk(x, x, layout), mk(res, res, layout + 1), mk(res, None, 4 - layout)
    else:
        mk = lambda a, fill: HostArray(hl, a.shape, f32, fill=fill)
        xi, ri, oo = mk(x, x), mk(res, res), mk(res, None)
    try:
        bufs = [hl.Buffer(wt.copy())] + [hl.Buffer(v.copy()) for v in vec]
        ran = _launches(hl, lambda: hl.debug_resnet50_layer(xi.buf, *bufs, ri.buf if mode == "residual_relu" else None, stride, pad, mode, oo.buf, general_only=general))
        assert ran == [_expected_launch(hl, co, k * k * ci, general)], (ran, shape)
        got = oo.result()   # (and every byte around the output is as it was)
        if layout:
            xi.result(), ri.result()
        return got
    finally:
        xi.free(), ri.free(), oo.free()


PATHS = pytest.mark.parametrize("general", [False, True], ids=["default", "general"])
MODES = pytest.mark.parametrize("mode", rn.MODES)


@pytest.mark.gpu
@PATHS
@MODES
@pytest.mark.parametrize("shape", LAYER_SHAPES + BIG_SHAPES)
def test_the_layer_hook_equals_the_checker(hl, shape, mode, general):
    layout = (LAYER_SHAPES + BIG_SHAPES).index(shape) % 4
    want = _layer_want(hl.canon_fma(), *shape, mode)
    _same(_layer_gpu(hl, shape, mode, general, layout=layout), want, f"{shape} {mode} general {general} layout {layout}")


def test_the_shapes_reach_every_variant_of_the_plan(hl):
    """restated predicate only (no GPU): the small shapes run the one-wave tile, the big ones the four-wave tile; K odd, K below, at and off
    the chunk are all there"""
    if not hl.canon_fma():
        return
    npix = lambda s: rn.out_extent(s[2], s[4], s[5], PAD_OF[s[4]]) * rn.out_extent(s[3], s[4], s[5], PAD_OF[s[4]])
    K = lambda s: s[0] * s[4] ** 2
    assert {_expected_launch(hl, s[1], K(s), False) for s in LAYER_SHAPES} == {MFMA, GENERAL}
    on_mfma = [s for s in LAYER_SHAPES + BIG_SHAPES if _expected_launch(hl, s[1], K(s), False) == MFMA]
    assert set(BIG_SHAPES) <= set(on_mfma)
    Ks = [K(s) for s in on_mfma]
    assert any(k % 2 for k in Ks) and any(k % KC == 0 for k in Ks) and any(k > KC and k % KC for k in Ks) and any(k < KC for k in Ks) and 147 in Ks
    assert {s[0] for s in on_mfma} >= {1, 3, 5, 64} and {s[1] for s in on_mfma} >= {1, 8, 63, 64, 65, 130}
    assert any(npix(s) > 4 * TILE for s in on_mfma) and any(npix(s) == 1 for s in on_mfma) and TILE == 64
    # either side of the predicate's two thresholds
    assert _expected_launch(hl, TILE, SHORT_K, False) == GENERAL and _expected_launch(hl, TILE + 1, SHORT_K, False) == MFMA
    assert _expected_launch(hl, TILE, SHORT_K + 1, False) == MFMA


@pytest.mark.gpu
@PATHS
@pytest.mark.parametrize("layout", [1, 2, 3])
def test_buffers_off_the_16_byte_grid_with_padded_strides(hl, on_stream, general, layout):
    for shape in ((5, 63, 9, 8, 3, 2), (3, 130, 40, 36, 3, 1)):
        want = _layer_want(hl.canon_fma(), *shape, "residual_relu")
        _same(_layer_gpu(hl, shape, "residual_relu", general, layout=layout), want, f"{shape} layout {layout}")


@pytest.mark.gpu
@PATHS
@pytest.mark.parametrize("shape", ORDER_SHAPES + [(64, 130, 40, 36, 1, 1)])
def test_the_order_sensitive_input(hl, general, shape):
    _same(_layer_gpu(hl, shape, "raw", general, kind="order"), _layer_want(hl.canon_fma(), *shape, "raw", "order"), f"order-sensitive {shape}")


@pytest.mark.gpu
@PATHS
@pytest.mark.parametrize("trap", TRAPS)
def test_minus_zero_at_an_odd_k(hl, general, trap):
    ci, co, w, h, k, co0, i0, j0 = trap
    x, wt = _minus_zero_trap(*trap)
    pad = PAD_OF[k]
    o = hl.Buffer(np.full((rn.out_extent(h, k, 1, pad), rn.out_extent(w, k, 1, pad), co), 7, f32))
    z = [hl.Buffer(np.ones(co, f32)) for _ in range(4)]
    hl.debug_resnet50_layer(hl.Buffer(x), hl.Buffer(wt), *z, None, 1, pad, "raw", o, general_only=general)
    got = o.numpy()
    assert got.view(u32)[j0, i0, co0] == (0x80000000 if hl.canon_fma() else 0), hex(got.view(u32)[j0, i0, co0])
    _same(got, rn.conv(x, wt, stride=1, pad=pad), f"-0 {trap}")


@pytest.mark.gpu
@PATHS
@pytest.mark.parametrize("mode", ["raw", "scaled"])
@pytest.mark.parametrize("shape", SPECIAL_SHAPES)
def test_special_values(hl, general, shape, mode):
    want = _layer_want(hl.canon_fma(), *shape, mode, "special")
    _same_or_nan(_layer_gpu(hl, shape, mode, general, kind="special"), want, f"special values {shape} {mode}")


@pytest.mark.gpu
def test_subnormal_chains_stay_subnormal(hl):
    shape = (5, 65, 9, 8, 3, 2)
    x, wt, _, _ = _layer_case(*shape)
    x, wt = (x * f32(2.0 ** -75)).astype(f32), (wt * f32(2.0 ** -70)).astype(f32)
    want = rn.conv(x, wt, stride=2, pad=1)
    assert (np.abs(want) < np.finfo(f32).tiny).all() and np.count_nonzero(want) > 0.9 * want.size
    for general in (False, True):
        o = hl.Buffer(np.zeros(want.shape, f32))
        z = [hl.Buffer(np.ones(65, f32)) for _ in range(4)]
        hl.debug_resnet50_layer(hl.Buffer(x), hl.Buffer(wt), *z, None, 2, 1, "raw", o, general_only=general)
        _same(o.numpy(), want, f"subnormal general {general}")


# ---------------------------------------------------------------------------------------------------- GPU: the pool and tail hooks
@pytest.mark.gpu
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_the_max_pool_hook(hl, shape):
    c, w, h, k, stride, pad = shape
    for lo, layout in ((0.0, 0), (-3.0, 2)):
        x = (_noise((h, w, c), 5) + f32(lo)).astype(f32)
        want = rn.maxpool(x, k, stride, pad)
        xi = DevArray(hl, x.shape, f32, row_stride=c + layout, offset=4 * layout, fill=x)
        oo = DevArray(hl, want.shape, f32, row_stride=c + 3 - layout, offset=4 * (3 - layout))
        try:
            assert _launches(hl, lambda: hl.debug_resnet50_maxpool(xi.buf, k, stride, pad, oo.buf)) == ["resnet50_maxpool"]
            _same(oo.result(), want, f"max pool {shape} {lo}")
        finally:
            xi.free(), oo.free()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", TAIL_SHAPES + [(2048, 7, 7, 1000)])
def test_the_tail_hook(hl, shape):
    c, w, h, n = shape
    x, fw, fb = _tail_case(shape)
    want = rn.tail(x, fw, fb)["out"]
    assert np.isfinite(want).all()
    o = hl.Buffer(np.zeros(n, f32))
    ran = _launches(hl, lambda: hl.debug_resnet50_tail(hl.Buffer(x), hl.Buffer(fw), hl.Buffer(fb), o))
    assert ran == ["resnet50_avgpool", "resnet50_fc", "resnet50_softmax"]
    _same(o.numpy(), want, f"tail {shape}")


@pytest.mark.gpu
def test_the_tail_hook_with_logits_past_exps_range(hl):
    x, fw, fb = _tail_case((64, 7, 7, 10))
    fb = fb.copy()
    fb[[2, 7]], fb[4] = 200.0, -200.0
    want = rn.tail(x, fw, fb)
    assert np.isnan(want["out"][[2, 7]]).all() and want["e"][4] == 0 and np.count_nonzero(np.isnan(want["out"])) == 2
    o = hl.Buffer(np.full(10, 5, f32))
    hl.debug_resnet50_tail(hl.Buffer(x), hl.Buffer(fw), hl.Buffer(fb), o)
    _same_or_nan(o.numpy(), want["out"], "overflowing logits")


# ---------------------------------------------------------------------------------------------------- GPU: the whole network
def _launch_counts(hl, fn):
    """{kernel name: launches} of one call (parity_helpers.launches names each kernel once)"""
    hl.kernel_timing(True)
    hl.kernel_timing_reset()
    try:
        fn()
        return {e["name"]: e["calls"] for e in hl.kernel_timing_report()}
    finally:
        hl.kernel_timing(False)
        hl.kernel_timing_reset()


def _buffers(hl, image, params):
    return hl.Buffer(image.copy()), [hl.Buffer(p.copy()) for p in params]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_the_whole_network_on_every_path(hl, seed):
    sd, image, params, want = _net_case(seed)
    inp, par = _buffers(hl, image, params)
    # default path, host buffers; the launch list: 53 convolutions, two pools, fc, softmax
    o = hl.Buffer(np.zeros(1000, f32))
    ran = _launch_counts(hl, lambda: hl.resnet50(inp, par, o))
    others = {"resnet50_maxpool": 1, "resnet50_avgpool": 1, "resnet50_fc": 1, "resnet50_softmax": 1}
    convs = {n: c for n, c in ran.items() if n not in others}
    assert {n: c for n, c in ran.items() if n in others} == others and sum(convs.values()) == 53
    # conv_plan() restated over the 53 layers
    expect = {}
    for ci, co, k, stride, pad, size in CONVS:
        name = _expected_launch(hl, co, k * k * ci, False)
        expect[name] = expect.get(name, 0) + 1
    assert convs == expect, (convs, expect)
    _same(o.numpy(), want["out"], "default path")
    # the same buffers are now device-resident: again, by name, and into a box [10, 20)
    o = hl.Buffer(np.zeros(1000, f32))
    hl.resnet50(inp, dict(zip(hl.RESNET50_PARAM_NAMES, par)), o)
    _same(o.numpy(), want["out"], "device-resident buffers, parameters by name")
    box = hl.Buffer(np.full(10, 9, f32), mins=[10])
    hl.resnet50(inp, par, box)
    _same(box.numpy(), want["out"][10:20], "output box [10, 20)")
    # general path
    o = hl.Buffer(np.zeros(1000, f32))
    ran = _launch_counts(hl, lambda: hl.debug_resnet50_general(inp, par, o))
    assert ran == dict(others, **{GENERAL: 53})
    _same(o.numpy(), want["out"], "general path")
    # through _argv
    o = hl.Buffer(np.zeros(1000, f32))
    assert call_argv(hl, "resnet50", inp, *par, o) == 0
    _same(o.numpy(), want["out"], "resnet50_argv")


@pytest.mark.gpu
def test_torch_op_equals_the_python_call_and_refuses_float64(hl):
    import torch
    import halide_amd.torch_ops  # noqa: F401
    sd, image, params, want = _net_case(SEEDS[0])
    ti = torch.from_numpy(image.copy()).cuda()
    tp = [torch.from_numpy(p.copy()).cuda() for p in params]
    out = torch.ops.hlmi.resnet50(ti, tp)
    torch.cuda.synchronize()
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (1000,)
    _same(out.cpu().numpy(), want["out"], "torch op against the checker")
    inp, par = _buffers(hl, image, params)
    o = hl.Buffer(np.zeros(1000, f32))
    hl.resnet50(inp, par, o)
    _same(out.cpu().numpy(), o.numpy(), "torch op against hl.resnet50")
    assert np.array_equal(ti.cpu().numpy(), image)
    with pytest.raises(TypeError):
        torch.ops.hlmi.resnet50(ti.double(), tp)
    with pytest.raises(TypeError):
        torch.ops.hlmi.resnet50(ti, tp[:3] + [tp[3].double()] + tp[4:])


@pytest.mark.gpu
def test_two_calls_from_two_host_threads_give_the_bits_of_one(hl):
    sd, image, params, want = _net_case(SEEDS[0])
    image2 = np.random.default_rng(77).random((224, 224, 3), dtype=f32)
    want2 = rn.network(image2, params)["out"]
    inp, par = _buffers(hl, image, params)
    inp2 = hl.Buffer(image2.copy())
    outs = [hl.Buffer(np.zeros(1000, f32)) for _ in range(4)]
    errors = []

    def work(which):
        try:
            for o in outs[which::2]:
                hl.resnet50(inp if which == 0 else inp2, par, o)
        except Exception as e:   # noqa: BLE001
            errors.append(e)

    hl.resnet50(inp, par, hl.Buffer(np.zeros(1000, f32)))   # the parameters are on the device before the threads start
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i, o in enumerate(outs):
        _same(o.numpy(), want["out"] if i % 2 == 0 else want2, f"thread {i % 2} call {i // 2}")
