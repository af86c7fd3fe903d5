"""The float pipelines whose own tests feed them smooth values in roughly [0, 1] (unsharp, harris, nl_means, max_filter, iir_blur,
interpolate, bilateral_grid) on noise with single elements replaced by the values where a device expression and its C restatement
part ways: both zeros, denormals, FLT_MIN, values whose squares and sums overflow, the infinities, NaN.  Bit patterns are compared.
Where the oracle has a NaN the library must have a NaN and nothing else is compared there: sign and payload of a NaN that an
operation produces belong to the processor (test_wavelet.py words it the same way).

Which values a pipeline gets is decided by what its reference defines, not by what passes; each exclusion is stated at its table
row.  A CPU test holds the images themselves to two conditions on the oracle alone, in both canonical forms: at most a quarter of
the output is NaN (so that the comparison still compares), and the special elements reach outputs that differ from the all-noise
result (so that they are not simply clamped away)."""
import functools
from typing import Callable, NamedTuple

import numpy as np
import pytest

import parity_helpers as ph

f32 = np.float32
W, H = 64, 48
_bits = lambda *b: np.array(b, np.uint32).view(f32)
# 0, -0, a denormal and its negative, FLT_MIN, then numbers
COMMON = np.concatenate([_bits(0x00000000, 0x80000000, 0x00012345, 0x80012345, 0x00800000), np.array([1e-30, -0.25, 4, 3e18, -3e18, 1e37], f32)])
INF, NAN = np.array([np.inf, -np.inf], f32), np.array([np.nan], f32)
MAX_NAN_SHARE = 0.25


class Special(NamedTuple):
    shape: tuple
    twice: np.ndarray     # values that replace two elements each
    once: np.ndarray      # values that replace one element each
    planes: Callable      # value -> the planes it may go to
    run: Callable         # (hl, input Buffer, output Buffer)
    want: Callable        # (oracle, input) -> output
    out_shape: tuple
    out_mins: tuple = None


_any3, _none = (lambda v: (0, 1, 2)), np.array([], f32)
SPECIALS = {
    "unsharp": Special((3, H, W), np.concatenate([COMMON, INF, NAN]), _none, _any3,
                       lambda hl, a, o: hl.unsharp(a, o), lambda oracle, d: oracle.unsharp(d), (3, H, W)),
    "harris": Special((3, H, W), np.concatenate([COMMON, INF, NAN]), _none, _any3,
                      lambda hl, a, o: hl.harris(a, o), lambda oracle, d: oracle.harris(d), (H - 6, W - 6), (3, 3)),
    "nl_means": Special((3, H, W), np.concatenate([COMMON, INF, NAN]), _none, _any3,
                        lambda hl, a, o: hl.nl_means(a, 7, 7, 0.12, o), lambda oracle, d: oracle.nl_means(d, 7, 7, 0.12), (3, H, W)),
    # no NaN and never both zeros in one image (the noise holds no zero, +0 is left out); exactly one of each infinity: see
    # test_hip_special_values's docstring
    "max_filter": Special((3, H, W), COMMON[1:], INF, _any3,
                          lambda hl, a, o: hl.max_filter(a, o), lambda oracle, d: oracle.max_filter(d), (3, H, W)),
    # finite values only: the filter is recursive over whole rows and columns, one inf or NaN would fill the image
    "iir_blur_0.3": Special((3, H, W), COMMON, _none, _any3,
                            lambda hl, a, o: hl.iir_blur(a, 0.3, o), lambda oracle, d: oracle.iir_blur(d, 0.3), (3, H, W)),
    "iir_blur_1.0": Special((3, H, W), COMMON, _none, _any3,
                            lambda hl, a, o: hl.iir_blur(a, 1.0, o), lambda oracle, d: oracle.iir_blur(d, 1.0), (3, H, W)),
    # finite values only, and magnitudes above 4 in the colour planes only: in alpha they reach every level of the pyramid and the
    # oracle's whole output is NaN
    "interpolate": Special((4, H, W), COMMON, _none, lambda v: (0, 1, 2) if abs(v) > 4 else (0, 1, 2, 3),
                           lambda hl, a, o: hl.interpolate(a, o), lambda oracle, d: oracle.interpolate(d), (3, H, W)),
    # no NaN: its bin index is an undefined float-to-int conversion (test_device_math.py records the same limit)
    "bilateral_grid": Special((H, W), np.concatenate([COMMON, INF]), _none, lambda v: (),
                              lambda hl, a, o: hl.bilateral_grid(a, 0.1, o), lambda oracle, d: oracle.bilateral_grid(d, 0.1), (H, W)),
}


def test_table_names_the_pipelines_in_scope():
    assert {n.rsplit("_", 1)[0] if n.startswith("iir_blur_") else n for n in SPECIALS} == {"unsharp", "harris", "nl_means", "max_filter", "iir_blur", "interpolate", "bilateral_grid"}


@functools.lru_cache(maxsize=None)
def _images(name):
    """(the all-noise image, the same with the special values in, the indices of the replaced elements)"""
    s = SPECIALS[name]
    rng = np.random.default_rng(len(name) + 40)
    base = ph.noise(s.shape, seed=len(name) + 41)
    img, taken = base.copy(), set()
    for v in list(s.twice) * 2 + list(s.once):
        while True:
            at = tuple(int(rng.integers(0, n)) for n in s.shape[-2:])
            if len(s.shape) == 3:
                at = (int(rng.choice(s.planes(v))),) + at
            if at not in taken:
                break
        taken.add(at)
        img[at] = v
    assert 20 <= len(taken) <= 30 and (base != 0).all()
    base.setflags(write=False), img.setflags(write=False)
    return base, img, sorted(taken)


@functools.lru_cache(maxsize=None)
def _want(name, canon, special=True):
    import oracle_lib
    assert oracle_lib.get_canon() == canon
    w = SPECIALS[name].want(oracle_lib, _images(name)[1 if special else 0])
    w.setflags(write=False)
    return w


@pytest.mark.parametrize("name", SPECIALS)
def test_images_hold_what_their_row_says(name):
    s = SPECIALS[name]
    base, img, at = _images(name)
    put = np.array([img[a] for a in at], f32)
    assert sorted(put.view(np.uint32).tolist()) == sorted(np.concatenate([s.twice, s.twice, s.once]).view(np.uint32).tolist())
    changed = np.argwhere(img.view(np.uint32) != base.view(np.uint32))
    assert sorted(map(tuple, changed.tolist())) == at
    if name == "max_filter":
        assert not np.isnan(img).any() and np.count_nonzero(img == np.inf) == 1 and np.count_nonzero(img == -np.inf) == 1
        assert not (img.view(np.uint32) == 0).any()   # -0 is there, +0 is not
    if name.startswith("iir_blur") or name == "interpolate":
        assert np.isfinite(img).all()
    if name == "interpolate":
        assert (np.abs(img[3]) <= 4).all() and (np.abs(img[:3]) > 4).any()
    if name == "bilateral_grid":
        assert not np.isnan(img).any() and np.isinf(img).sum() == 4


@pytest.mark.parametrize("name", SPECIALS)
def test_oracle_output_is_mostly_numbers_and_the_special_values_reach_it(each_canon, name):
    want, plain = _want(name, each_canon), _want(name, each_canon, special=False)
    assert want.shape == SPECIALS[name].out_shape and np.isfinite(plain).all()
    nan = np.isnan(want)
    print(f"{name} canon {each_canon}: NaN {nan.mean():.1%}, inf {np.isinf(want).mean():.1%}, "
          f"other differences from noise {np.mean((want.view(np.uint32) != plain.view(np.uint32)) & ~nan):.1%}")
    assert nan.mean() <= MAX_NAN_SHARE
    assert ((want.view(np.uint32) != plain.view(np.uint32)) & ~nan).any(), "no special element survives to a comparable output"


@pytest.mark.gpu
@pytest.mark.parametrize("name", SPECIALS)
def test_hip_special_values(hl, oracle, name):
    """Bit for bit against the oracle, NaN for NaN.

    max_filter gets no NaN, at most one kind of zero per image and one of each infinity.  The reference's max is
    `a > b ? a : b`, whose result depends on the order of evaluation when an operand is a NaN (the comparison is false either way
    round) and when -0 meets +0 (they compare equal, so whichever stands second wins).  The generator's closed form (a table of
    maxima over power-of-two runs, two of them per column) evaluates in another order than the plain loop over the disc; both are
    the reference, and only inputs on which the order cannot show are specified."""
    s = SPECIALS[name]
    _, img, _ = _images(name)
    a, o = hl.Buffer(img.copy()), hl.Buffer(np.zeros(s.out_shape, f32), mins=s.out_mins)
    s.run(hl, a, o)
    ph.same_bits_or_nan(o.numpy(), _want(name, oracle.get_canon()), name)
