"""resize: box / linear / cubic / lanczos resampling for f32, u8 and u16, 24 AOT variants (apps/resize).

The checker is tests/cpp/resize_check.c, a plain C restatement of apps/resize/resize_generator.cpp:12-46, :85-147 in both
canonical float forms, built and driven through ctypes by tests/checker_lib.py.  The CPU tests hold the
checker to an independent numpy float64 evaluation and to properties that follow from the generator's text; the GPU tests
hold the library to the checker bit for bit.  Like every float pipeline here, resize is pinned to this repository's
restatement only: no output of a real Halide build is involved."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import checker_lib
from checker_lib import RESIZE_KERNELS as KERNELS, RESIZE_TAPS as TAPS, resize_out_size as out_size
from parity_helpers import ROOT, RUNGEN, call_argv, launches, load_fuzz_parity, same_bits as _same

TYPES = {"float32": np.float32, "uint8": np.uint8, "uint16": np.uint16}
DOWN_FACTORS = (0.125, 0.23, 0.37, 0.5, 0.9, 1.0)
UP_FACTORS = (0.6, 1.0, 1.7, 2.0, 3.3, 4.0)
VARIANTS = [f"resize_{k}_{t}_{d}" for k in KERNELS for t in TYPES for d in ("up", "down")]


# ---------------------------------------------------------------------------------------------------- the checker
@pytest.fixture(scope="session")
def rc():
    return checker_lib.resize


@pytest.fixture(params=[0, 1], ids=["canon0", "canon1"])
def each_canon_rc(request):
    with checker_lib.canon(request.param):
        yield request.param


@pytest.fixture
def canon0_rc():
    """for the tests whose tolerance was measured in canonical form 0"""
    with checker_lib.canon(0):
        yield


@pytest.fixture
def canon_rc(hl, rc):
    """the checker in the form the loaded library was built for"""
    with checker_lib.canon(hl.canon_fma()):
        yield rc


def image(tname, shape, seed):
    rng = np.random.default_rng(seed)
    if tname == "float32":
        return rng.random(shape, dtype=np.float32)
    return rng.integers(0, np.iinfo(TYPES[tname]).max + 1, shape, dtype=np.int64).astype(TYPES[tname])


# ---------------------------------------------------------------------------------------------------- float64 evaluation
def _kernel64(kernel, x):
    ax = np.abs(x)
    if kernel == "box":
        return np.where(ax <= 0.5, 1.0, 0.0)
    if kernel == "linear":
        return np.where(ax < 1.0, 1.0 - ax, 0.0)
    if kernel == "cubic":
        a = -0.5
        inner = (a + 2.0) * ax ** 3 - (a + 3.0) * ax ** 2 + 1
        outer = a * ax ** 3 - 5 * a * ax ** 2 + 8 * a * ax - 4.0 * a
        return np.where(ax < 1.0, inner, np.where(ax < 2.0, outer, 0.0))
    pi = float(np.float32(3.14159265359))
    with np.errstate(invalid="ignore", divide="ignore"):
        v = (np.sin(x * pi) / (x * pi)) * (np.sin(x / 3 * pi) / (x / 3 * pi))
    v = np.where(x == 0.0, 1.0, v)
    return np.where((x > 3) | (x < -3), 0.0, v)


def _axis64(kernel, up, scale, n, extent):
    """begin (from the f32 computation, op by op: it is a specified quantity, like inv) and float64 normalised weights [k][i]"""
    f = np.float32
    t = TAPS[kernel]
    inv = f(1.0) / f(scale)
    iks = f(1.0) if up else inv
    taps = int(np.ceil(f(t) * iks))
    radius = f(0.5 * t) * iks
    xf = np.arange(n).astype(np.float32) + f(0.5)
    begin = np.ceil((xf * inv - f(0.5)) - radius).astype(np.int64)
    begin = np.maximum(np.minimum(begin, extent - taps), 0)
    source = xf.astype(np.float64) * float(inv) - 0.5
    k = np.arange(taps)[:, None]
    u = _kernel64(kernel, ((k + begin[None, :]) - source[None, :]) * (1.0 if up else float(f(scale))))
    return begin, u / u.sum(0)


def ref64(kernel, img, scale, up):
    c, h, w = img.shape
    ow, oh = out_size(w, h, scale)
    bx, wx = _axis64(kernel, up, scale, ow, w)
    by, wy = _axis64(kernel, up, scale, oh, h)
    a = img.astype(np.float64)

    def along_x(a):
        return sum(wx[k][None, None, :] * a[:, :, bx + k] for k in range(wx.shape[0]))

    def along_y(a):
        return sum(wy[k][None, :, None] * a[:, by + k, :] for k in range(wy.shape[0]))

    r = along_y(along_x(a)) if up else along_x(along_y(a))
    if img.dtype == np.float32:
        return np.clip(r, 0.0, 1.0), (bx, by)
    return np.trunc(np.clip(r, 0, np.iinfo(img.dtype).max)), (bx, by)


# The largest |checker - float64| measured for f32 images in [0, 1) on the cases of the test below (131 x 97 x 3, seed 131 + 97,
# canonical form 0, no code under test involved): linear 6.95e-6, cubic 8.73e-6, lanczos 9.84e-6.  The f32 source coordinate
# (x + 0.5) * inv - 0.5 carries about |source| * 2^-24 = 130 * 6e-8 = 8e-6, which moves every weight by as much; the roundings of
# the sums themselves are an order below.  Other seeds vary, so 4 x the largest value seen is allowed.
F32_VS_FLOAT64 = 4 * 9.84e-6


# ---------------------------------------------------------------------------------------------------- CPU: the library's surface
def test_every_variant_is_exported_with_argv_and_metadata(hl):
    lib = C.CDLL(hl.LIB_PATH)
    assert len(VARIANTS) == 24
    for name in VARIANTS:
        for suffix in ("", "_argv", "_metadata"):
            assert hasattr(lib, name + suffix), name + suffix
        md = hl.metadata(name)
        assert md.version == 1 and md.num_arguments == 3 and md.name.decode() == name and b"hip" in md.target
        a = [md.arguments[i] for i in range(3)]
        assert [x.kind for x in a] == [1, 0, 2] and [x.name.decode() for x in a] == ["input", "scale_factor", "output"]
        assert [x.dimensions for x in a] == [3, 0, 3]
        code, bits = {"float32": (2, 32), "uint8": (1, 8), "uint16": (1, 16)}[name.split("_")[2]]
        assert (a[0].type.code, a[0].type.bits) == (code, bits) == (a[2].type.code, a[2].type.bits)
        assert (a[1].type.code, a[1].type.bits) == (2, 32)
    assert hasattr(lib, "hlmi_resize_general")


def test_every_variant_has_its_aot_header():
    for name in VARIANTS:
        text = open(os.path.join(ROOT, "include", "aot", name + ".h")).read()
        assert "hlmi_pipelines.h" in text
    decl = open(os.path.join(ROOT, "include", "hlmi_pipelines.h")).read()
    for name in VARIANTS:
        assert f"int {name}(struct halide_buffer_t *input, float scale_factor, struct halide_buffer_t *output);" in decl


def test_without_a_gpu_every_variant_refuses_to_run(hl):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    for name in VARIANTS:
        _, kernel, tname, d = name.split("_")
        a, o = hl.Buffer(np.zeros((3, 16, 16), TYPES[tname])), hl.Buffer(np.zeros((3, 8, 8), TYPES[tname]))
        with pytest.raises(hl.HalideError) as e:
            hl.resize(a, 0.5, o, kernel, upsample=(d == "up"))
        assert e.value.code == -29, name


def test_python_picks_the_variant_from_type_name_and_direction(hl):
    a = hl.Buffer(np.zeros((3, 8, 8), np.uint16))
    assert hl.resize_variant(a, 0.5) == "resize_cubic_uint16_down"
    assert hl.resize_variant(a, 1.0, "box") == "resize_box_uint16_down"          # resize.cpp:126: up only above 1
    assert hl.resize_variant(a, 1.5, "lanczos") == "resize_lanczos_uint16_up"
    assert hl.resize_variant(a, 0.6, "linear", upsample=True) == "resize_linear_uint16_up"
    with pytest.raises(ValueError):
        hl.resize_variant(a, 0.5, "nearest")
    with pytest.raises(TypeError):
        hl.resize_variant(hl.Buffer(np.zeros((3, 8, 8), np.int32)), 0.5)


@pytest.mark.parametrize("name", ["resize_lanczos_float32_down", "resize_cubic_uint8_down", "resize_linear_uint16_up"])
def test_entry_protocol_through_argv(hl, name):
    _, kernel, tname, d = name.split("_")
    dt = TYPES[tname]
    other = np.uint16 if tname != "uint16" else np.uint8
    scale = 0.5 if d == "down" else 2.0
    mk = lambda shape, dtype=dt: hl.Buffer(np.zeros(shape, dtype))
    good_in, good_out = (3, 32, 32), ((3, 16, 16) if d == "down" else (3, 64, 64))
    call = lambda i, o, s=scale: call_argv(hl, name, i, s, o)
    assert call(None, mk(good_out)) == -12 and call(mk(good_in), None) == -12
    assert call(mk(good_in, other), mk(good_out)) == -3 and call(mk(good_in), mk(good_out, other)) == -3
    assert call(mk(good_in[1:]), mk(good_out)) == -43 and call(mk(good_in), mk(good_out[1:])) == -43
    # interleaved: x is not the innermost dimension
    packed_in = hl.Buffer(np.zeros(good_in[1:] + (3,), dt).transpose(2, 0, 1))
    packed_out = hl.Buffer(np.zeros(good_out[1:] + (3,), dt).transpose(2, 0, 1))
    assert call(packed_in, mk(good_out)) == -8 and call(mk(good_in), packed_out) == -8
    # the output's channels must lie inside the input's
    assert call(mk((2,) + good_in[1:]), mk(good_out)) == -4
    assert call(mk(good_in), hl.Buffer(np.zeros((1,) + good_out[1:], dt), mins=(0, 0, 3))) == -4
    # the window of `taps` inputs must fit the input in x and in y
    if d == "down":
        t = TAPS[kernel] * 2
        assert call(mk((3, 32, t - 1)), mk(good_out)) == -4 and call(mk((3, t - 1, 32)), mk(good_out)) == -4
        for bad in (0.0, -0.5, float("nan"), float("inf")):   # inf: 0 taps
            assert call(mk(good_in), mk(good_out), bad) == -4, bad
    else:
        t = TAPS[kernel]
        assert call(mk((3, 32, t - 1)), mk(good_out)) == -4 and call(mk((3, t - 1, 32)), mk(good_out)) == -4
    # order: type before dimensionality before stride before the regions
    assert call(mk(good_in[1:], other), mk(good_out)) == -3
    assert call(mk(good_in[1:]), packed_out) == -43
    assert call(packed_in, mk((5,) + good_out[1:])) == -8
    # with everything in order only the device is missing here
    import torch
    if not torch.cuda.is_available():
        assert call(mk(good_in), mk(good_out)) == -29


def test_the_issues_own_example_of_too_many_taps(hl):
    """8-pixel-wide input, lanczos _down, factor 0.5: 12 taps"""
    a, o = hl.Buffer(np.zeros((3, 32, 8), np.float32)), hl.Buffer(np.zeros((3, 16, 4), np.float32))
    assert call_argv(hl, "resize_lanczos_float32_down", a, 0.5, o) == -4
    assert "12-tap" in hl.last_error()


def test_bounds_queries(hl):
    q = hl.Buffer.bounds_query(np.uint8, 3, mins=(5, 6, 1), extents=(40, 30, 2))
    a = hl.Buffer(np.zeros((3, 64, 64), np.uint8))
    assert call_argv(hl, "resize_cubic_uint8_down", a, 0.5, q) == 0
    assert [(q.raw.dim[i].min, q.raw.dim[i].extent) for i in range(3)] == [(5, 40), (6, 30), (1, 2)]
    assert (q.raw.type.code, q.raw.type.bits) == (1, 8)
    qi = hl.Buffer.bounds_query(np.uint8, 3, mins=(2, 3, 0), extents=(64, 48, 0))
    o = hl.Buffer(np.zeros((2, 30, 40), np.uint8), mins=(5, 6, 1))
    assert call_argv(hl, "resize_cubic_uint8_down", qi, 0.5, o) == 0
    assert [(qi.raw.dim[i].min, qi.raw.dim[i].extent) for i in range(3)] == [(2, 64), (3, 48), (1, 2)]


# ---------------------------------------------------------------------------------------------------- CPU: halide_sin
def test_halide_sin_is_no_worse_than_glibc_plus_one_ulp(canon_rc):
    """Every float of both signs in [2^-12, 9.5] against (float)sin((double)x): the yardstick is glibc's sinf measured the same
    way, the margin one ulp for not having its table-driven reduction.  Measured: halide_sin 0.783 ulp, glibc 0.561 ulp."""
    lo, hi = int(np.float32(2.0 ** -12).view(np.uint32)), int(np.float32(9.5).view(np.uint32))
    ulp, where = (C.c_double * 2)(), (C.c_float * 2)()
    canon_rc.lib.rc_sin_sweep(lo, hi, ulp, where)
    print(f"halide_sin: {ulp[0]:.4f} ulp at {where[0]!r}; glibc sinf: {ulp[1]:.4f} ulp at {where[1]!r}")
    assert ulp[1] < 1.0, "the yardstick itself is off"
    assert ulp[0] <= ulp[1] + 1.0


def test_halide_sin_is_the_same_in_both_canonical_forms(rc):
    x = np.linspace(-9.5, 9.5, 200001).astype(np.float32)
    with checker_lib.canon(0):
        a = rc.sin(x)
    with checker_lib.canon(1):
        b = rc.sin(x)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert rc.sin(np.zeros(1, np.float32))[0] == 0.0


# ---------------------------------------------------------------------------------------------------- CPU: checker vs float64
@pytest.mark.parametrize("kernel", ["linear", "cubic", "lanczos"])
@pytest.mark.parametrize("tname", list(TYPES))
def test_checker_against_float64(rc, canon0_rc, kernel, tname):
    img = image(tname, (3, 97, 131), 131 + 97)
    worst = 0.0
    for up, factors in ((False, DOWN_FACTORS), (True, UP_FACTORS)):
        for scale in factors:
            got = rc.resize(kernel, img, scale, up)
            want, (bx, by) = ref64(kernel, img, scale, up)
            assert got.shape == want.shape and got.size > 0
            # the two evaluations share begin (a specified quantity), and no f32 kernel sum is zero (no NaN weights)
            for n, extent, b in ((got.shape[2], 131, bx), (got.shape[1], 97, by)):
                cb, cw, sums = rc.tables(kernel, up, scale, 0, n, 0, extent)
                assert np.array_equal(cb, b), (kernel, scale, up)
                assert np.all(sums != 0.0) and np.all(np.isfinite(cw))
            d = float(np.max(np.abs(got.astype(np.float64) - want)))
            worst = max(worst, d)
            if tname == "float32":
                assert d <= F32_VS_FLOAT64, (kernel, scale, up, d)
            else:
                assert d <= 1, (kernel, scale, up, d)
    print(f"{kernel} {tname}: largest |checker - float64| = {worst:.3g}")


@pytest.mark.parametrize("n", [2, 3, 4])
def test_box_up_by_an_integer_is_pixel_replication(rc, each_canon_rc, n):
    img = image("uint16", (3, 40, 50), n)
    got = rc.resize("box", img, float(n), True)
    assert np.array_equal(got, np.repeat(np.repeat(img, n, axis=1), n, axis=2))


@pytest.mark.parametrize("n", [2, 4, 8])
def test_box_down_by_one_nth_has_n_equal_weights_per_axis(rc, each_canon_rc, n):
    for extent in (64, 40):
        begin, w, sums = rc.tables("box", False, 1.0 / n, 0, extent // n, 0, extent)
        assert w.shape[0] == n and np.all(w == np.float32(1.0) / np.float32(n)) and np.all(sums == n)
        assert np.array_equal(begin, np.arange(extent // n) * n)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("up", [True, False], ids=["up", "down"])
def test_factor_one_returns_an_integer_image(rc, each_canon_rc, kernel, up):
    """Box, linear and cubic weights at integer offsets are exactly 0 and 1, so factor 1.0 is the identity.  Lanczos is not:
    sin(3.14159265359f * k) is not 0 in f32, the weights at the other integer offsets are tiny but not zero, and the cast
    truncates, so a value may lose 1 LSB (a numpy prototype: 2286 of 6000 values, each by exactly 1)."""
    img = image("uint8", (3, 40, 50), 50 * 40)
    got = rc.resize(kernel, img, 1.0, up)
    if kernel == "lanczos":
        assert np.max(np.abs(got.astype(int) - img.astype(int))) <= 1
    else:
        assert np.array_equal(got, img)


@pytest.mark.parametrize("kernel", KERNELS)
def test_a_constant_image_stays_constant_within_one_lsb(rc, canon0_rc, kernel):
    """follows from |checker - float64| <= 1: the float64 evaluation of a constant image is that constant"""
    for tname, value in (("uint8", 200), ("uint16", 51234)):
        img = np.full((2, 97, 131), value, TYPES[tname])
        for up, factors in ((False, DOWN_FACTORS), (True, UP_FACTORS)):
            for scale in factors:
                got = rc.resize(kernel, img, scale, up)
                assert np.max(np.abs(got.astype(int) - value)) <= 1, (kernel, tname, scale, up)


def test_checker_crop_equals_the_region_of_the_full_result(rc, each_canon_rc):
    img = image("uint16", (3, 97, 131), 5)
    full = rc.resize("cubic", img, 0.5, False)
    crop = rc.resize("cubic", img, 0.5, False, out_shape=(2, 20, 30), out_min=(17, 9, 1))
    assert np.array_equal(crop, full[1:3, 9:29, 17:47])


# ---------------------------------------------------------------------------------------------------- GPU
def _gpu(hl, kernel, img, scale, up, out_shape=None, out_min=(0, 0, 0), in_min=(0, 0, 0), general=False):
    if out_shape is None:
        out_shape = (img.shape[0],) + out_size(img.shape[2], img.shape[1], scale)[::-1]
    a, o = hl.Buffer(np.ascontiguousarray(img), mins=in_min), hl.Buffer(np.zeros(out_shape, img.dtype), mins=out_min)
    if general:
        hl.debug_resize_general(hl.resize_variant(a, scale, kernel, up), a, scale, o)
    else:
        hl.resize(a, scale, o, kernel, upsample=up)
    return o.numpy()


FUSED, GENERAL = {"rs_tables", "rs_fused"}, {"rs_tables", "rs_pass_x", "rs_pass_y"}


@pytest.mark.gpu
@pytest.mark.parametrize("name", VARIANTS)
def test_hip_matches_checker_all_variants(hl, canon_rc, on_stream, name):
    _, kernel, tname, d = name.split("_")
    up = d == "up"
    img = image(tname, (3, 97, 131), 97)
    factors = list(UP_FACTORS if up else DOWN_FACTORS)
    for scale in factors:
        _same(_gpu(hl, kernel, img, scale, up), canon_rc.resize(kernel, img, scale, up), f"{name} x {scale}")


@pytest.mark.gpu
def test_the_name_decides_the_direction_not_the_factor(hl, canon_rc):
    img = image("uint8", (3, 97, 131), 11)
    _same(_gpu(hl, "lanczos", img, 0.6, True), canon_rc.resize("lanczos", img, 0.6, True), "_up at 0.6")
    _same(_gpu(hl, "lanczos", img, 1.0, False), canon_rc.resize("lanczos", img, 1.0, False), "_down at 1.0")
    assert not np.array_equal(canon_rc.resize("lanczos", img, 0.6, True), canon_rc.resize("lanczos", img, 0.6, False))


# Which path a call takes (halide_amd/csrc/resize.hip, fused_fits): the fused tile's footprint in floats is
#   _down: 16 rows x (ceil(64 / factor) + taps + 3) columns     _up: (ceil(32 / factor) + taps + 3) rows x 64 columns
# against 12288 floats (48 KiB).
#   cubic _down 0.5:    16 x (128 + 8 + 3) = 2224                 fused
#   lanczos _down 0.05 on 2048 wide: 16 x (1280 + 120 + 3) = 22448 general; its x pass spans 256 * 20 + 120 floats per row > 2048: global gather
#   linear _down 0.1:   16 x (640 + 20 + 3) = 10608                fused;   box _down 0.07: 16 x (915 + 15 + 3) = 14928 general, x pass
#                       256 / 0.07 + 15 = 3673 floats > 2048: global gather;  every fused case is repeated on the general path (hlmi_resize_general),
#                       where its x pass stages the spans in LDS (cubic _down 0.5: 512 + 8 floats per row)
#   cubic _up 4:        (8 + 4 + 3) x 64 = 960                     fused
#   linear _up 0.15:    (214 + 2 + 3) x 64 = 14016                 general (an _up name far below 1)
PATH_CASES = [
    ("cubic", "uint8", False, 0.5, (3, 200, 300), FUSED),
    ("lanczos", "uint16", False, 0.05, (1, 300, 2048), GENERAL),
    ("linear", "float32", False, 0.1, (2, 200, 700), FUSED),
    ("box", "uint8", False, 0.07, (2, 150, 900), GENERAL),
    ("cubic", "float32", True, 4.0, (3, 60, 80), FUSED),
    ("lanczos", "uint8", True, 1.7, (3, 97, 131), FUSED),
    ("linear", "uint16", True, 0.15, (2, 300, 400), GENERAL),
]


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,tname,up,scale,shape,path", PATH_CASES)
def test_each_path_runs_and_matches_the_checker(hl, canon_rc, kernel, tname, up, scale, shape, path):
    img = image(tname, shape, shape[1])
    want = canon_rc.resize(kernel, img, scale, up)
    got = {}
    assert set(launches(hl, lambda: got.update(a=_gpu(hl, kernel, img, scale, up)))) == path
    _same(got["a"], want, "by size")
    assert set(launches(hl, lambda: got.update(b=_gpu(hl, kernel, img, scale, up, general=True)))) == GENERAL
    _same(got["b"], want, "general path")


@pytest.mark.gpu
@pytest.mark.parametrize("tname", ["uint8", "float32"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_the_references_own_configurations(hl, canon_rc, kernel, tname):
    """apps/resize/Makefile:53-79: 0.5 down on the full image, 4.0 up on the image reduced by 0.125, at this project's usual size"""
    big = image(tname, (3, 2560, 1536), 1536)
    _same(_gpu(hl, kernel, big, 0.5, False), canon_rc.resize(kernel, big, 0.5, False), "1536 x 2560 x 0.5")
    _same(_gpu(hl, kernel, big, 0.5, False, general=True), canon_rc.resize(kernel, big, 0.5, False), "1536 x 2560 x 0.5, general path")
    small = image(tname, (3, 320, 192), 192)
    _same(_gpu(hl, kernel, small, 4.0, True), canon_rc.resize(kernel, small, 4.0, True), "192 x 320 x 4.0")
    _same(_gpu(hl, kernel, small, 4.0, True, general=True), canon_rc.resize(kernel, small, 4.0, True), "192 x 320 x 4.0, general path")


@pytest.mark.gpu
def test_4k_u8_cubic_half(hl, canon_rc):
    img = image("uint8", (3, 2160, 3840), 4)
    want = canon_rc.resize("cubic", img, 0.5, False)
    _same(_gpu(hl, "cubic", img, 0.5, False), want, "3840 x 2160 x 0.5")
    _same(_gpu(hl, "cubic", img, 0.5, False, general=True), want, "3840 x 2160 x 0.5, general path")


@pytest.mark.gpu
@pytest.mark.parametrize("general", [False, True], ids=["by_size", "general"])
@pytest.mark.parametrize("kernel,tname,up,scale", [("cubic", "uint16", False, 0.37), ("lanczos", "float32", True, 3.3), ("linear", "uint8", False, 0.9)])
def test_crops_and_mins(hl, canon_rc, on_stream, kernel, tname, up, scale, general):
    img = image(tname, (4, 97, 131), 3)
    full = canon_rc.resize(kernel, img, scale, up)
    c, h, w = full.shape
    # an output crop equals that region of the full output
    crop = _gpu(hl, kernel, img, scale, up, out_shape=(2, h - 9 - 5, w - 17 - 3), out_min=(17, 9, 1), general=general)
    _same(crop, full[1:3, 9:h - 5, 17:w - 3], "crop at (17, 9, 1)")
    # a 1 x 1 output, one channel
    one = _gpu(hl, kernel, img, scale, up, out_shape=(1, 1, 1), out_min=(w - 1, h - 1, 3), general=general)
    _same(one, full[3:4, h - 1:h, w - 1:w], "1 x 1")
    # an input with a non-zero min: the checker is given the same geometry
    mins = (-7, 12, 2)
    o_min = (int(np.floor(mins[0] * scale)) + 2, int(np.floor(mins[1] * scale)) + 1, 3)
    want = canon_rc.resize(kernel, img, scale, up, out_shape=(2, h - 10, w - 10), out_min=o_min, in_min=mins)
    got = _gpu(hl, kernel, img, scale, up, out_shape=(2, h - 10, w - 10), out_min=o_min, in_min=mins, general=general)
    _same(got, want, "input min (-7, 12, 2)")
    # 1 channel
    _same(_gpu(hl, kernel, img[:1], scale, up, general=general), full[:1], "1 channel")
    _same(_gpu(hl, kernel, img, scale, up, general=general), full, "4 channels")


@pytest.mark.gpu
def test_device_halide_sin_is_the_checkers_bit_for_bit(hl, canon_rc):
    """every float of both signs in [2^-12, 9.5], the range halide_sin is specified and measured on"""
    f = hl.lib.hlmi_debug_math
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    lo, hi = int(np.float32(2.0 ** -12).view(np.uint32)), int(np.float32(9.5).view(np.uint32))
    step = 1 << 24
    for sign in (0, 0x80000000):
        for start in range(lo, hi + 1, step):
            x = (np.arange(start, min(start + step, hi + 1), dtype=np.uint32) | np.uint32(sign)).view(np.float32)
            got = np.empty_like(x)
            assert f(5, x.ctypes.data, None, None, got.ctypes.data, x.size) == 0
            want = canon_rc.sin(x)
            bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
            assert bad.size == 0, f"{bad.size} differ, first at x = {x[bad[0]]!r}: {got[bad[0]]!r} vs {want[bad[0]]!r}"


@pytest.mark.gpu
def test_device_tables_through_a_one_pixel_image_edge_cases(hl, canon_rc):
    """windows clamped at both borders and taps == extent: the smallest inputs the entry checks admit"""
    for kernel in KERNELS:
        t = TAPS[kernel]
        img = image("uint16", (1, t, t), t)
        _same(_gpu(hl, kernel, img, 3.0, True), canon_rc.resize(kernel, img, 3.0, True), f"{kernel} {t} x {t} up 3")
        img = image("uint16", (1, 2 * t, 2 * t), t)
        _same(_gpu(hl, kernel, img, 0.5, False), canon_rc.resize(kernel, img, 0.5, False), f"{kernel} {2 * t} x {2 * t} down 0.5")


# ---------------------------------------------------------------------------------------------------- torch
def test_torch_op_shape_function_and_cpu_refusal():
    import torch
    import halide_amd.torch_ops  # noqa: F401
    for dt in (torch.uint8, torch.uint16, torch.float32):
        meta = torch.empty((3, 97, 131), dtype=dt, device="meta")
        assert torch.ops.hlmi.resize(meta, 0.37).shape == (3, 35, 48) and torch.ops.hlmi.resize(meta, 3.3, "lanczos", None).dtype == dt
    with pytest.raises(RuntimeError, match="GPU"):
        torch.ops.hlmi.resize(torch.zeros((3, 16, 16), dtype=torch.uint16), 0.5)
    with pytest.raises(TypeError):
        torch.ops.hlmi.resize(torch.zeros((3, 16, 16), dtype=torch.int32), 0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("tname", list(TYPES))
def test_torch_op_equals_the_c_entry(hl, canon_rc, tname):
    import torch
    import halide_amd.torch_ops  # noqa: F401
    img = image(tname, (3, 97, 131), 21)
    t = torch.from_numpy(img).cuda()
    ptr = t.data_ptr()
    for kernel, scale, up in (("cubic", 0.5, None), ("lanczos", 1.7, None), ("linear", 0.6, True), ("box", 1.0, False)):
        out = torch.ops.hlmi.resize(t, scale, kernel, up)
        torch.cuda.synchronize()
        direction = (scale > 1.0) if up is None else up
        assert out.is_cuda and out.dtype == t.dtype and t.data_ptr() == ptr
        _same(out.cpu().numpy(), _gpu(hl, kernel, img, scale, direction), f"torch {kernel} {scale}")
        _same(out.cpu().numpy(), canon_rc.resize(kernel, img, scale, direction), f"torch {kernel} {scale} vs checker")
    assert np.array_equal(t.cpu().numpy(), img)


# ---------------------------------------------------------------------------------------------------- the RunGen-compatible runner
def test_runner_describes_a_variant_by_name():
    out = subprocess.run([RUNGEN, "--name=resize_cubic_uint8_down", "--describe"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'Input "input" is of type Buffer<uint8> with 3 dimensions' in out.stdout
    assert 'Input "scale_factor" is of type float32' in out.stdout and 'Output "output" is of type Buffer<uint8> with 3 dimensions' in out.stdout


@pytest.mark.gpu
def test_runner_resizes_a_ppm(tmp_path, rc):
    """hlmi_rungen finds pipelines by name and needs no entry of its own: PPM in, PPM out, the checker's pixels"""
    lib = C.CDLL(os.environ.get("HLMI_LIB") or os.path.join(ROOT, "halide_amd", "lib", "libhlmi.so"))   # the library the runner loads
    lib.hlmi_canon_fma.restype = C.c_int
    rgb = np.random.default_rng(8).integers(0, 256, (24, 40, 3), dtype=np.uint8)
    with open(tmp_path / "in.ppm", "wb") as f:
        f.write(b"P6\n40 24\n255\n" + rgb.tobytes())
    p = subprocess.run([RUNGEN, "--name=resize_cubic_uint8_down", f"input={tmp_path / 'in.ppm'}", "scale_factor=0.5", "--output_extents=[20,12,3]",
                        f"output={tmp_path / 'out.ppm'}"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    raw = open(tmp_path / "out.ppm", "rb").read()
    assert raw.split()[:4] == [b"P6", b"20", b"12", b"255"]
    got = np.frombuffer(raw[-20 * 12 * 3:], np.uint8).reshape(12, 20, 3).transpose(2, 0, 1)
    with checker_lib.canon(lib.hlmi_canon_fma()):
        want = rc.resize("cubic", np.ascontiguousarray(rgb.transpose(2, 0, 1)), 0.5, False)
    assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------- a seeded slice of the fuzzer
@pytest.mark.gpu
def test_seeded_fuzz_slice_of_resize():
    """scripts/fuzz_parity.py's resize case (random type, kernel, direction, factor in [0.05, 8], sizes, origins, crops), a fixed
    number of cases from a fixed seed"""
    mod = load_fuzz_parity()
    rng = np.random.default_rng(20261016)
    for i in range(40):
        desc, ok = mod.CASES["resize"](rng)
        assert ok, f"case {i}: {desc}"
