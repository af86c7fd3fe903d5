"""linear_blur and simple_blur: the 3x3 box blur of apps/linear_blur, in linear light and plain.

The checker is tests/cpp/linear_blur_check.c, a plain C restatement of apps/linear_blur/simple_blur_generator.cpp:5-22,
srgb_to_linear_generator.cpp:14-16, linear_to_srgb_generator.cpp:14-16 and linear_blur_generator.cpp:8-27 in both canonical float
forms, built and driven through ctypes by tests/checker_lib.py; it takes halide_pow and the mul+sub pair from
oracle/oracle_common.h.  The CPU tests hold the checker to a numpy float64 evaluation and to properties that follow from the
generators' text, and the entry points to their contract; the GPU tests hold the library to the checker bit for bit.  Like every
float pipeline here, the two are pinned to this repository's restatement only: no output of a real Halide build is involved."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import checker_lib
from parity_helpers import ROOT, RUNGEN, call_argv, call_direct, load_fuzz_parity, noise
from parity_helpers import gpu_present as _gpu_present, launches as _launches, same_bits as _same

NAMES = ["linear_blur", "simple_blur"]
f32 = np.float32
T_LINEAR, T_SRGB = f32(0.04045), f32(0.0031308)   # the thresholds of the two conversions


# ---------------------------------------------------------------------------------------------------- the checker
@pytest.fixture(scope="session")
def lc():
    return checker_lib.linear_blur


@pytest.fixture(params=[0, 1], ids=["canon0", "canon1"])
def each_canon_lc(request):
    with checker_lib.canon(request.param):
        yield request.param


@pytest.fixture
def canon_lc(hl, lc):
    """the checker in the form the loaded library was built for"""
    with checker_lib.canon(hl.canon_fma()):
        yield lc


# ---------------------------------------------------------------------------------------------------- CPU: the library's surface
EST = [0, 1536, 0, 2560, 0, 4]


def test_the_entry_points_are_exported_with_argv_and_metadata(hl):
    lib = C.CDLL(hl.LIB_PATH)
    for name in NAMES:
        for suffix in ("", "_argv", "_metadata"):
            assert hasattr(lib, name + suffix), name + suffix
        assert not hasattr(lib, name + "_auto_schedule")   # the reference builds no such object
        assert hl._fn[name] is not None
    assert hasattr(lib, "hlmi_linear_blur_general")
    est = lambda a: [a.buffer_estimates[j].contents.value for j in range(2 * a.dimensions)] if a.buffer_estimates else None
    md = hl.metadata("linear_blur")
    assert md.version == 1 and md.num_arguments == 2 and md.name.decode() == "linear_blur" and b"hip" in md.target
    a = [md.arguments[i] for i in range(2)]
    assert [x.name.decode() for x in a] == ["input", "output"] and [x.kind for x in a] == [1, 2] and [x.dimensions for x in a] == [3, 3]
    assert [(x.type.code, x.type.bits) for x in a] == [(2, 32), (2, 32)]
    assert est(a[0]) == EST and est(a[1]) == EST   # linear_blur_generator.cpp:20-21
    md = hl.metadata("simple_blur")
    assert md.version == 1 and md.num_arguments == 4 and md.name.decode() == "simple_blur" and b"hip" in md.target
    a = [md.arguments[i] for i in range(4)]
    assert [x.name.decode() for x in a] == ["input", "width", "height", "output"] and [x.kind for x in a] == [1, 0, 0, 2]
    assert [x.dimensions for x in a] == [3, 0, 0, 3] and [(x.type.code, x.type.bits) for x in a] == [(2, 32), (0, 32), (0, 32), (2, 32)]
    for x in a:   # built without estimates, and the generator declares no default and no range
        assert not x.scalar_def and not x.scalar_min and not x.scalar_max and not x.scalar_estimate and not x.buffer_estimates


def test_the_aot_headers_compile_as_c(tmp_path):
    decl = open(os.path.join(ROOT, "include", "hlmi_pipelines.h")).read()
    assert "int linear_blur(struct halide_buffer_t *input, struct halide_buffer_t *output);" in decl
    assert "int simple_blur(struct halide_buffer_t *input, int32_t width, int32_t height, struct halide_buffer_t *output);" in decl
    src = tmp_path / "both.c"
    src.write_text('#include "aot/linear_blur.h"\n#include "aot/simple_blur.h"\n'
                   "int (*const f)(struct halide_buffer_t *, struct halide_buffer_t *) = linear_blur;\n"
                   "int (*const g)(struct halide_buffer_t *, int32_t, int32_t, struct halide_buffer_t *) = simple_blur;\n"
                   "int (*const fa)(void **) = linear_blur_argv;\nint (*const ga)(void **) = simple_blur_argv;\n"
                   "const struct halide_filter_metadata_t *(*const fm)(void) = linear_blur_metadata;\n"
                   "const struct halide_filter_metadata_t *(*const gm)(void) = simple_blur_metadata;\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "both.o")], check=True)
    for name in NAMES:   # each alone, too
        one = tmp_path / (name + ".c")
        one.write_text(f'#include "aot/{name}.h"\nint (*const a)(void **) = {name}_argv;\n')
        subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(one), "-o", str(tmp_path / (name + ".o"))], check=True)


def test_runner_describes_both_by_name():
    out = subprocess.run([RUNGEN, "--name=linear_blur", "--describe"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'Input "input" is of type Buffer<float32> with 3 dimensions' in out.stdout and 'Output "output" is of type Buffer<float32> with 3 dimensions' in out.stdout
    out = subprocess.run([RUNGEN, "--name=simple_blur", "--describe"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'Input "input" is of type Buffer<float32> with 3 dimensions' in out.stdout and 'Input "width" is of type int32' in out.stdout
    assert 'Input "height" is of type int32' in out.stdout and 'Output "output" is of type Buffer<float32> with 3 dimensions' in out.stdout


# ---------------------------------------------------------------------------------------------------- CPU: the entry protocol
def _args(name, inp, width, height, out):
    """the entry point's own arguments: linear_blur takes no width and no height"""
    return (inp, out) if name == "linear_blur" else (inp, width, height, out)


HOW = pytest.mark.parametrize("how", [call_direct, call_argv], ids=["direct_call", "argv"])


@HOW
@pytest.mark.parametrize("name", NAMES)
def test_entry_protocol(hl, name, how):
    ok = 0 if _gpu_present() else -29   # with everything in order only the device can be missing
    mk = lambda shape=(3, 32, 40), dtype=f32, mins=None: hl.Buffer(np.zeros(shape, dtype), mins=mins)
    strided = lambda mins=None: hl.Buffer(np.zeros((3, 32, 80), f32)[:, :, ::2], mins=mins)   # stride.0 == 2
    call = lambda i, o, w=40, h=32: how(hl, name, *_args(name, i, w, h, o))
    assert call(None, mk()) == -12 and call(mk(), None) == -12
    assert call(mk(dtype=np.uint16), mk()) == -3 and call(mk(), mk(dtype=np.uint16)) == -3
    assert call(mk((32, 40)), mk()) == -43 and call(mk(), mk((32, 40))) == -43
    assert call(strided(), mk()) == -8 and "input.stride.0" in hl.last_error()
    assert call(mk(), strided()) == -8 and "output.stride.0" in hl.last_error()
    # the channels the output names must be the input's
    assert call(mk(), mk((4, 32, 40))) == -4 and "dimension 2" in hl.last_error()
    assert call(mk(), mk(mins=(0, 0, -1))) == -4 and "dimension 2" in hl.last_error()
    assert call(mk((5, 32, 40), mins=(0, 0, -2)), mk(mins=(0, 0, -1))) == ok
    # order: type before dimensionality before the constraints before the bounds
    assert call(mk((32, 40), np.uint16), mk()) == -3
    assert call(mk((32, 40)), strided()) == -43
    assert call(strided(), mk((4, 32, 40))) == -8
    assert call(None, mk((32, 40), np.uint16)) == -12
    # padded row and plane strides, any output region
    wide = lambda shape=(3, 32, 40): np.zeros((shape[0], shape[1] + 3, shape[2] + 5), f32)[:, 1:1 + shape[1], 2:2 + shape[2]]
    assert call(hl.Buffer(wide()), hl.Buffer(wide((3, 50, 70)), mins=(-20, -7, 0))) == ok
    assert call(mk(), mk((3, 5, 7), mins=(400, -300, 0))) == ok


@HOW
def test_linear_blur_clamps_to_the_extents_whatever_the_mins(hl, how):
    """width and height are the input's EXTENTS: the clamp is to [0, extent - 1] in absolute coordinates, so an input with mins
    (5, 0, 0) does not hold column 0, which an output at x 0 reads"""
    ok = 0 if _gpu_present() else -29
    inp = lambda mins: hl.Buffer(np.zeros((3, 32, 40), f32), mins=mins)
    out = lambda shape, mins: hl.Buffer(np.zeros(shape, f32), mins=mins)
    call = lambda i, o: how(hl, "linear_blur", i, o)
    assert call(inp((5, 0, 0)), out((3, 32, 40), (0, 0, 0))) == -4 and "dimension 0" in hl.last_error() and "before" in hl.last_error()
    assert call(inp((5, 0, 0)), out((3, 32, 40), (4, 0, 0))) == -4
    assert call(inp((5, 0, 0)), out((3, 32, 40), (5, 0, 0))) == ok     # columns 5 .. 39 (clamped at extent - 1 = 39)
    assert call(inp((5, 0, 0)), out((3, 32, 10), (30, 0, 0))) == ok
    assert call(inp((0, 3, 0)), out((3, 8, 40), (0, 2, 0))) == -4 and "dimension 1" in hl.last_error()
    assert call(inp((0, 3, 0)), out((3, 8, 40), (0, 3, 0))) == ok
    # negative mins: the input ends before extent - 1, which an output reaching that far reads
    assert call(inp((-2, 0, 0)), out((3, 32, 40), (0, 0, 0))) == -4 and "beyond" in hl.last_error()   # reads up to column 39, the input ends at 37
    assert call(inp((-2, 0, 0)), out((3, 32, 36), (0, 0, 0))) == ok    # reads columns 0 .. 37
    assert call(inp((-2, 0, 0)), out((3, 32, 37), (0, 0, 0))) == -4    # reads column 38


@HOW
@pytest.mark.parametrize("width", [25, 40, 60], ids=["narrower", "equal", "wider"])
def test_simple_blur_requires_its_box_down_to_the_edge_cell(hl, how, width):
    """the buffer is 40 wide and 32 tall; the output region [ox, ox + ow) reads columns cx(ox) .. cx(ox + ow + 1), the same in y"""
    ok = 0 if _gpu_present() else -29
    cl = lambda v, n: max(min(v, n - 1), 0)
    for ox, ow in ((0, 20), (3, 30), (-5, 12), (10, 38), (50, 4)):
        lo, hi = cl(ox, width), cl(ox + ow + 1, width)
        for axis in (0, 1):   # the same box along x (against `width`) and along y (against `height`)
            def call(in_min, in_ext):
                shape, mins, omin, oshape = [3, 32, 40], [0, 0, 0], [0, 0, 0], [3, 8, 8]
                shape[2 - axis], mins[axis], omin[axis], oshape[2 - axis] = in_ext, in_min, ox, ow
                w, h = (width, 32) if axis == 0 else (40, width)
                return how(hl, "simple_blur", hl.Buffer(np.zeros(shape, f32), mins=mins), w, h, hl.Buffer(np.zeros(oshape, f32), mins=omin))
            what = f"width {width} region [{ox}, {ox + ow}) axis {axis}: box [{lo}, {hi}]"
            assert call(lo, hi - lo + 1) == ok, what
            assert call(lo - 2, hi - lo + 5) == ok, what
            assert call(lo + 1, max(hi - lo, 1)) == -4 and f"dimension {axis}" in hl.last_error() and "before" in hl.last_error(), what
            if hi > lo:
                assert call(lo, hi - lo) == -4 and f"dimension {axis}" in hl.last_error() and "beyond" in hl.last_error(), what


@HOW
def test_bounds_queries(hl, how):
    dims = lambda b: [(b.raw.dim[i].min, b.raw.dim[i].extent) for i in range(3)]
    real = lambda shape=(3, 48, 64), mins=(2, 3, 0): hl.Buffer(np.zeros(shape, f32), mins=mins)
    query = lambda mins, ext, dtype=f32: hl.Buffer.bounds_query(dtype, 3, mins=mins, extents=ext)
    # simple_blur, the input asked for: exactly the box, whatever was passed
    for (w, h, omin, oshape), want in {
        (5, 20, (-3, 2, 1), (3, 8, 8)): [(0, 5), (2, 10), (1, 3)],
        (100, 100, (-3, 2, 1), (3, 8, 8)): [(0, 7), (2, 10), (1, 3)],          # ox < 0 < ox + ow
        (1, 1, (-3, 2, -2), (2, 8, 8)): [(0, 1), (0, 1), (-2, 2)],             # width 1: column 0 only
        (0, -3, (7, 2, 0), (3, 8, 8)): [(0, 1), (0, 1), (0, 3)],               # width 0: the formula reads column 0 everywhere
        (100, 100, (90, 95, 0), (1, 30, 30)): [(90, 10), (95, 5), (0, 1)],     # clamped at width - 1
        (100, 100, (400, -300, 0), (1, 30, 30)): [(99, 1), (0, 1), (0, 1)],    # wholly outside
    }.items():
        q = query((11, 12, 13), (14, 15, 16), np.uint8)
        assert how(hl, "simple_blur", q, w, h, real(oshape, omin)) == 0
        assert dims(q) == want and (q.raw.type.code, q.raw.type.bits) == (2, 32) and [q.raw.dim[i].stride for i in range(3)] == [1, want[0][1], want[0][1] * want[1][1]]
    # the output asked for: it is the request and stays as passed; a real input is left alone
    q, a = query((5, 6, 1), (40, 30, 2)), real()
    assert how(hl, "simple_blur", a, 64, 48, q) == 0
    assert dims(q) == [(5, 40), (6, 30), (1, 2)] and dims(a) == [(2, 64), (3, 48), (0, 3)]
    # both asked for (RunGen's way): the output's shape is the request
    q, qi = query((5, 6, 1), (40, 30, 2)), query((0, 0, 0), (0, 0, 0))
    assert how(hl, "simple_blur", qi, 64, 48, q) == 0
    assert dims(q) == [(5, 40), (6, 30), (1, 2)] and dims(qi) == [(5, 42), (6, 32), (1, 2)]
    # linear_blur: its box depends on the input's own extents, so x and y stay as passed and the channels are the output's
    qi = query((2, 3, 0), (64, 48, 5))
    assert how(hl, "linear_blur", qi, real((3, 30, 40), (-5, 100, 1))) == 0
    assert dims(qi) == [(2, 64), (3, 48), (1, 3)]
    q, a = query((5, 6, 1), (40, 30, 2)), real()
    assert how(hl, "linear_blur", a, q) == 0
    assert dims(q) == [(5, 40), (6, 30), (1, 2)] and dims(a) == [(2, 64), (3, 48), (0, 3)]
    q, qi = query((5, 6, 1), (40, 30, 2), np.uint16), query((0, 0, 0), (64, 48, 3))
    assert how(hl, "linear_blur", qi, q) == 0
    assert dims(q) == [(5, 40), (6, 30), (1, 2)] and dims(qi) == [(0, 64), (0, 48), (1, 2)] and (q.raw.type.code, q.raw.type.bits) == (2, 32)
    # a query with the wrong dimensionality stays an error
    assert how(hl, "linear_blur", hl.Buffer.bounds_query(f32, 2, mins=(0, 0), extents=(4, 4)), real()) == -43


def test_without_a_gpu_the_python_calls_refuse_to_run(hl):
    a, o = hl.Buffer(np.zeros((3, 16, 16), f32)), hl.Buffer(np.zeros((3, 16, 16), f32))
    with pytest.raises(hl.HalideError) as e:
        hl.debug_linear_blur_general("wavelet", a, 16, 16, o)
    assert e.value.code == -8
    if _gpu_present():
        return   # what follows is the statement about a machine without one
    for fn in (lambda: hl.linear_blur(a, o), lambda: hl.simple_blur(a, 16, 16, o), lambda: hl.debug_linear_blur_general("linear_blur", a, 0, 0, o),
               lambda: hl.debug_linear_blur_general("simple_blur", a, 16, 16, o)):
        with pytest.raises(hl.HalideError) as e:
            fn()
        assert e.value.code == -29


# ---------------------------------------------------------------------------------------------------- CPU: what follows from the text
def test_an_impulse_pins_the_off_centre_window(lc, each_canon_lc):
    img = np.zeros((1, 16, 12), f32)
    img[0, 7, 5] = 1.0   # x 5, y 7
    for name in NAMES:
        out = lc.blur(name, img)
        ys, xs = np.nonzero(out[0])
        assert sorted(set(xs)) == [3, 4, 5] and sorted(set(ys)) == [5, 6, 7] and len(xs) == 9, name   # the window is x .. x + 2, y .. y + 2
    third = f32(1) / f32(3)
    assert np.all(lc.blur("simple_blur", img)[0, 5:8, 3:6] == f32(f32(third) * third))


def test_width_and_height_one_make_a_channel_constant(lc, each_canon_lc):
    img = noise((3, 9, 11), 4)
    out = lc.blur("simple_blur", img, 1, 1, out_shape=(3, 20, 30), out_min=(-4, -5, 0))
    for c in range(3):
        v = img[c, 0, 0]
        third = f32(1) / f32(3)
        bx = f32(f32(f32(v + v) + v) * third)
        assert np.all(out[c] == f32(f32(f32(bx + bx) + bx) * third))
    one = lc.blur("linear_blur", img[:, :1, :1], out_shape=(3, 20, 30), out_min=(-4, -5, 0))   # an input of 1 x 1
    for c in range(3):
        assert np.all(one[c].view(np.uint32) == one[c, 0, 0].view(np.uint32))
    # width <= 0 needs no special case: column 0 everywhere
    assert np.array_equal(lc.blur("simple_blur", img, 0, -3), lc.blur("simple_blur", img, 1, 1))


@pytest.mark.parametrize("name", NAMES)
def test_a_crop_equals_that_region(lc, each_canon_lc, name):
    img = noise((3, 45, 70), 3)
    big = lc.blur(name, img, out_shape=(3, 60, 100), out_min=(-10, -5, 0))
    assert np.array_equal(lc.blur(name, img, out_shape=(2, 20, 30), out_min=(17, 9, 1)).view(np.uint32), big[1:3, 14:34, 27:57].view(np.uint32))
    assert np.array_equal(lc.blur(name, img).view(np.uint32), big[:, 5:50, 10:80].view(np.uint32))
    if name == "simple_blur":   # it moves with the clamp window, not with the buffer: a buffer over a part of [0, width) x [0, height)
        part = lc.blur(name, img[:, 5:40, 10:60], 70, 45, out_shape=(3, 30, 45), out_min=(10, 5, 0), in_min=(10, 5, 0))
        assert np.array_equal(part.view(np.uint32), big[:, 10:40, 20:65].view(np.uint32))
    lc.blur(name, img, out_shape=(3, 45, 70), out_min=(0, 0, 0), in_min=(5, 0, 0), expect=-4)   # both: column 0 is not in such an input


def test_the_thresholds_take_the_branch_the_comparison_says(lc, each_canon_lc, oracle):
    up, down = lambda v: np.nextafter(v, f32(np.inf)), lambda v: np.nextafter(v, f32(-np.inf))
    k_lin, k_div, one_a, a = f32(1) / f32(12.92), f32(1) / f32(f32(1) + f32(0.055)), f32(f32(1) + f32(0.055)), f32(0.055)
    assert one_a == f32(1.055)   # 1 + .055f folded in f32 is the constant the contract names
    inv_gamma = f32(1) / f32(2.4)
    with oracle.canon(each_canon_lc):
        for s in (down(down(T_LINEAR)), down(T_LINEAR), T_LINEAR, up(T_LINEAR), up(up(T_LINEAR)), f32(0), f32(-0.25), f32(1), f32(4)):
            low, high = f32(s * k_lin), f32(oracle.halide_pow(float(f32(f32(s + a) * k_div)), 2.4))
            assert lc.to_linear(s).view(np.uint32) == (low if s <= T_LINEAR else high).view(np.uint32), s
        for l in (down(down(T_SRGB)), down(T_SRGB), T_SRGB, up(T_SRGB), up(up(T_SRGB)), f32(0), f32(-0.25), f32(1), f32(4)):
            p = f32(oracle.halide_pow(float(l), float(inv_gamma)))
            high = f32(np.float64(one_a) * np.float64(p) - np.float64(a)) if each_canon_lc else f32(f32(one_a * p) - a)   # one rounding: the f64 product is exact
            assert lc.to_srgb(l).view(np.uint32) == (f32(l * f32(12.92)) if l <= T_SRGB else high).view(np.uint32), l
    # the two branches of each conversion differ at the threshold's upper neighbour, so the comparison above can tell them apart
    assert f32(up(T_LINEAR) * k_lin) != lc.to_linear(up(T_LINEAR)) and f32(up(T_SRGB) * f32(12.92)) != lc.to_srgb(up(T_SRGB))


# ---------------------------------------------------------------------------------------------------- CPU: checker vs float64
def ref64(name, img, width=None, height=None):
    """the image's own region in float64: np.power, the same clamps, the generators' f32 constants and the branch the f32 sample takes"""
    c, h, w = img.shape
    width, height = w if width is None else width, h if height is None else height
    v = img.astype(np.float64)
    if name == "linear_blur":
        with np.errstate(invalid="ignore"):
            v = np.where(img <= T_LINEAR, v / np.float64(f32(12.92)), np.power((v + np.float64(f32(0.055))) / np.float64(f32(1.055)), np.float64(f32(2.4))))
    cx = lambda k: np.clip(np.arange(w) + k, 0, max(width - 1, 0))
    cy = lambda k: np.clip(np.arange(h) + k, 0, max(height - 1, 0))
    bx = (v[:, :, cx(0)] + v[:, :, cx(1)] + v[:, :, cx(2)]) / 3.0
    out = (bx[:, cy(0)] + bx[:, cy(1)] + bx[:, cy(2)]) / 3.0
    if name == "linear_blur":
        with np.errstate(invalid="ignore"):
            out = np.where(out <= np.float64(T_SRGB), out * np.float64(f32(12.92)),
                           np.float64(f32(1.055)) * np.power(out, 1.0 / np.float64(f32(2.4))) - np.float64(f32(0.055)))
    return out


CPU_SHAPE = (3, 168, 200)   # 200 x 168 x 3
CPU_SEEDS = (200 + 168, 1, 2)

# The largest |checker - float64| measured for noise in [0, 1) at 200 x 168 x 3 with the checker alone (no code under test involved),
# seeds 368 / 1 / 2: linear_blur 1.59e-7 / 1.69e-7 / 1.47e-7 in canonical form 0 and 1.59e-7 / 1.48e-7 / 1.42e-7 in form 1; simple_blur
# 1.46e-7 / 1.72e-7 / 1.52e-7 in both (it has no fused operation).  Far below the 1e-5 at which the restatement would be suspect: the
# sums are eight f32 additions and two multiplications of values below 1 (2^-24 = 6e-8 each at most), and halide_pow adds about as
# much again on outputs near 0.5.  Other seeds vary, so 4 x the largest value seen is allowed.
F32_VS_FLOAT64 = {"linear_blur": 4 * 1.69e-7, "simple_blur": 4 * 1.72e-7}


@pytest.mark.parametrize("seed", CPU_SEEDS)
@pytest.mark.parametrize("name", NAMES)
def test_checker_against_float64(lc, each_canon_lc, name, seed):
    img = noise(CPU_SHAPE, seed)
    d = float(np.max(np.abs(lc.blur(name, img).astype(np.float64) - ref64(name, img))))
    print(f"{name} canon {each_canon_lc} seed {seed}: largest |checker - float64| = {d:.3g}")
    assert d <= F32_VS_FLOAT64[name]
    if name == "simple_blur":   # a clamp window smaller than the image
        d = float(np.max(np.abs(lc.blur(name, img, 150, 100).astype(np.float64) - ref64(name, img, 150, 100))))
        assert d <= F32_VS_FLOAT64[name]


# ---------------------------------------------------------------------------------------------------- GPU
def _strided(shape, padded):
    """a zeroed (C, H, W) array; padded: inside a wider and taller allocation (row stride != width, plane stride != rows * row stride)"""
    if not padded:
        return np.zeros(shape, f32)
    return np.zeros((shape[0], shape[1] + 3, shape[2] + 5), f32)[:, 1:1 + shape[1], 2:2 + shape[2]]


def _gpu(hl, name, img, width=None, height=None, out_shape=None, out_min=None, in_min=(0, 0, 0), general=False, padded=False):
    out_shape = img.shape if out_shape is None else out_shape
    out_min = in_min if out_min is None else out_min
    src = _strided(img.shape, padded)
    src[...] = img
    a, o = hl.Buffer(src, mins=in_min), hl.Buffer(_strided(out_shape, padded), mins=out_min)
    width, height = img.shape[2] if width is None else width, img.shape[1] if height is None else height
    if general:
        hl.debug_linear_blur_general(name, a, width, height, o)
    elif name == "linear_blur":
        hl.linear_blur(a, o)
    else:
        hl.simple_blur(a, width, height, o)
    assert np.array_equal(src, img, equal_nan=True)
    return np.ascontiguousarray(o.numpy())


@pytest.fixture(params=["by_size", "general"])
def general(request):
    """Both implementations (halide_amd/csrc/linear_blur.hip): the one launch every shape takes, and the unfused composition through
    the hook.  The kernel has no forced-tile switch: one tile shape serves every size."""
    return request.param == "general"


# x, y, c: the smallest image; an extent below the 3-tap window; a single column; one past four 64-wide tiles; odd sizes; exact
# multiples of the 64 x 32 tile, three tiles in x and two in y
SHAPES = [(1, 1, 1), (2, 1, 3), (1, 40, 1), (257, 2, 4), (131, 97, 3), (192, 64, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sizes(hl, canon_lc, on_stream, name, shape, general):
    img = noise(shape[::-1], shape[0] * shape[1] * shape[2])
    _same(_gpu(hl, name, img, general=general), canon_lc.blur(name, img), f"{name} {shape}")


@pytest.fixture(scope="module")
def region_image():
    return noise((3, 97, 131), 5)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_regions(hl, canon_lc, on_stream, name, region_image, general):
    img = region_image
    both = lambda what, **kw: _same(_gpu(hl, name, img, general=general, **kw), canon_lc.blur(name, img, **{k: v for k, v in kw.items() if k != "padded"}), f"{name} {what}")
    both("around the input", out_shape=(3, 120, 170), out_min=(-20, -7, 0))
    both("outside the input: every tap clamps", out_shape=(3, 20, 30), out_min=(400, -300, 0))
    both("channel mins -2", in_min=(0, 0, -2))
    both("channels 1 .. 2 of an input at -2", in_min=(0, 0, -2), out_shape=(2, 97, 131), out_min=(0, 0, -1))
    both("padded row and plane strides", padded=True)
    both("padded strides around the input", padded=True, out_shape=(2, 120, 170), out_min=(-20, -7, 1))
    if name == "linear_blur":
        # input mins (17, -9, 0): the clamp stays [0, 130] x [0, 96], the input holds columns 17 .. 147 and rows -9 .. 87
        both("input mins (17, -9, 0)", in_min=(17, -9, 0), out_shape=(3, 30, 40), out_min=(20, 3, 0))
        both("input mins (17, -9, 0), up to the clamp's last column", in_min=(17, -9, 0), out_shape=(3, 70, 200), out_min=(17, 0, 0))
    else:
        for width, height in ((50, 40), (131, 97), (1, 1), (0, -3)):
            both(f"width {width} height {height}", width=width, height=height)
        both("a window past the buffer, the region inside it", width=500, height=400, out_shape=(3, 90, 120), out_min=(2, 3, 0))
        both("input mins (17, -9, 0) under a window of 140 x 80", width=140, height=80, in_min=(17, -9, 0), out_shape=(3, 100, 150), out_min=(17, 0, 0))


def _special_image():
    """64 x 8 x 1: sixteen 4-column blocks, each constant, so that every special value also meets itself in whole windows"""
    up, down = lambda v: np.nextafter(v, f32(np.inf)), lambda v: np.nextafter(v, f32(-np.inf))
    tiny, denormal = f32(np.finfo(f32).tiny), np.uint32(0x00012345).view(f32)
    vals = [down(T_LINEAR), T_LINEAR, up(T_LINEAR), down(T_SRGB), T_SRGB, up(T_SRGB), f32(0), f32(-0.25), f32(1), f32(4), tiny, denormal,
            f32(T_SRGB * f32(12.92)), f32(0.5), f32(-0.0), f32(0.04)]
    return np.repeat(np.array(vals, f32), 4)[None, None, :].repeat(8, axis=1).copy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_special_values(hl, canon_lc, on_stream, name, general):
    img = _special_image()
    assert img.shape == (1, 8, 64)
    _same(_gpu(hl, name, img, general=general), canon_lc.blur(name, img), f"{name} thresholds, their neighbours, 0, -0.25, 1, 4, tiny, denormal")
    # a NaN and a +inf: NaN where the checker has NaN (payloads are not pinned), bits elsewhere
    img = noise((1, 8, 64), 8)
    img[0, 3, 10], img[0, 5, 40] = np.nan, np.inf
    got, want = _gpu(hl, name, img, general=general), canon_lc.blur(name, img)
    assert np.isnan(want).any() and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])


@pytest.mark.gpu
def test_the_paths_launch_what_they_say(hl):
    for shape in ((3, 97, 131), (1, 1, 1)):   # one launch for every shape
        img = noise(shape, 2)
        assert _launches(hl, lambda: _gpu(hl, "linear_blur", img)) == ["lb_fused"]
        assert _launches(hl, lambda: _gpu(hl, "simple_blur", img)) == ["sb_fused"]
        assert _launches(hl, lambda: _gpu(hl, "linear_blur", img, general=True)) == ["lb_blur_general", "lb_to_linear", "lb_to_srgb"]
        assert _launches(hl, lambda: _gpu(hl, "simple_blur", img, general=True)) == ["lb_blur_general"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("shape", [(257, 2, 4), (131, 97, 3), (192, 64, 4)], ids=lambda s: "x".join(map(str, s)))
def test_fused_equals_general(hl, on_stream, name, shape):
    img = noise(shape[::-1], 11) * f32(1.5) - f32(0.2)
    kw = dict(out_shape=(shape[2], shape[1] + 9, shape[0] + 12), out_min=(-5, -4, 0))
    _same(_gpu(hl, name, img, **kw), _gpu(hl, name, img, general=True, **kw), f"{name} {shape}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_argv_equals_the_direct_call(hl, on_stream, name):
    img = noise((3, 45, 70), 6)
    outs = []
    for how in (call_direct, call_argv):
        a, o = hl.Buffer(img.copy()), hl.Buffer(np.zeros((3, 45, 70), f32))
        assert how(hl, name, *_args(name, a, 61, 33, o)) == 0   # a width and a height that are not the buffer's, and not each other's
        outs.append(np.ascontiguousarray(o.numpy()))
    assert outs[0].tobytes() == outs[1].tobytes() and outs[0].any()


# ---------------------------------------------------------------------------------------------------- torch
def test_torch_ops_shape_functions_and_cpu_refusal():
    import torch
    import halide_amd.torch_ops  # noqa: F401
    meta = torch.empty((3, 45, 70), dtype=torch.float32, device="meta")
    for op in (torch.ops.hlmi.linear_blur, torch.ops.hlmi.simple_blur):
        assert op(meta).shape == (3, 45, 70) and op(meta).dtype == torch.float32
        with pytest.raises(RuntimeError, match="GPU"):
            op(torch.zeros((3, 16, 16)))
        with pytest.raises(TypeError):
            op(torch.zeros((3, 16, 16), dtype=torch.int32))
        with pytest.raises(TypeError):
            op(torch.zeros((16, 16)))


@pytest.mark.gpu
def test_torch_ops_equal_the_checker(hl, canon_lc):
    import torch
    import halide_amd.torch_ops  # noqa: F401
    img = noise((3, 45, 70), 21)
    t = torch.from_numpy(img).cuda()
    for name, op in (("linear_blur", torch.ops.hlmi.linear_blur), ("simple_blur", torch.ops.hlmi.simple_blur)):
        out = op(t)
        torch.cuda.synchronize()
        assert out.is_cuda and out.shape == t.shape and out.dtype == torch.float32
        _same(out.cpu().contiguous().numpy(), canon_lc.blur(name, img), f"torch {name}")
    assert np.array_equal(t.cpu().numpy(), img)


# ---------------------------------------------------------------------------------------------------- a seeded slice of the fuzzer
@pytest.mark.gpu
def test_seeded_fuzz_slice_of_linear_blur(on_stream):
    """scripts/fuzz_parity.py's linear_blur case (both entry points), a fixed number of cases from a fixed seed"""
    mod = load_fuzz_parity()
    rng = np.random.default_rng(20261018)
    for i in range(40):
        desc, ok = mod.CASES["linear_blur"](rng)
        assert ok, f"case {i}: {desc}"
