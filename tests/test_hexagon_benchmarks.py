"""hexagon_benchmarks: conv3x3a16, conv3x3a32, dilate3x3, median3x3, gaussian5x5 and sobel, six u8 stencils (apps/hexagon_benchmarks).

The contract is integer arithmetic over repeat_edge of the input's own box (include/hlmi_pipelines.h).  The checker
is tests/cpp/hexagon_benchmarks_check.c, plain C with two restatements per filter — hb_<name> from the generator, hb_<name>_verify
from the matching verifier of the reference's process.h — built and driven through ctypes by tests/hexagon_benchmarks_checker.py.
The CPU tests hold the two to each other and to an independent numpy evaluation (int64 with explicit masks, np.sort for the median),
name the contract's traps one by one, and hold the entry points to their protocol; the GPU tests hold the library to hb_<name> bit
for bit, on the default path and on the one-thread-per-pixel path.  No float operation is involved, so the same bytes are expected
of both library builds: each is compared with the same checker output."""
import ctypes as C
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import hexagon_benchmarks_checker as hb
from parity_helpers import ROOT, RUNGEN, call_argv, call_direct, load_fuzz_parity
from parity_helpers import gpu_present as _gpu_present, launches as _launches, same_bits as _same

u8, i8, i32, i64 = np.uint8, np.int8, np.int32, np.int64
NAMES, MASKED = hb.NAMES, hb.MASKED
VALS = np.array([0, 1, 127, 128, 254, 255], u8)
ALL16 = np.full((3, 3), 16, i8)


def _geometry():
    """the sliding kernel's constants, read from its source: the sizes below straddle them, and a kernel without them fails here"""
    src = open(os.path.join(ROOT, "halide_amd", "csrc", "hexagon_benchmarks.hip")).read()
    val = lambda n: int(re.search(rf"^constexpr int {n} = (\d+);", src, re.M).group(1))
    return val("PX"), val("OUT_LANES"), val("ROWS"), val("WAVES")


PX, OUT_LANES, ROWS, WAVES = _geometry()
WAVE_PX, GROUP_ROWS = OUT_LANES * PX, WAVES * ROWS   # a wave's span in pixels (a workgroup's is the same: its waves are stacked in y)


def _mask_for(name, mask=hb.DRIVER_MASK):
    return mask if name in MASKED else None


# ---------------------------------------------------------------------------------------------------- the independent evaluation
def _np_eval(name, img, mask=None, region=None):
    """the contract in int64: taps gathered with clipped indices, wraps as explicit masks, the median by np.sort"""
    ih, iw = img.shape
    ox, oy, ow, oh = region if region is not None else (0, 0, iw, ih)
    X, Y = ox + np.arange(ow), oy + np.arange(oh)
    tap = lambda dx, dy: img[np.clip(Y + dy, 0, ih - 1)[:, None], np.clip(X + dx, 0, iw - 1)[None, :]].astype(i64)
    wrap16 = lambda v: ((v + 32768) & 0xffff) - 32768
    if name == "dilate3x3":
        out = np.max([tap(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)
    elif name == "median3x3":
        out = np.sort(np.stack([tap(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]), axis=0)[4]
    elif name == "sobel":
        gx = sum(w * (tap(dx, -1) - tap(dx, 1)) for dx, w in ((-1, 1), (0, 2), (1, 1)))
        gy = sum(w * (tap(-1, dy) - tap(1, dy)) for dy, w in ((-1, 1), (0, 2), (1, 1)))
        out = np.minimum(np.abs(gx) + np.abs(gy), 255)
    elif name == "gaussian5x5":
        k = (1, 4, 6, 4, 1)
        true = sum(k[dx + 2] * k[dy + 2] * tap(dx, dy) for dy in range(-2, 3) for dx in range(-2, 3))
        out = (wrap16(true) >> 8) & 0xff
        assert np.array_equal(out, true // 256)   # the wrap is undone: floor(true sum / 256)
    else:
        m = np.asarray(mask).astype(i64)
        s = sum(m[i + 1, j + 1] * tap(j, i) for i in (-1, 0, 1) for j in (-1, 0, 1))
        out = np.clip((wrap16(s) if name == "conv3x3a16" else s) >> 4, 0, 255)
    return out.astype(u8)


def _noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=u8)


def _six_values(w, h, seed):
    return VALS[np.random.default_rng(seed).integers(0, 6, (h, w))]


@pytest.fixture(scope="module")
def driver_scene():
    """the driver's setting shrunk: seeded noise at 257 x 131, the driver's mask; (image, {name: the checker's output}), computed once
    and never written to"""
    img = _noise(257, 131, 1)
    img.setflags(write=False)
    want = {n: hb.run(n, img, _mask_for(n)) for n in NAMES}
    for v in want.values():
        v.setflags(write=False)
    return img, want


# ---------------------------------------------------------------------------------------------------- CPU: the two restatements and numpy
@pytest.mark.parametrize("name", NAMES)
def test_the_two_restatements_agree_with_each_other_and_with_numpy(name, driver_scene):
    rng = np.random.default_rng(7)
    masks = [hb.DRIVER_MASK, ALL16, np.full((3, 3), -128, i8), np.full((3, 3), 127, i8)] + [rng.integers(-128, 128, (3, 3)).astype(i8) for _ in range(4)]
    images = [driver_scene[0], _noise(37, 11, 2), _six_values(64, 33, 3), _six_values(5, 7, 4), _noise(1, 1, 5), _noise(2, 9, 6), _noise(9, 2, 7)]
    for img in images:
        h, w = img.shape
        regions = [None, (0, 0, w + 9, h + 5), (-4, -3, w + 8, h + 7), (w + 2, h + 1, 5, 4), (-9, 2, 6, 3)]
        for mask in (masks if name in MASKED else [None]):
            for region in regions:
                a, b = hb.run(name, img, mask, region), hb.run(name, img, mask, region, verify=True)
                _same(a, b, f"{name} generator vs verifier {img.shape} {region}")
                _same(a, _np_eval(name, img, mask, region), f"{name} vs numpy {img.shape} {region}")
    _same(driver_scene[1][name], _np_eval(name, driver_scene[0], _mask_for(name)), name)


@pytest.mark.parametrize("lo,hi", [(0, 255), (127, 128), (254, 255), (0, 1)])
def test_the_network_is_the_median_on_every_window_over_a_two_value_alphabet(lo, hi):
    """all 512 3x3 windows of {lo, hi}, tiled 32 x 16 into one image: the centre of each tile sees exactly its window, and the median
    of nine values from two is hi iff five or more are"""
    img = np.zeros((16 * 3, 32 * 3), u8)
    want = np.zeros((16, 32), u8)
    for n in range(512):
        win = np.array([(n >> k) & 1 for k in range(9)]).reshape(3, 3)
        ty, tx = divmod(n, 32)
        img[3 * ty:3 * ty + 3, 3 * tx:3 * tx + 3] = np.where(win, hi, lo)
        want[ty, tx] = hi if win.sum() >= 5 else lo
    for verify in (False, True):
        _same(np.ascontiguousarray(hb.run("median3x3", img, verify=verify)[1::3, 1::3]), want, f"verify={verify}")
    _same(np.ascontiguousarray(_np_eval("median3x3", img)[1::3, 1::3]), want, "numpy")


# ---------------------------------------------------------------------------------------------------- CPU: the traps, one by one
def test_the_trap_conv3x3a16_wraps_where_conv3x3a32_saturates():
    """all 255 under all 16: the sum is 36720; int32 gives 2295 -> 255; int16 wraps to -28816, >> 4 is -1801 -> 0.  A saturating
    accumulator would write 255."""
    img = np.full((6, 9), 255, u8)
    assert (hb.conv_sum(img, ALL16) == 36720).all()
    assert 36720 - 65536 == -28816 and -28816 >> 4 == -1801
    for verify in (False, True):
        assert (hb.run("conv3x3a16", img, ALL16, verify=verify) == 0).all()
        assert (hb.run("conv3x3a32", img, ALL16, verify=verify) == 255).all()


def test_conv3x3a16_equals_conv3x3a32_exactly_where_the_sum_fits_int16():
    """The int16 sum is the int32 sum wherever -32768 <= sum < 32768, and the outputs agree there; nowhere else is it: it is the sum
    modulo 2^16, and the output follows the wrapped value.  A sum in [32768, 65536) wraps negative: 0 against 255, always.  One in
    [-65536, -32768) wraps to w >= 0: clamp(w >> 4) against 0, which differ unless w < 16."""
    rng = np.random.default_rng(11)
    img = _six_values(40, 30, 12)
    above = below = 0
    for _ in range(64):
        mask = rng.integers(-128, 128, (3, 3)).astype(i8)
        if rng.random() < 0.5:
            mask = rng.choice(np.array([-128, -127, 127, 100, -100], i8), (3, 3))
        s = hb.conv_sum(img, mask).astype(i64)
        padded = np.pad(img, 1, mode="edge").astype(i64)
        assert np.array_equal(s, sum(int(mask[i + 1, j + 1]) * padded[1 + i:31 + i, 1 + j:41 + j] for i in (-1, 0, 1) for j in (-1, 0, 1)))
        a16, a32 = hb.run("conv3x3a16", img, mask), hb.run("conv3x3a32", img, mask)
        w = ((s + 32768) & 0xffff) - 32768
        fits = (s >= -32768) & (s < 32768)
        assert np.array_equal(w == s, fits)
        assert np.array_equal(a16[fits], a32[fits])
        assert np.array_equal(a16, np.clip(w >> 4, 0, 255)) and np.array_equal(a32, np.clip(s >> 4, 0, 255))
        hi, lo = (s >= 32768) & (s < 65536), (s >= -65536) & (s < -32768)
        assert (a16[hi] == 0).all() and (a32[hi] == 255).all()
        assert np.array_equal(a16[lo] != a32[lo], w[lo] >= 16)
        above, below = above + int(hi.sum()), below + int(lo.sum())
    assert above > 1000 and below > 1000
    # the driver's mask never wraps: its extreme sums are 7650 and -3825
    m = hb.DRIVER_MASK.astype(i64)
    assert 255 * m[m > 0].sum() == 7650 and 255 * m[m < 0].sum() == -3825


def test_the_trap_gaussian5x5_truncates_and_does_not_round():
    """one pixel of 255 in a field of 0: floor(255 wi wj / 256); a round-to-nearest evaluation differs"""
    img = np.zeros((9, 9), u8)
    img[4, 4] = 255
    k = np.array([1, 4, 6, 4, 1], i64)
    table = 255 * np.outer(k, k)
    for verify in (False, True):
        got = hb.run("gaussian5x5", img, verify=verify)
        assert np.array_equal(got[2:7, 2:7], table // 256) and got.sum() == (table // 256).sum()
    assert not np.array_equal((table + 128) // 256, table // 256)
    assert (table // 256)[2, 2] == 35 and ((table + 128) // 256)[2, 2] == 36


@pytest.mark.parametrize("v", [0, 1, 127, 128, 254, 255])
def test_constant_images_come_back_unchanged(v):
    """gaussian5x5 included: 256 v wraps in int16 from v = 128 on, and the shift and the cast undo it; nothing is clamped"""
    img = np.full((7, 11), v, u8)
    for name in ("dilate3x3", "median3x3", "gaussian5x5"):
        for verify in (False, True):
            assert (hb.run(name, img, region=(-3, -3, 17, 13), verify=verify) == v).all(), name
    assert (hb.run("sobel", img) == 0).all()
    ident = np.zeros((3, 3), i8)
    ident[1, 1] = 16
    for name in MASKED:
        assert (hb.run(name, img, ident) == v).all()


def test_sobel_saturates_at_255_and_reaches_it():
    img = np.zeros((8, 8), u8)
    img[:, 4:] = 255            # a vertical edge: |gy| = 4 * 255 beside it
    out = hb.run("sobel", img)
    assert out.max() == 255 and (out[:, 3:5] == 255).all() and (out[:, :2] == 0).all()
    img = np.zeros((8, 8), u8)
    img[:, 4:] = 60             # 4 * 60 = 240 < 255: not saturated; 64 gives 256 -> 255
    assert (hb.run("sobel", img)[:, 3:5] == 240).all()
    img[:, 4:] = 64
    assert (hb.run("sobel", img)[:, 3:5] == 255).all()
    assert (_np_eval("sobel", img)[:, 3:5] == 255).all()


def test_sobel_of_the_transpose_is_the_transpose():
    for img in (_noise(23, 17, 21), _six_values(16, 9, 22)):
        a = hb.run("sobel", img)
        b = hb.run("sobel", np.ascontiguousarray(img.T))
        _same(np.ascontiguousarray(b.T), a, "transpose")


def test_reads_clamp_into_the_inputs_box_not_the_outputs():
    """an output larger than the input, or wholly outside it, reads only clamped samples"""
    img = _noise(5, 4, 31)
    padded = np.pad(img, 6, mode="edge")
    for name in NAMES:
        mask = _mask_for(name)
        big = hb.run(name, img, mask, (-4, -4, 13, 12))
        _same(big, np.ascontiguousarray(hb.run(name, padded, mask)[2:14, 2:15]), name)
    one = np.array([[77]], u8)
    assert (hb.run("gaussian5x5", one, region=(0, 0, 70, 9)) == 77).all()
    assert (hb.run("sobel", one, region=(-30, 40, 70, 9)) == 0).all()


# ---------------------------------------------------------------------------------------------------- CPU: the library's surface
def _arg_names(name):
    return ["input", "mask", "output"] if name in MASKED else ["input", "output"]


@pytest.mark.parametrize("name", NAMES)
def test_the_entry_points_are_exported_with_argv_and_metadata(hl, name):
    lib = C.CDLL(hl.LIB_PATH)
    for suffix in ("", "_argv", "_metadata"):
        assert hasattr(lib, name + suffix), name + suffix
    assert not hasattr(lib, name + "_auto_schedule")
    assert hasattr(lib, "hlmi_hexagon_benchmarks_general")
    assert hl._fn[name] is not None and callable(getattr(hl, name)) and callable(hl.debug_hexagon_benchmarks_general)
    assert hl.HEXAGON_BENCHMARKS == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_metadata_states_the_arguments_without_estimates(hl, name):
    md = hl.metadata(name)
    names = _arg_names(name)
    assert md.version == 1 and md.num_arguments == len(names) and md.name.decode() == name and b"hip" in md.target
    a = [md.arguments[i] for i in range(len(names))]
    assert [x.name.decode() for x in a] == names
    assert [x.kind for x in a] == [1] * (len(names) - 1) + [2]
    assert [(x.type.code, x.type.bits) for x in a] == ([(1, 8), (0, 8), (1, 8)] if name in MASKED else [(1, 8), (1, 8)])
    assert [x.dimensions for x in a] == [2] * len(names)
    for x in a:   # the generators declare no estimates
        assert not x.buffer_estimates or all(not x.buffer_estimates[i] for i in range(4))
        assert not x.scalar_def and not x.scalar_min and not x.scalar_max and not x.scalar_estimate


@pytest.mark.parametrize("name", NAMES)
def test_the_aot_headers_compile_as_c(tmp_path, name):
    decl = " ".join(open(os.path.join(ROOT, "include", "hlmi_pipelines.h")).read().split())
    B = "struct halide_buffer_t *"
    assert f"int {name}(" + ", ".join(B + n for n in _arg_names(name)) + ");" in decl
    src = tmp_path / "c.c"
    sig = ", ".join([B.strip()] * len(_arg_names(name)))
    src.write_text(f'#include "aot/{name}.h"\nint (*const f)({sig}) = {name};\nint (*const a)(void **) = {name}_argv;\n'
                   f"const struct halide_filter_metadata_t *(*const m)(void) = {name}_metadata;\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "c.o")], check=True)


@pytest.mark.parametrize("name", NAMES)
def test_runner_describes_each_filter_by_name(name):
    out = subprocess.run([RUNGEN, f"--name={name}", "--describe"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'Input "input" is of type Buffer<uint8> with 2 dimensions' in out.stdout
    assert ('Input "mask" is of type Buffer<int8> with 2 dimensions' in out.stdout) == (name in MASKED)
    assert 'Output "output" is of type Buffer<uint8> with 2 dimensions' in out.stdout


# ---------------------------------------------------------------------------------------------------- CPU: the entry protocol
HOW = pytest.mark.parametrize("how", [call_direct, call_argv], ids=["direct_call", "argv"])
W0, H0 = 20, 6


def _mk(hl, shape=(H0, W0), dtype=u8, mins=None):
    return hl.Buffer(np.zeros(shape, dtype), mins=mins)


def _call(hl, how, name, **over):
    """the entry point on a W0 x H0 input, a 3 x 3 mask and a W0 x H0 output, with the named arguments replaced"""
    args = {"input": _mk(hl), "mask": _mk(hl, (3, 3), i8), "output": _mk(hl)}
    args.update(over)
    return how(hl, name, *[args[n] for n in _arg_names(name)])


@HOW
@pytest.mark.parametrize("name", NAMES)
def test_entry_protocol(hl, how, name):
    ok = 0 if _gpu_present() else -29   # with everything in order only the device can be missing
    call = lambda **over: _call(hl, how, name, **over)
    names = _arg_names(name)
    other = lambda n: (3, 3) if n == "mask" else (H0, W0)
    assert call() == ok
    for n in names:
        assert call(**{n: None}) == -12 and n in hl.last_error()
    for n in names:
        assert call(**{n: _mk(hl, other(n), np.uint16)}) == -3 and n in hl.last_error()
    assert call(input=_mk(hl, dtype=i8)) == -3 and call(output=_mk(hl, dtype=i8)) == -3
    if name in MASKED:
        assert call(mask=_mk(hl, (3, 3), u8)) == -3 and "mask" in hl.last_error()
    for n in names:
        assert call(**{n: _mk(hl, (2,) + other(n), i8 if n == "mask" else u8)}) == -43 and n in hl.last_error()
    # order: null, then a buffer's type, then its dimensionality, then the pinned mins, then sizes and coverage
    assert call(input=None, output=_mk(hl, dtype=np.uint16)) == -12
    assert call(input=_mk(hl, (2, H0, W0), np.uint16)) == -3
    assert call(input=_mk(hl, (2, H0, W0)), output=_mk(hl, mins=(1, 0))) == -43
    for d in (0, 1):
        mins = tuple(3 if i == d else 0 for i in range(2))
        assert call(input=_mk(hl, mins=mins)) == -8 and f"input.min.{d}" in hl.last_error()
        assert call(input=_mk(hl, mins=tuple(-m for m in mins))) == -8
        if name != "sobel":
            assert call(output=_mk(hl, mins=mins)) == -8 and f"output.min.{d}" in hl.last_error()
            assert call(output=_mk(hl, mins=tuple(-m for m in mins))) == -8
    empty = lambda cut: hl.Buffer(np.zeros((H0, W0), u8)[cut])   # an empty view: the strides stay
    assert call(input=_mk(hl, mins=(1, 0)), output=empty(np.s_[:, :0])) == -8     # a pinned min before anything else
    assert call(input=_mk(hl, mins=(0, 2)), **({"mask": _mk(hl, (2, 3), i8)} if name in MASKED else {})) == -8   # and before coverage
    strided = lambda: hl.Buffer(np.zeros((H0, 2 * W0), u8)[..., ::2])   # stride.0 == 2
    assert call(input=strided()) == -8 and "input.stride.0" in hl.last_error()
    assert call(output=strided()) == -8 and "output.stride.0" in hl.last_error()
    # an input the clamp cannot serve: an empty one
    assert call(input=empty(np.s_[:, :0])) == -4 and "input" in hl.last_error()
    assert call(input=empty(np.s_[:0])) == -4 and "input" in hl.last_error()
    if name in MASKED:   # the mask covers [0, 3) x [0, 3); its mins and strides are otherwise free
        for bad in (_mk(hl, (3, 2), i8), _mk(hl, (2, 3), i8), _mk(hl, (3, 3), i8, mins=(1, 0)), _mk(hl, (3, 3), i8, mins=(0, -1)),
                    _mk(hl, (4, 4), i8, mins=(-2, 0))):
            assert call(mask=bad) == -4 and "mask" in hl.last_error()
        assert call(mask=_mk(hl, (5, 5), i8, mins=(-1, -2))) == ok
        assert call(mask=hl.Buffer(np.zeros((5, 11), i8)[:, :5], mins=(-2, -2))) == ok
        assert call(input=strided(), mask=_mk(hl, (2, 3), i8)) == -8   # a constraint before coverage
    # the output's extents are the caller's: smaller, larger, one pixel, empty
    for shape in ((H0 - 2, W0 - 3), (H0 + 9, W0 + 70), (1, 1)):
        assert call(output=_mk(hl, shape)) == ok
    assert call(output=empty(np.s_[:, :0])) == ok and call(output=empty(np.s_[:0])) == ok
    assert call(input=_mk(hl, (1, 1)), output=_mk(hl, (9, 70))) == ok


@HOW
def test_sobel_accepts_the_output_origin_the_others_refuse(hl, how):
    ok = 0 if _gpu_present() else -29
    for mins in ((5, 0), (0, -7), (-40, 30), (W0 + 8, H0 + 8), (-2 ** 20, 2 ** 20)):
        assert _call(hl, how, "sobel", output=_mk(hl, mins=mins)) == ok, mins
        for name in NAMES:
            if name != "sobel":
                assert _call(hl, how, name, output=_mk(hl, mins=mins)) == -8, (name, mins)
                assert "output.min." in hl.last_error()


def test_sizes_beyond_one_launch_and_beyond_int32_are_refused(hl):
    """-5 / -6 come from the shared shape checks (|extent * stride| and the product of extents below 2^31), before any device is
    asked for; shapes are given through bounds-query-like descriptors that own no memory, so nothing that large is allocated"""
    def shaped(extents, strides):
        b = hl.Buffer(np.zeros((1, 1), u8))
        for i in range(2):
            b.dim(i).extent, b.dim(i).stride = extents[i], strides[i]
        return b
    for name in NAMES:
        extra = [_mk(hl, (3, 3), i8)] if name in MASKED else []
        assert call_direct(hl, name, _mk(hl), *extra, shaped((70000, 70000), (1, 70000))) in (-5, -6)
        assert call_direct(hl, name, _mk(hl), *extra, shaped((2, 2 ** 30), (1, 4))) == -5
        assert call_direct(hl, name, shaped((2 ** 16, 2 ** 16), (1, 2 ** 16)), *extra, _mk(hl)) in (-5, -6)


@HOW
@pytest.mark.parametrize("name", NAMES)
def test_bounds_queries_leave_input_and_output_and_answer_the_mask(hl, how, name):
    dims = lambda b: [(b.raw.dim[i].min, b.raw.dim[i].extent) for i in range(b.raw.dimensions)]
    out_min = (-3, 2) if name == "sobel" else (0, 0)
    # the input asked for: the clamp's bound is the input's own box, so it stays as passed
    q, o = hl.Buffer.bounds_query(u8, 2, mins=(0, 0), extents=(14, 15)), _mk(hl, mins=out_min)
    assert _call(hl, how, name, input=q, output=o) == 0
    assert dims(q) == [(0, 14), (0, 15)] and dims(o) == [(out_min[0], W0), (out_min[1], H0)]
    # the output asked for: the request, as passed
    q = hl.Buffer.bounds_query(u8, 2, mins=out_min, extents=(30, 40))
    assert _call(hl, how, name, output=q) == 0 and dims(q) == [(out_min[0], 30), (out_min[1], 40)]
    if name in MASKED:
        q, o = hl.Buffer.bounds_query(i8, 2, mins=(11, 12), extents=(14, 15)), _mk(hl)
        assert _call(hl, how, name, mask=q, output=o) == 0 and dims(q) == [(0, 3), (0, 3)] and dims(o) == [(0, W0), (0, H0)]
        assert [q.raw.dim[i].stride for i in range(2)] == [1, 3]
        q = hl.Buffer.bounds_query(np.uint16, 2)   # a wrong type is rewritten
        assert _call(hl, how, name, mask=q) == 0 and dims(q) == [(0, 3), (0, 3)] and (q.raw.type.code, q.raw.type.bits) == (0, 8)
    # a query with the wrong dimensionality stays an error, and the pinned mins hold in a query too
    assert _call(hl, how, name, input=hl.Buffer.bounds_query(u8, 3)) == -43
    assert _call(hl, how, name, input=hl.Buffer.bounds_query(u8, 2, mins=(1, 0), extents=(4, 4))) == -8


def test_without_a_gpu_the_python_calls_refuse_to_run(hl):
    if _gpu_present():
        return   # the statement is about a machine without one
    a, m, o = _mk(hl), _mk(hl, (3, 3), i8), _mk(hl)
    for name in NAMES:
        args = [a, m, o] if name in MASKED else [a, o]
        for fn in (lambda: getattr(hl, name)(*args), lambda: hl.debug_hexagon_benchmarks_general(name, a, m if name in MASKED else None, o)):
            with pytest.raises(hl.HalideError) as e:
                fn()
            assert e.value.code == -29
    with pytest.raises(hl.HalideError) as e:
        hl.debug_hexagon_benchmarks_general("erode3x3", a, None, o)
    assert e.value.code == -8


@pytest.mark.parametrize("name", NAMES)
def test_torch_shape_functions_and_refusals(name):
    import torch
    import halide_amd.torch_ops  # noqa: F401
    op = getattr(torch.ops.hlmi, name)
    extra = [torch.empty((3, 3), dtype=torch.int8, device="meta")] if name in MASKED else []
    out = op(torch.empty((45, 70), dtype=torch.uint8, device="meta"), *extra)
    assert out.shape == (45, 70) and out.dtype == torch.uint8
    img, mask = torch.zeros((8, 9), dtype=torch.uint8), [torch.zeros((3, 3), dtype=torch.int8)] if name in MASKED else []
    with pytest.raises(RuntimeError, match="GPU"):
        op(img, *mask)
    for bad in (img.float(), torch.zeros((2, 8, 9), dtype=torch.uint8), torch.zeros(9, dtype=torch.uint8)):
        with pytest.raises(TypeError):
            op(bad, *mask)
    if name in MASKED:
        for bad in (torch.zeros((3, 3), dtype=torch.uint8), torch.zeros((3, 4), dtype=torch.int8), torch.zeros(9, dtype=torch.int8)):
            with pytest.raises(TypeError):
                op(img, bad)


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(params=["default", "general"])
def general(request):
    """Both implementations (halide_amd/csrc/hexagon_benchmarks.hip): the sliding kernel every shape takes, and one thread per
    output pixel through the hook."""
    return request.param == "general"


def _strided(h, w, row_pad=0):
    """a zeroed uint8 (H, W) view with rows row_pad longer than W (the device allocation mirrors the strides)"""
    return np.lib.stride_tricks.as_strided(np.zeros(h * (w + row_pad) + 8, u8), (h, w), (w + row_pad, 1))


def _run(hl, name, a, m, o, general):
    if general:
        hl.debug_hexagon_benchmarks_general(name, a, m, o)
    else:
        getattr(hl, name)(*([a, m, o] if name in MASKED else [a, o]))


def _gpu(hl, name, img, mask=None, region=None, general=False, in_pad=0, out_pad=0):
    """the call on host buffers with rows in_pad / out_pad longer than the planes; returns the output region, contiguous"""
    ih, iw = img.shape
    ox, oy, ow, oh = region if region is not None else (0, 0, iw, ih)
    src = _strided(ih, iw, in_pad)
    src[...] = img
    o = hl.Buffer(_strided(oh, ow, out_pad), mins=(ox, oy))
    _run(hl, name, hl.Buffer(src), None if mask is None else hl.Buffer(np.ascontiguousarray(mask, i8)), o, general)
    return np.ascontiguousarray(o.numpy())


def _gpu_dev(hl, name, img, mask=None, region=None, general=False, in_layout=(None, 0), out_layout=(None, 0)):
    """the call on planes inside device allocations of their own: layout = (row stride or None for dense, byte offset of the first
    element); also asserts that no byte outside the output plane was written"""
    ih, iw = img.shape
    ox, oy, ow, oh = region if region is not None else (0, 0, iw, ih)
    a, o = hb.DevPlane(hl, ih, iw, *in_layout, fill=img), hb.DevPlane(hl, oh, ow, *out_layout, mins=(ox, oy))
    try:
        _run(hl, name, a.buf, None if mask is None else hl.Buffer(np.ascontiguousarray(mask, i8)), o.buf, general)
        return o.result()
    finally:
        a.free(), o.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_the_drivers_setting_shrunk(hl, driver_scene, on_stream, general, name):
    img, want = driver_scene
    _same(_gpu(hl, name, img, _mask_for(name), general=general), want[name], name)


# Widths on both sides of a lane's word (8), of two and of eight words, and of a wave's span (OUT_LANES words; a workgroup's is the
# same); heights on both sides of the window (3 or 5 rows), of the rows a wave slides over and of a workgroup's rows.
WIDTHS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, WAVE_PX - 1, WAVE_PX, WAVE_PX + 1, WAVE_PX + 8, 2 * WAVE_PX + 8]
HEIGHTS = [1, 2, 3, 4, 5, ROWS - 1, ROWS, ROWS + 1, GROUP_ROWS - 1, GROUP_ROWS, GROUP_ROWS + 1]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_widths_and_heights(hl, on_stream, general, name):
    mask = _mask_for(name)
    for w in WIDTHS:
        for h in (HEIGHTS if w in (8, 17, 64, WAVE_PX, WAVE_PX + 8) else [1, 3, ROWS + 1]):
            img = _noise(w, h, 1000 * w + h)
            _same(_gpu(hl, name, img, mask, general=general), hb.run(name, img, mask), f"{name} {w} x {h}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_row_strides_and_base_pointers(hl, on_stream, general, name):
    """row strides that are no multiple of 8, for input and output separately; base pointers at byte offsets 1 .. 7, likewise; widths
    that would take the 8-byte path if the layout allowed it and widths that would not"""
    mask = _mask_for(name)
    for w, h in ((WAVE_PX + 8, ROWS + 3), (64, 5), (67, 9)):
        img = _noise(w, h, 7 * w + h)
        want = hb.run(name, img, mask)
        for in_pad, out_pad in ((0, 0), (8, 16), (1, 0), (0, 3), (5, 11), (8, 0), (0, 8)):
            _same(_gpu(hl, name, img, mask, None, general, in_pad, out_pad), want, f"{name} {w} x {h} row pads {in_pad}, {out_pad}")
        for off in range(1, 8):
            _same(_gpu_dev(hl, name, img, mask, None, general, (None, off), (None, 0)), want, f"{name} {w} x {h} input at byte {off}")
            _same(_gpu_dev(hl, name, img, mask, None, general, (None, 0), (None, off)), want, f"{name} {w} x {h} output at byte {off}")
        _same(_gpu_dev(hl, name, img, mask, None, general, (w + 8, 8), (w + 16, 16)), want, f"{name} {w} x {h} both on the grid, off the start")
        _same(_gpu_dev(hl, name, img, mask, None, general, (w + 3, 5), (w + 1, 3)), want, f"{name} {w} x {h} both off the grid")


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_outputs_larger_than_the_input(hl, on_stream, general, name):
    mask = _mask_for(name)
    for (iw, ih), (ow, oh) in (((1, 1), (70, 9)), ((64, 5), (WAVE_PX + 16, 12)), ((8, 3), (8 * 70, ROWS + 2)), ((40, 33), (24, 8)),
                               ((WAVE_PX + 16, 9), (2 * WAVE_PX, 20)), ((9, 40), (100, 70))):
        img = _noise(iw, ih, 31 * iw + ih)
        _same(_gpu(hl, name, img, mask, (0, 0, ow, oh), general), hb.run(name, img, mask, (0, 0, ow, oh)), f"{name} {iw} x {ih} under {ow} x {oh}")


@pytest.mark.gpu
def test_sobel_at_origins_that_are_negative_and_past_the_input(hl, on_stream, general):
    for (iw, ih), regions in (((64, 12), [(-8, -3, 88, 20), (-16, 5, 16, 4), (-600, -40, 560, 9), (64, 12, 40, 5), (72, 0, 8, 12), (-3, -2, 70, 16),
                                          (5, 1, 64, 12), (24, -20, 32, 50)]),
                              ((2 * WAVE_PX, 9), [(-8, 0, 2 * WAVE_PX + 16, 9), (8, -1, 2 * WAVE_PX, 11), (WAVE_PX, 2, WAVE_PX + 64, 5), (-1, 0, 2 * WAVE_PX, 9)]),
                              ((1, 1), [(-30, 40, 70, 9)])):
        img = _noise(iw, ih, iw + ih)
        for region in regions:
            _same(_gpu(hl, "sobel", img, None, region, general), hb.run("sobel", img, None, region), f"{iw} x {ih} region {region}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", MASKED)
def test_masks(hl, on_stream, general, name):
    rng = np.random.default_rng(5)
    img = _noise(WAVE_PX + 24, 11, 41)
    ones = np.full((7, 72), 255, u8)
    # the pinned example: all 255 under all 16
    _same(_gpu(hl, name, ones, ALL16, general=general), np.full((7, 72), 0 if name == "conv3x3a16" else 255, u8), "all 255 under all 16")
    masks = [hb.DRIVER_MASK, ALL16, np.full((3, 3), -128, i8), np.full((3, 3), 127, i8)] + [rng.integers(-128, 128, (3, 3)).astype(i8) for _ in range(12)]
    masks += [rng.choice(np.array([-128, -127, 127], i8), (3, 3)) for _ in range(4)]
    for mask in masks:
        for im in (img, ones, _six_values(65, 9, 42)):
            _same(_gpu(hl, name, im, mask, general=general), hb.run(name, im, mask), f"{name} mask {mask.tolist()}")
    # a mask buffer with negative mins, extent 5 and a row stride of 11
    box = rng.integers(-128, 128, (5, 11)).astype(i8)
    box[2:5, 1:4] = hb.DRIVER_MASK
    src, o = hl.Buffer(img.copy()), hl.Buffer(np.zeros_like(img))
    _run(hl, name, src, hl.Buffer(box[:, :5], mins=(-1, -2)), o, general)
    _same(o.numpy(), hb.run(name, img, hb.DRIVER_MASK), "mask box")


@pytest.mark.gpu
def test_default_equals_general_and_both_launch_what_they_say(hl):
    for name in NAMES:
        mask = _mask_for(name)
        for w, h in ((WAVE_PX + 8, ROWS + 1), (3, 1)):   # one launch for every shape
            img = _noise(w, h, 51)
            outs = {}
            for general, kernel in ((False, "hb_" + name), (True, "hb_" + name + "_general")):
                assert _launches(hl, lambda: outs.__setitem__(general, _gpu(hl, name, img, mask, general=general))) == [kernel]
            _same(outs[False], outs[True], f"{name} {w} x {h}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_an_empty_output_launches_nothing(hl, on_stream, general, name):
    a, m = hl.Buffer(_noise(9, 5, 1)), hl.Buffer(hb.DRIVER_MASK.copy()) if name in MASKED else None
    for cut in (np.s_[:, :0], np.s_[:0]):
        o = hl.Buffer(np.zeros((5, 5), u8)[cut])   # an empty view: the strides stay
        assert _launches(hl, lambda: _run(hl, name, a, m, o, general)) == []


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_argv_equals_the_direct_call(hl, on_stream, driver_scene, name):
    img, want = driver_scene
    outs = []
    for how in (call_direct, call_argv):
        o = hl.Buffer(np.zeros_like(img))
        extra = [hl.Buffer(hb.DRIVER_MASK.copy())] if name in MASKED else []
        assert how(hl, name, hl.Buffer(img.copy()), *extra, o) == 0
        outs.append(np.ascontiguousarray(o.numpy()))
    _same(outs[1], outs[0], "argv")
    _same(outs[0], want[name], "direct")


@pytest.mark.gpu
def test_a_host_dirty_buffer_without_host_memory_is_refused(hl):
    """-34, the last of the reference's checks: everything else in order, a device there, and an input whose newer copy is said to
    be on a host that is not there"""
    img = _noise(9, 5, 1)
    a, o = hb.DevPlane(hl, 5, 9, fill=img), hl.Buffer(np.zeros((5, 9), u8))
    try:
        assert call_direct(hl, "dilate3x3", a.buf, o) == 0
        _same(o.numpy(), hb.run("dilate3x3", img), "device-only input")
        a.buf.set_host_dirty()
        for name in NAMES:
            extra = [hl.Buffer(hb.DRIVER_MASK.copy())] if name in MASKED else []
            assert call_direct(hl, name, a.buf, *extra, o) == -34 and "input" in hl.last_error()
    finally:
        a.buf.set_host_dirty(False)
        a.free()


@pytest.mark.gpu
def test_more_workgroups_than_one_launch_holds_are_refused(hl):
    """-6 from the launch itself: the sliding kernel takes GROUP_ROWS rows per workgroup row, the general one a single row, and a grid
    holds 65535 workgroup rows"""
    a = hl.Buffer(_noise(4, 4, 1))
    tall = hl.Buffer(np.zeros((65536, 1), u8))
    assert call_direct(hl, "dilate3x3", a, tall) == 0
    _same(tall.numpy(), hb.run("dilate3x3", a.array, region=(0, 0, 1, 65536)), "65536 rows")
    with pytest.raises(hl.HalideError) as e:
        hl.debug_hexagon_benchmarks_general("dilate3x3", a, None, tall)
    assert e.value.code == -6
    taller = hl.Buffer(np.zeros((65535 * GROUP_ROWS + 1, 1), u8))
    for name in NAMES:
        extra = [hl.Buffer(hb.DRIVER_MASK.copy())] if name in MASKED else []
        assert call_direct(hl, name, a, *extra, taller) == -6


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_torch_ops_equal_the_checker(hl, name):
    import torch
    import halide_amd.torch_ops  # noqa: F401
    op = getattr(torch.ops.hlmi, name)
    mask = _mask_for(name)
    for w, h in ((160, 24), (WAVE_PX + 9, 5)):
        img = _noise(w, h, 61)
        t = torch.from_numpy(img).cuda()
        extra = [torch.from_numpy(mask.copy()).cuda()] if mask is not None else []
        out = op(t, *extra)
        torch.cuda.synchronize()
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (h, w)
        _same(out.cpu().contiguous().numpy(), hb.run(name, img, mask), f"torch {name} {w} x {h}")
        assert np.array_equal(t.cpu().numpy(), img)
        # a view with longer rows and a first element off the 8-byte grid
        big = torch.zeros((h + 2, w + 13), dtype=torch.uint8).cuda()
        big[1:h + 1, 3:w + 3] = t
        _same(op(big[1:h + 1, 3:w + 3], *extra).cpu().contiguous().numpy(), hb.run(name, img, mask), f"torch view {name} {w} x {h}")


@pytest.mark.gpu
def test_calls_from_8_host_threads(hl):
    """eight threads on the library's shared stream, each with its own filter, image, mask and size"""
    rng = np.random.default_rng(8)
    jobs = []
    for i in range(8):
        name = NAMES[i % len(NAMES)]
        img = _noise(500 + 9 * i, 6 + i, 70 + i)
        mask = rng.integers(-128, 128, (3, 3)).astype(i8) if name in MASKED else None
        jobs.append((name, img, mask, hb.run(name, img, mask)))
    errors = []

    def worker(i):
        try:
            name, img, mask, want = jobs[i]
            for rep in range(4):
                if not np.array_equal(_gpu(hl, name, img, mask, general=rep % 2 == 1), want):
                    errors.append(f"thread {i} rep {rep}: differs")
        except Exception as e:  # noqa: BLE001
            errors.append(f"thread {i}: {e!r}")

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


@pytest.mark.gpu
def test_seeded_fuzz_slice_of_hexagon_benchmarks(on_stream):
    """scripts/fuzz_parity.py's hexagon_benchmarks case, a fixed number of cases from a fixed seed"""
    mod = load_fuzz_parity()
    rng = np.random.default_rng(20261019)
    for i in range(60):
        desc, ok = mod.CASES["hexagon_benchmarks"](rng)
        assert ok, f"case {i}: {desc}"
