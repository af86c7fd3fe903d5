"""haar_x, inverse_haar_x, daubechies_x and inverse_daubechies_x: the one-level horizontal wavelet transforms of apps/wavelet.

The checker is tests/cpp/wavelet_check.c, a plain C restatement of apps/wavelet/haar_x_generator.cpp:15-21,
inverse_haar_x_generator.cpp:15-20, daubechies_x_generator.cpp:15-20, inverse_daubechies_x_generator.cpp:15-20 and
daubechies_constants.h:4-7 in both canonical float forms, built and driven through ctypes by tests/wavelet_checker.py; it takes the
fused helpers and the integer division from oracle/oracle_common.h.  The CPU tests hold the checker to a numpy float64 evaluation
and to properties that follow from the generators' text, and the entry points to their contract; the GPU tests hold the library to
the checker bit for bit.  Like every float pipeline here, the two are pinned to this repository's restatement only: no output of a
real Halide build is involved."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import wavelet_checker as wc
from parity_helpers import ROOT, RUNGEN, call_argv, call_direct, load_fuzz_parity, noise
from parity_helpers import gpu_present as _gpu_present, launches as _launches, same_bits as _same

NAMES = list(wc.NAMES)
FORWARD, INVERSE = [n for n in NAMES if not wc.is_inverse(n)], [n for n in NAMES if wc.is_inverse(n)]
f32 = np.float32
U = 2.0 ** -24   # the unit roundoff of binary32


# ---------------------------------------------------------------------------------------------------- the checker
@pytest.fixture(params=[0, 1], ids=["canon0", "canon1"])
def each_canon_wc(request):
    with wc.canon(request.param):
        yield request.param


@pytest.fixture
def canon_wc(hl):
    """the checker in the form the loaded library was built for"""
    with wc.canon(hl.canon_fma()):
        yield wc


# ---------------------------------------------------------------------------------------------------- CPU: the library's surface
def test_the_entry_points_are_exported_with_argv_and_metadata(hl):
    lib = C.CDLL(hl.LIB_PATH)
    for name in NAMES:
        for suffix in ("", "_argv", "_metadata"):
            assert hasattr(lib, name + suffix), name + suffix
        assert not hasattr(lib, name + "_auto_schedule")   # the reference builds no such object
        assert hl._fn[name] is not None
        md = hl.metadata(name)
        assert md.version == 1 and md.num_arguments == 2 and md.name.decode() == name and b"hip" in md.target
        a = [md.arguments[i] for i in range(2)]
        assert [x.name.decode() for x in a] == ["in", "out"] and [x.kind for x in a] == [1, 2]
        assert [x.dimensions for x in a] == ([3, 2] if wc.is_inverse(name) else [2, 3])
        assert [(x.type.code, x.type.bits) for x in a] == [(2, 32), (2, 32)]
        for x in a:   # the generators declare no estimates
            assert not x.buffer_estimates and not x.scalar_def and not x.scalar_min and not x.scalar_max and not x.scalar_estimate
    assert hasattr(lib, "hlmi_wavelet_general")


def test_the_aot_headers_compile_as_c(tmp_path):
    decl = open(os.path.join(ROOT, "include", "hlmi_pipelines.h")).read()
    inc = ["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c"]
    for name in NAMES:
        assert f"int {name}(struct halide_buffer_t *in, struct halide_buffer_t *out);" in decl
    src = tmp_path / "all.c"
    src.write_text("".join(f'#include "aot/{n}.h"\n' for n in NAMES)
                   + "".join(f"int (*const f_{n})(struct halide_buffer_t *, struct halide_buffer_t *) = {n};\nint (*const a_{n})(void **) = {n}_argv;\n"
                             f"const struct halide_filter_metadata_t *(*const m_{n})(void) = {n}_metadata;\n" for n in NAMES))
    subprocess.run(inc + [str(src), "-o", str(tmp_path / "all.o")], check=True)
    for name in NAMES:   # each alone, too
        one = tmp_path / (name + ".c")
        one.write_text(f'#include "aot/{name}.h"\nint (*const a)(void **) = {name}_argv;\n')
        subprocess.run(inc + [str(one), "-o", str(tmp_path / (name + ".o"))], check=True)


@pytest.mark.parametrize("name", NAMES)
def test_runner_describes_each_by_name(name):
    out = subprocess.run([RUNGEN, f"--name={name}", "--describe"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    din, dout = (3, 2) if wc.is_inverse(name) else (2, 3)
    assert f'Input "in" is of type Buffer<float32> with {din} dimensions' in out.stdout
    assert f'Output "out" is of type Buffer<float32> with {dout} dimensions' in out.stdout


# ---------------------------------------------------------------------------------------------------- CPU: the entry protocol
HOW = pytest.mark.parametrize("how", [call_direct, call_argv], ids=["direct_call", "argv"])


def _shapes(name):
    """(input shape, output shape) of the driver's call on a 80 x 32 image, numpy order"""
    return ((2, 32, 40), (32, 80)) if wc.is_inverse(name) else ((32, 80), (2, 32, 40))


@HOW
@pytest.mark.parametrize("name", NAMES)
def test_entry_protocol(hl, name, how):
    ok = 0 if _gpu_present() else -29   # with everything in order only the device can be missing
    si, so = _shapes(name)
    mk = lambda shape, dtype=f32, mins=None: hl.Buffer(np.zeros(shape, dtype), mins=mins)
    strided = lambda shape: hl.Buffer(np.zeros(shape[:-1] + (2 * shape[-1],), f32)[..., ::2])   # stride.0 == 2
    call = lambda i, o: how(hl, name, i, o)
    assert call(None, mk(so)) == -12 and call(mk(si), None) == -12
    assert call(mk(si, np.uint16), mk(so)) == -3 and call(mk(si), mk(so, np.uint16)) == -3
    # a 3-D input to the forwards, a 2-D input to the inverses; the same on the output side
    assert call(mk(so), mk(so)) == -43 and call(mk(si), mk(si)) == -43
    assert call(strided(si), mk(so)) == -8 and "in.stride.0" in hl.last_error()
    assert call(mk(si), strided(so)) == -8 and "out.stride.0" in hl.last_error()
    # order: null before type before dimensionality before the constraints
    assert call(mk(so, np.uint16), mk(so)) == -3
    assert call(mk(so), strided(so)) == -43
    assert call(None, mk(si, np.uint16)) == -12
    # every read is clamped: any region, channel range and mins pass, with padded strides
    pad = lambda shape: np.zeros(shape[:-2] + (shape[-2] + 3, shape[-1] + 5), f32)[..., 1:1 + shape[-2], 2:2 + shape[-1]]
    far = (400, -300) if wc.is_inverse(name) else (400, -300, -7)
    assert call(hl.Buffer(pad(si)), hl.Buffer(pad(so), mins=far)) == ok
    assert call(mk(si, mins=(17, -9, 5)[:len(si)]), mk(so)) == ok
    if wc.is_inverse(name):
        assert call(mk((1, 32, 40), mins=(0, 0, 1)), mk(so)) == ok and call(mk((5, 32, 40), mins=(0, 0, -2)), mk(so)) == ok
    else:
        assert call(mk(si), mk((1, 32, 40), mins=(0, 0, 1))) == ok and call(mk(si), mk((3, 32, 40), mins=(0, 0, -1))) == ok
    # an input with an empty dimension has no edge to repeat: -4, found where gaussian_blur_direct finds it, with the device in hand;
    # nothing is read where the output is empty
    for d in range(len(si)):
        empty = lambda: hl.Buffer(np.zeros(si, f32)[tuple(slice(0, 0) if j == d else slice(None) for j in range(len(si)))])   # the strides stay
        assert call(empty(), mk(so)) == (-4 if _gpu_present() else -29), d
        if _gpu_present():
            assert "empty" in hl.last_error()
        assert call(empty(), hl.Buffer(np.zeros(so, f32)[..., :0])) == ok


@HOW
@pytest.mark.parametrize("name", NAMES)
def test_bounds_queries_leave_both_buffers_as_passed(hl, name, how):
    si, so = _shapes(name)
    dims = lambda b: [(b.raw.dim[i].min, b.raw.dim[i].extent) for i in range(b.raw.dimensions)]
    real = lambda shape, mins: hl.Buffer(np.zeros(shape, f32), mins=mins)
    query = lambda n, dtype=f32: hl.Buffer.bounds_query(dtype, n, mins=(11, 12, 13)[:n], extents=(14, 15, 16)[:n])
    ni, no = len(si), len(so)
    want_q = lambda n: [(11, 14), (12, 15), (13, 16)][:n]
    # the input asked for: every read clamps into whatever the input is, so there is nothing to tell it
    q, o = query(ni), real(so, (-3, 2, 1)[:no])
    assert how(hl, name, q, o) == 0
    assert dims(q) == want_q(ni) and dims(o) == [(m, e) for m, e in zip((-3, 2, 1), so[::-1])]
    # the output asked for: it is the request
    a, q = real(si, (2, 3, 0)[:ni]), query(no)
    assert how(hl, name, a, q) == 0
    assert dims(q) == want_q(no) and dims(a) == [(m, e) for m, e in zip((2, 3, 0), si[::-1])]
    # both (RunGen's way), one of them with the wrong type: rewritten, as for every query
    qi, qo = query(ni, np.uint8), query(no)
    assert how(hl, name, qi, qo) == 0
    assert dims(qi) == want_q(ni) and dims(qo) == want_q(no) and (qi.raw.type.code, qi.raw.type.bits) == (2, 32)
    # a query with the wrong dimensionality stays an error
    assert how(hl, name, query(no), real(so, None)) == -43


def test_without_a_gpu_the_python_calls_refuse_to_run(hl):
    a, o = hl.Buffer(np.zeros((16, 16), f32)), hl.Buffer(np.zeros((2, 16, 8), f32))
    with pytest.raises(hl.HalideError) as e:
        hl.debug_wavelet_general("compositing", a, o)
    assert e.value.code == -8
    if _gpu_present():
        return   # what follows is the statement about a machine without one
    for name in NAMES:
        i, j = (o, a) if wc.is_inverse(name) else (a, o)
        for fn in (lambda: getattr(hl, name)(i, j), lambda: hl.debug_wavelet_general(name, i, j)):
            with pytest.raises(hl.HalideError) as e:
                fn()
            assert e.value.code == -29


# ---------------------------------------------------------------------------------------------------- CPU: what follows from the text
def _mul(*v):
    """the f32 product of f32 values"""
    r = f32(v[0])
    for x in v[1:]:
        r = f32(r * f32(x))
    return r


def test_the_constants_are_the_d4_taps():
    d = wc.constants()
    s2, s3 = np.sqrt(2.0), np.sqrt(3.0)
    want = [(1 + s3) / (4 * s2), (3 + s3) / (4 * s2), (3 - s3) / (4 * s2), (1 - s3) / (4 * s2)]
    assert [float(x) for x in d] == [float(f32(x)) for x in want] and d[3] < 0


def test_an_impulse_pins_the_taps_of_the_forward_transforms(each_canon_wc):
    D = wc.constants()
    img = np.zeros((3, 24), f32)
    img[1, 11] = 1.0   # x = 2k + 1, k = 5
    out = wc.forward("daubechies_x", img)
    lo, hi = out[0, 1], out[1, 1]
    assert not out[:, 0].any() and not out[:, 2].any()
    # lo(x) = D0 in(2x - 1) + D1 in(2x) + D2 in(2x + 1) + D3 in(2x + 2): sample 2k + 1 is tap D2 of pair k and tap D0 of pair k + 1
    assert list(np.nonzero(lo)[0]) == [5, 6] and lo[5] == D[2] and lo[6] == D[0]
    # hi(x) = D3 in(2x - 1) - D2 in(2x) + D1 in(2x + 1) - D0 in(2x + 2)
    assert list(np.nonzero(hi)[0]) == [5, 6] and hi[5] == D[1] and hi[6] == D[3]
    img[:] = 0
    img[1, 10] = 1.0   # x = 2k: tap D1 / -D2 of pair k, tap D3 / -D0 of pair k - 1
    out = wc.forward("daubechies_x", img)
    assert list(np.nonzero(out[0, 1])[0]) == [4, 5] and out[0, 1, 4] == D[3] and out[0, 1, 5] == D[1]
    assert list(np.nonzero(out[1, 1])[0]) == [4, 5] and out[1, 1, 4] == -D[0] and out[1, 1, 5] == -D[2]
    out = wc.forward("haar_x", img)
    assert list(np.nonzero(out[0, 1])[0]) == [5] and out[0, 1, 5] == f32(0.5) and out[1, 1, 5] == f32(0.5)
    img[:] = 0
    img[1, 11] = 1.0
    out = wc.forward("haar_x", img)
    assert list(np.nonzero(out[1, 1])[0]) == [5] and out[0, 1, 5] == f32(0.5) and out[1, 1, 5] == f32(-0.5)


def test_an_impulse_pins_the_taps_of_the_inverses(each_canon_wc):
    D = wc.constants()
    for c, even, odd in ((0, (D[2], D[0]), (D[3], D[1])), (1, (D[1], D[3]), (-D[0], -D[2]))):
        img = np.zeros((2, 3, 12), f32)
        img[c, 1, 5] = 1.0   # pair 5 of plane c: read as pair x/2 by outputs 10 and 11 and as pair x/2 + 1 by outputs 8 and 9
        out = wc.inverse("inverse_daubechies_x", img)
        assert not out[0].any() and not out[2].any() and list(np.nonzero(out[1])[0]) == [8, 9, 10, 11]
        # even x: D2 p + D1 q + D0 r + D3 s; odd x: D3 p - D0 q + D1 r - D2 s
        assert (out[1, 10], out[1, 8]) == even and (out[1, 11], out[1, 9]) == odd, c
        out = wc.inverse("inverse_haar_x", img)
        assert list(np.nonzero(out[1])[0]) == [10, 11] and out[1, 10] == 1 and out[1, 11] == (1 if c == 0 else -1)


@pytest.mark.parametrize("name", FORWARD)
def test_every_channel_other_than_0_is_the_difference_row(each_canon_wc, name):
    img = noise((5, 40), 3)
    both = wc.forward(name, img)
    for c in (2, -1, 1, 7):
        _same(wc.forward(name, img, out_shape=(1, 5, 20), out_min=(0, 0, c)), both[1:2], f"{name} c {c}")
    _same(wc.forward(name, img, out_shape=(1, 5, 20), out_min=(0, 0, 0)), both[0:1], name)
    wide = wc.forward(name, img, out_shape=(3, 5, 20), out_min=(0, 0, -1))
    _same(wide, both[[1, 0, 1]], name)
    assert not np.array_equal(both[0], both[1])


@pytest.mark.parametrize("name", INVERSE)
def test_negative_x_takes_floor_and_the_euclidean_remainder(each_canon_wc, name):
    img = noise((2, 2, 10), 4) + f32(0.5)
    out = wc.inverse(name, img, out_shape=(2, 12), out_min=(-4, 0), in_min=(-3, 0, 0))   # pairs -3 .. 6, outputs -4 .. 7
    daub = name == "inverse_daubechies_x"
    D = [np.float64(v) for v in wc.constants()]
    at = lambda c, k: np.float64(img[c, 0, k + 3])
    for x, k, even in ((-1, -1, False), (-2, -1, True), (-3, -2, False), (-4, -2, True), (0, 0, True), (1, 0, False)):
        p, q, r, s = at(0, k), at(1, k), at(0, k + 1), at(1, k + 1)
        if not daub:
            want = p + q if even else p - q
        else:
            want = D[2] * p + D[1] * q + D[0] * r + D[3] * s if even else D[3] * p - D[0] * q + D[1] * r - D[2] * s
        assert abs(out[0, x + 4] - want) <= 4 * U * 4, (x, k)   # four terms below 1: a wrong tap misses by far more


@pytest.mark.parametrize("name", NAMES)
def test_the_clamp_on_each_side_and_on_rows(each_canon_wc, name):
    if wc.is_inverse(name):
        img = noise((2, 4, 6), 5)
        out = wc.inverse(name, img, out_shape=(10, 40), out_min=(-14, -3))
        rows = np.clip(np.arange(-3, 7), 0, 3)
        edge = lambda v: np.repeat(v[:, :, None], 6, 2)   # every pair the edge pair
        left, right = wc.inverse(name, edge(img[:, :, 0]))[rows], wc.inverse(name, edge(img[:, :, 5]))[rows]
        # outputs left of pair 0 see the first pair twice, outputs right of the last pair the last one: x = -14 .. -3 and 12 .. 25
        _same(out[:, :12], np.tile(left[:, :2], 6), f"{name} left")
        _same(out[:, 26:], np.tile(right[:, :2], 7), f"{name} right")
        _same(out[:, 14:26][3:7], wc.inverse(name, img), f"{name} inside")
    else:
        img = noise((4, 12), 5)
        out = wc.forward(name, img, out_shape=(2, 10, 20), out_min=(-7, -3, 0))
        rows = np.clip(np.arange(-3, 7), 0, 3)
        const = lambda v: wc.forward(name, np.repeat(v[:, None], 12, 1))[:, rows]
        # pairs x <= -1 read column 0 only (2x + 2 <= 0), pairs x >= 6 column 11 only (2x - 1 >= 11): x = -7 .. -1 and 6 .. 12
        _same(out[:, :, :7], np.repeat(const(img[:, 0])[:, :, :1], 7, 2), f"{name} left")
        _same(out[:, :, 13:], np.repeat(const(img[:, 11])[:, :, :1], 7, 2), f"{name} right")
        _same(out[:, 3:7, 7:13], wc.forward(name, img), f"{name} inside")


@pytest.mark.parametrize("name", INVERSE)
def test_an_input_that_holds_channel_1_alone_is_read_by_both_taps(each_canon_wc, name):
    img = noise((1, 3, 8), 6)
    _same(wc.inverse(name, img, in_min=(0, 0, 1)), wc.inverse(name, np.concatenate([img, img])), name)
    _same(wc.inverse(name, img, in_min=(0, 0, -4)), wc.inverse(name, np.concatenate([img, img])), name)   # ... or a channel below 0
    three = noise((3, 3, 8), 7)
    _same(wc.inverse(name, three), wc.inverse(name, three[:2]), name)   # [0, 3): channel 2 is not read
    _same(wc.inverse(name, three, in_min=(0, 0, -1)), wc.inverse(name, three[1:]), name)


@pytest.mark.parametrize("name", NAMES)
def test_a_crop_equals_that_region(each_canon_wc, name):
    if wc.is_inverse(name):
        img = noise((2, 9, 35), 3)
        big = wc.inverse(name, img, out_shape=(15, 110), out_min=(-21, -3))
        _same(wc.inverse(name, img, out_shape=(4, 31), out_min=(-7, 2)), big[5:9, 14:45], name)
        _same(wc.inverse(name, img), big[3:12, 21:91], name)
        # it moves with the input's mins
        _same(wc.inverse(name, img, out_shape=(15, 110), out_min=(-21 + 8, -3 - 2), in_min=(4, -2, 0)), big, name)
    else:
        img = noise((9, 70), 3)
        big = wc.forward(name, img, out_shape=(3, 15, 60), out_min=(-11, -3, -1))
        _same(wc.forward(name, img, out_shape=(2, 4, 31), out_min=(-7, 2, 0)), big[1:3, 5:9, 4:35], name)
        _same(wc.forward(name, img), big[1:3, 3:12, 11:46], name)
        _same(wc.forward(name, img, out_shape=(3, 15, 60), out_min=(-11 + 2, -3 - 2, -1), in_min=(4, -2)), big, name)
    for d in range(img.ndim):   # an empty dimension: -4 under an output that is not empty
        shape = tuple(0 if j == d else n for j, n in enumerate(img.shape))
        wc.run(name, np.zeros(shape, f32), out_shape=(2, 2, 2)[:5 - img.ndim], expect=-4)
        wc.run(name, np.zeros(shape, f32), out_shape=(2, 2, 0)[-(5 - img.ndim):], expect=0)


def test_haar_has_one_form_and_daubechies_two():
    a, b = noise((9, 70), 8), noise((2, 9, 35), 9)
    res, before = [], wc.get_canon()
    for canon in (0, 1):
        with wc.canon(canon):
            assert wc.get_canon() == canon
            res.append([wc.run(n, b if wc.is_inverse(n) else a) for n in NAMES])
        assert wc.get_canon() == before   # restored
    for name, r0, r1 in zip(NAMES, *res):
        if "haar" in name:
            _same(r0, r1, name)   # no multiply feeds an add
        else:
            assert np.count_nonzero(r0.view(np.uint32) != r1.view(np.uint32)) > r0.size // 20, name


# ---------------------------------------------------------------------------------------------------- CPU: checker vs float64
def _taps64(name, v):
    """Per output of the driver's call: (value, sum of |c_i| |v_i|) in float64 from the float32 constants; v: the input as float64"""
    D = [np.float64(x) for x in wc.constants()]
    if not wc.is_inverse(name):
        w = v.shape[1]
        at = lambda k: v[:, np.clip(2 * np.arange(w // 2) + k, 0, w - 1)]
        a, b, c, d = at(-1), at(0), at(1), at(2)
        if name == "haar_x":
            terms = [[0.5 * b, 0.5 * c], [0.5 * b, -0.5 * c]]
        else:
            terms = [[D[0] * a, D[1] * b, D[2] * c, D[3] * d], [D[3] * a, -D[2] * b, D[1] * c, -D[0] * d]]
        return np.stack([sum(t) for t in terms]), np.stack([sum(np.abs(x) for x in t) for t in terms])
    w2 = v.shape[2]
    k = np.arange(2 * w2) // 2
    k1 = np.clip(k + 1, 0, w2 - 1)
    even = (np.arange(2 * w2) % 2 == 0)[None, :]
    p, q, r, s = v[0][:, k], v[1][:, k], v[0][:, k1], v[1][:, k1]
    if name == "inverse_haar_x":
        te, to = [p, q], [p, -q]
    else:
        te, to = [D[2] * p, D[1] * q, D[0] * r, D[3] * s], [D[3] * p, -D[0] * q, D[1] * r, -D[2] * s]
    val = np.where(even, sum(te), sum(to))
    mag = np.where(even, sum(np.abs(x) for x in te), sum(np.abs(x) for x in to))
    return val, mag


def _noise_away_from_zero(shape, seed):
    """seeded noise in [1/256, 1)"""
    return (noise(shape, seed) * f32(255.0 / 256.0) + f32(1.0 / 256.0)).astype(f32)


@pytest.mark.parametrize("seed", (1, 2, 64))
@pytest.mark.parametrize("name", NAMES)
def test_checker_against_float64(each_canon_wc, name, seed):
    """Daubechies: |checker - f64| <= gamma_4 sum |c_i| |v_i| per output, gamma_4 = 4u / (1 - 4u): four roundings at the most on any
    path through a sum of four products, fused or not.  Haar forward: exactly float32 of the float64 value (the sum is exact in
    float64, the halving exact).  Haar inverse: one rounding, within u |value|."""
    img = _noise_away_from_zero((2, 5, 32) if wc.is_inverse(name) else (5, 64), seed)
    assert img.min() >= f32(1.0 / 256.0) and img.max() < 1
    got = wc.run(name, img).astype(np.float64)
    val, mag = _taps64(name, img.astype(np.float64))
    err = np.abs(got - val)
    if "daubechies" in name:
        gamma4 = 4 * U / (1 - 4 * U)
        print(f"{name} canon {each_canon_wc} seed {seed}: largest |checker - float64| / sum|c||v| = {float(np.max(err / mag)) / U:.3g} u")
        assert np.all(err <= gamma4 * mag)
    elif name == "haar_x":
        assert np.array_equal(got, val.astype(f32).astype(np.float64))
    else:
        assert np.all(err <= U * np.abs(val))


def test_reconstruction_in_float64():
    """inverse_haar_x(haar_x(a)) == a and inverse_daubechies_x(daubechies_x(a))(x) == a(x + 1): the D4 pair as written reconstructs
    with a one-sample shift.  Away from the clamped edges, within 16 * 2^-25 * max|a|: eight products of two constants, each rounded
    to float32.  The last two outputs are edge-affected.  This pins the tap order of the inverse, which no other test can."""
    a = _noise_away_from_zero((3, 64), 11).astype(np.float64)
    bound = 16 * 2.0 ** -25 * a.max()
    for fwd, inv, shift in (("haar_x", "inverse_haar_x", 0), ("daubechies_x", "inverse_daubechies_x", 1)):
        t, _ = _taps64(fwd, a)
        back, _ = _taps64(inv, t)
        d = np.abs(back[:, :64 - 2] - a[:, shift:64 - 2 + shift])
        print(f"{inv}({fwd}(a)): largest error away from the edge {float(d.max()):.3g}, bound {bound:.3g}")
        assert d.max() <= bound
    # and the checker itself does what the float64 evaluation does: the same shift, in float32.  Each stage is within gamma_4 *
    # sum|c||v| <= 4u * 1.7 * 1.5 of its float64 value (the taps' magnitudes sum to 1.68, the values stay below 1.5), and the
    # first stage's error passes through taps that sum to 1.68: 28u in all, 32u allowed.  Haar: three roundings of values below 1
    a32 = a.astype(f32)
    for canon in (0, 1):
        with wc.canon(canon):
            back = wc.inverse("inverse_daubechies_x", wc.forward("daubechies_x", a32))
            assert np.max(np.abs(back[:, :62].astype(np.float64) - a[:, 1:63])) <= bound + 32 * U
            back = wc.inverse("inverse_haar_x", wc.forward("haar_x", a32))
            assert np.max(np.abs(back.astype(np.float64) - a)) <= 3 * U


# ---------------------------------------------------------------------------------------------------- GPU
def _place(shape, padded):
    """a zeroed (H, W) or (C, H, W) array; padded: inside a larger allocation with an ODD row stride (the 16-byte accesses are legal
    on some rows only) and a padded plane stride"""
    if not padded:
        return np.zeros(shape, f32)
    h, w = shape[-2:]
    row = (w + 4) | 1
    return np.zeros(tuple(shape[:-2]) + (h + 2, row), f32)[..., 1:1 + h, :w]


def _defaults(name, img, out_shape, out_min, in_min):
    if wc.is_inverse(name):
        return (img.shape[1], 2 * img.shape[2]) if out_shape is None else out_shape, (0, 0) if out_min is None else out_min, (0, 0, 0) if in_min is None else in_min
    return (2, img.shape[0], img.shape[1] // 2) if out_shape is None else out_shape, (0, 0, 0) if out_min is None else out_min, (0, 0) if in_min is None else in_min


def _run(hl, name, a, o, general):
    if general:
        hl.debug_wavelet_general(name, a, o)
    else:
        getattr(hl, name)(a, o)


def _gpu(hl, name, img, out_shape=None, out_min=None, in_min=None, general=False, padded=False):
    out_shape, out_min, in_min = _defaults(name, img, out_shape, out_min, in_min)
    src = _place(img.shape, padded)
    src[...] = img
    a, o = hl.Buffer(src, mins=in_min), hl.Buffer(_place(out_shape, padded), mins=out_min)
    _run(hl, name, a, o, general)
    assert np.array_equal(src, img, equal_nan=True)
    return np.ascontiguousarray(o.numpy())


def _gpu_offset(hl, name, img, out_shape=None, out_min=None, in_min=None, general=False):
    """the same call on device memory whose first element lies one float past a 16-byte boundary, rows 1 float longer than the
    image's: views of torch tensors, wrapped without a copy"""
    import torch
    from halide_amd.torch_ops import _Wrapped
    out_shape, out_min, in_min = _defaults(name, img, out_shape, out_min, in_min)
    view = lambda shape: torch.zeros(tuple(shape[:-1]) + (shape[-1] + 1,), dtype=torch.float32, device="cuda")[..., 1:]
    ti, to = view(img.shape), view(out_shape)
    assert ti.data_ptr() % 16 == 4 and to.data_ptr() % 16 == 4
    ti.copy_(torch.from_numpy(img))
    with _Wrapped(ti, to) as (a, o):
        _run(hl, name, a.set_min(*in_min), o.set_min(*out_min), general)
    torch.cuda.synchronize()
    return to.cpu().contiguous().numpy()


@pytest.fixture(params=["by_size", "general"])
def general(request):
    """Both implementations (halide_amd/csrc/wavelet.hip): the one launch every shape takes, and one thread per output through the
    hook."""
    return request.param == "general"


def _input_for(name, w, h, seed):
    """the driver's input for a W x H image: the image for the forwards, its (2, H, W / 2) transform's shape for the inverses"""
    return noise((2, h, max(w // 2, 1)), seed) if wc.is_inverse(name) else noise((h, w), seed)


# input W x H.  A wave owns 128 pairs of one row and a workgroup 4 rows: one lane; an output past the input (3 x 1: 2x + 1 clamps);
# a partial wave; 63 / 65 / 127 / 129 pairs: below and past one wave, 129 = one wave on the wide path and one lane beside it; 5 rows: a
# second workgroup in y; 515 pairs: five workgroups in x
SIZES = [(2, 1), (3, 1), (8, 2), (126, 3), (130, 2), (254, 3), (258, 5), (1030, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "x".join(map(str, s)))
def test_sizes(hl, canon_wc, on_stream, name, size, general):
    w, h = size
    img = _input_for(name, w, h, w * h)
    kw = {}
    if size == (3, 1):
        kw = dict(out_shape=(1, 3), out_min=(0, 0)) if wc.is_inverse(name) else dict(out_shape=(2, 1, 2), out_min=(0, 0, 0))
    _same(_gpu(hl, name, img, general=general, **kw), canon_wc.run(name, img, **kw), f"{name} {size}")
    if w >= 258:   # wide enough for the 16-byte path: an odd row stride makes it legal on some rows only
        _same(_gpu(hl, name, img, general=general, padded=True, **kw), canon_wc.run(name, img, **kw), f"{name} {size} padded")


REGIONS_FORWARD = [   # out_shape (C, H, W), out_min (x, y, c), in_min (x, y)
    ("x min odd", (2, 9, 20), (3, 0, 0), None), ("x min even", (2, 9, 20), (4, 0, 0), None), ("x min -5", (2, 9, 30), (-5, 0, 0), None),
    ("wider than the input on both sides", (2, 9, 60), (-10, 0, 0), None), ("y from -3 past the last row", (2, 14, 35), (0, -3, 0), None),
    ("rows past the last one only", (2, 3, 35), (0, 11, 0), None), ("input mins (3, -2)", (2, 12, 45), (-2, -4, 0), (3, -2)),
    ("channels [1, 2)", (1, 9, 35), (0, 0, 1), None), ("channels [0, 1)", (1, 9, 35), (0, 0, 0), None),
    ("channels [-1, 2)", (3, 9, 35), (0, 0, -1), None), ("channels [0, 3)", (3, 9, 35), (0, 0, 0), None), ("one pair", (2, 1, 1), (17, 4, 0), None)]
REGIONS_INVERSE = [   # out_shape (H, W), out_min (x, y), in_min (x, y, c), input channels
    ("x min odd", (9, 41), (3, 0), None, 2), ("x min even", (9, 40), (4, 0), None, 2), ("x min -5", (9, 50), (-5, 0), None, 2),
    ("wider than the input on both sides", (9, 100), (-12, 0), None, 2), ("y from -3 past the last row", (14, 70), (0, -3), None, 2),
    ("rows past the last one only", (3, 70), (0, 11), None, 2), ("input mins (3, -2, 0)", (12, 80), (1, -4), (3, -2, 0), 2),
    ("input channels [0, 3)", (9, 70), (0, 0), (0, 0, 0), 3), ("input channels [1, 2)", (9, 70), (0, 0), (0, 0, 1), 1),
    ("one output", (1, 1), (33, 4), None, 2), ("one odd output at -1", (1, 1), (-1, 4), None, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_regions(hl, canon_wc, on_stream, name, general):
    """one 70 x 9 image (its transform's 35 pairs for the inverses): regions, mins, channel ranges, strides and a base off by a float"""
    inverse, todo = wc.is_inverse(name), []
    for what, out_shape, out_min, in_min, *nc in (REGIONS_INVERSE if inverse else REGIONS_FORWARD):
        img = noise((nc[0], 9, 35), 5) if inverse else noise((9, 70), 5)
        kw = dict(out_shape=out_shape, out_min=out_min, in_min=in_min)
        want = canon_wc.run(name, img, **{k: v for k, v in kw.items() if v is not None})
        _same(_gpu(hl, name, img, general=general, **kw), want, f"{name} {what}")
        _same(_gpu(hl, name, img, general=general, padded=True, **kw), want, f"{name} {what}, padded strides")
        todo.append((what, img, kw, want))
    for what, img, kw, want in todo:   # last: wrapping a torch tensor moves the library to torch's stream
        _same(_gpu_offset(hl, name, img, general=general, **kw), want, f"{name} {what}, base off by one float")


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_regions_across_whole_waves(hl, canon_wc, name, general):
    """600 x 6: regions whose middle wave takes the 16-byte path between two that clamp; an odd x min shifts every output off the
    16-byte grid; a base off by one float makes the wide path illegal everywhere"""
    if wc.is_inverse(name):
        img = noise((2, 6, 300), 12)
        cases = [dict(out_shape=(8, 700), out_min=(-52, -1)), dict(out_shape=(8, 700), out_min=(-51, -1)), dict(out_shape=(6, 600), out_min=(6, 0), in_min=(3, 0, 0))]
    else:
        img = noise((6, 600), 12)
        cases = [dict(out_shape=(2, 8, 340), out_min=(-20, -1, 0)), dict(out_shape=(3, 8, 300), out_min=(1, -1, -1)), dict(out_shape=(2, 6, 290), out_min=(3, 0, 0), in_min=(5, 0))]
    for kw in cases:
        want = canon_wc.run(name, img, **kw)
        _same(_gpu(hl, name, img, general=general, **kw), want, f"{name} {kw}")
        _same(_gpu(hl, name, img, general=general, padded=True, **kw), want, f"{name} {kw} padded")
        _same(_gpu_offset(hl, name, img, general=general, **kw), want, f"{name} {kw} base off by one float")


def _special_image(name):
    """264 x 2 (132 pairs: a wave on the wide path and four lanes beside it), noise with the special values next to one another
    at the start, across the wave's end and in the tail"""
    big, tiny, den = f32(np.finfo(f32).max), f32(np.finfo(f32).tiny), np.uint32(0x00012345).view(f32)
    vals = np.array([np.nan, 1, np.inf, np.inf, -np.inf, 2, -0.0, -0.0, 0.0, -0.0, den, den, -den, tiny, big, -big, big, big, -np.inf, np.inf, 3, np.nan], f32)
    img = noise((2, 264), 13) - f32(0.5)
    for at in (0, 40, 240):
        img[0, at:at + vals.size] = vals
        img[1, at + 1:at + 1 + vals.size] = vals[::-1]
    if not wc.is_inverse(name):
        return img
    return np.stack([img[:, :132], np.roll(img, 7, 1)[:, 132:]]).copy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_special_values(hl, canon_wc, on_stream, name, general):
    """NaN, +-inf, -0, denormals, FLT_MAX next to -FLT_MAX, compared as bits; a NaN where the checker has a NaN (the sign and payload
    of a NaN that an operation makes are the processor's, not the algorithm's)"""
    img = _special_image(name)
    got, want = _gpu(hl, name, img, general=general), canon_wc.run(name, img)
    nan = np.isnan(want)
    assert nan.any() and np.isinf(want).any()
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("size", [(130, 2), (258, 5), (1030, 4)], ids=lambda s: "x".join(map(str, s)))
def test_default_equals_general(hl, on_stream, name, size):
    w, h = size
    img = _input_for(name, w, h, 11) * f32(1.5) - f32(0.2)
    kw = dict(out_shape=(h + 3, w + 31), out_min=(-14, -2)) if wc.is_inverse(name) else dict(out_shape=(3, h + 3, w // 2 + 15), out_min=(-6, -2, -1))
    _same(_gpu(hl, name, img, **kw), _gpu(hl, name, img, general=True, **kw), f"{name} {size}")


@pytest.mark.gpu
def test_the_paths_launch_what_they_say(hl):
    for w, h in ((1030, 4), (2, 1)):   # one launch for every shape
        for name in NAMES:
            img = _input_for(name, w, h, 2)
            kind = "wv_inv" if wc.is_inverse(name) else "wv_fwd"
            assert _launches(hl, lambda: _gpu(hl, name, img)) == [kind]
            assert _launches(hl, lambda: _gpu(hl, name, img, general=True)) == [kind + "_general"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_argv_equals_the_direct_call(hl, on_stream, name):
    img = _input_for(name, 300, 7, 6)
    out_shape, _, _ = _defaults(name, img, None, None, None)
    outs = []
    for how in (call_direct, call_argv):
        a, o = hl.Buffer(img.copy()), hl.Buffer(np.zeros(out_shape, f32))
        assert how(hl, name, a, o) == 0
        outs.append(np.ascontiguousarray(o.numpy()))
    assert outs[0].tobytes() == outs[1].tobytes() and outs[0].any()


# ---------------------------------------------------------------------------------------------------- torch
def test_torch_ops_shape_functions_and_cpu_refusal():
    import torch
    import halide_amd.torch_ops  # noqa: F401
    meta2, meta3 = torch.empty((45, 70), dtype=torch.float32, device="meta"), torch.empty((2, 45, 35), dtype=torch.float32, device="meta")
    for op in (torch.ops.hlmi.haar_x, torch.ops.hlmi.daubechies_x):
        assert op(meta2).shape == (2, 45, 35) and op(meta2).dtype == torch.float32
        assert op(torch.empty((4, 7), dtype=torch.float32, device="meta")).shape == (2, 4, 3)
        with pytest.raises(RuntimeError, match="GPU"):
            op(torch.zeros((16, 16)))
        with pytest.raises(TypeError):
            op(torch.zeros((16, 16), dtype=torch.int32))
        with pytest.raises(TypeError):
            op(torch.zeros((2, 16, 16)))
    for op in (torch.ops.hlmi.inverse_haar_x, torch.ops.hlmi.inverse_daubechies_x):
        assert op(meta3).shape == (45, 70) and op(meta3).dtype == torch.float32
        with pytest.raises(RuntimeError, match="GPU"):
            op(torch.zeros((2, 16, 8)))
        with pytest.raises(TypeError):
            op(torch.zeros((2, 16, 8), dtype=torch.int32))
        with pytest.raises(TypeError):
            op(torch.zeros((16, 16)))
        with pytest.raises(TypeError):
            op(torch.zeros((3, 16, 8)))


@pytest.mark.gpu
def test_torch_ops_equal_the_checker(hl, canon_wc):
    import torch
    import halide_amd.torch_ops  # noqa: F401
    for name in NAMES:
        img = _input_for(name, 300, 9, 21)
        t = torch.from_numpy(img).cuda()
        out = getattr(torch.ops.hlmi, name)(t)
        torch.cuda.synchronize()
        want = canon_wc.run(name, img)
        assert out.is_cuda and tuple(out.shape) == want.shape and out.dtype == torch.float32
        _same(out.cpu().contiguous().numpy(), want, f"torch {name}")
        assert np.array_equal(t.cpu().numpy(), img)


# ---------------------------------------------------------------------------------------------------- the driver's protocol
@pytest.mark.gpu
def test_the_drivers_protocol(hl, canon_wc, on_stream):
    """apps/wavelet/wavelet.cpp:60-75 on a 96 x 40 image: haar_x -> inverse_haar_x -> daubechies_x -> inverse_daubechies_x through one
    (48, 40, 2) buffer and one (96, 40) buffer, each stage against the checker on the same input"""
    img = noise((40, 96), 60)
    a, t, back = hl.Buffer(img.copy()), hl.Buffer(np.zeros((2, 40, 48), f32)), hl.Buffer(np.zeros((40, 96), f32))
    for fwd, inv in (("haar_x", "inverse_haar_x"), ("daubechies_x", "inverse_daubechies_x")):
        assert getattr(hl, fwd)(a, t) == 0
        got_t = np.ascontiguousarray(t.numpy()).copy()
        _same(got_t, canon_wc.forward(fwd, img), fwd)
        assert getattr(hl, inv)(t, back) == 0
        _same(np.ascontiguousarray(back.numpy()), canon_wc.inverse(inv, got_t), inv)
    _same(np.ascontiguousarray(a.numpy()), img, "the input")


# ---------------------------------------------------------------------------------------------------- a seeded slice of the fuzzer
@pytest.mark.gpu
def test_seeded_fuzz_slice_of_wavelet(on_stream):
    """scripts/fuzz_parity.py's wavelet case (all four entry points), a fixed number of cases from a fixed seed"""
    mod = load_fuzz_parity()
    rng = np.random.default_rng(20261018)
    for i in range(40):
        desc, ok = mod.CASES["wavelet"](rng)
        assert ok, f"case {i}: {desc}"
