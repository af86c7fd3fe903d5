"""gaussian_blur: the direct separable blur and its 36 resampled variants gaussian_blur_<U>_<D>_<F> (apps/gaussian_blur).

The checker is tests/cpp/gaussian_blur_check.c, a plain C restatement of apps/gaussian_blur/gaussian_blur_generator.cpp:18-63,
:117-150, :160-214 in both canonical float forms, built and driven through ctypes by tests/checker_lib.py; it
takes halide_exp from oracle/oracle_common.h.  The CPU tests hold the checker to an independent numpy float64 evaluation
(per-axis matrices: the pipelines are separable, out = M_y img M_x^T) and to properties that follow from the generator's text;
the GPU tests hold the library to the checker bit for bit.  Like every float pipeline here, gaussian_blur is pinned to this
repository's restatement only: no output of a real Halide build is involved."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import checker_lib
from parity_helpers import ROOT, RUNGEN, call_argv, call_direct, launches, load_fuzz_parity, noise, same_bits as _same

ORDERS_UP, ORDERS_DOWN, FACTORS = (2, 3, 4), (1, 2, 3), (2, 4, 8, 16)
UDF = [(u, d, f) for u in ORDERS_UP for d in ORDERS_DOWN for f in FACTORS]
VARIANTS = [f"gaussian_blur_{u}_{d}_{f}" for u, d, f in UDF]
NAMES = ["gaussian_blur_direct"] + VARIANTS
FOUR = [(3, 2, 8), (4, 3, 16), (2, 3, 16), (2, 1, 2)]


# ---------------------------------------------------------------------------------------------------- the checker
@pytest.fixture(scope="session")
def gc():
    return checker_lib.gaussian_blur


@pytest.fixture(params=[0, 1], ids=["canon0", "canon1"])
def each_canon_gc(request):
    with checker_lib.canon(request.param):
        yield request.param


@pytest.fixture
def canon0_gc():
    """for the tests whose tolerance was measured in canonical form 0"""
    with checker_lib.canon(0):
        yield


@pytest.fixture
def canon_gc(hl, gc):
    """the checker in the form the loaded library was built for"""
    with checker_lib.canon(hl.canon_fma()):
        yield gc


# ---------------------------------------------------------------------------------------------------- float64 evaluation
def _kn64(sigma, radius):
    r = np.arange(-radius, radius + 1, dtype=np.float64)
    k = np.exp(-(r * r) / (2.0 * sigma * sigma))
    return k / k.sum()


def _spline64(order, factor):
    box = np.full(factor, 1.0 / factor)
    k = box
    for _ in range(1, order):
        k = np.convolve(np.convolve(k, box), [0.5, 0.5])
    assert k.size == order * factor
    return k


def _variance64(order, factor):
    return order * (factor * factor - 1) / 12.0 + (order - 1) / 4.0


def _scatter(shape, rows, cols, vals):
    m = np.zeros(shape)
    np.add.at(m, (rows, cols), vals)
    return m


def direct_matrix(n_in, in_min, out_min, n_out, sigma, radius):
    """M[o, i]: weight of input sample i (edge-clamped) in output sample o"""
    o, r = np.meshgrid(np.arange(n_out), np.arange(-radius, radius + 1), indexing="ij")
    cols = np.clip(out_min + o + r - in_min, 0, n_in - 1)
    return _scatter((n_out, n_in), o, cols, np.broadcast_to(_kn64(sigma, radius), o.shape))


def resampled_matrix(axis, n_in, in_min, n_out, udf, sigma, radius_lo):
    """Up . Blur . Down along one axis; the radius is the specified integer (from the f32 sigma_lo), everything else float64"""
    u, d, f = udf
    dk, uk = _spline64(d, f), _spline64(u, f)
    shift = ((u - d) * f) // 2
    sigma_lo = np.sqrt(max(sigma * sigma - _variance64(u, f) - _variance64(d, f), 1e-4)) / f
    b0, b1 = -(u - 1), (n_out - 1) // f
    if axis == "y":   # the rows of the low-resolution image are clamped (:191), its columns are not
        l0, l1 = -u, -(-n_in // f)
        at = lambda v: np.clip(v, l0, l1)
    else:
        l0, l1 = b0 - radius_lo, b1 + radius_lo
        at = lambda v: v
    l, rx = np.meshgrid(np.arange(l0, l1 + 1), np.arange(f * d), indexing="ij")
    down = _scatter((l1 - l0 + 1, n_in), l - l0, np.clip(f * l + rx + shift, in_min, in_min + n_in - 1) - in_min, np.broadcast_to(dk, l.shape))
    b, r = np.meshgrid(np.arange(b0, b1 + 1), np.arange(-radius_lo, radius_lo + 1), indexing="ij")
    blur = _scatter((b1 - b0 + 1, l1 - l0 + 1), b - b0, at(b + r) - l0, np.broadcast_to(_kn64(sigma_lo, radius_lo), b.shape))
    o, i = np.meshgrid(np.arange(n_out), np.arange(u), indexing="ij")
    up = _scatter((n_out, b1 - b0 + 1), o, o // f - i - b0, uk[i * f + o % f] * f)
    return up @ blur @ down


def ref64_direct(gc, img, sigma, trunc):
    h, w = img.shape
    s = float(np.float32(sigma))
    radius = gc.radius(sigma, trunc)
    return direct_matrix(h, 0, 0, h, s, radius) @ img.astype(np.float64) @ direct_matrix(w, 0, 0, w, s, radius).T


def ref64_resampled(gc, udf, img, sigma, trunc):
    h, w = img.shape
    s = float(np.float32(sigma))
    radius = gc.radius(gc.sigma_lo(*udf, sigma), trunc)
    return resampled_matrix("y", h, 0, h, udf, s, radius) @ img.astype(np.float64) @ resampled_matrix("x", w, 0, w, udf, s, radius).T


CPU_SHAPE = (168, 200)   # 200 x 168
DIRECT_CASES = [(1.5, 3), (1.5, 5), (10.0, 3), (10.0, 5)]
RESAMPLED_CASES = [(udf, sigma) for udf in [(2, 1, 2), (3, 2, 8), (4, 3, 16), (2, 3, 16), (3, 2, 4)] for sigma in (10.0, 4.0)]

# The largest |checker - float64| measured for noise in [0, 1) at 200 x 168 (seed 200 + 168, canonical form 0, no code under test
# involved) over DIRECT_CASES and RESAMPLED_CASES at trunc 5: direct 1.47e-7 (sigma 1.5, trunc 3), 2.46e-7 (1.5, 5), 3.63e-7 (10, 3),
# 5.03e-7 (10, 5); resampled at sigma 10 / sigma 4: (2,1,2) 4.85e-7 / 3.48e-7, (3,2,8) 2.43e-7 / 1.46e-7, (4,3,16) 1.69e-7 / 1.69e-7,
# (2,3,16) 1.95e-7 / 1.95e-7, (3,2,4) 1.91e-7 / 1.51e-7.  The sums have up to
# 2 * 101 f32 additions of values below 1, each rounding at most 2^-24 of a partial sum below 1, and the expansions scale nothing up
# (their coefficients sum to 1), so a few 1e-7 is the expected size.  Other seeds vary, so 4 x the largest value seen is allowed.
F32_VS_FLOAT64 = 4 * 5.03e-7


# ---------------------------------------------------------------------------------------------------- CPU: the library's surface
def test_every_entry_point_is_exported_with_argv_and_metadata(hl):
    lib = C.CDLL(hl.LIB_PATH)
    assert len(NAMES) == 37
    for name in NAMES:
        for suffix in ("", "_argv", "_metadata"):
            assert hasattr(lib, name + suffix), name + suffix
        md = hl.metadata(name)
        assert md.version == 1 and md.num_arguments == 4 and md.name.decode() == name and b"hip" in md.target
        a = [md.arguments[i] for i in range(4)]
        assert [x.kind for x in a] == [1, 0, 0, 2] and [x.name.decode() for x in a] == ["input", "sigma", "trunc", "output"]
        assert [x.dimensions for x in a] == [2, 0, 0, 2]
        assert [(x.type.code, x.type.bits) for x in a] == [(2, 32), (2, 32), (0, 32), (2, 32)]
        for x in a:   # the generator declares no estimates and no ranges
            assert not x.scalar_def and not x.scalar_min and not x.scalar_max and not x.scalar_estimate and not x.buffer_estimates
    assert hasattr(lib, "gaussian_blur_direct_auto_schedule") and hasattr(lib, "hlmi_gaussian_blur_general")


def test_every_entry_point_has_its_aot_header():
    decl = open(os.path.join(ROOT, "include", "hlmi_pipelines.h")).read()
    everything = open(os.path.join(ROOT, "include", "aot", "gaussian_blur_all.h")).read()
    for name in NAMES:
        text = open(os.path.join(ROOT, "include", "aot", name + ".h")).read()
        assert "hlmi_pipelines.h" in text
        assert f"int {name}(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);" in decl
        assert f'#include "{name}.h"' in everything
    assert "halide_error_code_unaligned_host_ptr = -24" in open(os.path.join(ROOT, "include", "hlmi_abi.h")).read()


def test_the_all_header_compiles_as_c(tmp_path):
    src = tmp_path / "all.c"
    src.write_text('#include "aot/gaussian_blur_all.h"\nint (*const f)(struct halide_buffer_t *, float, int32_t, struct halide_buffer_t *) = gaussian_blur_4_3_16;\n'
                   "int (*const g)(struct halide_buffer_t *, float, int32_t, struct halide_buffer_t *) = gaussian_blur_direct_auto_schedule;\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "all.o")], check=True)


def test_python_names_the_variant(hl):
    assert hl.gaussian_blur_variant() == "gaussian_blur_3_2_8" and hl.gaussian_blur_variant(4, 3, 16) == "gaussian_blur_4_3_16"
    for bad in ((1, 2, 8), (5, 2, 8), (3, 0, 8), (3, 4, 8), (3, 2, 3), (3, 2, 32)):
        with pytest.raises(ValueError):
            hl.gaussian_blur_variant(*bad)


def test_aligned_array(hl):
    for shape in ((45, 70), (1, 1), (3, 97, 131)):
        a = hl.aligned_array(shape)
        assert a.shape == shape and a.dtype == np.float32 and not a.any()
        assert a.ctypes.data % 64 == 0 and (a.strides[-2] // 4) % 16 == 0 and a.strides[-1] == 4
        b = hl.Buffer(a)
        assert b.dim(1).stride % 16 == 0 and b.dim(0).extent == shape[-1]


# ---------------------------------------------------------------------------------------------------- CPU: the entry protocol
@pytest.mark.parametrize("how", [call_direct, call_argv], ids=["direct_call", "argv"])
@pytest.mark.parametrize("name", ["gaussian_blur_direct", "gaussian_blur_3_2_8", "gaussian_blur_2_3_16"])
def test_entry_protocol(hl, name, how):
    resampled = name != "gaussian_blur_direct"
    mk = lambda shape=(32, 40), dtype=np.float32: hl.Buffer(hl.aligned_array(shape, dtype))
    call = lambda i, o, s=2.0, t=3: how(hl, name, i, s, t, o)
    assert call(None, mk()) == -12 and call(mk(), None) == -12
    assert call(mk(dtype=np.uint16), mk()) == -3 and call(mk(), mk(dtype=np.uint16)) == -3
    assert call(mk((3, 32, 40)), mk()) == -43 and call(mk(), mk((3, 32, 40))) == -43
    # the scalars the algorithm has no answer for
    for bad in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        assert call(mk(), mk(), bad) == -9, bad
        assert "sigma" in hl.last_error()
    assert call(mk(), mk(), 2.0, -1) == -9 and "trunc" in hl.last_error()
    # x is the innermost dimension of both buffers
    assert call(hl.Buffer(np.zeros((40, 32), np.float32).T), mk()) == -8
    if resampled:
        plain = np.zeros((32 * 40 + 64), np.float32)
        off = (-plain.ctypes.data % 64) // 4
        assert call(mk(), hl.Buffer(hl.aligned_array((32, 40)), mins=(1, 0))) == -8 and "output.min.0" in hl.last_error()
        assert call(mk(), hl.Buffer(hl.aligned_array((32, 40)), mins=(0, -2))) == -8 and "output.min.1" in hl.last_error()
        assert call(mk(), hl.Buffer(plain[off:off + 32 * 40].reshape(32, 40))) == -8 and "output.stride.1" in hl.last_error()   # stride 40, aligned
        # a host pointer off the 64-byte grid: 16 bytes into an aligned row of stride 64
        wide = hl.aligned_array((32, 64))
        assert wide[:, 4:44].ctypes.data % 64 == 16
        assert call(mk(), hl.Buffer(wide[:, 4:44])) == -24 and "64" in hl.last_error()
        # order: the constraints before the alignment; the scalars before everything but the null check
        assert call(mk(), hl.Buffer(wide[:, 4:44], mins=(0, 3))) == -8
        assert call(mk(dtype=np.uint16), hl.Buffer(wide[:, 4:44]), 0.0) == -9
        assert call(None, hl.Buffer(wide[:, 4:44]), 0.0) == -12
        # input mins are free
        free = lambda: call(hl.Buffer(hl.aligned_array((32, 40)), mins=(17, -9)), mk())
    else:
        # any output region, any input min, no alignment and no stride asked for
        free = lambda: call(hl.Buffer(np.zeros((32, 40), np.float32), mins=(17, -9)), hl.Buffer(np.zeros((5, 7), np.float32)[:, 1:6], mins=(-200, 300)))
    # order: type before dimensionality before the constraints
    assert call(mk((3, 32, 40), np.uint16), mk()) == -3
    assert call(mk((3, 32, 40)), hl.Buffer(np.zeros((40, 32), np.float32).T)) == -43
    import torch
    if not torch.cuda.is_available():   # with everything in order only the device is missing here
        assert free() == -29 and call(mk(), mk()) == -29


@pytest.mark.parametrize("how", [call_direct, call_argv], ids=["direct_call", "argv"])
def test_bounds_queries(hl, how):
    dims = lambda b: [(b.raw.dim[i].min, b.raw.dim[i].extent) for i in range(2)]
    real = lambda: hl.Buffer(hl.aligned_array((48, 64)), mins=(2, 3))
    # direct: repeat_edge needs nothing beyond the input's own region; both stay as passed
    q = hl.Buffer.bounds_query(np.uint8, 2, mins=(5, 6), extents=(40, 30))
    assert how(hl, "gaussian_blur_direct", real(), 10.0, 5, q) == 0
    assert dims(q) == [(5, 40), (6, 30)] and (q.raw.type.code, q.raw.type.bits) == (2, 32)
    qi = hl.Buffer.bounds_query(np.float32, 2, mins=(2, 3), extents=(64, 48))
    assert how(hl, "gaussian_blur_direct", qi, 10.0, 5, hl.Buffer(np.zeros((30, 40), np.float32), mins=(-5, 100))) == 0
    assert dims(qi) == [(2, 64), (3, 48)]
    # resampled: a queried output gets mins 0; the input stays as passed
    q = hl.Buffer.bounds_query(np.float32, 2, mins=(5, 6), extents=(40, 30))
    assert how(hl, "gaussian_blur_3_2_8", real(), 10.0, 5, q) == 0
    assert dims(q) == [(0, 40), (0, 30)]
    qi = hl.Buffer.bounds_query(np.float32, 2, mins=(2, 3), extents=(64, 48))
    assert how(hl, "gaussian_blur_3_2_8", qi, 10.0, 5, hl.Buffer(hl.aligned_array((30, 40)))) == 0
    assert dims(qi) == [(2, 64), (3, 48)]


def test_without_a_gpu_the_python_calls_refuse_to_run(hl):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    a, o = hl.Buffer(np.zeros((16, 16), np.float32)), hl.Buffer(hl.aligned_array((16, 16)))
    for fn in (lambda: hl.gaussian_blur_direct(a, 2.0, 3, o), lambda: hl.gaussian_blur(a, 2.0, 3, o), lambda: hl.gaussian_blur(a, 2.0, 3, o, 4, 3, 16),
               lambda: hl.debug_gaussian_blur_general("gaussian_blur_2_1_2", a, 2.0, 3, o)):
        with pytest.raises(hl.HalideError) as e:
            fn()
        assert e.value.code == -29
    with pytest.raises(hl.HalideError) as e:
        hl.debug_gaussian_blur_general("gaussian_blur_5_5_5", a, 2.0, 3, o)
    assert e.value.code == -8


# ---------------------------------------------------------------------------------------------------- CPU: tables
@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_resampling_tables_are_exact_and_sum_to_one(gc, canon_gc, order, factor):
    k = gc.resampling_kernel(order, factor)
    want = _spline64(order, factor)
    assert np.array_equal(k.astype(np.float64), want)                     # f32 and f64 evaluations agree exactly
    assert float(np.sum(k.astype(np.float64))) == 1.0 and np.float32(0) + np.sum(k, dtype=np.float32) == np.float32(1)
    m = k.astype(np.float64) * 2.0 ** 19
    n = m.astype(np.int64)
    assert np.all(m == n) and np.all(n // (n & -n) < 2 ** 16)             # dyadic rationals over 2^19 at the finest, under 16 significant bits
    assert np.array_equal((k * np.float32(factor)).astype(np.float64), want * factor)
    assert float(gc.lib.gc_variance(order, factor)) == float(np.float32(np.float32(np.float32(order * (factor * factor - 1)) / np.float32(12)) + np.float32((order - 1) / 4.0)))


def test_kernel_table_and_small_sigma(gc, each_canon_gc, oracle):
    kn, s = gc.kernel_table(1.5, 5)
    assert kn.size == 11 and np.array_equal(kn, kn[::-1]) and abs(float(kn.astype(np.float64).sum()) - 1) < 1e-6
    with oracle.canon(each_canon_gc):   # kernel(x) is the oracle's halide_exp of one correctly rounded quotient
        k = np.array([oracle.halide_exp(float(np.float32(-(x * x)) / np.float32(np.float32(2 * 1.5) * np.float32(1.5)))) for x in range(-5, 6)], np.float32)
    total = np.float32(0)
    for v in k:   # ascending x, one add each
        total = np.float32(total + v)
    assert total == s and np.array_equal(kn.view(np.uint32), (k / total).view(np.uint32))
    # sigma 4 with F = 16: sigma^2 <= the variances + 1e-4, so sigma_lo = sqrt(1e-4f) / 16, radius_lo <= 1, table {0, 1, 0}
    sl = gc.sigma_lo(3, 2, 16, 4.0)
    assert sl == float(np.sqrt(np.float32(1e-4)) / np.float32(16))
    for trunc in (3, 5, 100):
        r = gc.radius(sl, trunc)
        assert r == 1
        kn, s = gc.kernel_table(sl, r)
        assert kn.tolist() == [0.0, 1.0, 0.0] and s == 1.0   # halide_exp(-1.28e6) is exactly 0
    assert gc.radius(sl, 0) == 0


# ---------------------------------------------------------------------------------------------------- CPU: checker vs float64
def _psnr(a, b):
    return 10.0 * np.log10(1.0 / np.mean((np.asarray(a, np.float64) - b) ** 2))


@pytest.fixture(scope="module")
def cpu_image():
    return noise(CPU_SHAPE, 200 + 168)


@pytest.fixture(scope="module")
def truth64(cpu_image):
    """the float64 direct blur at trunc 8, per sigma: what the quality of a truncated or resampled blur is measured against"""
    cache = {}

    def get(gc, sigma):
        if sigma not in cache:
            cache[sigma] = ref64_direct(gc, cpu_image, sigma, 8)
        return cache[sigma]
    return get


@pytest.mark.parametrize("sigma,trunc", DIRECT_CASES)
def test_checker_direct_against_float64(gc, canon0_gc, cpu_image, sigma, trunc):
    d = float(np.max(np.abs(gc.direct(cpu_image, sigma, trunc).astype(np.float64) - ref64_direct(gc, cpu_image, sigma, trunc))))
    print(f"direct sigma {sigma} trunc {trunc}: largest |checker - float64| = {d:.3g}")
    assert d <= F32_VS_FLOAT64


@pytest.mark.parametrize("udf,sigma", RESAMPLED_CASES, ids=lambda v: "_".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_checker_resampled_against_float64(gc, canon0_gc, cpu_image, udf, sigma):
    d = float(np.max(np.abs(gc.resampled(udf, cpu_image, sigma, 5).astype(np.float64) - ref64_resampled(gc, udf, cpu_image, sigma, 5))))
    print(f"{udf} sigma {sigma}: largest |checker - float64| = {d:.3g}")
    assert d <= F32_VS_FLOAT64


@pytest.mark.parametrize("udf", [c[0] for c in RESAMPLED_CASES[::2]], ids=lambda v: "_".join(map(str, v)))
def test_quality_of_the_resampled_checker_is_the_float64_evaluations(gc, each_canon_gc, cpu_image, truth64, udf):
    """PSNR against the float64 direct blur at trunc 8, sigma 10: a wrong shift or phase costs tens of dB.  For orientation, a float64
    prototype gave 68.1 dB for (3, 2, 8) and 83.6 dB for (3, 2, 4); no number is stored here."""
    truth = truth64(gc, 10.0)
    mine, theirs = _psnr(gc.resampled(udf, cpu_image, 10.0, 5), truth), _psnr(ref64_resampled(gc, udf, cpu_image, 10.0, 5), truth)
    print(f"{udf}: checker {mine:.2f} dB, float64 {theirs:.2f} dB")
    assert abs(mine - theirs) <= 0.5 and theirs > 40.0


@pytest.mark.parametrize("trunc", [3, 4])
def test_quality_of_the_direct_checker_is_the_float64_evaluations(gc, each_canon_gc, cpu_image, truth64, trunc):
    """Truncation at 3 and 4 sigmas (a float64 prototype: 82.8 and 114.9 dB).  At trunc 5 the float64 evaluation reaches 155.8 dB, past
    what any f32 sum can: 2^-24 relative per addition is a floor near 140 dB, so that case has no 0.5 dB statement to make."""
    truth = truth64(gc, 10.0)
    mine, theirs = _psnr(gc.direct(cpu_image, 10.0, trunc), truth), _psnr(ref64_direct(gc, cpu_image, 10.0, trunc), truth)
    print(f"direct trunc {trunc}: checker {mine:.2f} dB, float64 {theirs:.2f} dB")
    assert abs(mine - theirs) <= 0.5


# ---------------------------------------------------------------------------------------------------- CPU: identities
def test_radius_zero_is_a_bit_exact_copy(gc, each_canon_gc):
    img = noise((45, 70), 1)
    assert gc.radius(1.5, 0) == 0
    assert np.array_equal(gc.direct(img, 1.5, 0).view(np.uint32), img.view(np.uint32))
    crop = gc.direct(img, 10.0, 0, out_shape=(10, 20), out_min=(65, 40))   # past the right and lower edges: the clamped pixels
    want = img[np.clip(np.arange(40, 50), 0, 44)][:, np.clip(np.arange(65, 85), 0, 69)]
    assert np.array_equal(crop.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("udf", UDF, ids=lambda v: "_".join(map(str, v)))
def test_a_constant_image_stays_constant(gc, canon0_gc, udf):
    """follows from |checker - float64| <= the tolerance: every row of every float64 matrix sums to 1"""
    img = np.full((45, 70), 0.7, np.float32)
    for sigma in (10.0, 4.0):
        assert np.max(np.abs(gc.resampled(udf, img, sigma, 5).astype(np.float64) - float(np.float32(0.7)))) <= F32_VS_FLOAT64, sigma
    assert np.max(np.abs(gc.direct(img, 10.0, 5).astype(np.float64) - float(np.float32(0.7)))) <= F32_VS_FLOAT64


def test_float64_matrices_have_unit_row_sums():
    for udf in FOUR:
        for axis in "xy":
            assert np.allclose(resampled_matrix(axis, 97, 0, 131, udf, 10.0, 3).sum(1), 1.0, atol=1e-12)
    assert np.allclose(direct_matrix(97, -3, -20, 140, 10.0, 50).sum(1), 1.0, atol=1e-12)


def test_checker_crop_and_origin(gc, each_canon_gc):
    img = noise((45, 70), 3)
    full = gc.direct(img, 1.5, 3)
    assert np.array_equal(gc.direct(img, 1.5, 3, out_shape=(20, 30), out_min=(17, 9)), full[9:29, 17:47])
    assert np.array_equal(gc.direct(img, 1.5, 3, in_min=(17, -9)), full)                     # a direct blur moves with its input
    # a resampled blur's grid is anchored at the output's origin: an output crop at (0, 0) equals that region
    whole = gc.resampled((3, 2, 8), img, 10.0, 5)
    assert np.array_equal(gc.resampled((3, 2, 8), img, 10.0, 5, out_shape=(24, 40)), whole[:24, :40])


# ---------------------------------------------------------------------------------------------------- GPU
def _padded(shape, pad=5):
    """a zeroed array of `shape` whose rows sit in a wider allocation (row stride != width)"""
    return np.zeros((shape[0], shape[1] + pad), np.float32)[:, 2:2 + shape[1]]


def _gpu_direct(hl, img, sigma, trunc, out_shape=None, out_min=None, in_min=(0, 0), general=False, padded=False):
    out_shape = img.shape if out_shape is None else out_shape
    out_min = in_min if out_min is None else out_min
    src = img
    if padded:
        src = _padded(img.shape)
        src[...] = img
    a = hl.Buffer(src, mins=in_min)
    o = hl.Buffer(_padded(out_shape) if padded else np.zeros(out_shape, np.float32), mins=out_min)
    if general:
        hl.debug_gaussian_blur_general("gaussian_blur_direct", a, sigma, trunc, o)
    else:
        hl.gaussian_blur_direct(a, sigma, trunc, o)
    return np.ascontiguousarray(o.numpy())


def _gpu_resampled(hl, udf, img, sigma, trunc, out_shape=None, in_min=(0, 0), general=False):
    a = hl.Buffer(np.ascontiguousarray(img), mins=in_min)
    o = hl.Buffer(hl.aligned_array(img.shape if out_shape is None else out_shape))
    if general:
        hl.debug_gaussian_blur_general(hl.gaussian_blur_variant(*udf), a, sigma, trunc, o)
    else:
        hl.gaussian_blur(a, sigma, trunc, o, *udf)
    return np.ascontiguousarray(o.numpy())


@pytest.fixture(params=["by_size", "general", "tile16", "tile4"])
def general(request, monkeypatch):
    """Every path a blur pass can take (halide_amd/csrc/gaussian_blur.hip, run_blur): chosen by size, the general kernels through the
    hook, and either tile shape forced through HLMI_GB_TILE.  The value is what the helpers below pass as `general`."""
    if request.param.startswith("tile"):
        monkeypatch.setenv("HLMI_GB_TILE", request.param[4:])
    return request.param == "general"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(97, 131), (1, 1), (40, 1), (2, 257), (33, 65), (32, 64)], ids=lambda s: f"{s[1]}x{s[0]}")
def test_direct_sizes_and_radii(hl, canon_gc, on_stream, shape, general):
    img = noise(shape, shape[0] * shape[1])
    for sigma, trunc in ((1.5, 3), (10.0, 5), (1.5, 0), (0.4, 1)):   # R = 5, 50 (more than half of 97), 0, 1
        _same(_gpu_direct(hl, img, sigma, trunc, general=general), canon_gc.direct(img, sigma, trunc), f"sigma {sigma} trunc {trunc}")


@pytest.mark.gpu
def test_direct_radius_beyond_both_extents(hl, canon_gc, general):
    img = noise((23, 37), 37)
    assert canon_gc.radius(10.0, 5) == 50
    _same(_gpu_direct(hl, img, 10.0, 5, general=general), canon_gc.direct(img, 10.0, 5), "37 x 23, R = 50")


@pytest.mark.gpu
@pytest.mark.parametrize("sigma,trunc", [(1.5, 3), (10.0, 5)])
def test_direct_regions(hl, canon_gc, on_stream, sigma, trunc, general):
    img = noise((97, 131), 5)
    # mins (-20, -7) and extents beyond the input on every side
    want = canon_gc.direct(img, sigma, trunc, out_shape=(120, 170), out_min=(-20, -7))
    _same(_gpu_direct(hl, img, sigma, trunc, out_shape=(120, 170), out_min=(-20, -7), general=general), want, "around the input")
    # wholly outside the input: every tap clamps
    want = canon_gc.direct(img, sigma, trunc, out_shape=(20, 30), out_min=(400, -300))
    _same(_gpu_direct(hl, img, sigma, trunc, out_shape=(20, 30), out_min=(400, -300), general=general), want, "outside the input")
    # input mins (17, -9), the output over the same region and over a crop of it
    want = canon_gc.direct(img, sigma, trunc, in_min=(17, -9))
    _same(_gpu_direct(hl, img, sigma, trunc, in_min=(17, -9), general=general), want, "input min (17, -9)")
    _same(_gpu_direct(hl, img, sigma, trunc, out_shape=(20, 30), out_min=(40, 3), in_min=(17, -9), general=general), want[12:32, 23:53], "crop")
    # row strides padded on both buffers
    _same(_gpu_direct(hl, img, sigma, trunc, padded=True, general=general), canon_gc.direct(img, sigma, trunc), "padded rows")


@pytest.mark.gpu
@pytest.mark.parametrize("udf", UDF, ids=lambda v: "_".join(map(str, v)))
def test_resampled_all_variants(hl, canon_gc, udf):
    img = noise((45, 70), 70)
    _same(_gpu_resampled(hl, udf, img, 10.0, 5), canon_gc.resampled(udf, img, 10.0, 5), str(udf))


@pytest.mark.gpu
@pytest.mark.parametrize("udf", FOUR, ids=lambda v: "_".join(map(str, v)))
def test_resampled_sizes_sigmas_and_mins(hl, canon_gc, on_stream, udf, general):
    for shape in ((97, 131), (3, 5), (64, 128)):   # odd, smaller than F, exact multiples
        img = noise(shape, shape[1])
        for sigma, trunc in ((10.0, 5), (4.0, 5), (10.0, 3)):   # sigma 4: the clamped sigma_lo for F = 16
            _same(_gpu_resampled(hl, udf, img, sigma, trunc, general=general), canon_gc.resampled(udf, img, sigma, trunc), f"{shape} sigma {sigma} trunc {trunc}")
    img = noise((97, 131), 9)
    _same(_gpu_resampled(hl, udf, img, 10.0, 5, in_min=(17, -9), general=general), canon_gc.resampled(udf, img, 10.0, 5, in_min=(17, -9)), "input min (17, -9)")
    # an output of another size than the input
    _same(_gpu_resampled(hl, udf, img, 10.0, 5, out_shape=(120, 100), general=general), canon_gc.resampled(udf, img, 10.0, 5, out_shape=(120, 100)), "100 x 120 output")


def _launches(hl, fn):
    return set(launches(hl, fn))   # which kernels, however often


TILED, GENERAL = {"gb_tables", "gb_blur_y", "gb_blur_x"}, {"gb_tables", "gb_blur_y_general", "gb_blur_x_general"}


@pytest.mark.gpu
def test_the_paths_launch_what_they_say(hl, monkeypatch):
    img = noise((45, 70), 2)
    assert _launches(hl, lambda: _gpu_direct(hl, img, 1.5, 3)) == GENERAL   # by size: too few pixels for a tile to pay
    assert _launches(hl, lambda: _gpu_resampled(hl, (3, 2, 8), img, 10.0, 5, general=True)) == GENERAL | {"gb_down", "gb_up"}
    for tile in ("16", "4"):
        monkeypatch.setenv("HLMI_GB_TILE", tile)
        assert _launches(hl, lambda: _gpu_direct(hl, img, 1.5, 3)) == TILED
        assert _launches(hl, lambda: _gpu_direct(hl, img, 1.5, 3, general=True)) == GENERAL   # the hook wins
        assert _launches(hl, lambda: _gpu_resampled(hl, (3, 2, 8), img, 10.0, 5)) == TILED | {"gb_down", "gb_up"}
    monkeypatch.setenv("HLMI_GB_TILE", "0")
    assert _launches(hl, lambda: _gpu_direct(hl, img, 1.5, 3)) == GENERAL


@pytest.mark.gpu
def test_the_benchmarked_size_by_size(hl, canon_gc):
    """1536 x 2560, sigma 10, trunc 5: the direct blur takes the larger tiles, the low-resolution blur of (2, 1, 2) the smaller ones
    and that of (3, 2, 8) the general kernels, each because of its size alone"""
    img = noise((2560, 1536), 1536)
    got = {}
    assert _launches(hl, lambda: got.update(d=_gpu_direct(hl, img, 10.0, 5))) == TILED
    _same(got["d"], canon_gc.direct(img, 10.0, 5), "direct")
    assert _launches(hl, lambda: got.update(a=_gpu_resampled(hl, (2, 1, 2), img, 10.0, 5))) == TILED | {"gb_down", "gb_up"}
    _same(got["a"], canon_gc.resampled((2, 1, 2), img, 10.0, 5), "(2, 1, 2)")
    assert _launches(hl, lambda: got.update(b=_gpu_resampled(hl, (3, 2, 8), img, 10.0, 5))) == GENERAL | {"gb_down", "gb_up"}
    _same(got["b"], canon_gc.resampled((3, 2, 8), img, 10.0, 5), "(3, 2, 8)")


@pytest.mark.gpu
def test_direct_radius_past_the_staged_span(hl, canon_gc, monkeypatch):
    """Forced tiles at R = 400 and R = 2100: four spans of 256 + 2 R floats fit 64 KiB up to R = 1916 and sixteen up to R = 380, so the
    x pass takes its one-row tile at 400 whatever is asked for, and the general kernel at 2100; 2 R + 1 taps, most of them clamped"""
    img = noise((9, 40), 4)
    assert canon_gc.radius(80.0, 5) == 400 and canon_gc.radius(420.0, 5) == 2100
    for tile in ("16", "4"):
        monkeypatch.setenv("HLMI_GB_TILE", tile)
        assert _launches(hl, lambda: _same(_gpu_direct(hl, img, 80.0, 5), canon_gc.direct(img, 80.0, 5), "R = 400")) == TILED
        assert _launches(hl, lambda: _same(_gpu_direct(hl, img, 420.0, 5), canon_gc.direct(img, 420.0, 5), "R = 2100")) == {"gb_tables", "gb_blur_y", "gb_blur_x_general"}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["gaussian_blur_direct", "gaussian_blur_3_2_8"])
def test_argv_equals_the_direct_call(hl, name):
    img = noise((45, 70), 6)
    outs = []
    for how in (call_direct, call_argv):
        a, o = hl.Buffer(img.copy()), hl.Buffer(hl.aligned_array((45, 70)))
        assert how(hl, name, a, 3.0, 4, o) == 0
        outs.append(np.ascontiguousarray(o.numpy()))
    assert outs[0].tobytes() == outs[1].tobytes() and outs[0].any()


# ---------------------------------------------------------------------------------------------------- torch
def test_torch_op_shape_function_and_cpu_refusal():
    import torch
    import halide_amd.torch_ops  # noqa: F401
    meta = torch.empty((45, 70), dtype=torch.float32, device="meta")
    assert torch.ops.hlmi.gaussian_blur(meta, 10.0).shape == (45, 70) and torch.ops.hlmi.gaussian_blur(meta, 10.0, 5, 3, 2, 8).dtype == torch.float32
    with pytest.raises(RuntimeError, match="GPU"):
        torch.ops.hlmi.gaussian_blur(torch.zeros((16, 16)), 2.0)
    with pytest.raises(ValueError):
        torch.ops.hlmi.gaussian_blur(torch.zeros((16, 16)), 2.0, 5, 3, 2, 7)
    with pytest.raises(TypeError):
        torch.ops.hlmi.gaussian_blur(torch.zeros((16, 16), dtype=torch.int32), 2.0)


@pytest.mark.gpu
def test_torch_op_equals_the_checker(hl, canon_gc):
    import torch
    import halide_amd.torch_ops  # noqa: F401
    img = noise((45, 70), 21)
    t = torch.from_numpy(img).cuda()
    out = torch.ops.hlmi.gaussian_blur(t, 10.0)
    torch.cuda.synchronize()
    assert out.is_cuda and out.shape == t.shape and out.dtype == torch.float32
    _same(out.cpu().contiguous().numpy(), canon_gc.direct(img, 10.0, 5), "torch direct")
    for udf in ((3, 2, 8), (4, 3, 16)):
        out = torch.ops.hlmi.gaussian_blur(t, 10.0, 4, *udf)
        torch.cuda.synchronize()
        assert out.shape == t.shape and out.stride(0) % 16 == 0
        _same(out.cpu().contiguous().numpy(), canon_gc.resampled(udf, img, 10.0, 4), f"torch {udf}")
    assert np.array_equal(t.cpu().numpy(), img)


# ---------------------------------------------------------------------------------------------------- the RunGen-compatible runner
def test_runner_describes_a_variant_by_name():
    out = subprocess.run([RUNGEN, "--name=gaussian_blur_3_2_8", "--describe"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'Input "input" is of type Buffer<float32> with 2 dimensions' in out.stdout and 'Input "sigma" is of type float32' in out.stdout
    assert 'Input "trunc" is of type int32' in out.stdout and 'Output "output" is of type Buffer<float32> with 2 dimensions' in out.stdout


# ---------------------------------------------------------------------------------------------------- a seeded slice of the fuzzer
@pytest.mark.gpu
def test_seeded_fuzz_slice_of_gaussian_blur():
    """scripts/fuzz_parity.py's gaussian_blur case, a fixed number of cases from a fixed seed"""
    mod = load_fuzz_parity()
    rng = np.random.default_rng(20261017)
    for i in range(40):
        desc, ok = mod.CASES["gaussian_blur"](rng)
        assert ok, f"case {i}: {desc}"
