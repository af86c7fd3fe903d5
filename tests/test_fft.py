"""fft: the 2-D f32 transforms of apps/fft — c2c forward, c2c inverse, r2c, c2r — and their four 16 x 16 entry points.

The contract (include/hlmi_pipelines.h) is tests/cpp/fft_check.c, plain C, built and bound by tests/fft_checker.py:
the reference's Stockham passes, codelets, radix_factor, zip / unzip with V = 8 and the DC / Nyquist row, with every choice the
reference leaves open made and named there, in both canonical float forms.  The CPU tests hold the checker to things that are not
the checker (numpy's float64 DFT within eps log2(N0 N1), the reference's own two acceptance protocols restated), pin its structure
(round trip, r2c against c2c, exact linearity in power-of-two gains, inputs that tell V = 8 from 4 and 16 and form 0 from form 1),
compare radix_factor and the size predicate with the library's for every N, and hold the entry points to their protocol; the GPU
tests hold hl.fft2d (the line kernels), hl.debug_fft2d_general (one thread per line), the four fixed entry points and the torch op
to the checker bit for bit, NaN for NaN, in the library's form."""
import ctypes as C
import functools
import os
import subprocess
import threading

import numpy as np
import pytest

import fft_checker as fc
from parity_helpers import ROOT, DevArray, HostArray, call_argv, call_direct, kernel_const, load_fuzz_parity
from parity_helpers import gpu_present as _gpu_present, launches as _launches, same_bits as _same, same_bits_or_nan as _same_or_nan

f32, f64, u32 = np.float32, np.float64, np.uint32
EPS = 2.0 ** -23
KINDS = fc.KINDS
REAL_KINDS = ("r2c", "c2r")

# the plan's constants, read from the source: a kernel without them fails here
V, MAX_N, LDS_COMPLEX, MAX_LINES, MIN_COLS, WANT_GROUPS, ONE_GROUP_BYTES = (
    kernel_const("fft.hip", n) for n in ("V", "MAX_N", "LDS_COMPLEX", "MAX_LINES", "MIN_COLS", "WANT_GROUPS", "ONE_GROUP_BYTES"))

# the issue's sizes (N0, N1): the reference's 16 x 16, skip_zip (8 x 8, 12 x 6), radix 6, N0 < 4V both ways, four passes both ways
ISSUE_SIZES = [(16, 16), (8, 8), (12, 6), (48, 36), (32, 16), (16, 32), (96, 64), (4096, 2), (2, 4096)]
# and, for the GPU: the largest image the one-workgroup launch takes (ONE_GROUP_BYTES / 8 complex elements) and the next sizes above it
# in either dimension; a column tile that does not divide N0 (36 columns in tiles of MIN_COLS, on the two-pass path at 36 x 64); N1
# above LDS_COMPLEX / MIN_COLS (the column tile shrinks to 4); and enough rows for two rows per workgroup (1024 / WANT_GROUPS)
AT_THE_BUDGET, ABOVE_THE_BUDGET = (32, ONE_GROUP_BYTES // 8 // 32), [(48, ONE_GROUP_BYTES // 8 // 32), (ONE_GROUP_BYTES // 8 // 32, 36)]
GPU_SIZES = ISSUE_SIZES + [AT_THE_BUDGET] + ABOVE_THE_BUDGET + [(36, 48), (36, 64), (16, 2048), (8, 1024)]


def one_group(n0, n1):
    """the whole transform in one workgroup, one launch: the N0 x N1 complex image fits the plan's LDS budget"""
    return 8 * n0 * n1 <= ONE_GROUP_BYTES


# ---------------------------------------------------------------------------------------------------- the contract, restated
def radix_factor(n):
    """fft.cpp:1066-1097"""
    special = {16: [4, 4], 32: [8, 4], 64: [8, 8], 128: [8, 4, 4], 256: [8, 8, 4]}
    if n in special:
        return special[n]
    R = []
    for r in (8, 6, 4, 2):
        while n % r == 0 and n > 0:
            R.append(r)
            n //= r
    if n != 1 or not R:
        R.append(n)
    return R


def size_ok(n):
    return 2 <= n <= 4096 and all(r in (8, 6, 4, 2) for r in radix_factor(n))


def zip_width(kind, n0, n1, v=8):
    """0: the reference goes through c2c (skip_zip)"""
    from math import gcd
    if kind == "r2c":
        return 0 if n0 < 2 * v or (n0 < 4 * v and n0 % (2 * v) != 0) else gcd(v, n0 // 2)
    if kind == "c2r":
        return 0 if n0 < 2 * v else gcd(gcd(v, n1 // 2), n0 // 2)
    return 0


def expected_launches(kind, n0, n1, general, in_layout=(0, 0), out_layout=(0, 0)):
    """fft_plan() of fft.hip restated; a layout is (device address, row stride in floats) of a buffer"""
    if general:
        return ["fft_general_a", "fft_general_b"]
    zipped = zip_width(kind, n0, n1) > 0
    a_cols, b_cols = kind == "r2c" and zipped, not (kind == "r2c" and zipped)
    vec_a = kind == "r2c" or (in_layout[0] % 8 == 0 and in_layout[1] % 2 == 0)
    vec_b = kind == "c2r" or (out_layout[0] % 8 == 0 and out_layout[1] % 2 == 0)
    if one_group(n0, n1):
        return ["fft_whole" if vec_a and vec_b else "fft_whole_elem"]
    return sorted(("fft_cols" if cols else "fft_rows") + ("" if vec else "_elem") for cols, vec in ((a_cols, vec_a), (b_cols, vec_b)))


def lines_per_group(cols, n, lines):
    cap = max(1, min(MAX_LINES, LDS_COMPLEX // n))
    b = max(1, min(cap, lines // WANT_GROUPS))
    if cols:
        b = max(b, min(cap, MIN_COLS))
    return min(b, lines)


def bound(n0, n1):
    """the classical growth of a floating-point FFT's relative L2 error, c eps log2(N), with c = 1"""
    return EPS * np.log2(n0 * n1)


# ---------------------------------------------------------------------------------------------------- inputs
def _noise(shape, seed):
    """[-1, 1)"""
    return (np.random.default_rng(seed).random(shape, dtype=f32) * 2 - 1).astype(f32)


def _input(kind, n0, n1, seed=0, extra_rows=0):
    """Noise in [-1, 1) in the kind's input shape.  c2r takes the top N1/2 + 1 rows of a real image's spectrum, and the reference
    unzips the DC and Nyquist rows on the assumption that they are Hermitian along dimension 0: its input here is the spectrum
    (float64, rounded to float32) of real noise scaled by 1 / sqrt(N0 N1), so that it is one; `extra_rows` rows of plain noise follow."""
    shape = fc.in_shape(kind, n0, n1)
    key = 1000 * KINDS.index(kind) + 7 * n0 + n1 + 100000 * seed
    if kind != "c2r":
        return _noise((shape[0] + extra_rows,) + shape[1:], key)
    spec = np.fft.fft2(_noise((n1, n0), key).astype(f64))[:n1 // 2 + 1] / np.sqrt(n0 * n1)
    return np.concatenate([np.stack([spec.real, spec.imag], -1).astype(f32), _noise((extra_rows, n0, 2), key + 1)])


def _cplx(a):
    return a[..., 0].astype(f64) + 1j * a[..., 1].astype(f64)


def _pair(z):
    return np.stack([z.real, z.imag], -1).astype(f32)


def _dft64(kind, x, n1):
    """numpy's float64 transform of the float32 input, gain 1, in the checker's output shape (as a complex or real float64 array)"""
    if kind == "c2c_forward":
        return np.fft.fft2(_cplx(x))
    if kind == "c2c_inverse":
        return np.fft.ifft2(_cplx(x)) * x.shape[0] * x.shape[1]
    if kind == "r2c":
        return np.fft.fft2(x.astype(f64))[:n1 // 2 + 1]
    # c2r: the reference reads rows 0 .. N1/2, extends them by conjugate symmetry and keeps the real part; of the DC and Nyquist rows
    # it uses only what survives re(ifft): build the whole spectrum that way
    n0, h = x.shape[1], n1 // 2
    s = _cplx(x[:h + 1])
    full = np.zeros((n1, n0), complex)
    full[:h + 1] = s
    for m in range(h + 1, n1):
        full[m] = np.conj(s[n1 - m][(-np.arange(n0)) % n0])
    return np.fft.ifft2(full).real * n0 * n1


def _rel(got, want):
    g = _cplx(got) if got.ndim == 3 else got.astype(f64)
    return np.linalg.norm(g - want) / np.linalg.norm(want)


@pytest.fixture(autouse=True)
def _form_of_the_library(hl):
    """every test starts with the checker in the library's canonical form and on the library's own table function"""
    fc.use_twiddles(hl.fft_twiddles_address())
    fc.set_canon(hl.canon_fma())
    yield
    fc.use_twiddles(None)


@functools.lru_cache(maxsize=None)
def _want(kind, n0, n1, gain, canon, seed=0, extra_rows=0):
    """the checker's output on _input(...), computed once per module and never written to"""
    with fc.canon(canon):
        out = fc.run(kind, _input(kind, n0, n1, seed, extra_rows), n1=n1, gain=gain)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------- CPU 1: against float64
@pytest.mark.parametrize("canon", [0, 1])
@pytest.mark.parametrize("n0,n1", ISSUE_SIZES)
def test_the_checker_is_within_eps_log2_n_of_the_float64_dft(n0, n1, canon):
    for kind in KINDS:
        x = _input(kind, n0, n1)
        e = _rel(_want(kind, n0, n1, 1.0, canon), _dft64(kind, x, n1))
        print(f"{kind} {n0}x{n1} form {canon}: {e / bound(n0, n1):.3f} of the bound")
        assert e <= bound(n0, n1), (kind, e, bound(n0, n1))


def test_the_twiddle_tables_are_the_stated_function(hl):
    """(cosf(a), sinf(a)) * gain of a = ((float)(sign 2) kPi (float)k) / (float)n, a true f32 division; the library's exported
    function and the checker's own give the same bits, and stay within an ulp and the angle's rounding of the float64 values"""
    lib = C.CDLL(hl.LIB_PATH)
    lib.hlmi_fft_twiddles.restype, lib.hlmi_fft_twiddles.argtypes = None, [C.c_int32, C.c_int32, C.c_float, C.c_void_p]
    for n, sign, gain in [(64, -1, 1.0), (4096, 1, 1.0), (48, -1, 1.0 / 256), (512, 1, 3.0)]:
        mine = fc.twiddles(n, sign, gain)
        theirs = np.empty((n, 2), f32)
        lib.hlmi_fft_twiddles(n, sign, gain, theirs.ctypes.data)
        _same(theirs, mine, f"table {n} {sign} {gain}")
        k = np.arange(n, dtype=f32)
        ang = (f32(sign * 2) * f32(np.pi) * k) / f32(n)
        exact = np.stack([np.cos(ang.astype(f64)), np.sin(ang.astype(f64))], -1) * f64(f32(gain))
        assert np.abs(mine - exact).max() <= 2 * EPS * abs(gain)
        ideal = np.stack([np.cos(2 * np.pi * sign * np.arange(n) / n), np.sin(2 * np.pi * sign * np.arange(n) / n)], -1) * gain
        assert np.abs(mine - ideal).max() <= 12 * EPS * abs(gain)   # the f32 angle: two roundings and kPi's own error at up to 2 pi, ~1e-6, plus the function's ulp


# ---------------------------------------------------------------------------------------------------- CPU 2: the reference's protocols
def _signal_1d(fn):
    i = np.arange(16)
    return sum(fn(2 * np.pi * (k * (i / 16.0) + k / 16.0)) for k in range(1, 5)).astype(f32)


def _aot_signals():
    """the four inputs of fft_aot_test.cpp"""
    sr, si = _signal_1d(np.cos), _signal_1d(np.sin)
    r2c = (sr[None, :] + sr[:, None]).astype(f32)
    c2r = np.zeros((16, 16, 2), f32)
    t = f32(1.0 / (2.0 * np.sqrt(2.0)))
    c2r[0, 1], c2r[0, 15] = (t, t), (t, -t)
    fwd = np.stack([sr[None, :] + sr[:, None], si[None, :] + si[:, None]], -1).astype(f32)
    inv = np.zeros((16, 16, 2), f32)
    inv[0, 1], inv[0, 15] = (0.5, 0.5), (0.5, 0.5)
    return {"r2c": r2c, "c2r": c2r, "c2c_forward": fwd, "c2c_inverse": inv}


AOT_GAIN = {"r2c": 1.0 / 256, "c2r": 1.0, "c2c_forward": 1.0 / 256, "c2c_inverse": 1.0}
AOT_ENTRY = {"r2c": "fft_forward_r2c", "c2r": "fft_inverse_c2r", "c2c_forward": "fft_forward_c2c", "c2c_inverse": "fft_inverse_c2c"}


def _accept_aot(kind, out):
    """fft_aot_test.cpp's checks of one output: bin magnitudes and phases, everything else near zero, the inverse cases near their
    cosines; all within 1e-3"""
    i = np.arange(16)
    if kind in ("r2c", "c2c_forward"):
        mag = 0.5 if kind == "r2c" else 1.0
        z = _cplx(out)
        for k in range(1, 5):
            for b in (z[0, k], z[k, 0]):
                assert abs(abs(b) - mag) <= 1e-3 and abs(np.angle(b) - k / 16.0 * 2 * np.pi) <= 1e-3, (kind, k, b)
        rest = np.ones(z.shape, bool)
        rest[0, 1:5] = rest[1:5, 0] = False
        if kind == "r2c":
            rest[0, 12:] = False
        assert np.abs(z.real[rest]).max() <= 1e-3 and np.abs(z.imag[rest]).max() <= 1e-3
    elif kind == "c2r":
        assert np.abs(out - np.cos(2 * np.pi * (i / 16.0 + 0.125))[None, :]).max() <= 1e-3
    else:
        a, b = 2 * np.pi * (i / 16.0 + 0.125), 2 * np.pi * (i * 15 / 16.0 + 0.125)
        assert np.abs(out[..., 0] - (np.cos(a) + np.cos(b))[None, :] / np.sqrt(2)).max() <= 1e-3
        assert np.abs(out[..., 1] - (np.sin(a) + np.sin(b))[None, :] / np.sqrt(2)).max() <= 1e-3


@pytest.mark.parametrize("canon", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_the_checker_passes_the_aot_test_of_the_reference(kind, canon):
    with fc.canon(canon):
        _accept_aot(kind, fc.run(kind, _aot_signals()[kind], n1=16, gain=AOT_GAIN[kind]))


def _cmul32(a, b):
    """the driver's dft_in * dft_kernel on float32 pairs"""
    return np.stack([a[..., 0] * b[..., 0] - a[..., 1] * b[..., 1], a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]], -1).astype(f32)


@pytest.mark.parametrize("canon", [0, 1])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_checker_passes_the_box_filter_convolution_of_the_reference(seed, canon):
    """main.cpp at its default 32 x 32: a 3 x 3 box filter applied in the frequency domain through c2c and through r2c / c2r with
    inverse gain 1 / (W H), against the direct circular mean within the driver's own 1e-6"""
    W = H = 32
    img = np.random.default_rng(seed).random((H, W), dtype=f32)
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    kernel = np.where((np.minimum(x, W - x) <= 1) & (np.minimum(y, H - y) <= 1), f32(1.0 / 9), f32(0)).astype(f32)
    correct = np.zeros((H, W), f32)
    for i in (-1, 0, 1):
        for j in (-1, 0, 1):
            correct = (correct + np.roll(img, (-i, -j), (0, 1))).astype(f32)
    correct = (correct / f32(9)).astype(f32)
    z = lambda r: np.stack([r, np.zeros_like(r)], -1)
    with fc.canon(canon):
        c2c = fc.run("c2c_inverse", _cmul32(fc.run("c2c_forward", z(img)), fc.run("c2c_forward", z(kernel))), gain=1.0 / (W * H))[..., 0]
        r2c = fc.run("c2r", _cmul32(fc.run("r2c", img), fc.run("r2c", kernel)), n1=H, gain=1.0 / (W * H))
    print(f"seed {seed} form {canon}: worst c2c {np.abs(c2c - correct).max():.3e}, r2c {np.abs(r2c - correct).max():.3e}")
    assert np.abs(c2c - correct).max() <= 1e-6 and np.abs(r2c - correct).max() <= 1e-6


# ---------------------------------------------------------------------------------------------------- CPU 3: structure
@pytest.mark.parametrize("n0,n1", [(16, 16), (8, 8), (48, 36), (32, 16), (96, 64)])
def test_forward_then_inverse_returns_the_input(n0, n1):
    x = _input("c2c_forward", n0, n1)
    back = fc.run("c2c_inverse", fc.run("c2c_forward", x, gain=1.0 / (n0 * n1)), gain=1.0)
    assert _rel(back, _cplx(x)) <= bound(n0, n1)
    r = _input("r2c", n0, n1)
    back = fc.run("c2r", fc.run("r2c", r, gain=1.0 / (n0 * n1)), n1=n1, gain=1.0)
    assert _rel(back, r.astype(f64)) <= bound(n0, n1)


@pytest.mark.parametrize("n0,n1", [(16, 16), (48, 36), (32, 16), (96, 64)])
def test_r2c_is_the_top_of_c2c_within_rounding_and_not_bit_for_bit(n0, n1):
    r = _input("r2c", n0, n1)
    half = fc.run("r2c", r)
    full = fc.run("c2c_forward", np.stack([r, np.zeros_like(r)], -1))[:n1 // 2 + 1]
    assert _rel(half, _cplx(full)) <= bound(n0, n1)
    assert (half.view(u32) != full.view(u32)).any(), "the zipped r2c has the bits of c2c: nothing would stop a rewrite through c2c"


def test_r2c_through_c2c_where_the_reference_skips_the_zip():
    for n0, n1 in [(8, 8), (12, 6)]:
        assert fc.zip_width("r2c", n0, n1) == 0 == zip_width("r2c", n0, n1)
        r = _input("r2c", n0, n1)
        _same(fc.run("r2c", r), fc.run("c2c_forward", np.stack([r, np.zeros_like(r)], -1))[:n1 // 2 + 1], "skip_zip")
    assert [fc.zip_width("r2c", n, 16) for n in (16, 24, 32, 48)] == [8, 0, 8, 8] == [zip_width("r2c", n, 16) for n in (16, 24, 32, 48)]
    assert [fc.zip_width("c2r", 48, n) for n in (36, 6, 16)] == [2, 1, 8] == [zip_width("c2r", 48, n) for n in (36, 6, 16)]


@pytest.mark.parametrize("kind", KINDS)
def test_a_power_of_two_gain_scales_exactly(kind):
    for n0, n1 in [(16, 16), (48, 36), (8, 8)]:
        x = _input(kind, n0, n1)
        one = fc.run(kind, x, n1=n1, gain=1.0)
        for g in (0.25, 2.0, 1.0 / 256):
            _same(fc.run(kind, x, n1=n1, gain=g), (one * f32(g)).astype(f32), f"{kind} gain {g}")
        # a negative one too, up to the sign of the zeros the unzip writes as literals (the imaginary parts of r2c's four real bins)
        assert np.array_equal(fc.run(kind, x, n1=n1, gain=-2.0), (one * f32(-2.0)).astype(f32))


@pytest.mark.parametrize("kind", REAL_KINDS)
@pytest.mark.parametrize("n0,n1", [(16, 16), (48, 36), (32, 16), (16, 32), (96, 64)])
def test_the_gpu_inputs_tell_v_8_from_4_and_16(kind, n0, n1):
    x, want = _input(kind, n0, n1), _want(kind, n0, n1, 1.0, 1)
    told = 0
    with fc.canon(1):
        for v in (4, 16):
            other = fc.run(kind, x, n1=n1, v=v)
            if fc.zip_width(kind, n0, n1, v) == fc.zip_width(kind, n0, n1, 8):
                _same(other, want, "the same pairing")   # the zip width is a gcd with N0 / 2, for c2r also with N1 / 2
                continue
            told += 1
            assert (other.view(u32) != want.view(u32)).any(), (kind, n0, n1, v)
    assert told == sum(zip_width(kind, n0, n1, v) != zip_width(kind, n0, n1, 8) for v in (4, 16))


def test_some_gpu_size_tells_v_8_from_both_neighbours():
    for kind in REAL_KINDS:
        for v in (4, 16):
            assert any(fc.zip_width(kind, n0, n1, v) != fc.zip_width(kind, n0, n1, 8) for n0, n1 in GPU_SIZES), (kind, v)


@pytest.mark.parametrize("kind", KINDS)
def test_the_gpu_inputs_tell_form_0_from_form_1(kind):
    for n0, n1 in [(16, 16), (48, 36), (96, 64)]:   # a pass with S > 1, or radix 6 or 8, has a complex product
        assert (_want(kind, n0, n1, 1.0, 0).view(u32) != _want(kind, n0, n1, 1.0, 1).view(u32)).any(), (kind, n0, n1)


# ---------------------------------------------------------------------------------------------------- CPU 4: radix_factor, sizes
def test_radix_factor_and_the_size_predicate_for_every_n(hl):
    assert radix_factor(16) == [4, 4] and radix_factor(256) == [8, 8, 4] and radix_factor(4096) == [8] * 4 and radix_factor(12) == [6, 2]
    for n in range(1, 4101):
        assert hl.fft_radix_factor(n) == radix_factor(n) == fc.radix_factor(n), n
        assert hl.fft_size_ok(n) == size_ok(n) == fc.size_ok(n), n
    assert MAX_N == 4096 and V == 8 == fc.V
    assert not size_ok(1) and not size_ok(10) and not size_ok(18) and size_ok(36) and size_ok(3072) and not size_ok(8192)
    assert max(len(radix_factor(n)) for n in range(2, 4097) if size_ok(n)) == 4


# ---------------------------------------------------------------------------------------------------- CPU 5: the library's surface
ENTRIES = tuple(AOT_ENTRY.values())


def test_the_entry_points_are_exported_with_argv_and_metadata(hl):
    lib = C.CDLL(hl.LIB_PATH)
    for name in ENTRIES:
        for sym in (name, name + "_argv", name + "_metadata"):
            assert hasattr(lib, sym), sym
        assert not hasattr(lib, name + "_auto_schedule")
        assert hl._fn[name] is not None and callable(getattr(hl, name))
    for sym in ("hlmi_fft2d", "hlmi_fft2d_general", "hlmi_fft_twiddles", "hlmi_fft_radix_factor", "hlmi_fft_size_ok"):
        assert hasattr(lib, sym), sym
    assert callable(hl.fft2d) and callable(hl.debug_fft2d_general)


@pytest.mark.parametrize("name", ENTRIES)
def test_metadata_states_two_3d_f32_buffers(hl, name):
    md = hl.metadata(name)
    assert md.version == 1 and md.num_arguments == 2 and md.name.decode() == name and b"hip" in md.target
    a = [md.arguments[i] for i in range(2)]
    assert [x.name.decode() for x in a] == ["input", "output"] and [x.kind for x in a] == [1, 2]
    assert [(x.type.code, x.type.bits, x.dimensions) for x in a] == [(2, 32, 3)] * 2


def test_the_aot_headers_compile_as_c(tmp_path):
    decl = " ".join(open(os.path.join(ROOT, "include", "hlmi_pipelines.h")).read().split())
    for name in ENTRIES:
        assert f"int {name}(struct halide_buffer_t *input, struct halide_buffer_t *output);" in decl
        src = tmp_path / f"{name}.c"
        src.write_text(f'#include "aot/{name}.h"\nint (*const f)(struct halide_buffer_t *, struct halide_buffer_t *) = {name};\n'
                       f"int (*const a)(void **) = {name}_argv;\nconst struct halide_filter_metadata_t *(*const m)(void) = {name}_metadata;\n")
        subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / f"{name}.o")], check=True)


# ---- the entry protocol
def _mk(hl, kind, side, n0=16, n1=16, dtype=f32, rows=None, row_pad=0):
    """a zeroed buffer for the input (side 0) or output (side 1) of `kind`, its rows `row_pad` elements longer than dense"""
    shape = (fc.in_shape if side == 0 else fc.out_shape)(kind, n0, n1)
    shape = shape if len(shape) == 3 else shape + (1,)
    if rows is not None:
        shape = (rows,) + shape[1:]
    rs = shape[1] * shape[2] + row_pad
    flat = np.zeros(shape[0] * rs, dtype)
    return hl.fft_buffer(np.lib.stride_tricks.as_strided(flat, shape, (rs * flat.itemsize, shape[2] * flat.itemsize, flat.itemsize)))


def _ok():
    return 0 if _gpu_present() else -29   # with everything in order only the device can be missing


def _call(hl, kind, n0=16, n1=16, gain=1.0, symbol="hlmi_fft2d", **over):
    args = {"input": _mk(hl, kind, 0, n0, n1), "output": _mk(hl, kind, 1, n0, n1)}
    args.update(over)
    return hl._fft_hook(symbol)(KINDS.index(kind), n0, n1, gain, *[None if args[k] is None else args[k].ptr for k in ("input", "output")])


HOW = pytest.mark.parametrize("how", [call_direct, call_argv], ids=["direct_call", "argv"])
KIND = pytest.mark.parametrize("kind", KINDS)


def _entry(hl, how, kind, **over):
    args = {"input": _mk(hl, kind, 0), "output": _mk(hl, kind, 1)}
    args.update(over)
    return how(hl, AOT_ENTRY[kind], args["input"], args["output"])


@HOW
@KIND
def test_a_call_in_order_reaches_the_device(hl, how, kind):
    assert _entry(hl, how, kind) == _ok()
    assert _call(hl, kind) == _ok() and _call(hl, kind, symbol="hlmi_fft2d_general") == _ok()
    assert _call(hl, kind, 48, 36) == _ok()


@HOW
@KIND
def test_a_bounds_query_fills_the_query_buffers(hl, how, kind):
    dims = lambda b: [(b.dim(i).min, b.dim(i).extent, b.dim(i).stride) for i in range(3)]
    ci, co = (1 if kind == "r2c" else 2), (1 if kind == "c2r" else 2)
    ri, ro = (9 if kind == "c2r" else 16), (9 if kind == "r2c" else 16)
    qi, qo = hl.Buffer.bounds_query(f32, 3, mins=(5, 6, 7), extents=(1, 2, 3)), hl.Buffer.bounds_query(f32, 3)
    assert _entry(hl, how, kind, input=qi, output=qo) == 0
    assert dims(qi) == [(0, 16, ci), (0, ri, 16 * ci), (0, ci, 1)] and dims(qo) == [(0, 16, co), (0, ro, 16 * co), (0, co, 1)]
    # a real buffer beside the query stays as it is
    real, q = _mk(hl, kind, 1), hl.Buffer.bounds_query(np.uint16, 3)
    before = dims(real)
    assert _entry(hl, how, kind, input=q, output=real) == 0 and dims(real) == before and dims(q)[0] == (0, 16, ci)
    assert (q.raw.type.code, q.raw.type.bits) == (2, 32)
    assert _entry(hl, how, kind, input=hl.Buffer.bounds_query(f32, 2)) == -43
    q = hl.Buffer.bounds_query(f32, 3)
    assert _call(hl, kind, 48, 36, output=q) == 0 and dims(q)[:2] == [(0, 48, co), (0, 19 if kind == "r2c" else 36, 48 * co)]


@HOW
@KIND
@pytest.mark.parametrize("which", ["input", "output"])
def test_null_wrong_type_and_wrong_dimensions_are_refused(hl, how, kind, which):
    side = ("input", "output").index(which)
    assert _entry(hl, how, kind, **{which: None}) == -12 and which in hl.last_error()
    assert _entry(hl, how, kind, **{which: _mk(hl, kind, side, dtype=np.float64)}) == -3 and which in hl.last_error()
    assert _entry(hl, how, kind, **{which: _mk(hl, kind, side, dtype=np.int32)}) == -3
    assert _entry(hl, how, kind, **{which: hl.Buffer(np.zeros((16, 16), f32))}) == -43 and which in hl.last_error()


@KIND
@pytest.mark.parametrize("which", ["input", "output"])
def test_the_strides_and_the_component_dimension_are_pinned(hl, kind, which):
    side = ("input", "output").index(which)

    def broken(fix):
        b = _mk(hl, kind, side)
        fix(b)
        return _call(hl, kind, **{which: b})

    def set_dim(d, **kw):
        def fix(b):
            for k, v in kw.items():
                setattr(b.dim(d), k, v)
        return fix

    comps = 1 if (kind, side) in (("r2c", 0), ("c2r", 1)) else 2
    assert broken(set_dim(2, stride=2)) == -8 and f"{which}.stride.2" in hl.last_error()
    assert broken(set_dim(2, min=1)) == -8 and f"{which}.min.2" in hl.last_error()
    assert broken(set_dim(2, extent=3 - comps)) == -8 and f"{which}.extent.2" in hl.last_error()
    assert broken(set_dim(0, stride=3 - comps)) == -8 and f"{which}.stride.0" in hl.last_error()
    assert broken(set_dim(1, stride=16 * comps - 1)) == -8 and f"{which}.stride.1" in hl.last_error()
    padded = _mk(hl, kind, side, row_pad=3)
    assert padded.dim(1).stride == 16 * comps + 3 and _call(hl, kind, **{which: padded}) == _ok()
    if side == 1:
        assert broken(set_dim(0, extent=15)) == -8 and broken(set_dim(1, min=1)) == -8 and broken(set_dim(1, extent=b_rows(kind) + 1)) == -8
    else:
        assert broken(set_dim(0, extent=15)) == -4 and broken(set_dim(1, extent=(9 if kind == "c2r" else 16) - 1)) == -4


def b_rows(kind):
    return 9 if kind == "r2c" else 16


def test_a_c2r_input_may_be_taller_than_it_is_read(hl):
    assert _call(hl, "c2r", input=_mk(hl, "c2r", 0, rows=16)) == _ok()
    assert _call(hl, "c2r", input=_mk(hl, "c2r", 0, rows=8)) == -4


@pytest.mark.parametrize("symbol", ["hlmi_fft2d", "hlmi_fft2d_general"])
def test_a_disallowed_size_is_refused(hl, symbol):
    for kind, n0, n1 in [("c2c_forward", 10, 16), ("c2c_inverse", 16, 1), ("c2c_forward", 8192, 16), ("c2c_forward", 18, 18), ("r2c", 16, 0),
                         ("c2r", 16, 22), ("c2c_forward", -16, 16)]:
        i, o = hl.fft_buffer(np.zeros((4, 4, 2), f32)), hl.fft_buffer(np.zeros((4, 4, 2), f32))
        assert hl._fft_hook(symbol)(KINDS.index(kind), n0, n1, 1.0, i.ptr, o.ptr) == -8 and "sizes" in hl.last_error(), (kind, n0, n1)
    assert size_ok(6) and size_ok(12)
    i, o = hl.fft_buffer(np.zeros((4, 4, 2), f32)), hl.fft_buffer(np.zeros((4, 4, 2), f32))
    assert hl._fft_hook(symbol)(7, 16, 16, 1.0, i.ptr, o.ptr) == -8 and "kind" in hl.last_error()
    assert _call(hl, "c2c_forward", 12, 6, symbol=symbol) == _ok() and _call(hl, "c2c_forward", 2, 2, symbol=symbol) == _ok()


def test_input_and_output_may_not_overlap(hl):
    whole = np.zeros((33, 16, 2), f32)
    assert _call(hl, "c2c_forward", input=hl.fft_buffer(whole[:16]), output=hl.fft_buffer(whole[:16])) == -8 and "alias" in hl.last_error()
    assert _call(hl, "c2c_inverse", input=hl.fft_buffer(whole[:16]), output=hl.fft_buffer(whole[15:31])) == -8   # one shared row
    assert _call(hl, "c2c_forward", input=hl.fft_buffer(whole[:16]), output=hl.fft_buffer(whole[16:32])) == _ok()   # neighbours
    assert _call(hl, "r2c", input=hl.fft_buffer(whole[:8].reshape(16, 16)), output=hl.fft_buffer(whole[7:16])) == -8
    # a c2r input's rows above N1/2 are not read: the output may lie there
    assert _call(hl, "c2r", input=hl.fft_buffer(whole[:17]), output=hl.fft_buffer(whole[9:17].reshape(16, 16))) == _ok()


def test_the_order_of_the_checks(hl):
    assert _call(hl, "r2c", input=None, output=_mk(hl, "r2c", 1, dtype=np.int32)) == -12       # null before everything
    assert _call(hl, "r2c", 10, 16, output=_mk(hl, "r2c", 1, dtype=np.int32)) == -8            # the sizes before the buffers
    assert _call(hl, "r2c", input=hl.Buffer(np.zeros((16, 16), np.int32))) == -3               # type before dimensionality
    a = _mk(hl, "c2c_forward", 0)
    b = _mk(hl, "c2c_forward", 1)
    b.dim(2).stride = 2
    assert _call(hl, "c2c_forward", input=a, output=a) == -8 and "alias" in hl.last_error()
    assert _call(hl, "c2c_forward", input=b, output=b) == -8 and "stride.2" in hl.last_error()   # the pins before the alias check


def test_without_a_gpu_the_python_calls_refuse_to_run(hl):
    if _gpu_present():
        return   # the statement is about a machine without one
    for kind in KINDS:
        i, o = _mk(hl, kind, 0), _mk(hl, kind, 1)
        for fn in (lambda: hl.fft2d(kind, i, o), lambda: hl.debug_fft2d_general(kind, i, o, 0.5), lambda: getattr(hl, AOT_ENTRY[kind])(i, o)):
            with pytest.raises(hl.HalideError) as e:
                fn()
            assert e.value.code == -29


def test_torch_shape_function_and_refusals():
    import torch
    import halide_amd.torch_ops  # noqa: F401
    op = torch.ops.hlmi.fft2d
    meta = lambda *s: torch.empty(s, dtype=torch.float32, device="meta")
    assert op(meta(36, 48, 2), "c2c_forward", 1.0).shape == (36, 48, 2) and op(meta(36, 48), "r2c", 1.0).shape == (19, 48, 2)
    assert op(meta(19, 48, 2), "c2r", 1.0).shape == (36, 48) and op(meta(16, 16, 2), "c2c_inverse", 0.5).dtype == torch.float32
    with pytest.raises(RuntimeError, match="GPU"):
        op(torch.zeros((16, 16, 2)), "c2c_forward", 1.0)
    for bad, kind in ((torch.zeros((16, 16)), "c2c_forward"), (torch.zeros((16, 16, 2)), "r2c"), (torch.zeros((16, 16, 3)), "c2r"),
                      (torch.zeros((16, 16, 2), dtype=torch.float64), "c2c_inverse"), (torch.zeros((16, 16, 2)), "dct")):
        with pytest.raises(TypeError):
            op(bad, kind, 1.0)


def test_the_fuzzer_has_the_case():
    src = open(os.path.join(ROOT, "scripts", "fuzz_parity.py")).read()
    assert "def fuzz_fft(rng):" in src and 'CASES["fft"] = fuzz_fft' in src and "def case_fft" not in src


# ---------------------------------------------------------------------------------------------------- GPU
PATHS = pytest.mark.parametrize("general", [False, True], ids=["default", "general"])


def _strided(hl, cls, arr, row_pad=0, offset=0, fill=None, shape=None):
    """A (rows, N0, comps) or (rows, N0) float32 array in a HostArray or DevArray of its own (sentinels around it, rows `row_pad`
    floats longer than they need be, the first element `offset` bytes into the allocation), wrapped as the generator's buffer."""
    shape = arr.shape if shape is None else shape
    rows, n0, comps = shape if len(shape) == 3 else shape + (1,)
    rs = n0 * comps + row_pad
    a = cls(hl, (rows, n0 * comps), f32, row_stride=rs, offset=offset, fill=None if arr is None else np.asarray(arr, f32).reshape(rows, n0 * comps))
    if cls is DevArray:
        a.buf.device_detach()
        a.buf = hl.Buffer.wrap_device(a.p.value + offset, f32, [n0, rows, comps], [comps, rs, 1])
    else:
        a.buf = hl.fft_buffer(np.lib.stride_tricks.as_strided(a.host, (rows, n0, comps), (4 * rs, 4 * comps, 4)))
    a.row_stride, a.dense_shape = rs, shape
    return a


def _layout(a):
    return (a.buf.raw.device, a.row_stride)


def _gpu(hl, kind, x, n1, gain=1.0, general=False, cls=(HostArray, HostArray), pads=(0, 0), offsets=(0, 0), names=True):
    """the call on buffers of the given layouts; returns the output (the bytes around it checked) and asserts the launch names"""
    n0 = x.shape[1]
    i = _strided(hl, cls[0], x, pads[0], offsets[0])
    o = _strided(hl, cls[1], None, pads[1], offsets[1], shape=fc.out_shape(kind, n0, n1))
    try:
        run = lambda: (hl.debug_fft2d_general if general else hl.fft2d)(kind, i.buf, o.buf, gain, sizes=(n0, n1))
        if names:
            got_names = _launches(hl, run)
            assert sorted(set(got_names)) == sorted(set(expected_launches(kind, n0, n1, general, _layout(i), _layout(o)))), (kind, n0, n1, got_names)
        else:
            run()
        out = o.result().reshape(fc.out_shape(kind, n0, n1))
        i.result()   # the input and the bytes around it are as they were
        return out
    finally:
        i.free(), o.free()


@pytest.mark.gpu
@PATHS
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n0,n1", GPU_SIZES)
def test_sizes(hl, n0, n1, kind, general):
    canon = hl.canon_fma()
    _same(_gpu(hl, kind, _input(kind, n0, n1), n1, general=general), _want(kind, n0, n1, 1.0, canon), f"{kind} {n0}x{n1}")


@pytest.mark.gpu
def test_the_batching_constants_are_what_the_sizes_above_assume():
    assert ONE_GROUP_BYTES == 16384 and one_group(*AT_THE_BUDGET) and 8 * AT_THE_BUDGET[0] * AT_THE_BUDGET[1] == ONE_GROUP_BYTES
    assert not any(one_group(*s) for s in ABOVE_THE_BUDGET) and all(size_ok(a) and size_ok(b) for a, b in ABOVE_THE_BUDGET + [AT_THE_BUDGET])
    assert one_group(16, 16) and one_group(48, 36) and not one_group(36, 64) and not one_group(96, 64) and not one_group(4096, 2)
    assert expected_launches("c2c_forward", 16, 16, False) == ["fft_whole"] and expected_launches("r2c", 96, 64, False) == ["fft_cols", "fft_rows"]
    assert lines_per_group(True, 64, 36) == MIN_COLS and 36 % MIN_COLS != 0          # a last column tile of 4
    assert lines_per_group(True, 2048, 16) == LDS_COMPLEX // 2048 < MIN_COLS         # the LDS budget caps the tile
    assert lines_per_group(False, 8, 1024) == 2                                       # two rows per workgroup
    assert lines_per_group(True, 2, 4096) == MIN_COLS and lines_per_group(False, 4096, 2) == 1


@pytest.mark.gpu
@PATHS
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("gain", [0.0, -1.0, 0.3, 1.0 / 256])
def test_gains(hl, kind, gain, general):
    for n0, n1 in [(16, 16), (48, 36), (8, 8)]:
        _same(_gpu(hl, kind, _input(kind, n0, n1), n1, gain=gain, general=general), _want(kind, n0, n1, gain, hl.canon_fma()), f"{kind} gain {gain}")


@pytest.mark.gpu
@PATHS
@pytest.mark.parametrize("kind", KINDS)
def test_device_arrays_padded_rows_and_pointers_off_the_grid(hl, kind, general):
    """host and device buffers, rows 2 and 3 floats longer than dense, pointers 1 .. 3 floats off 16 bytes: the _elem kernels take every
    complex buffer that is not on 8 bytes with even rows; sentinels around both buffers must survive"""
    for n0, n1 in [(48, 36), (96, 64)]:   # one launch; two passes
        _layouts(hl, kind, general, n0, n1)


def _layouts(hl, kind, general, n0, n1):
    x, want = _input(kind, n0, n1), _want(kind, n0, n1, 1.0, hl.canon_fma())
    for cls, pads, offsets in [((DevArray, DevArray), (0, 0), (0, 0)), ((DevArray, HostArray), (2, 4), (0, 0)), ((HostArray, DevArray), (3, 3), (0, 0)),
                               ((DevArray, DevArray), (0, 0), (4, 0)), ((DevArray, DevArray), (0, 0), (0, 12)), ((DevArray, DevArray), (2, 6), (8, 8)),
                               ((DevArray, DevArray), (1, 0), (12, 4))]:
        _same(_gpu(hl, kind, x, n1, general=general, cls=cls, pads=pads, offsets=offsets), want, f"{kind} {cls} {pads} {offsets}")


@pytest.mark.gpu
def test_the_elem_kernels_are_chosen_by_alignment(hl):
    assert expected_launches("c2c_forward", 96, 64, False, (256, 192), (256, 192)) == ["fft_cols", "fft_rows"]
    assert expected_launches("c2c_forward", 96, 64, False, (260, 192), (256, 192)) == ["fft_cols", "fft_rows_elem"]
    assert expected_launches("c2c_forward", 96, 64, False, (256, 192), (256, 195)) == ["fft_cols_elem", "fft_rows"]
    assert expected_launches("r2c", 96, 64, False, (260, 97), (264, 192)) == ["fft_cols", "fft_rows"]
    assert expected_launches("r2c", 96, 64, False, (256, 96), (260, 192)) == ["fft_cols", "fft_rows_elem"]
    assert expected_launches("r2c", 8, 512, False, (256, 8), (260, 16)) == ["fft_cols_elem", "fft_rows"]
    assert expected_launches("c2r", 96, 64, False, (260, 192), (260, 97)) == ["fft_cols", "fft_rows_elem"]
    assert expected_launches("c2c_forward", 48, 36, False, (256, 96), (256, 96)) == ["fft_whole"]
    assert expected_launches("c2c_forward", 48, 36, False, (260, 96), (256, 96)) == ["fft_whole_elem"]
    assert expected_launches("c2r", 48, 36, False, (256, 96), (260, 49)) == ["fft_whole"]
    assert expected_launches("r2c", 48, 36, False, (260, 49), (256, 99)) == ["fft_whole_elem"]


@pytest.mark.gpu
@PATHS
def test_a_taller_c2r_input_whose_extra_rows_hold_nan(hl, general):
    for n0, n1 in [(16, 16), (48, 36), (8, 8)]:
        x = _input("c2r", n0, n1, extra_rows=3).copy()
        x[n1 // 2 + 1:] = np.nan
        want = _want("c2r", n0, n1, 1.0, hl.canon_fma(), 0, 3)
        _same(fc.run("c2r", x, n1=n1), want, "the checker reads no row above N1/2")
        assert not np.isnan(want).any()
        _same(_gpu(hl, "c2r", x, n1, general=general), want, f"c2r {n0}x{n1} under NaN rows")


def _subnormal(kind, n0, n1):
    return (_input(kind, n0, n1, seed=3) * f32(2.0 ** -130)).astype(f32)


FINITE_SPECIALS = np.array([0.0, -0.0, 1e-40, -3e-39, 2.0 ** -100, -2.0 ** -126, 1e36, -1e36], f32)
NON_FINITE = np.array([np.inf, -np.inf, np.nan, 3e38, -3e38], f32)   # +-3e38: a complex product of two of them overflows


def _special(kind, n0, n1, pool):
    """Noise with values of `pool` at the crossings of max(1, N0 / 16) columns and max(1, N1 / 16) rows"""
    rng = np.random.default_rng(n0 * 31 + n1)
    x = _input(kind, n0, n1, seed=4).copy()
    cols, rows = rng.choice(n0, max(1, n0 // 16), replace=False), rng.choice(x.shape[0], max(1, n1 // 16), replace=False)
    for r in rows:
        for c in cols:
            x[r, c] = rng.choice(pool, x[r, c].shape)
    return x


@pytest.mark.gpu
@PATHS
@pytest.mark.parametrize("kind", KINDS)
def test_subnormal_and_special_values(hl, kind, general):
    """Subnormal inputs; signed zeros, subnormals and magnitudes from 2^-126 to 1e36 among noise; and NaN, Inf and overflow.
    The cap on NaNs: every output of a 2-D transform depends on every input — the first dimension's pass spreads a NaN along its
    line, and every line of the second dimension crosses that line — so ONE NaN or Inf in the input reaches every output, however few
    lines hold them (a component stays finite only where the codelets happen not to mix it in).  No cap below "all" can be stated for
    them, and none is asserted.  The finite specials (at most (N0 / 16)(N1 / 16) values of 1e36: no sum overflows) leave the checker
    without any NaN, which is asserted; the non-finite inputs are compared NaN for NaN, Inf for Inf and number for number."""
    for n0, n1 in [(16, 16), (96, 64), (32, 16)]:
        with fc.canon(hl.canon_fma()):
            x = _subnormal(kind, n0, n1)
            want = fc.run(kind, x, n1=n1)
            assert np.abs(want).max() < 2.0 ** -115 and (want != 0).any()
            _same(_gpu(hl, kind, x, n1, general=general), want, f"{kind} subnormal {n0}x{n1}")
            x = _special(kind, n0, n1, FINITE_SPECIALS)
            want = fc.run(kind, x, n1=n1)
            assert np.isfinite(want).all()   # (so the cap of a quarter holds trivially: with no NaN in, none comes out)
            _same(_gpu(hl, kind, x, n1, general=general), want, f"{kind} finite specials {n0}x{n1}")
            x = _special(kind, n0, n1, NON_FINITE)
            x[0, 0] = np.nan if kind == "r2c" else (np.inf, 1.0)   # at least one, in a row that c2r reads
            want = fc.run(kind, x, n1=n1)
        assert not np.isfinite(want).all(), (kind, n0, n1)
        _same_or_nan(_gpu(hl, kind, x, n1, general=general), want, f"{kind} non-finite {n0}x{n1}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_the_four_entry_points_on_the_signals_of_the_reference(hl, kind, on_stream):
    x = _aot_signals()[kind]
    with fc.canon(hl.canon_fma()):
        want = fc.run(kind, x, n1=16, gain=AOT_GAIN[kind])
    for how in (call_direct, call_argv):
        i = hl.fft_buffer(np.ascontiguousarray(x))
        o = hl.fft_buffer(np.zeros(want.shape, f32))
        assert how(hl, AOT_ENTRY[kind], i, o) == 0
        got = o.numpy().reshape(want.shape)
        _same(got, want, AOT_ENTRY[kind])
        _accept_aot(kind, got)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_torch_op(hl, kind):
    import torch
    import halide_amd.torch_ops  # noqa: F401
    for n0, n1 in [(16, 16), (48, 36), (96, 64)]:
        x = _input(kind, n0, n1)
        got = torch.ops.hlmi.fft2d(torch.from_numpy(x).cuda(), kind, 0.5).cpu().numpy()
        _same(got, _gpu(hl, kind, x, n1, gain=0.5, names=False), f"torch {kind} {n0}x{n1} against hl.fft2d")
        _same(got, _want(kind, n0, n1, 0.5, hl.canon_fma()), f"torch {kind} {n0}x{n1}")
        # against torch.fft in complex128 on the CPU
        if kind == "c2c_forward":
            ref = torch.fft.fft2(torch.view_as_complex(torch.from_numpy(x.astype(f64)))).numpy() * 0.5
        elif kind == "c2c_inverse":
            ref = torch.fft.ifft2(torch.view_as_complex(torch.from_numpy(x.astype(f64))), norm="forward").numpy() * 0.5
        elif kind == "r2c":
            ref = torch.fft.fft2(torch.from_numpy(x.astype(f64))).numpy()[:n1 // 2 + 1] * 0.5
        else:   # irfft2 halves its last dimension: hand it dimension 1 there
            z = torch.view_as_complex(torch.from_numpy(x.astype(f64)))
            ref = torch.fft.irfft2(z.T, s=(n0, n1), norm="forward").T.numpy() * 0.5
        assert _rel(got, ref) <= bound(n0, n1)
    # a complex tensor's real view goes in and comes out without a copy
    z = torch.view_as_complex(torch.from_numpy(_input("c2c_forward", 16, 16)).cuda())
    out = torch.view_as_complex(torch.ops.hlmi.fft2d(torch.view_as_real(z), "c2c_forward", 1.0))
    assert torch.allclose(out.cpu(), torch.fft.fft2(z.cpu()), atol=1e-4)


@pytest.mark.gpu
def test_seeded_fuzz_slice_of_fft(on_stream):
    fuzz = load_fuzz_parity()
    rng = np.random.default_rng(20261019)
    for i in range(20 if on_stream == "device" else 6):
        desc, ok = fuzz.CASES["fft"](rng)
        assert ok, f"fft case {i} on the {on_stream} stream: {desc}"


@pytest.mark.gpu
def test_two_host_threads(hl):
    """two threads, each with its own buffers, calling different kinds at once: the shared twiddle cache and the arena under contention"""
    errors = []

    def worker(kinds, seed):
        try:
            for rep in range(6):
                for kind in kinds:
                    n0, n1 = [(16, 16), (48, 36), (96, 64)][(rep + seed) % 3]
                    x = _input(kind, n0, n1)
                    i, o = hl.fft_buffer(x.copy()), hl.fft_buffer(np.zeros(fc.out_shape(kind, n0, n1), f32))
                    hl.fft2d(kind, i, o, 1.0, sizes=(n0, n1))
                    if not np.array_equal(o.numpy().reshape(fc.out_shape(kind, n0, n1)).view(u32), _want(kind, n0, n1, 1.0, hl.canon_fma()).view(u32)):
                        errors.append((kind, n0, n1, rep))
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))

    for kind in KINDS:   # the references, before the threads start
        for n0, n1 in [(16, 16), (48, 36), (96, 64)]:
            _want(kind, n0, n1, 1.0, hl.canon_fma())
    ts = [threading.Thread(target=worker, args=(KINDS[:2], 0)), threading.Thread(target=worker, args=(KINDS[2:], 1))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
