"""Known-answer tests restated from the reference's own correctness tests (paths relative to /root/reference).

Every GPU parity test in this suite judges a kernel by the CPU oracle (oracle/).  The tests here judge the oracle's primitives
and its boundary handling by what the reference's tests and IR documentation state, and hold the kernels to the same
statements where the statement needs no oracle:

  1. integer division and modulo   src/IR.h:145-166, test/correctness/mod.cpp, mul_div_mod.cpp, div_round_to_zero.cpp
  2. float lerp                    test/correctness/lerp.cpp:59-73 (acceptance), :208-216 (ranges); src/Lerp.cpp:82-83,127-128
  3. repeat_edge clamps to the     test/correctness/boundary_conditions.cpp:62-83, src/BoundaryConditions.h:160-168
     input buffer, not its allocation
  4. saturating / wrapping casts   test/correctness/saturating_casts.cpp; apps/camera_pipe/camera_pipe_generator.cpp:369-403
     in camera_pipe's sharpen
  5. pyramid downsample            test/generator/pyramid_aottest.cpp (the reduction of a pyramid level, checked exactly on
                                   small integers; the reference's pyramid is a 2x2 box, local_laplacian's is [1 3 3 1] / 8)

Item 3 covers the pipelines whose generators apply repeat_edge to the caller's buffer: local_laplacian, bilateral_grid, nl_means,
unsharp and stencil_chain.  It leaves out the pipelines where the property does not hold as stated:
  lens_blur     the cost pyramid clamps to {0, w}, the input's own size (apps/lens_blur/lens_blur_generator.cpp:63), so a padded
                input changes the result;
  bgu           clamps internal Funcs, not the input;
  hist, max_filter   require an input min of 0;
  interpolate   runs at pinned shapes only.
"""
import ctypes as C

import numpy as np
import pytest

INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1


# ---------------------------------------------------------------------------------------------------------------------------
# 1. integer division and modulo
# ---------------------------------------------------------------------------------------------------------------------------
def _wrap32(v):
    return ((np.asarray(v, np.int64) + (1 << 31)) % (1 << 32)) - (1 << 31)


def _euclid(a, b):
    """Halide's Div / Mod (src/IR.h:145-166) on int64 arrays: a % b is in [0, |b|), (a / b) * b + a % b == a, x / 0 == x % 0 == 0,
    and the quotient wraps to int32 (INT_MIN / -1 == INT_MIN)."""
    a, b = np.broadcast_arrays(np.asarray(a, np.int64), np.asarray(b, np.int64))
    nz = b != 0
    babs = np.where(nz, np.abs(b), 1)
    r = np.where(nz, np.mod(a, babs), 0)
    q = np.where(nz, (a - r) // np.where(nz, b, 1), 0)
    return _wrap32(q), r


def test_div_mod_euclidean_on_a_dense_grid(oracle):
    """src/IR.h:145-166 and test/correctness/mod.cpp, mul_div_mod.cpp (div_mod over signed types), div_round_to_zero.cpp (which
    restates that plain `/` does NOT round to zero): every a in [-4096, 4096] against every b in [-64, 64], zero included.
    C's truncating division differs from this for every negative a or b that does not divide evenly."""
    a, b = np.meshgrid(np.arange(-4096, 4097, dtype=np.int32), np.arange(-64, 65, dtype=np.int32))
    a, b = a.ravel(), b.ravel()
    q, r = _euclid(a, b)
    got_q, got_r = oracle.fdiv(a, b), oracle.fmod(a, b)
    bad = (got_q != q) | (got_r != r)
    assert not bad.any(), (int(bad.sum()), a[bad][:6], b[bad][:6], got_q[bad][:6], q[bad][:6], got_r[bad][:6], r[bad][:6])
    assert oracle.fdiv(-7, -2)[0] == 4 and oracle.fmod(-7, -2)[0] == 1   # the examples of src/IR.h
    assert oracle.fdiv(-7, 2)[0] == -4 and oracle.fmod(-7, 2)[0] == 1


def test_div_mod_int32_edges(oracle):
    """src/IR.h:152-155: INT_MIN / -1 wraps to INT_MIN, and INT_MIN % -1 == 0; division by zero gives 0 for both."""
    edges = [INT_MIN, INT_MIN + 1, -2, -1, 0, 1, 2, INT_MAX - 1, INT_MAX]
    a, b = np.meshgrid(np.array(edges, np.int32), np.array(edges, np.int32))
    a, b = a.ravel(), b.ravel()
    q, r = _euclid(a, b)
    assert np.array_equal(oracle.fdiv(a, b), q) and np.array_equal(oracle.fmod(a, b), r)
    assert oracle.fdiv(INT_MIN, -1)[0] == INT_MIN and oracle.fmod(INT_MIN, -1)[0] == 0
    assert oracle.fdiv(INT_MIN, 0)[0] == 0 and oracle.fmod(INT_MAX, 0)[0] == 0
    assert oracle.fmod(INT_MIN, INT_MIN)[0] == 0 and oracle.fmod(-1, INT_MIN)[0] == INT_MAX
    # Python integers, one at a time: the same statement without numpy in between
    for x in edges:
        for y in edges:
            if y == 0:
                continue
            want_r = x % abs(y)
            want_q = (x - want_r) // y
            want_q = (want_q + (1 << 31)) % (1 << 32) - (1 << 31)
            assert (int(oracle.fdiv(x, y)[0]), int(oracle.fmod(x, y)[0])) == (want_q, want_r), (x, y)


def test_div_mod_euclidean_identity(oracle):
    """src/IR.h:158-160: (a / b) * b + a % b == a for b != 0 (int32 arithmetic, so INT_MIN / -1 holds it by wrapping), with
    0 <= a % b < |b|.  Random operands over all of int32 and small divisors of both signs."""
    rng = np.random.default_rng(3)
    a = rng.integers(INT_MIN, INT_MAX, 1 << 18, dtype=np.int64, endpoint=True).astype(np.int32)
    b = np.concatenate([rng.integers(INT_MIN, INT_MAX, 1 << 17, dtype=np.int64, endpoint=True),
                        rng.integers(-300, 301, 1 << 17)]).astype(np.int32)
    b[b == 0] = 1
    q, r = oracle.fdiv(a, b).astype(np.int64), oracle.fmod(a, b).astype(np.int64)
    assert np.array_equal(_wrap32(q * b + r), a.astype(np.int64))
    assert np.all((r >= 0) & (r < np.abs(b.astype(np.int64))))


def test_host_floor_div_is_only_used_with_positive_divisors():
    """halide_amd/csrc/hlmi_internal.h's floor_div rounds toward -inf for b > 0 only (its documented precondition).  Every call
    site divides by a positive constant: 2 (camera_pipe, interpolate, lens_blur, local_laplacian), 4 and S = 8 (bilateral_grid).
    The oracle's o_fdiv carries the full semantics; the host helper does not need them."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "halide_amd", "csrc")
    divisors = set()
    for name in sorted(os.listdir(csrc)):
        if not name.endswith((".hip", ".cpp")):
            continue
        with open(os.path.join(csrc, name)) as f:
            text = f.read()
        i = 0
        while True:
            i = text.find("floor_div(", i)
            if i < 0:
                break
            j, depth = i + len("floor_div("), 1
            while depth:
                depth += {"(": 1, ")": -1}.get(text[j], 0)
                j += 1
            divisors.add(text[i + len("floor_div("):j - 1].rsplit(",", 1)[1].strip())
            i = j
    assert divisors and divisors <= {"2", "4", "S"}, divisors
    with open(os.path.join(csrc, "bilateral_grid.hip")) as f:
        assert re.search(r"constexpr int S = 8;", f.read())


# ---------------------------------------------------------------------------------------------------------------------------
# 2. float lerp
# ---------------------------------------------------------------------------------------------------------------------------
def _lerp_grids():
    """lerp.cpp's float ranges (:208-216): values (i + min) * scale + offset evaluated in float, 100 of each.  Weights in 0...1 by
    1/100.  Returns (zero, one, w) as the full 100 x 100 x 100 product for each value grid."""
    f = np.float32
    idx = np.arange(100, dtype=np.float32)
    w = idx * f(0.01)
    out = []
    for scale, offset in ((f(0.01), f(0.0)), (f(0.1), f(-5.0))):
        v = idx * scale + offset
        z, o, ww = np.meshgrid(v, v, w, indexing="ij")
        out.append((z.ravel(), o.ravel(), ww.ravel()))
    return out


def _lerp_acceptance(zero, one, w, got):
    """lerp.cpp:59-73: relatively_equal against zero * (1 - w) + one * w in double: |diff| < 1e-4 or relative error < 2e-7."""
    want = zero.astype(np.float64) * (1.0 - w.astype(np.float64)) + one.astype(np.float64) * w.astype(np.float64)
    g = got.astype(np.float64)
    diff = np.abs(g - want)
    den = np.maximum(np.abs(g), np.abs(want))
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(den > 0, diff / den, 0.0)
    ok = (g == want) | (diff < 1e-4) | (rel < 2e-7)
    return ok


def _check_lerp(fn):
    for zero, one, w in _lerp_grids():
        got = fn(zero, one, w)
        ok = _lerp_acceptance(zero, one, w, got)
        assert ok.all(), (int((~ok).sum()), zero[~ok][:4], one[~ok][:4], w[~ok][:4], got[~ok][:4])
        # the endpoints exactly (src/Lerp.cpp:82-83: zero * (1 - w) + one * w)
        for wv, want in ((0.0, zero), (1.0, one)):
            ww = np.full_like(w, wv)
            got = fn(zero, one, ww)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) or np.array_equal(got, want), \
                (wv, int(np.count_nonzero(got != want)))


def _oracle_lerp(oracle):
    fn = oracle._lib.oracle_lerp_v
    fn.restype = None
    fn.argtypes = [C.c_void_p] * 4 + [C.c_size_t]

    def run(a, b, w):
        a, b, w = (np.ascontiguousarray(x, np.float32) for x in (a, b, w))
        out = np.empty_like(a)
        fn(a.ctypes.data, b.ctypes.data, w.ctypes.data, out.ctypes.data, a.size)
        return out
    return run


def test_oracle_lerp_acceptance_and_endpoints(oracle, each_canon):
    """lerp.cpp:59-73 acceptance over its float grids (:208-216), in both canonical forms of o_lerp (src/Lerp.cpp:127-128:
    zero * (1 - w) + one * w, the second product contracted under canon 1); w = 0 gives zero and w = 1 gives one exactly."""
    _check_lerp(_oracle_lerp(oracle))


@pytest.mark.gpu
def test_device_lerp_acceptance_and_endpoints(hl):
    """The same statement for the device's dev::lerpf (hlmi_debug_math, fn 4), in the canonical form the library was built for."""
    f = hl.lib.hlmi_debug_math
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]

    def run(a, b, w):
        a, b, w = (np.ascontiguousarray(x, np.float32) for x in (a, b, w))
        out = np.empty_like(a)
        assert f(4, a.ctypes.data, b.ctypes.data, w.ctypes.data, out.ctypes.data, a.size) == 0
        return out
    _check_lerp(run)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. repeat_edge clamps to the input buffer, not to its allocation
# ---------------------------------------------------------------------------------------------------------------------------
# boundary_conditions.cpp:62-83 realizes repeat_edge over a window wider than a buffer that is itself a crop of a larger
# allocation, and checks every pixel against clamp(x, min, min + extent - 1) of the crop.  The metamorphic form below needs no
# oracle as judge:
#   (A) the crop, passed as a strided view into a larger random image whose pixels around the crop differ from its edge, with
#       set_min at the crop's absolute coordinates;
#   (B) np.pad(crop, p, mode="edge"), dense, with its min moved by -p so that every original pixel keeps its coordinate.
# With p at least the pipeline's footprint radius, both equal the pipeline over the crop's window bit for bit.  A kernel (or
# oracle) that clamps to the allocation, to the output window or to a stride-derived extent sees the real neighbours in (A).
# Crops: widths that are no multiple of 4, 64 or the tile widths; odd and negative origins; 1-3 pixels in one dimension.
CROPS = [(37, 23, -13, 5), (2, 41, 7, -9), (67, 3, -131, 201), (1, 17, 0, 0), (130, 66, 61, -3)]
CROP_IDS = ["37x23@-13,5", "2x41@7,-9", "67x3@-131,201", "1x17@0,0", "130x66@61,-3"]


def _embed(crop, seed, margin=(5, 3, 4, 6)):
    """A larger random image holding `crop` at offset (margin[0], margin[1]) with margin[2] / margin[3] more columns / rows on the
    right / bottom; the pixels around the crop are made to differ from the crop's own edge."""
    lx, ty, rx, by = margin
    h, w = crop.shape[-2:]
    rng = np.random.default_rng(seed)
    shape = crop.shape[:-2] + (ty + h + by, lx + w + rx)
    if crop.dtype == np.uint16:
        big = rng.integers(0, 65536, shape, dtype=np.uint16)
        flip = lambda v: v ^ np.uint16(0x8000)
    else:
        big = rng.random(shape, dtype=np.float32)
        flip = lambda v: (v + np.float32(0.5)) % np.float32(1.0)
    big[..., ty:ty + h, lx:lx + w] = crop
    # the ring around the crop: each neighbour differs from the edge pixel next to it
    big[..., ty - 1, lx:lx + w] = flip(crop[..., 0, :])
    big[..., ty + h, lx:lx + w] = flip(crop[..., h - 1, :])
    big[..., ty:ty + h, lx - 1] = flip(crop[..., :, 0])
    big[..., ty:ty + h, lx + w] = flip(crop[..., :, w - 1])
    view = big[..., ty:ty + h, lx:lx + w]
    assert np.array_equal(view, crop) and not view.flags.c_contiguous or w == big.shape[-1]
    return big, view


def _pad(crop, p):
    return np.pad(crop, [(0, 0)] * (crop.ndim - 2) + [(p, p), (p, p)], mode="edge")


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _ll_footprint(x0, y0, w, h, J=8):
    """local_laplacian reads its input on G_0 (oracle/local_laplacian_oracle.c): R_0 = the output window,
    R_{j+1} = [fdiv(min - 1, 2), fdiv(max + 1, 2)] (upsample's source), G_{J-1} = R_{J-1},
    G_j = R_j U [2 min G_{j+1} - 1, 2 max G_{j+1} + 2] (downsample's source).  Returns the largest reach past the window."""
    def reach(lo, hi):
        R = [(lo, hi)]
        for _ in range(J - 1):
            R.append(((R[-1][0] - 1) // 2, (R[-1][1] + 1) // 2))
        G = R[-1]
        for j in range(J - 2, -1, -1):
            G = (min(2 * G[0] - 1, R[j][0]), max(2 * G[1] + 2, R[j][1]))
        return max(lo - G[0], G[1] - hi)
    return max(reach(x0, x0 + w - 1), reach(y0, y0 + h - 1))


def _ll_image(w, h, seed):
    return np.random.default_rng(seed).integers(0, 65536, (3, h, w), dtype=np.uint16)


def _gray_image(w, h, seed):
    return np.random.default_rng(seed).random((h, w), dtype=np.float32)


def _rgb_float(w, h, seed):
    return np.random.default_rng(seed).random((3, h, w), dtype=np.float32)


def _u16_image(w, h, seed):
    return np.random.default_rng(seed).integers(0, 65536, (h, w), dtype=np.uint16)


# footprint radius per pipeline (p below):
#   bilateral_grid  s_sigma = 8: the output reads grid cells [x / 8 - 2, x / 8 + 3] (blurx / blury 5 taps, the slice's lerp to
#                   xi + 1); cell X histograms clamped(8 X - 4 ... 8 X + 3): at most 7 + 16 + 4 = 27 left and 24 + 3 = 27 right
#   nl_means        patch / 2 + search / 2 (the patch sum of the search offset's difference image): 3 + 3 = 6 for 7 x 7
#   unsharp         the 7-tap blur in y, then in x: 3
#   stencil_chain   32 stages of a 5 x 5 stencil: 2 * 32 = 64
#   local_laplacian _ll_footprint: J = 8 pyramid levels reach 366 to 380 pixels past the windows of CROPS
BG_PAD, NLM_PAD, UNSHARP_PAD, STENCIL_PAD = 27, 6, 3, 64


@pytest.mark.parametrize("w,h,x0,y0", CROPS, ids=CROP_IDS)
@pytest.mark.parametrize("levels", [4, 8])
def test_oracle_repeat_edge_local_laplacian(oracle, w, h, x0, y0, levels):
    """local_laplacian_generator.cpp:28 repeat_edge(input); the pyramid taps are at absolute coordinates, so (A) and (B) are
    evaluated at the same origin.  The oracle's (A) is the crop itself: its clamp has only the crop to clamp to."""
    crop = _ll_image(w, h, seed=w * 7 + h)
    p = _ll_footprint(x0, y0, w, h)
    a = oracle.local_laplacian(crop, levels, 1.0 / 7, 1.0, origin=(x0, y0))
    b = oracle.local_laplacian(_pad(crop, p), levels, 1.0 / 7, 1.0, origin=(x0 - p, y0 - p))[:, p:p + h, p:p + w]
    assert _same(a, b), f"{np.count_nonzero(a != b)} of {a.size} differ (p = {p})"


@pytest.mark.parametrize("w,h,x0,y0", CROPS, ids=CROP_IDS)
def test_oracle_repeat_edge_bilateral_grid(oracle, w, h, x0, y0):
    """bilateral_grid_generator.cpp:18 repeat_edge(input); the grid cells are at absolute coordinates (x / s_sigma)."""
    crop = _gray_image(w, h, seed=w + 3 * h)
    p = BG_PAD
    a = oracle.bilateral_grid(crop, 0.1, origin=(x0, y0))
    b = oracle.bilateral_grid(_pad(crop, p), 0.1, origin=(x0 - p, y0 - p))[p:p + h, p:p + w]
    assert _same(a, b), f"{np.count_nonzero(_bits(a) != _bits(b))} of {a.size} differ"


@pytest.mark.parametrize("w,h,x0,y0", CROPS, ids=CROP_IDS)
def test_oracle_repeat_edge_translation_invariant_pipelines(oracle, w, h, x0, y0):
    """nl_means_generator.cpp:27, unsharp_generator.cpp:20, stencil_chain_generator.cpp:18: repeat_edge(input), no dependence on
    the absolute coordinate (the nl_means and stencil_chain oracles take none)."""
    rgb = _rgb_float(w, h, seed=w * h + 1)
    p = NLM_PAD
    a, b = oracle.nl_means(rgb, 7, 7, 0.12), oracle.nl_means(_pad(rgb, p), 7, 7, 0.12)[:, p:p + h, p:p + w]
    assert _same(a, b), "nl_means"
    p = UNSHARP_PAD
    a = oracle.unsharp(rgb, out_origin=(x0, y0), in_origin=(x0, y0))
    b = oracle.unsharp(_pad(rgb, p), out_origin=(x0, y0), out_size=(w, h), in_origin=(x0 - p, y0 - p))
    assert _same(a, b), "unsharp"
    g = _u16_image(w, h, seed=w + h)
    p = STENCIL_PAD
    a, b = oracle.stencil_chain(g), oracle.stencil_chain(_pad(g, p))[p:p + h, p:p + w]
    assert _same(a, b), "stencil_chain"


def test_repeat_edge_footprints_are_tight_enough_to_matter(oracle):
    """The pads above are not vacuous: one pixel less of padding than the footprint, filled with other values, changes the
    window's result (so (A) would see a kernel that reads past the crop), for the pipelines with the largest reach."""
    w, h, x0, y0 = 37, 23, -13, 5
    crop = _ll_image(w, h, seed=1)
    p = _ll_footprint(x0, y0, w, h)
    big, _ = _embed(crop, seed=2, margin=(p, p, p, p))
    a = oracle.local_laplacian(crop, 4, 1.0 / 7, 1.0, origin=(x0, y0))
    b = oracle.local_laplacian(big, 4, 1.0 / 7, 1.0, origin=(x0 - p, y0 - p))[:, p:p + h, p:p + w]
    assert not _same(a, b)
    g = _u16_image(w, h, seed=3)
    big, _ = _embed(g, seed=4, margin=(STENCIL_PAD,) * 4)
    s = STENCIL_PAD
    assert not _same(oracle.stencil_chain(g), oracle.stencil_chain(big)[s:s + h, s:s + w])


@pytest.fixture(params=["two_launches", "one_launch"])
def bg_path(request, monkeypatch):
    """bilateral_grid's two paths (tests/test_bilateral_grid.py): HLMI_BG_ONE_LAUNCH=1 selects the one-launch form."""
    if request.param == "one_launch":
        monkeypatch.setenv("HLMI_BG_ONE_LAUNCH", "1")
    return request.param


def _gpu_ab(hl, run, crop, p, x0, y0, seed):
    """Runs `run(in_buffer, out_buffer)` on (A) and (B); both outputs cover the crop's window at (x0, y0)."""
    nd = crop.ndim
    zmins = (0,) * (nd - 2)
    _, view = _embed(crop, seed)
    a_in = hl.Buffer(view).set_min(x0, y0, *zmins)
    a_out = hl.Buffer(np.zeros_like(crop)).set_min(x0, y0, *zmins)
    run(a_in, a_out)
    b_in = hl.Buffer(_pad(crop, p)).set_min(x0 - p, y0 - p, *zmins)
    b_out = hl.Buffer(np.zeros_like(crop)).set_min(x0, y0, *zmins)
    run(b_in, b_out)
    return a_out.numpy(), b_out.numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,x0,y0", CROPS, ids=CROP_IDS)
@pytest.mark.parametrize("levels", [4, 8])
def test_hip_repeat_edge_local_laplacian(hl, oracle, on_stream, w, h, x0, y0, levels):
    crop = _ll_image(w, h, seed=w * 7 + h)
    p = _ll_footprint(x0, y0, w, h)
    a, b = _gpu_ab(hl, lambda i, o: hl.local_laplacian(i, levels, 1.0 / 7, 1.0, o), crop, p, x0, y0, seed=5)
    want = oracle.local_laplacian(crop, levels, 1.0 / 7, 1.0, origin=(x0, y0))
    assert _same(a, b), f"(A) and (B) differ in {np.count_nonzero(a != b)} of {a.size}"
    assert _same(a, want), f"{np.count_nonzero(a != want)} of {a.size} differ from the oracle"


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,x0,y0", CROPS, ids=CROP_IDS)
def test_hip_repeat_edge_bilateral_grid(hl, oracle, bg_path, w, h, x0, y0):
    crop = _gray_image(w, h, seed=w + 3 * h)
    a, b = _gpu_ab(hl, lambda i, o: hl.bilateral_grid(i, 0.1, o), crop, BG_PAD, x0, y0, seed=6)
    want = oracle.bilateral_grid(crop, 0.1, origin=(x0, y0))
    assert _same(a, b), f"(A) and (B) differ in {np.count_nonzero(_bits(a) != _bits(b))} of {a.size}"
    assert _same(a, want), f"{np.count_nonzero(_bits(a) != _bits(want))} of {a.size} differ from the oracle"


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,x0,y0", CROPS, ids=CROP_IDS)
def test_hip_repeat_edge_translation_invariant_pipelines(hl, oracle, w, h, x0, y0):
    rgb = _rgb_float(w, h, seed=w * h + 1)
    a, b = _gpu_ab(hl, lambda i, o: hl.nl_means(i, 7, 7, 0.12, o), rgb, NLM_PAD, x0, y0, seed=7)
    assert _same(a, b), "nl_means: (A) and (B) differ"
    assert _same(a, oracle.nl_means(rgb, 7, 7, 0.12)), "nl_means: oracle"
    a, b = _gpu_ab(hl, hl.unsharp, rgb, UNSHARP_PAD, x0, y0, seed=8)
    assert _same(a, b), "unsharp: (A) and (B) differ"
    assert _same(a, oracle.unsharp(rgb, out_origin=(x0, y0), in_origin=(x0, y0))), "unsharp: oracle"
    g = _u16_image(w, h, seed=w + h)
    a, b = _gpu_ab(hl, hl.stencil_chain, g, STENCIL_PAD, x0, y0, seed=9)
    assert _same(a, b), "stencil_chain: (A) and (B) differ"
    assert _same(a, oracle.stencil_chain(g)), "stencil_chain: oracle"


# ---------------------------------------------------------------------------------------------------------------------------
# 4. saturating and wrapping casts in camera_pipe's sharpen
# ---------------------------------------------------------------------------------------------------------------------------
# camera_pipe_generator.cpp:369-403 under Halide's cast rules (test/correctness/saturating_casts.cpp, src/IROperator.cpp):
#   strength_x32 = u8_sat(sharpen * 32)          clamp to [0, 255] in float, then truncate
#   mask = i16(curved) - i16(unsharp)            |mask| <= 255: the difference of two u8 values
#   mask * strength_x32                          int16 (x) uint8 -> int16: wraps
#   / 32                                         floor division
#   u8(curved) + ...                             int16; u8_sat of it at the end
# strength 7.96875 is the largest that does not saturate (7.96875 * 32 = 255); 7.97, 8 and 1000 saturate to 255; 7.9 pins the
# truncation (252.8 -> 252); -1 clamps to 0.
SHARPEN = [0.0, 1.0 / 32, 4.0, 7.9, 7.96875, 7.97, 8.0, 1000.0, -1.0]


def _strength_x32(sharpen):
    return int(np.clip(np.float32(sharpen) * np.float32(32.0), 0, 255))   # float -> uint8 truncates


def _sharpen_int64(curved, strength, floor=True, wrap=True):
    """int64 restatement of the sharpen stage on curved (3, H + 2, W + 2) -> (3, H, W).  floor / wrap = False give the readings
    the cast rules exclude (C's truncating division, an unwrapped product), to show that the inputs tell them apart."""
    c = curved.astype(np.int64)
    avg = lambda a, b: (a + b + 1) >> 1                                             # blur121's rounding average, :20-22
    uy = avg(avg(c[:, :-2, :], c[:, 2:, :]), c[:, 1:-1, :])                        # unsharp_y on rows 0..H-1
    un = avg(avg(uy[:, :, :-2], uy[:, :, 2:]), uy[:, :, 1:-1])
    centre = c[:, 1:-1, 1:-1]
    mask = centre - un
    prod = (mask * strength + 32768) % 65536 - 32768 if wrap else mask * strength  # int16 (x) uint8 -> int16 wraps
    q = prod // 32 if floor else np.trunc(prod / 32).astype(np.int64)              # floor division
    v = (centre + q + 32768) % 65536 - 32768
    return np.clip(v, 0, 255).astype(np.uint8), mask, prod


def _extreme_curved(w, h, seed):
    """Curved values that reach |mask| near its bounds (isolated 255 on 0, 0 on 255, random extremes) next to mid-range noise."""
    rng = np.random.default_rng(seed)
    cv = rng.integers(0, 256, (3, h + 2, w + 2)).astype(np.uint8)
    cv[0, :, w // 2:] = np.where(rng.random((h + 2, w + 2 - w // 2)) < 0.5, 0, 255)
    cv[1, :, w // 2:] = 0
    cv[1, 2::4, w // 2 + 2::4] = 255
    cv[2, :, w // 2:] = 255
    cv[2, 2::4, w // 2 + 2::4] = 0
    return cv


@pytest.mark.parametrize("sharpen", SHARPEN)
def test_oracle_camera_pipe_sharpen_casts(oracle, sharpen):
    """The oracle's strength (setup) and sharpen stage against the int64 restatement; the inputs drive every cast site."""
    from test_camera_pipe import M3200, M7000
    s = _strength_x32(sharpen)
    assert oracle.camera_pipe_setup(M3200, M7000, 3700.0, 2.0, 50.0, sharpen, 25, 1023)[2] == s
    cv = _extreme_curved(45, 31, seed=int(abs(sharpen) * 7) + 1)
    want, mask, prod = _sharpen_int64(cv, s)
    got = oracle.camera_pipe_sharpen(cv, s)
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} of {got.size} differ"
    assert mask.max() >= 190 and mask.min() <= -190                   # the extremes of blur121's mask
    if s >= 200:                                                   # the int16 product wraps, and that shows
        assert not np.array_equal(want, _sharpen_int64(cv, s, wrap=False)[0])
    if s:                                                          # the final u8_sat clamps both ways
        assert np.any(want == 0) and np.any(want == 255)
    if s % 32:                                                     # floor and truncation differ, and that shows
        assert not np.array_equal(want, _sharpen_int64(cv, s, floor=False)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("sharpen", SHARPEN)
def test_hip_camera_pipe_sharpen_saturation(hl, oracle, sharpen):
    """The GPU against the oracle at the strengths above, on raw input of isolated extremes (0 and 1023 Bayer samples): the
    curved image then has the largest masks a raw frame reaches."""
    from test_camera_pipe import M3200, M7000, PARAMS
    rng = np.random.default_rng(11)
    raw = np.where(rng.random((152, 200)) < 0.5, 0, 1023).astype(np.uint16)
    raw[::7, ::5] = 1023
    p = dict(PARAMS, sharpen=sharpen)
    bi, b3, b7 = hl.Buffer(raw), hl.Buffer(M3200.copy()), hl.Buffer(M7000.copy())
    bo = hl.Buffer(np.zeros((3, 120, 160), np.uint8))
    hl.camera_pipe(bi, b3, b7, p["color_temp"], p["gamma"], p["contrast"], p["sharpen"], p["black"], p["white"], bo)
    got = bo.numpy()
    want = oracle.camera_pipe(raw, M3200, M7000, p["color_temp"], p["gamma"], p["contrast"], p["sharpen"], p["black"], p["white"],
                              160, 120)
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} of {got.size} differ"


def test_camera_pipe_raw_extremes_reach_large_masks(oracle):
    """The raw input of the GPU case above does drive the mask far out: sharpen 0 leaves curved itself as the output."""
    from test_camera_pipe import M3200, M7000, PARAMS
    rng = np.random.default_rng(11)
    raw = np.where(rng.random((152, 200)) < 0.5, 0, 1023).astype(np.uint16)
    raw[::7, ::5] = 1023
    p = dict(PARAMS, sharpen=0.0)
    cv = oracle.camera_pipe(raw, M3200, M7000, p["color_temp"], p["gamma"], p["contrast"], 0.0, p["black"], p["white"], 160, 120)
    _, mask, _ = _sharpen_int64(cv, 255)
    assert mask.max() >= 120 and mask.min() <= -120, (mask.min(), mask.max())
    assert np.any(np.abs(mask * 255) > 32767)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. pyramid downsample
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ox,oy", [(0, 0), (-3, 5), (7, -2)])
def test_oracle_ll_downsample_is_exact_on_small_integers(oracle, each_canon, ox, oy):
    """test/generator/pyramid_aottest.cpp checks a pyramid level exactly against integer arithmetic.  local_laplacian's level
    (local_laplacian_generator.cpp:267-273) is [1 3 3 1] / 8 in y, then in x, taps 2x - 1 ... 2x + 2 at absolute coordinates:
    on integers below 16 every partial sum is exact in float, so the level equals the integer sum / 64 bit for bit."""
    rng = np.random.default_rng(abs(ox * 31 + oy))
    ow, oh = 13, 9
    X0, Y0 = 2 * ox - 1, 2 * oy - 1                                   # the plane covers exactly what the window reads
    plane = rng.integers(0, 16, (2 * oh + 2, 2 * ow + 2)).astype(np.int64)
    k = np.array([1, 3, 3, 1], np.int64)
    want = np.zeros((oh, ow), np.int64)
    for y in range(oh):
        for x in range(ow):
            want[y, x] = k @ plane[2 * y:2 * y + 4, 2 * x:2 * x + 4] @ k
    got = oracle.ll_downsample(plane.astype(np.float32), (X0, Y0), (ox, oy), (ow, oh))
    assert np.array_equal(got, (want / 64.0).astype(np.float32))
