"""reaction_diffusion_init, reaction_diffusion_update, reaction_diffusion_render and hlmi_reaction_diffusion_run: the simulation of
apps/HelloWasm.

The checker is tests/cpp/reaction_diffusion_check.c, a plain C restatement of apps/HelloWasm/generator/reaction_diffusion_generator.cpp
and of the random hash of src/Random.cpp in both canonical float forms, built and driven through ctypes by
tests/reaction_diffusion_checker.py.  The CPU tests hold the checker's hash to the reference's own acceptance
(test/correctness/random.cpp) and to an independent numpy restatement, its update to a float64 numpy reading of the generator and to
the order and geometry that follow from the generator's text, its render to a numpy restatement, and the entry points to their
contract; the GPU tests hold the library to the checker bit for bit.  Like every float pipeline here, the two are pinned to this
repository's restatement only: no output of a real Halide build is involved, and the (call id, definition tag) pairs the hash is fed
are derived by reading."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reaction_diffusion_checker as rc
from parity_helpers import ROOT, RUNGEN, DevArray, HostArray, call_argv, call_direct, load_fuzz_parity
from parity_helpers import gpu_present as _gpu_present, launches as _launches, same_bits as _same, same_bits_or_nan as _same_or_nan

NAMES = list(rc.NAMES)
f32, u32 = np.float32, np.uint32


@pytest.fixture(params=[0, 1], ids=["canon0", "canon1"])
def each_canon_rc(request):
    with rc.canon(request.param):
        yield request.param


@pytest.fixture
def canon_rc(hl):
    """the checker in the form the loaded library was built for"""
    with rc.canon(hl.canon_fma()):
        yield rc


def uniform(shape, seed, lo=0.0, hi=1.0):
    return (np.random.default_rng(seed).random(shape, dtype=f32) * f32(hi - lo) + f32(lo)).astype(f32)


# ---------------------------------------------------------------------------------------------------- CPU: the hash
C0, C1, C2 = u32(576942909), u32(1121052041), u32(1040796640)


def np_rng32(x):
    with np.errstate(over="ignore"):
        return (C2 * x + C1) * x + C0


def np_random_int(*e):
    """src/Random.cpp:66-90 on broadcast uint32 arrays, written from the source independently of the checker"""
    e = [np.asarray(v, np.int64).astype(u32) for v in e]
    r = np_rng32(e[0])
    with np.errstate(over="ignore"):
        for v in e[1:]:
            r = np_rng32(r + v)
    return r ^ (r >> u32(16))


def np_random_float(*e):
    bits = (u32(127 << 23) | (np_random_int(*e) >> u32(9))).astype(u32)
    return np.clip(bits.view(f32) - f32(1.0), f32(0), f32(1))


def test_the_checkers_hash_equals_a_numpy_restatement_bit_for_bit():
    rng = np.random.default_rng(5)
    n = 0
    for length in (1, 2, 3, 5, 6):
        lists = rng.integers(-2 ** 31, 2 ** 31, (800, length))
        lists[:50] = rng.integers(-3, 70, (50, length))   # the small arguments the pipelines feed it
        want_i, want_f = np_random_int(*lists.T), np_random_float(*lists.T)
        for e, wi, wf in zip(lists, want_i, want_f):
            assert rc.random_int(e) == int(wi), e
            assert rc.random_float(e).view(u32) == wf.view(u32), e
            n += 1
    assert n == 4000
    # the named calls feed it [id, tag, c, y, x], [frame, id, tag, c, v] and [frame, id, tag, c, y, x]
    t = rc.table()
    assert rc.init(((1, 1, 1)), mins=(5, 6, 2))[0, 0, 0] == np_random_float(*t["init"], 2, 6, 5)
    assert rc.edge_value("row_max", 9, 1, 33) == f32(np_random_float(9, *t["row_max"], 1, 33) * f32(0.2))
    assert rc.noise_value(-4, 3, 8, 2) == np_random_float(-4, *t["noise"], 2, 8, 3)


def test_the_table_of_ids_and_tags():
    """ids count the random_float calls of generate() from 0; tags count the Func definitions before the one that holds the call: init has
    none before its only one; update has the input's, repeat_edge's, blur_x, blur_y, blur and new_state's pure definition (0 .. 5), so the
    four edge updates are 6 .. 9 and noise 10"""
    assert rc.table() == {"init": (0, 0), "row_min": (0, 6), "row_max": (1, 7), "col_min": (2, 8), "col_max": (3, 9), "noise": (4, 10)}


@pytest.mark.parametrize("tag", [0, 1, 5, 9])
def test_the_hash_passes_the_references_acceptance(tag):
    """test/correctness/random.cpp on 1024 x 1024 of random_float(): mean, variance, mean and variance of the x and y gradients within
    0.01 of 0.5, 1/12, 0, 1/6; two seeds differ by 1/3 in mean absolute value; the same seed gives the same image.  The planes are made
    by the numpy restatement, which the test above holds equal to the checker's hash."""
    y, x = np.mgrid[0:1024, 0:1024]
    tol = 0.01
    plane = lambda *prefix: np_random_float(*prefix, 0, tag, y, x).astype(np.float64)   # [seed if given, id, tag, y, x]
    for r in (plane(), plane(1), plane(2)):
        assert abs(r.mean() - 0.5) < tol and abs(r.var() - 1 / 12) < tol
        for g in (r[:, 1:] - r[:, :-1], r[1:] - r[:-1]):
            assert abs(g.mean()) < tol and abs(g.var() - 1 / 6) < tol
    assert abs(np.abs(plane(1) - plane(2)).mean() - 1 / 3) < tol
    assert np.array_equal(plane(1), plane(1))
    # the checker's init is such a plane: [id, tag, c, y, x]
    t = rc.table()["init"]
    got = rc.init((1, 64, 64), mins=(3, 4, 2))
    assert np.array_equal(got[0], np_random_float(*t, 2, y[4:68, 3:67], x[4:68, 3:67]))


# ---------------------------------------------------------------------------------------------------- CPU: update against float64
def update64(state, mouse_x, mouse_y, frame, mins=(0, 0), pure_only=False):
    """The generator read in float64 numpy, its own words for the clamp, the edges and the clobber; the random values from the numpy hash.
    state (3, H, W) at mins (x, y); the output over the same box."""
    s = state.astype(np.float64)
    _, H, W = s.shape
    p = np.pad(s, ((0, 0), (2, 2), (2, 2)), mode="edge")   # repeat_edge
    at = lambda dx, dy: p[:, 2 + dy:2 + dy + H, 2 + dx:2 + dx + W]
    blur_x = at(-2, 0) + at(-1, 0) + at(0, 0) + at(1, 0) + at(2, 0)
    blur_y = at(0, -2) + at(0, -1) + at(0, 0) + at(0, 1) + at(0, 2)
    blur = (blur_x + blur_y) / 10
    R, G, B = blur
    s5 = 0.5
    R = R * ((1 - s5) + s5 * R * (3 - 2 * R))
    G = G * ((1 - s5) + s5 * G * (3 - 2 * G))
    B = B * ((1 - s5) + s5 * B * (3 - 2 * B))
    dR = B * (1 - R - G)
    dG = (1 - B) * (R - G)
    dB = 1 - B + 2 * G * R - R - G
    Y, X = np.mgrid[mins[1]:mins[1] + H, mins[0]:mins[0] + W]
    mx, my = mouse_x - X, mouse_y - Y
    boost = 5 * np.maximum(0, 1.0 - (mx * mx + my * my).astype(f32).astype(np.float64) * np.float64(f32(0.001))) + 1
    R = R + dR * np.float64(f32(0.14)) * boost
    G = G + dG * np.float64(f32(0.05)) * boost
    B = B + dB * np.float64(f32(0.065)) * boost
    out = np.clip(np.stack([R, G, B]), 0.0, 1.0)
    if pure_only:
        return out
    t = rc.table()
    c = np.arange(3)[:, None]
    fifth = f32(0.2)
    out[:, 0, :] = (np_random_float(frame, *t["row_min"], c, X[0][None, :]) * fifth).astype(np.float64)
    out[:, H - 1, :] = (np_random_float(frame, *t["row_max"], c, X[0][None, :]) * fifth).astype(np.float64)
    out[:, :, 0] = (np_random_float(frame, *t["col_min"], c, Y[:, 0][None, :]) * fifth).astype(np.float64)
    out[:, :, W - 1] = (np_random_float(frame, *t["col_max"], c, Y[:, 0][None, :]) * fifth).astype(np.float64)
    clamp = lambda v, lo, hi: max(min(v, hi), lo)
    x0, x1 = clamp(mouse_x - 10, 0, W - 1), clamp(mouse_x + 10, 0, W - 1)
    y0, y1 = clamp(mouse_y - 10, 0, H - 1), clamp(mouse_y + 10, 0, H - 1)
    n = lambda xx, yy: np_random_float(frame, *t["noise"], c[:, :, None], yy[None], xx[None])
    for yy in range(y0, y1 + 1):
        for xx in range(x0, x1 + 1):   # absolute coordinates
            if f32((xx - mouse_x) ** 2 + (yy - mouse_y) ** 2) < f32(100.0) and mins[0] <= xx < mins[0] + W and mins[1] <= yy < mins[1] + H:
                ax, ay = np.array([[xx]]), np.array([[yy]])
                v = f32(0.25) * (((n(ax, ay) + n(ax + 1, ay)) + n(ax + 1, ay + 1)) + n(ax, ay + 1))
                out[:, yy - mins[1], xx - mins[0]] = v[:, 0, 0]
    return out


def overridden(shape, mouse_x, mouse_y, mins=(0, 0)):
    """(edge mask, clobber mask) of an H x W frame at mins"""
    H, W = shape
    Y, X = np.mgrid[mins[1]:mins[1] + H, mins[0]:mins[0] + W]
    edge = (X == mins[0]) | (X == mins[0] + W - 1) | (Y == mins[1]) | (Y == mins[1] + H - 1)
    x0, x1, y0, y1 = rc.clobber_box(W, H, mouse_x, mouse_y)
    d2 = ((X - mouse_x) ** 2 + (Y - mouse_y) ** 2).astype(f32)
    return edge, (X >= x0) & (X <= x1) & (Y >= y0) & (Y <= y1) & (d2 < f32(100.0))


# The worst |checker - float64| of the pure stage measured over 300 steps of a 67 x 35 state with the edges re-noised, inputs uniform in
# [0, 1]: 2.33e-7 in canon 0, 2.29e-7 in canon 1.  The bound is four times the larger: a wrong tap, constant or order of
# the reaction terms misses by 1e-3 and more.
FLOAT64_BOUND = 4 * 2.33e-7


def test_update_against_a_float64_reading_of_the_generator(each_canon_rc):
    state = uniform((3, 35, 67), 1)
    worst = 0.0
    for step in range(12):
        mouse = ((30, 17), (0, 0), (66, 20), (1066, 17))[step % 4]
        got = rc.update(state, *mouse, step)
        want = update64(state, *mouse, step)
        edge, clob = overridden((35, 67), *mouse)
        free = ~(edge | clob)
        d = np.abs(got.astype(np.float64) - want)[:, free]
        worst = max(worst, float(d.max()))
        # the cap: the case is not one of saturated outputs
        assert np.count_nonzero((want == 0) | (want == 1)) <= want.size // 2 and np.unique(want).size > 8
        # the edge rows, the edge columns and the clobbered pixels are hash * 0.2f and blurry_noise exactly
        assert np.array_equal(got[:, edge | clob].astype(np.float64), want[:, edge | clob])
        if step % 4 == 0:
            assert clob.sum() > 250
        state = got
    print(f"canon {each_canon_rc}: largest |checker - float64| of the pure stage over 12 steps: {worst:.3g}")
    assert worst <= FLOAT64_BOUND


def test_the_two_forms_differ_on_update_and_agree_on_render():
    state = uniform((3, 35, 67), 2)
    with rc.canon(0):
        a, ra = rc.update(state, 30, 17, 0), rc.render(state)
    with rc.canon(1):
        b, rb = rc.update(state, 30, 17, 0), rc.render(state)
    assert np.count_nonzero(a.view(u32) != b.view(u32)) > a.size // 20
    assert np.array_equal(ra, rb)


# ---------------------------------------------------------------------------------------------------- CPU: order and geometry
def test_corners_carry_the_column_definitions_values(each_canon_rc):
    state = uniform((3, 9, 12), 3)
    out = rc.update(state, 1000, 1000, 7)
    for c in range(3):
        assert out[c, 0, 0] == rc.edge_value("col_min", 7, c, 0) and out[c, 8, 0] == rc.edge_value("col_min", 7, c, 8)
        assert out[c, 0, 11] == rc.edge_value("col_max", 7, c, 0) and out[c, 8, 11] == rc.edge_value("col_max", 7, c, 8)
        assert out[c, 0, 5] == rc.edge_value("row_min", 7, c, 5) and out[c, 8, 5] == rc.edge_value("row_max", 7, c, 5)
        assert out[c, 4, 0] == rc.edge_value("col_min", 7, c, 4) and out[c, 4, 11] == rc.edge_value("col_max", 7, c, 4)
    # stage by stage: the pure stage, then the edges, then the clobber
    pure, edges = rc.update(state, 1000, 1000, 7, stage=0), rc.update(state, 1000, 1000, 7, stage=1)
    assert np.array_equal(pure[:, 1:-1, 1:-1], out[:, 1:-1, 1:-1]) and np.array_equal(edges, out)
    assert not np.array_equal(pure[:, 0], out[:, 0])


def test_one_pixel_wide_and_high_states_carry_the_last_definitions_value(each_canon_rc):
    far = (1000, 1000)   # clobbers nothing within radius 10
    col = rc.update(uniform((3, 7, 1), 4), *far, 3)   # W = 1: column max is the last definition everywhere
    row = rc.update(uniform((3, 1, 7), 4), *far, 3)   # H = 1: row max, then the columns at the ends
    one = rc.update(uniform((3, 1, 1), 4), *far, 3)
    for c in range(3):
        assert [col[c, y, 0] for y in range(7)] == [rc.edge_value("col_max", 3, c, y) for y in range(7)]
        assert [row[c, 0, x] for x in range(1, 6)] == [rc.edge_value("row_max", 3, c, x) for x in range(1, 6)]
        assert row[c, 0, 0] == rc.edge_value("col_min", 3, c, 0) and row[c, 0, 6] == rc.edge_value("col_max", 3, c, 0)
        assert one[c, 0, 0] == rc.edge_value("col_max", 3, c, 0)


def test_the_mouse_on_a_corner_on_an_edge_and_far_outside(each_canon_rc):
    state = uniform((3, 30, 40), 5)
    H, W = 30, 40
    for mouse, some in (((0, 0), True), ((39, 29), True), ((20, 0), True), ((0, 15), True), ((20, 15), True), ((1039, 15), False), ((-1000, -1000), False)):
        out, edges = rc.update(state, *mouse, 11), rc.update(state, *mouse, 11, stage=1)
        _, clob = overridden((H, W), *mouse)
        assert bool(clob.any()) == some, mouse
        assert np.array_equal(out[:, ~clob], edges[:, ~clob])
        for y, x in np.argwhere(clob):   # the clobber wins over the edge noise
            for c in range(3):
                assert out[c, y, x] == rc.blurry_noise(11, int(x), int(y), c), (mouse, x, y)
        if some:
            edge, _ = overridden((H, W), *mouse)
            assert (clob & edge).any() == (mouse != (20, 15))
            assert not np.array_equal(out[:, clob], edges[:, clob])
    # the box is the bounding box: a pixel of the box outside the radius keeps its value
    assert rc.clobber_box(40, 30, 20, 15) == (10, 30, 5, 25) and rc.clobber_box(40, 30, 1039, 15) == (39, 39, 5, 25)
    assert rc.clobber_box(40, 30, -5, 100) == (0, 5, 29, 29)


def test_mins_move_the_edges_and_not_the_clobber(each_canon_rc):
    """a state with mins (-3, 5): the edges are at min / max, the clobber box at 0 .. W - 1, 0 .. H - 1 in absolute coordinates"""
    state = uniform((3, 35, 67), 6)
    mins, mouse = (-3, 5), (20, 20)
    out = rc.update(state, *mouse, 2, state_min=mins)
    want = update64(state, *mouse, 2, mins=mins)
    edge, clob = overridden((35, 67), *mouse, mins=mins)
    assert clob[20 - 5, 20 + 3] and clob.sum() > 250
    assert np.array_equal(out[:, edge | clob].astype(np.float64), want[:, edge | clob])
    assert np.abs(out.astype(np.float64) - want).max() <= FLOAT64_BOUND
    for c in range(3):
        assert out[c, 0, 10] == rc.edge_value("row_min", 2, c, 10 - 3) and out[c, 10, 66] == rc.edge_value("col_max", 2, c, 10 + 5)
        assert out[c, 15, 23] == rc.blurry_noise(2, 20, 20, c)
    # a mouse whose box leaves the frame: the output cannot hold it (x up to min(60 + 10, 66) = 66 > 63; y from max(8 - 10, 0) = 0 < 5)
    rc.update(state, 60, 20, 2, state_min=mins, expect=-4)
    rc.update(state, 20, 8, 2, state_min=mins, expect=-4)
    # a larger output holds it, and the pure stage continues the edge outside the frame
    big = rc.update(state, 60, 8, 2, state_min=mins, out_shape=(3, 45, 77), out_min=(-6, -2))
    pure = rc.update(state, 60, 8, 2, state_min=mins, out_shape=(3, 45, 77), out_min=(-6, -2), stage=0)
    assert np.array_equal(big[:, 42:, 4:69], pure[:, 42:, 4:69])       # below the last row: the pure stage of the repeated edge
    for c in range(3):   # the edge rows run over the OUTPUT's range in x, the columns over its range in y
        assert big[c, 7, 0] == rc.edge_value("row_min", 2, c, -6) and big[c, 0, 3] == rc.edge_value("col_min", 2, c, -2)
    # an output that misses a row or a column it must hold
    rc.update(state, 20, 20, 2, state_min=mins, out_shape=(3, 34, 67), out_min=mins, expect=-4)
    rc.update(state, 20, 20, 2, state_min=mins, out_shape=(3, 35, 66), out_min=(-2, 5), expect=-4)
    rc.update(np.zeros((3, 0, 5), f32), 0, 0, 0, out_shape=(3, 2, 2), out_min=(0, 0), expect=-4)


# ---------------------------------------------------------------------------------------------------- CPU: render
def render_np(state):
    """reaction_diffusion_generator.cpp:150-174 in float32 numpy"""
    s = state.astype(f32)
    v = s * (f32(1.01) - s) * f32(4)
    v = v * v
    v = v * v
    k = np.minimum(v, f32(1))
    R = np.minimum(k[0], (k[1] + k[2]) * f32(0.5))
    G = np.clip((k[1] + k[0] + k[2]) * f32(0.5), f32(0), f32(1))
    B = np.maximum(k[0], np.maximum(k[1], k[2]))
    ch = lambda a: (a * f32(255)).astype(np.uint32) & u32(0xff)
    return ch(B) | (ch(G) << u32(8)) | (ch(R) << u32(16)) | u32(255 << 24)


def render_grid():
    """every triple of 16 state values in [0, 1] — among them the constants 0, 0.5, 1 — and 1.01 beside them: (3, 17, 17 * 17)"""
    vals = np.array(sorted(set(np.linspace(0, 1, 13).astype(f32)) | {f32(0.6), f32(0.125), f32(0.99)}) + [f32(1.01)], f32)
    assert vals.size == 17
    a, b, c = np.meshgrid(vals, vals, vals, indexing="ij")
    return np.stack([a.reshape(17, 289), b.reshape(17, 289), c.reshape(17, 289)])


def test_render_against_a_numpy_restatement(each_canon_rc):
    grid = render_grid()
    assert np.array_equal(rc.render(grid), render_np(grid))
    noise_state = uniform((3, 35, 67), 8)
    assert np.array_equal(rc.render(noise_state), render_np(noise_state))
    for v, want in ((0.0, 0xff000000), (1.01, 0xff000000), (0.5, 0xffffffff)):
        assert rc.pack(v, v, v) == want, v
    # 1: v = (1 * 0.01f * 4)^4 = 2.56e-6 -> channel 0
    assert rc.pack(1.0, 1.0, 1.0) == 0xff000000
    # one channel lit: R = min(k0, (k1 + k2) / 2), G = sum / 2, B the largest
    assert rc.pack(0.5, 0.0, 0.0) == 0xff000000 | (127 << 8) | 255 and rc.pack(0.0, 0.5, 0.5) == 0xff000000 | (255 << 8) | 255


# ---------------------------------------------------------------------------------------------------- CPU: the library's surface
ARGS = {"reaction_diffusion_init": [("output", 2, 3, (2, 32))],
        "reaction_diffusion_update": [("state", 1, 3, (2, 32)), ("mouse_x", 0, 0, (0, 32)), ("mouse_y", 0, 0, (0, 32)), ("frame", 0, 0, (0, 32)),
                                      ("new_state", 2, 3, (2, 32))],
        "reaction_diffusion_render": [("state", 1, 3, (2, 32)), ("render", 2, 2, (1, 32))]}


def test_the_entry_points_are_exported_with_argv_and_metadata(hl):
    lib = C.CDLL(hl.LIB_PATH)
    for name in NAMES:
        for suffix in ("", "_argv", "_metadata"):
            assert hasattr(lib, name + suffix), name + suffix
        assert not hasattr(lib, name + "_auto_schedule")   # the reference builds no such object
        assert hl._fn[name] is not None
        md = hl.metadata(name)
        assert md.version == 1 and md.num_arguments == len(ARGS[name]) and md.name.decode() == name and b"hip" in md.target
        for x, (arg, kind, dims, typ) in zip((md.arguments[i] for i in range(md.num_arguments)), ARGS[name]):
            assert (x.name.decode(), x.kind, x.dimensions, (x.type.code, x.type.bits)) == (arg, kind, dims, typ)
            assert not x.buffer_estimates and not x.scalar_def and not x.scalar_min and not x.scalar_max and not x.scalar_estimate
    assert hasattr(lib, "hlmi_reaction_diffusion_run") and hasattr(lib, "hlmi_reaction_diffusion_general")
    for suffix in ("_argv", "_metadata"):   # a library extension, not an AOT entry point
        assert not hasattr(lib, "hlmi_reaction_diffusion_run" + suffix)


def test_the_aot_headers_compile_as_c(tmp_path):
    decl = open(os.path.join(ROOT, "include", "hlmi_pipelines.h")).read()
    assert "int reaction_diffusion_init(struct halide_buffer_t *output);" in decl
    assert "int reaction_diffusion_update(struct halide_buffer_t *state, int32_t mouse_x, int32_t mouse_y, int32_t frame, struct halide_buffer_t *new_state);" in decl
    assert "int reaction_diffusion_render(struct halide_buffer_t *state, struct halide_buffer_t *render);" in decl
    inc = ["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c"]
    src = tmp_path / "all.c"
    src.write_text("".join(f'#include "aot/{n}.h"\n' for n in NAMES)
                   + "int (*const f_init)(struct halide_buffer_t *) = reaction_diffusion_init;\n"
                   + "int (*const f_update)(struct halide_buffer_t *, int32_t, int32_t, int32_t, struct halide_buffer_t *) = reaction_diffusion_update;\n"
                   + "int (*const f_render)(struct halide_buffer_t *, struct halide_buffer_t *) = reaction_diffusion_render;\n"
                   + "int (*const f_run)(struct halide_buffer_t *, int32_t, int32_t, int32_t, int32_t, struct halide_buffer_t *, struct halide_buffer_t *) = "
                     "hlmi_reaction_diffusion_run;\n"
                   + "".join(f"int (*const a_{n})(void **) = {n}_argv;\nconst struct halide_filter_metadata_t *(*const m_{n})(void) = {n}_metadata;\n" for n in NAMES))
    subprocess.run(inc + [str(src), "-o", str(tmp_path / "all.o")], check=True)
    for name in NAMES:   # each alone, too
        one = tmp_path / (name + ".c")
        one.write_text(f'#include "aot/{name}.h"\nint (*const a)(void **) = {name}_argv;\n')
        subprocess.run(inc + [str(one), "-o", str(tmp_path / (name + ".o"))], check=True)


@pytest.mark.parametrize("name", NAMES)
def test_runner_describes_each_by_name(name):
    out = subprocess.run([RUNGEN, f"--name={name}", "--describe"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    for arg, kind, dims, typ in ARGS[name]:
        tname = {(2, 32): "float32", (0, 32): "int32", (1, 32): "uint32"}[typ]
        if kind == 0:
            assert f'Input "{arg}" is of type {tname}' in out.stdout, out.stdout
        else:
            assert f'{"Input" if kind == 1 else "Output"} "{arg}" is of type Buffer<{tname}> with {dims} dimensions' in out.stdout, out.stdout


# ---------------------------------------------------------------------------------------------------- CPU: the entry protocol
HOW = pytest.mark.parametrize("how", [call_direct, call_argv], ids=["direct_call", "argv"])


def _mk(hl, shape, dtype=f32, mins=None):
    return hl.Buffer(np.zeros(shape, dtype), mins=mins)


def _strided(hl, shape, dtype=f32):
    return hl.Buffer(np.zeros(shape[:-1] + (2 * shape[-1],), dtype)[..., ::2])   # stride.0 == 2


@HOW
def test_entry_protocol_of_init(hl, how):
    ok = 0 if _gpu_present() else -29   # with everything in order only the device can be missing
    call = lambda o: how(hl, "reaction_diffusion_init", o)
    assert call(None) == -12
    assert call(_mk(hl, (3, 4, 5), np.uint32)) == -3
    assert call(_mk(hl, (4, 5))) == -43
    assert call(_strided(hl, (3, 4, 5))) == -8 and "output.stride.0" in hl.last_error()
    assert call(_mk(hl, (3, 4, 5))) == ok and call(_mk(hl, (5, 4, 5), mins=(-7, 9, -2))) == ok   # any region and channel range


@HOW
def test_entry_protocol_of_update(hl, how):
    ok = 0 if _gpu_present() else -29
    call = lambda s, o, mouse=(8, 6), frame=0: how(hl, "reaction_diffusion_update", s, mouse[0], mouse[1], frame, o)
    S = (3, 12, 16)
    assert call(None, _mk(hl, S)) == -12 and call(_mk(hl, S), None) == -12
    assert call(_mk(hl, S, np.uint32), _mk(hl, S)) == -3 and call(_mk(hl, S), _mk(hl, S, np.float64)) == -3
    assert call(_mk(hl, S[1:]), _mk(hl, S)) == -43 and call(_mk(hl, S), _mk(hl, S[1:])) == -43
    assert call(_strided(hl, S), _mk(hl, S)) == -8 and "state.stride.0" in hl.last_error()
    assert call(_mk(hl, S), _strided(hl, S)) == -8 and "new_state.stride.0" in hl.last_error()
    # order: null before type before dimensionality before the constraints
    assert call(None, _mk(hl, S, np.uint32)) == -12 and call(_mk(hl, S[1:], np.uint32), _mk(hl, S)) == -3
    # c is pinned to [0, 3) on both
    assert call(_mk(hl, (4, 12, 16)), _mk(hl, S)) == -8 and "state.extent.2" in hl.last_error()
    assert call(_mk(hl, S), _mk(hl, (2, 12, 16))) == -8 and "new_state.extent.2" in hl.last_error()
    assert call(_mk(hl, S, mins=(0, 0, 1)), _mk(hl, S)) == -8 and "state.min.2" in hl.last_error()
    assert call(_mk(hl, S), _mk(hl, S, mins=(0, 0, -1))) == -8 and "new_state.min.2" in hl.last_error()
    # an output that misses a row, a column or a part of the clobber box it must hold
    assert call(_mk(hl, S), _mk(hl, (3, 11, 16))) == -4 and "new_state" in hl.last_error()
    assert call(_mk(hl, S), _mk(hl, (3, 11, 16), mins=(0, 1, 0))) == -4
    assert call(_mk(hl, S), _mk(hl, (3, 12, 15))) == -4 and call(_mk(hl, S), _mk(hl, (3, 12, 15), mins=(1, 0, 0))) == -4
    assert call(_mk(hl, S, mins=(-3, 5, 0)), _mk(hl, S, mins=(-3, 5, 0)), mouse=(8, 6)) == -4       # the box starts at y = 0 < 5
    assert call(_mk(hl, S, mins=(-3, 5, 0)), _mk(hl, S, mins=(-3, 5, 0)), mouse=(1, 11)) == -4      # ... and reaches x = 11 <= 12: held; y = 1 < 5
    assert call(_mk(hl, S, mins=(-3, 5, 0)), _mk(hl, S, mins=(-3, 5, 0)), mouse=(1, 15)) == ok      # x 0 .. 11, y 5 .. 11: inside [-3, 12] x [5, 16]
    # everything in order: the full frame, mins, padded strides, a larger output
    assert call(_mk(hl, S), _mk(hl, S)) == ok and call(_mk(hl, S), _mk(hl, (3, 20, 30), mins=(-5, -4, 0))) == ok
    pad = np.zeros((3, 15, 21), f32)[:, 1:13, 2:18]
    assert call(hl.Buffer(pad), hl.Buffer(pad.copy())) == ok
    # an empty state has no edge to repeat: -4, with the device in hand; nothing is read where the output is empty
    empty = lambda: hl.Buffer(np.zeros(S, f32)[:, :, :0])
    assert call(empty(), _mk(hl, S)) == (-4 if _gpu_present() else -29)
    assert call(empty(), hl.Buffer(np.zeros(S, f32)[:, :0])) == ok


@HOW
def test_entry_protocol_of_render(hl, how):
    ok = 0 if _gpu_present() else -29
    call = lambda s, r: how(hl, "reaction_diffusion_render", s, r)
    S, R = (3, 12, 16), (12, 16)
    assert call(None, _mk(hl, R, u32)) == -12 and call(_mk(hl, S), None) == -12
    assert call(_mk(hl, S, u32), _mk(hl, R, u32)) == -3 and call(_mk(hl, S), _mk(hl, R, f32)) == -3 and call(_mk(hl, S), _mk(hl, R, np.int32)) == -3
    assert call(_mk(hl, R), _mk(hl, R, u32)) == -43 and call(_mk(hl, S), _mk(hl, S, u32)) == -43
    assert call(_strided(hl, S), _mk(hl, R, u32)) == -8 and call(_mk(hl, S), _strided(hl, R, u32)) == -8
    # the state must cover render's x and y and channels [0, 3)
    assert call(_mk(hl, S), _mk(hl, (12, 17), u32)) == -4 and call(_mk(hl, S), _mk(hl, R, u32, mins=(0, 1))) == -4
    assert call(_mk(hl, (2, 12, 16)), _mk(hl, R, u32)) == -4 and call(_mk(hl, S, mins=(0, 0, 1)), _mk(hl, R, u32)) == -4
    assert call(_mk(hl, S), _mk(hl, R, u32)) == ok and call(_mk(hl, (5, 12, 16), mins=(0, 0, -1)), _mk(hl, (3, 4), u32, mins=(5, 6))) == ok


def _run(hl, s, n, o, r=None, mouse=(8, 6), frame0=0):
    fn = hl.lib.hlmi_reaction_diffusion_run
    fn.restype = C.c_int
    fn.argtypes = [hl._BP] + [C.c_int32] * 4 + [hl._BP] * 2
    return fn(s and s.ptr, mouse[0], mouse[1], frame0, n, o and o.ptr, r and r.ptr)


def test_runs_refusals(hl):
    ok = 0 if _gpu_present() else -29
    S, R = (3, 12, 16), (12, 16)
    assert _run(hl, None, 1, _mk(hl, S)) == -12 and _run(hl, _mk(hl, S), 1, None) == -12
    assert _run(hl, _mk(hl, S, u32), 1, _mk(hl, S)) == -3 and _run(hl, _mk(hl, S), 1, _mk(hl, S), _mk(hl, R)) == -3
    assert _run(hl, _mk(hl, S), 1, _mk(hl, S), _mk(hl, S, u32)) == -43
    for steps in (0, -1, -2 ** 31):
        assert _run(hl, _mk(hl, S), steps, _mk(hl, S)) == -8 and "steps" in hl.last_error()
    # unequal boxes
    assert _run(hl, _mk(hl, S), 2, _mk(hl, (3, 12, 17))) == -8 and "same box" in hl.last_error()
    assert _run(hl, _mk(hl, S), 2, _mk(hl, S, mins=(1, 0, 0))) == -8 and _run(hl, _mk(hl, S), 2, _mk(hl, (3, 20, 30), mins=(-5, -4, 0))) == -8
    assert _run(hl, _mk(hl, S), 2, _mk(hl, S), _mk(hl, (12, 15), u32)) == -8 and "render" in hl.last_error()
    # overlapping state and new_state: the same buffer, the same memory, memory that overlaps in part
    b = _mk(hl, S)
    assert _run(hl, b, 2, b) == -8 and "overlap" in hl.last_error()
    mem = np.zeros((4, 12, 16), f32)
    assert _run(hl, hl.Buffer(mem[:3]), 2, hl.Buffer(mem[:3])) == -8 and _run(hl, hl.Buffer(mem[:3]), 2, hl.Buffer(mem[1:])) == -8
    assert _run(hl, _mk(hl, (4, 12, 16)), 2, _mk(hl, S)) == -8 and "state.extent.2" in hl.last_error()
    assert _run(hl, _mk(hl, S, mins=(-3, 5, 0)), 2, _mk(hl, S, mins=(-3, 5, 0))) == -4   # the clobber box leaves the frame
    assert _run(hl, _mk(hl, S), 3, _mk(hl, S)) == ok and _run(hl, _mk(hl, S), 3, _mk(hl, S), _mk(hl, R, u32)) == ok


def _dims(b):
    return [(b.raw.dim[i].min, b.raw.dim[i].extent) for i in range(b.raw.dimensions)]


@HOW
def test_bounds_queries(hl, how):
    query = lambda dtype, n, mins=(11, 12, 13), ext=(14, 15, 16): hl.Buffer.bounds_query(dtype, n, mins=mins[:n], extents=ext[:n])
    # init: the output is the request
    q = query(f32, 3)
    assert how(hl, "reaction_diffusion_init", q) == 0 and _dims(q) == [(11, 14), (12, 15), (13, 16)]
    assert how(hl, "reaction_diffusion_init", query(f32, 2)) == -43
    # update, the output asked for: its own region and what the update definitions write, channels [0, 3)
    upd = lambda s, o, mouse=(8, 6): how(hl, "reaction_diffusion_update", s, mouse[0], mouse[1], 0, o)
    s, q = _mk(hl, (3, 12, 16), mins=(-3, 5, 0)), query(f32, 3, mins=(2, 7, 1), ext=(4, 3, 9))
    assert upd(s, q) == 0 and _dims(s) == [(-3, 16), (5, 12), (0, 3)]
    assert _dims(q) == [(-3, 19), (0, 17), (0, 3)]   # x: the frame -3 .. 12 and the box 0 .. 15; y: the box 0 .. 11 and the frame 5 .. 16
    q = query(f32, 3, mins=(-20, 30, 0), ext=(5, 5, 3))
    assert upd(s, q, mouse=(1, 15)) == 0 and _dims(q) == [(-20, 33), (5, 30), (0, 3)]
    # the state asked for: x and y as passed (every read clamps into whatever the state is), channels [0, 3)
    q, o = query(f32, 3), _mk(hl, (3, 12, 16))
    assert upd(q, o) == 0 and _dims(q) == [(11, 14), (12, 15), (0, 3)] and _dims(o) == [(0, 16), (0, 12), (0, 3)]
    # both (RunGen's way), one with the wrong type: rewritten
    qs, qo = query(np.uint8, 3, mins=(0, 0, 0), ext=(16, 12, 3)), query(f32, 3, mins=(0, 0, 0), ext=(16, 12, 3))
    assert upd(qs, qo) == 0 and _dims(qs) == _dims(qo) == [(0, 16), (0, 12), (0, 3)] and (qs.raw.type.code, qs.raw.type.bits) == (2, 32)
    assert upd(query(f32, 2), o) == -43
    # render: render is the request, the state gets its x and y and channels [0, 3)
    q, r = query(f32, 3), _mk(hl, (12, 16), u32, mins=(4, 5))
    assert how(hl, "reaction_diffusion_render", q, r) == 0 and _dims(q) == [(4, 16), (5, 12), (0, 3)] and _dims(r) == [(4, 16), (5, 12)]
    s, q = _mk(hl, (3, 12, 16)), query(u32, 2)
    assert how(hl, "reaction_diffusion_render", s, q) == 0 and _dims(q) == [(11, 14), (12, 15)] and _dims(s) == [(0, 16), (0, 12), (0, 3)]


def test_without_a_gpu_the_python_calls_refuse_to_run(hl):
    s, o, r = _mk(hl, (3, 12, 16)), _mk(hl, (3, 12, 16)), _mk(hl, (12, 16), u32)
    with pytest.raises(hl.HalideError) as e:
        hl.debug_reaction_diffusion_general("wavelet", s, out=o)
    assert e.value.code == -8
    if _gpu_present():
        return   # what follows is the statement about a machine without one
    for fn in (lambda: hl.reaction_diffusion_init(o), lambda: hl.reaction_diffusion_update(s, 1, 2, 3, o), lambda: hl.reaction_diffusion_render(s, r),
               lambda: hl.reaction_diffusion_run(s, 1, 2, 3, 4, o, r), lambda: hl.reaction_diffusion_run(s, 1, 2, 2 ** 31 - 3, 4, o),
               lambda: hl.debug_reaction_diffusion_general("reaction_diffusion_init", out=o),
               lambda: hl.debug_reaction_diffusion_general("reaction_diffusion_update", s, 1, 2, 3, out=o),
               lambda: hl.debug_reaction_diffusion_general("reaction_diffusion_render", s, render=r),
               lambda: hl.debug_reaction_diffusion_general("run", s, 1, 2, 3, 4, o, r)):
        with pytest.raises(hl.HalideError) as e:
            fn()
        assert e.value.code == -29


def test_torch_ops_shape_functions_and_cpu_refusal():
    import torch
    import halide_amd.torch_ops  # noqa: F401
    meta = torch.empty((3, 45, 70), dtype=torch.float32, device="meta")
    assert torch.ops.hlmi.reaction_diffusion_update(meta, 1, 2, 3).shape == (3, 45, 70)
    out = torch.ops.hlmi.reaction_diffusion_render(meta)
    assert out.shape == (45, 70) and out.dtype == torch.int32
    a, b = torch.ops.hlmi.reaction_diffusion_run(meta, 1, 2, 3, 4)
    assert a.shape == (3, 45, 70) and a.dtype == torch.float32 and b.shape == (45, 70) and b.dtype == torch.int32
    for op in (lambda t: torch.ops.hlmi.reaction_diffusion_update(t, 1, 2, 3), torch.ops.hlmi.reaction_diffusion_render,
               lambda t: torch.ops.hlmi.reaction_diffusion_run(t, 1, 2, 3, 4)):
        with pytest.raises(RuntimeError, match="GPU"):
            op(torch.zeros((3, 16, 16)))
        with pytest.raises(TypeError):
            op(torch.zeros((3, 16, 16), dtype=torch.int32))
        with pytest.raises(TypeError):
            op(torch.zeros((2, 16, 16)))
        with pytest.raises(TypeError):
            op(torch.zeros((16, 16)))
    with pytest.raises(RuntimeError, match="GPU"):
        torch.ops.hlmi.reaction_diffusion_init(4, 5, torch.device("cpu"))


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(params=["tiled", "general"])
def general(request, monkeypatch):
    """Both implementations (halide_amd/csrc/reaction_diffusion.hip): the LDS-tiled rd_steps<1> through the switch (rd_init and rd_render
    for the other two), and one thread per output through the hook.  The plan's own choice for update is the second."""
    if request.param == "tiled":
        monkeypatch.setenv("HLMI_RD_STEPS_PER_LAUNCH", "1")
    return request.param == "general"


# W x H.  Everything an edge; one row, one column; every pixel on an edge; smaller than the halo; every pixel inside the clobber box
# (the mouse in the centre); one past a 64 x 32 tile each way; 3 x 3 tiles with partial ones right and below
SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (4, 5), (21, 21), (67, 35), (130, 70)]
LAYOUTS = ["dense", "padded", "off1", "off3", "device_off2"]


def _arrays(hl, layout, shape, dtype, mins, fill=None):
    """a HostArray or DevArray of `shape` inside sentinels: dense; rows and planes padded to odd strides; the base 1 to 3 elements off"""
    h, w = shape[-2:]
    if layout == "dense":
        return HostArray(hl, shape, dtype, mins=mins, fill=fill)
    if layout == "padded":
        rs = (w + 5) | 1
        return HostArray(hl, shape, dtype, row_stride=rs, plane_stride=rs * (h + 2) + 3, mins=mins, fill=fill)
    if layout.startswith("off"):
        return HostArray(hl, shape, dtype, row_stride=w + 2, offset=int(layout[3:]) * np.dtype(dtype).itemsize, mins=mins, fill=fill)
    return DevArray(hl, shape, dtype, row_stride=w + 3, offset=2 * np.dtype(dtype).itemsize, mins=mins, fill=fill)


def _gpu_update(hl, state, mouse, frame, general, layout="dense", mins=(0, 0), out_shape=None, out_min=None):
    out_shape = state.shape if out_shape is None else out_shape
    out_min = mins if out_min is None else out_min
    a = _arrays(hl, layout, state.shape, f32, tuple(mins) + (0,), fill=state)
    o = _arrays(hl, layout, out_shape, f32, tuple(out_min) + (0,))
    if general:
        hl.debug_reaction_diffusion_general("reaction_diffusion_update", a.buf, mouse[0], mouse[1], frame, out=o.buf)
    else:
        hl.reaction_diffusion_update(a.buf, mouse[0], mouse[1], frame, o.buf)
    got = o.result()
    _same_or_nan(a.result(), state, "the state afterwards")
    a.free(), o.free()
    return got


def _gpu_render(hl, state, general, layout="dense", mins=(0, 0)):
    a = _arrays(hl, layout, state.shape, f32, tuple(mins) + (0,), fill=state)
    o = _arrays(hl, layout, state.shape[1:], u32, tuple(mins))
    if general:
        hl.debug_reaction_diffusion_general("reaction_diffusion_render", a.buf, render=o.buf)
    else:
        hl.reaction_diffusion_render(a.buf, o.buf)
    got = o.result()
    a.free(), o.free()
    return got


def _gpu_init(hl, shape, mins, general, layout="dense"):
    o = _arrays(hl, layout, shape, f32, mins)
    if general:
        hl.debug_reaction_diffusion_general("reaction_diffusion_init", out=o.buf)
    else:
        hl.reaction_diffusion_init(o.buf)
    got = o.result()
    o.free()
    return got


# parity_helpers' sentinel for uint32
from parity_helpers import SENTINEL  # noqa: E402
SENTINEL.setdefault(np.dtype(np.uint32), 0xA5C3A5C3)


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "x".join(map(str, s)))
def test_sizes(hl, canon_rc, on_stream, size, general):
    """init, update and render of a W x H frame: inputs uniform in [-0.5, 1.5], so that both clamp limits occur"""
    w, h = size
    state = uniform((3, h, w), w * 100 + h, -0.5, 1.5)
    mouse, frame = (w // 2, h // 2), 3 + w
    want = canon_rc.update(state, *mouse, frame)
    _same(_gpu_update(hl, state, mouse, frame, general), want, f"update {size}")
    if w >= 67:
        pure = canon_rc.update(state, *mouse, frame, stage=0)
        assert (pure == 0).any() and (pure == 1).any() and (want == 0).any() and (want == 1).any()
    if size == (21, 21):
        assert canon_rc.clobber_box(w, h, *mouse) == (0, 20, 0, 20)
    for layout in LAYOUTS[1:] if size in ((4, 5), (67, 35)) else ():
        _same(_gpu_update(hl, state, mouse, frame, general, layout), want, f"update {size} {layout}")
    inside = np.clip(state, 0, 1)
    _same(_gpu_render(hl, inside, general), canon_rc.render(inside), f"render {size}")
    _same(_gpu_init(hl, (3, h, w), (0, 0, 0), general), canon_rc.init((3, h, w)), f"init {size}")
    if size in ((4, 5), (67, 35), (130, 70)):
        for layout in LAYOUTS[1:]:
            _same(_gpu_render(hl, inside, general, layout, mins=(-3, 5)), canon_rc.render(inside), f"render {size} {layout}")
            _same(_gpu_init(hl, (4, h, w), (-3, 5, -1), general, layout), canon_rc.init((4, h, w), mins=(-3, 5, -1)), f"init {size} {layout}")


@pytest.mark.gpu
def test_mins_and_outputs_larger_than_the_frame(hl, canon_rc, on_stream, general):
    state = uniform((3, 35, 67), 21, -0.5, 1.5)
    mins = (-3, 5)
    for mouse in ((20, 20), (53, 15), (-1000, 20)):   # the box inside the frame, touching x max = 63 and y min = 5, degenerate at x = 0
        want = canon_rc.update(state, *mouse, 4, state_min=mins)
        for layout in ("dense", "padded", "off1"):
            _same(_gpu_update(hl, state, mouse, 4, general, layout, mins=mins), want, f"mins {mins} mouse {mouse} {layout}")
    # outputs larger than the frame: the general kernel on either path, the pure stage of the repeated edge around the frame
    for mouse, out_shape, out_min in (((60, 8), (3, 45, 77), (-6, -2)), ((30, 25), (3, 35, 140), (-3, 5)), ((2 ** 31 - 1, -2 ** 31), (3, 41, 70), (-3, -1))):
        want = canon_rc.update(state, *mouse, 4, state_min=mins, out_shape=out_shape, out_min=out_min)
        _same(_gpu_update(hl, state, mouse, 4, general, "padded", mins=mins, out_shape=out_shape, out_min=out_min), want, f"output {out_shape} at {out_min}")


def _special_state():
    """70 x 40 noise in [0, 1] with zeros of both signs, denormals, infinities and NaN inside, next to one another and on the edges"""
    big, tiny, den = f32(np.finfo(f32).max), f32(np.finfo(f32).tiny), np.uint32(0x00012345).view(f32)
    vals = np.array([np.nan, 1, np.inf, np.inf, -np.inf, 2, -0.0, -0.0, 0.0, -0.0, den, den, -den, tiny, big, -big, big, big, -np.inf, np.inf, 3, np.nan], f32)
    s = uniform((3, 40, 70), 31)
    s[0, 5, 3:3 + vals.size] = vals
    s[1, 6, 4:4 + vals.size] = vals[::-1]
    s[2, 20:20 + vals.size - 4, 60] = vals[4:]
    s[0, 0, 40:44] = (np.nan, np.inf, -0.0, den)          # on the edge row: repeated outwards
    s[1, 10:14, 69] = (-np.inf, -0.0, den, np.nan)
    s[:, 30:36, 10:30][:, ::2, ::3] = -0.0
    s[2, 30:36, 40:60] = den
    return s


@pytest.mark.gpu
def test_update_on_special_floats(hl, canon_rc, on_stream, general):
    """NaN, +-inf, -0, denormals, FLT_MAX next to -FLT_MAX, compared as bits; a NaN where the checker has a NaN"""
    state = _special_state()
    want = canon_rc.update(state, 500, 500, 1)
    assert np.isnan(want).any() or (want == 1).any()
    _same_or_nan(_gpu_update(hl, state, (500, 500), 1, general), want, "special values")
    _same_or_nan(_gpu_update(hl, state, (500, 500), 1, general, "padded", out_shape=(3, 50, 80), out_min=(-5, -5)),
                 canon_rc.update(state, 500, 500, 1, out_shape=(3, 50, 80), out_min=(-5, -5)), "special values, a larger output")


@pytest.mark.gpu
def test_the_paths_launch_what_they_say(hl, monkeypatch):
    s = uniform((3, 35, 67), 2)
    monkeypatch.delenv("HLMI_RD_STEPS_PER_LAUNCH", raising=False)
    assert _launches(hl, lambda: _gpu_update(hl, s, (5, 5), 0, False)) == ["rd_update_general"]   # the plan's choice: no instance beat it
    monkeypatch.setenv("HLMI_RD_STEPS_PER_LAUNCH", "3")
    with pytest.raises(hl.HalideError) as e:
        _gpu_update(hl, s, (5, 5), 0, False)
    assert e.value.code == -8
    monkeypatch.setenv("HLMI_RD_STEPS_PER_LAUNCH", "2")   # update is one step: any instance named takes rd_steps<1>
    for general, names in ((False, ("rd_steps1", "rd_render", "rd_init")), (True, ("rd_update_general", "rd_render_general", "rd_init_general"))):
        assert _launches(hl, lambda: _gpu_update(hl, s, (5, 5), 0, general)) == [names[0]]
        assert _launches(hl, lambda: _gpu_render(hl, s, general)) == [names[1]]
        assert _launches(hl, lambda: _gpu_init(hl, (3, 5, 7), (0, 0, 0), general)) == [names[2]]
    # an output that is not the full frame takes the general kernel under the switch too
    assert _launches(hl, lambda: _gpu_update(hl, s, (5, 5), 0, False, out_shape=(3, 36, 67))) == ["rd_update_general"]


@pytest.mark.gpu
def test_argv_equals_the_direct_call(hl, on_stream):
    s = uniform((3, 35, 67), 6)
    outs = []
    for how in (call_direct, call_argv):
        a, o, r, i = hl.Buffer(s.copy()), hl.Buffer(np.zeros_like(s)), hl.Buffer(np.zeros(s.shape[1:], u32)), hl.Buffer(np.zeros_like(s))
        assert how(hl, "reaction_diffusion_update", a, 30, 17, 5, o) == 0 and how(hl, "reaction_diffusion_render", a, r) == 0
        assert how(hl, "reaction_diffusion_init", i) == 0
        outs.append([np.ascontiguousarray(b.numpy()) for b in (o, r, i)])
    for x, y in zip(*outs):
        assert x.tobytes() == y.tobytes() and x.any()


@pytest.mark.gpu
def test_the_runner_runs_the_three(canon_rc, tmp_path):
    """hlmi_rungen goes through _metadata and the bounds queries: init -> update -> render through .npy files (the reference's layout: the
    shape tuple lists the Halide extents, x first)"""
    run = lambda *args: subprocess.run([RUNGEN, *args], capture_output=True, text=True, timeout=300)
    s, n, p = (str(tmp_path / f) for f in ("s.npy", "n.npy", "p.npy"))
    out = run("--name=reaction_diffusion_init", f"output={s}", "--output_extents=[40,24,3]")
    assert out.returncode == 0, out.stdout + out.stderr
    state = np.load(s).reshape(3, 24, 40)
    _same(state, canon_rc.init((3, 24, 40)), "rungen init")
    out = run("--name=reaction_diffusion_update", f"state={s}", "mouse_x=20", "mouse_y=12", "frame=3", f"new_state={n}", "--output_extents=[40,24,3]")
    assert out.returncode == 0, out.stdout + out.stderr
    new = np.load(n).reshape(3, 24, 40)
    _same(new, canon_rc.update(state, 20, 12, 3), "rungen update")
    out = run("--name=reaction_diffusion_render", f"state={n}", f"render={p}", "--output_extents=[40,24]")
    assert out.returncode == 0, out.stdout + out.stderr
    assert np.array_equal(np.load(p).reshape(24, 40), canon_rc.render(new))


# ---- run
RUN_SIZES = [(3, 3), (5, 4), (67, 35), (130, 70)]   # the first two smaller than every halo
RUN_STEPS = (1, 2, 3, 5, 9)
INT_MAX = 2 ** 31 - 1


def _launch_list(hl, fn):
    """names of the kernels one call launches, sorted, one entry per LAUNCH (the timing report has one entry per name, with its calls)"""
    hl.kernel_timing(True)
    hl.kernel_timing_reset()
    try:
        fn()
        return sorted(e["name"] for e in hl.kernel_timing_report() for _ in range(e["calls"]))
    finally:
        hl.kernel_timing(False)
        hl.kernel_timing_reset()


def _plan(S, steps):
    """launch sizes: steps of S, then the remainder in the next smaller instances"""
    out, s = [], S
    while steps:
        out += [s] * (steps // s)
        steps %= s
        s //= 2
    return out


def _chain(hl, state, mouse, frame0, steps):
    """the states after 1 .. steps single reaction_diffusion_update calls, and the render of each, on the GPU"""
    states, renders = [], []
    cur = hl.Buffer(state.copy())
    for k in range(steps):
        nxt, pix = hl.Buffer(np.zeros_like(state)), hl.Buffer(np.zeros(state.shape[1:], u32))
        hl.reaction_diffusion_update(cur, mouse[0], mouse[1], rc._i32(frame0 + k), nxt)
        hl.reaction_diffusion_render(nxt, pix)
        states.append(np.ascontiguousarray(nxt.numpy()).copy()), renders.append(np.ascontiguousarray(pix.numpy()).copy())
        cur = nxt
    return states, renders


@pytest.mark.gpu
@pytest.mark.parametrize("size", RUN_SIZES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("S", [0, 1, 2, 4], ids=["plan", "S1", "S2", "S4"])
def test_run_equals_single_updates_and_a_render(hl, canon_rc, on_stream, monkeypatch, size, S):
    """hlmi_reaction_diffusion_run by the plan's choice (one rd_update_general launch per step, then rd_render) and with S steps per launch through the switch: bit for bit that many reaction_diffusion_update calls and
    one reaction_diffusion_render, and the checker's; the mouse inside, on the border and outside; frame0 = 0 and 2^31 - 3 (the counter
    wraps as int32); render null and given; the state unchanged; a second run on the same buffers follows the new arguments"""
    if S:
        monkeypatch.setenv("HLMI_RD_STEPS_PER_LAUNCH", str(S))
    else:
        monkeypatch.delenv("HLMI_RD_STEPS_PER_LAUNCH", raising=False)
    w, h = size
    state = uniform((3, h, w), 7 * w + h, -0.5, 1.5)
    configs = [((w // 2, h // 2), 0), ((w - 1, 0), INT_MAX - 2), ((w + 500, -300), 5)]
    for ci, (mouse, frame0) in enumerate(configs):
        states, renders = _chain(hl, state, mouse, frame0, max(RUN_STEPS))
        _same(states[-1], canon_rc.run(state, *mouse, frame0, max(RUN_STEPS)), f"the chain of single updates {size} {mouse}")
        assert np.array_equal(renders[-1], canon_rc.render(states[-1]))
        a = _arrays(hl, "padded" if ci == 1 else "dense", state.shape, f32, (0, 0, 0), fill=state)
        o = _arrays(hl, "off1" if ci == 1 else "dense", state.shape, f32, (0, 0, 0))
        p = _arrays(hl, "off3" if ci == 1 else "dense", state.shape[1:], u32, (0, 0))
        for steps in RUN_STEPS:   # the same buffers again and again, with other arguments each time
            with_render = (steps + ci) % 2 == 0
            names = _launch_list(hl, lambda: hl.reaction_diffusion_run(a.buf, *mouse, frame0, steps, o.buf, p.buf if with_render else None))
            plan = _plan(S, steps) if S else None
            if S:
                want_names = [f"rd_steps{s}" for s in plan[:-1]] + [f"rd_steps{plan[-1]}" + ("_render" if with_render else "")]
            else:
                want_names = ["rd_update_general"] * steps + (["rd_render"] if with_render else [])
            assert names == sorted(want_names), (names, want_names)
            _same(o.result(), states[steps - 1], f"run {size} S {S} steps {steps} mouse {mouse} frame0 {frame0}")
            if with_render:
                assert np.array_equal(p.result(), renders[steps - 1]), f"render of run {size} S {S} steps {steps}"
            _same(a.result(), state, "the state afterwards")
        a.free(), o.free(), p.free()


@pytest.mark.gpu
def test_run_under_the_hook_is_one_launch_per_step(hl, canon_rc, on_stream):
    state = uniform((3, 35, 67), 9, -0.5, 1.5)
    a, o, p = hl.Buffer(state.copy()), hl.Buffer(np.zeros_like(state)), hl.Buffer(np.zeros(state.shape[1:], u32))
    names = _launch_list(hl, lambda: hl.debug_reaction_diffusion_general("run", a, 30, 17, INT_MAX, 3, o, p))
    assert names == ["rd_render_general"] + ["rd_update_general"] * 3
    want = canon_rc.run(state, 30, 17, INT_MAX, 3)
    _same(np.ascontiguousarray(o.numpy()), want, "run, general")
    assert np.array_equal(np.ascontiguousarray(p.numpy()), canon_rc.render(want))


# ---- torch
@pytest.mark.gpu
def test_torch_ops_equal_the_wrappers(hl, canon_rc):
    import torch
    import halide_amd.torch_ops  # noqa: F401
    state = uniform((3, 35, 67), 12, -0.5, 1.5)
    t = torch.from_numpy(state).cuda()
    side = torch.cuda.Stream()
    for stream in (torch.cuda.current_stream(), side):
        with torch.cuda.stream(stream):
            side.wait_stream(torch.cuda.default_stream())
            new = torch.ops.hlmi.reaction_diffusion_update(t, 30, 17, 5)
            pix = torch.ops.hlmi.reaction_diffusion_render(new)
            ran, ran_pix = torch.ops.hlmi.reaction_diffusion_run(t, 30, 17, 5, 3)
            first = torch.ops.hlmi.reaction_diffusion_init(35, 67, t.device)
        torch.cuda.synchronize()
        want = canon_rc.update(state, 30, 17, 5)
        _same(new.cpu().numpy(), want, "torch update")
        assert np.array_equal(pix.cpu().numpy().view(u32), canon_rc.render(want))
        want3 = canon_rc.run(state, 30, 17, 5, 3)
        _same(ran.cpu().numpy(), want3, "torch run")
        assert np.array_equal(ran_pix.cpu().numpy().view(u32), canon_rc.render(want3))
        _same(first.cpu().numpy(), canon_rc.init((3, 35, 67)), "torch init")
        assert np.array_equal(t.cpu().numpy(), state)
    # against the wrappers
    a, o = hl.Buffer(state.copy()), hl.Buffer(np.zeros_like(state))
    hl.reaction_diffusion_update(a, 30, 17, 5, o)
    _same(new.cpu().numpy(), np.ascontiguousarray(o.numpy()), "torch update against the wrapper")
    small = t[:, :9, :12].contiguous()
    torch.library.opcheck(torch.ops.hlmi.reaction_diffusion_update.default, (small, 3, 4, 5))
    torch.library.opcheck(torch.ops.hlmi.reaction_diffusion_render.default, (small,))
    torch.library.opcheck(torch.ops.hlmi.reaction_diffusion_run.default, (small, 3, 4, 5, 3))
    torch.library.opcheck(torch.ops.hlmi.reaction_diffusion_init.default, (9, 12, t.device))


# ---------------------------------------------------------------------------------------------------- a seeded slice of the fuzzer
@pytest.mark.gpu
def test_seeded_fuzz_slice_of_reaction_diffusion(on_stream):
    """scripts/fuzz_parity.py's reaction_diffusion case (the three entry points and run), a fixed number of cases from a fixed seed"""
    mod = load_fuzz_parity()
    rng = np.random.default_rng(20261021)
    for i in range(40):
        desc, ok = mod.CASES["reaction_diffusion"](rng)
        assert ok, f"case {i}: {desc}"
