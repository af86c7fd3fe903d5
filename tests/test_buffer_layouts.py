"""The eleven pipelines whose own test files only ever pass dense host arrays (stencil_chain, hist, halide_blur, bilateral_grid,
camera_pipe, unsharp, harris, max_filter, iir_blur, interpolate, nl_means) on rows and planes longer than the image and on device
arrays whose first element sits off the word grid.  The layout must not change one bit of the result, and everything outside the
arrays (the bytes before the first element, the padding of rows and planes, the bytes after the last row; all filled with a
sentinel) must come back as it was.

The first half is one table: every pipeline runs the same six layout cases at two sizes.  The second half builds, per host shim
that picks a kernel variant from the layout, the layouts its predicate selects on.  Launch names do not tell the variants apart, so
each of those cases restates the shim's predicate on the buffers it built and asserts the variant that follows from it."""
import functools
from typing import Callable, NamedTuple

import numpy as np
import pytest

import parity_helpers as ph
from test_camera_pipe import M3200, M7000, PARAMS

u8, u16, f32 = np.uint8, np.uint16, np.float32
K = ph.kernel_const


def _ints(hi, dtype):
    return lambda shape, seed: np.random.default_rng(seed).integers(0, hi, shape, dtype=dtype)


def _rgba_with_holes(shape, seed):
    img = ph.noise(shape, seed)
    img[3][np.random.default_rng(seed + 1).random(shape[1:]) < 0.4] = 0.0   # the app's purpose: transparent holes
    return img


def _camera_pipe(hl, bi, bo):
    p = PARAMS
    hl.camera_pipe(bi, hl.Buffer(M3200.copy()), hl.Buffer(M7000.copy()), p["color_temp"], p["gamma"], p["contrast"], p["sharpen"], p["black"],
                   p["white"], bo)


def _camera_pipe_want(oracle, raw, w=None, h=None):
    p = PARAMS
    w, h = (raw.shape[1] - 32, raw.shape[0] - 24) if w is None else (w, h)
    return oracle.camera_pipe(raw, M3200, M7000, p["color_temp"], p["gamma"], p["contrast"], p["sharpen"], p["black"], p["white"], w, h)


class Pipe(NamedTuple):
    in_dtype: type
    out_dtype: type
    sizes: tuple          # output (w, h): one whose width meets the shim's vector condition, one whose width does not
    in_shape: Callable    # (w, h) -> the input's numpy shape
    out_shape: Callable   # (w, h) -> the output's numpy shape
    out_mins: tuple       # the output's mins, or None for zeros
    data: Callable        # (shape, seed) -> the dense input
    run: Callable         # (hl, input Buffer, output Buffer): the entry point
    want: Callable        # (oracle, dense input) -> the oracle's dense output


_same = lambda w, h: (h, w)
_rgb = lambda w, h: (3, h, w)
# heights cross one tile row of the kernel where a tile has at most 40 rows (stencil_chain's 96, max_filter's, iir_blur's and
# nl_means's 64 do not fit the few seconds a case may take; their edge tiles are what these sizes run)
PIPES = {
    "stencil_chain": Pipe(u16, u16, ((66, 12), (67, 12)), _same, _same, None, _ints(65536, u16),
                          lambda hl, a, o: hl.stencil_chain(a, o), lambda oracle, d: oracle.stencil_chain(d)),
    "hist": Pipe(u8, u8, ((64, 12), (61, 11)), _rgb, _rgb, None, _ints(256, u8),
                 lambda hl, a, o: hl.hist(a, o), lambda oracle, d: oracle.hist(d)),
    "halide_blur": Pipe(u16, u16, ((64, 4 * K("blur.hip", "ROWS") + 4), (62, 4 * K("blur.hip", "ROWS") + 3)),
                        lambda w, h: (h + 2, w + 2), _same, None, _ints(65536, u16),
                        lambda hl, a, o: hl.halide_blur(a, o), lambda oracle, d: oracle.blur(d)),
    "bilateral_grid": Pipe(f32, f32, ((64, 40), (61, 37)), _same, _same, None, ph.noise,
                           lambda hl, a, o: hl.bilateral_grid(a, 0.1, o), lambda oracle, d: oracle.bilateral_grid(d, 0.1)),
    "camera_pipe": Pipe(u16, u8, ((40, 2 * K("camera_pipe.hip", "FTY") + 2), (41, 27)), lambda w, h: (h + 24, w + 32), _rgb, None,
                        _ints(1024, u16), _camera_pipe, _camera_pipe_want),
    "unsharp": Pipe(f32, f32, ((64, K("unsharp.hip", "TH") + 5), (61, K("unsharp.hip", "TH") + 2)), _rgb, _rgb, None, ph.noise,
                    lambda hl, a, o: hl.unsharp(a, o), lambda oracle, d: oracle.unsharp(d)),
    "harris": Pipe(f32, f32, ((64, K("harris.hip", "TH") + 5), (61, K("harris.hip", "TH") + 3)), lambda w, h: (3, h + 6, w + 6), _same, (3, 3),
                   ph.noise, lambda hl, a, o: hl.harris(a, o), lambda oracle, d: oracle.harris(d)),
    "max_filter": Pipe(f32, f32, ((64, 40), (61, 37)), _rgb, _rgb, None, ph.noise,
                       lambda hl, a, o: hl.max_filter(a, o), lambda oracle, d: oracle.max_filter(d)),
    "iir_blur": Pipe(f32, f32, ((64, 40), (61, 37)), _rgb, _rgb, None, ph.noise,
                     lambda hl, a, o: hl.iir_blur(a, 0.3, o), lambda oracle, d: oracle.iir_blur(d, 0.3)),
    "interpolate": Pipe(f32, f32, ((64, 40), (61, 37)), lambda w, h: (4, h, w), _rgb, None, _rgba_with_holes,
                        lambda hl, a, o: hl.interpolate(a, o), lambda oracle, d: oracle.interpolate(d)),
    "nl_means": Pipe(f32, f32, ((64, 24), (59, 21)), _rgb, _rgb, None, ph.noise,
                     lambda hl, a, o: hl.nl_means(a, 7, 7, 0.12, o), lambda oracle, d: oracle.nl_means(d, 7, 7, 0.12)),
}
SIZED = [(name, size) for name, p in PIPES.items() for size in p.sizes]


@functools.lru_cache(maxsize=None)
def _dense(name, size):
    p = PIPES[name]
    d = p.data(p.in_shape(*size), seed=sum(size) + len(name))
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _want(name, size, canon):
    """the oracle's result in canonical form `canon`, computed once for every case of (name, size)"""
    import oracle_lib
    assert oracle_lib.get_canon() == canon
    w = PIPES[name].want(oracle_lib, _dense(name, size))
    w.setflags(write=False)
    return w


# ---------------------------------------------------------------------------------------------------- the table itself, on the CPU
def test_table_names_the_pipelines_in_scope():
    assert sorted(PIPES) == sorted(["stencil_chain", "hist", "halide_blur", "bilateral_grid", "camera_pipe", "unsharp", "harris", "max_filter",
                                    "iir_blur", "interpolate", "nl_means"])


@pytest.mark.parametrize("name,size", SIZED, ids=[f"{n}-{w}x{h}" for n, (w, h) in SIZED])
def test_oracle_runs_on_the_dense_data_of_every_row(oracle, name, size):
    p, (w, h) = PIPES[name], size
    d = _dense(name, size)
    assert d.shape == p.in_shape(w, h) and d.dtype == p.in_dtype
    want = _want(name, size, oracle.get_canon())
    assert want.shape == p.out_shape(w, h) and want.dtype == p.out_dtype
    assert len(np.unique(want)) > 8, "a constant result would hide a misplaced row"


def test_sizes_meet_and_miss_the_vector_width():
    for name, p in PIPES.items():
        (w0, _), (w1, _) = p.sizes
        unit = 2 if name == "stencil_chain" else 4
        assert w0 % unit == 0 and w1 % unit != 0, name


# ---------------------------------------------------------------------------------------------------- six layouts for every pipeline
class Lay(NamedTuple):
    """where an array lies: in host memory (the library mirrors the strides on the device) or in a device allocation of the
    test's own; `cols` and `rows` more than the image per row and per plane; the first element `off` ELEMENTS past the start"""
    where: str = "host"
    cols: int = 0
    rows: int = 0
    off: int = 0


def _make(hl, lay, shape, dtype, mins=None, fill=None):
    h, w = shape[-2:]
    cls = ph.HostArray if lay.where == "host" else ph.DevArray
    return cls(hl, shape, dtype, w + lay.cols, (w + lay.cols) * (h + lay.rows) if len(shape) == 3 else None, lay.off * np.dtype(dtype).itemsize,
               mins, fill)


DENSE, DEV = Lay(), Lay("dev")
CASES = {   # each a list of (input layout, output layout)
    "input_rows_one_longer": [(Lay(cols=1), DENSE)],
    "output_rows_one_longer": [(DENSE, Lay(cols=1))],
    "rows_and_planes_of_both_padded": [(Lay(cols=5, rows=3), Lay(cols=5, rows=3))],
    "input_off_the_grid": [(Lay("dev", off=k), DEV) for k in (1, 2, 3)],
    "output_off_the_grid": [(DEV, Lay("dev", off=k)) for k in (1, 2, 3)],
    "both_off_the_grid_and_padded": [(Lay("dev", 5, 3, k), Lay("dev", 5, 3, 4 - k)) for k in (1, 2, 3)],
}


def _run_on(hl, p, dense, want, a, o, what):
    """the entry point on the arrays `a` and `o`: the oracle's bits, the input and everything around both arrays as they were"""
    try:
        p.run(hl, a.buf, o.buf)
        ph.same_bits(o.result(), want, what)
        ph.same_bits(a.result(), dense, what + ": the input")
    finally:
        a.free(), o.free()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("name,size", SIZED, ids=[f"{n}-{w}x{h}" for n, (w, h) in SIZED])
def test_hip_result_does_not_depend_on_the_layout(hl, oracle, name, size, case):
    p, dense, want = PIPES[name], _dense(name, size), _want(name, size, oracle.get_canon())
    for lin, lout in CASES[case]:
        a = _make(hl, lin, dense.shape, p.in_dtype, fill=dense)
        o = _make(hl, lout, want.shape, p.out_dtype, mins=p.out_mins)
        if lin.where == "dev":   # the precondition of the off-grid cases, on the buffers themselves
            assert a.buf.raw.device % 256 == lin.off * dense.itemsize and o.buf.raw.device % 256 == lout.off * want.itemsize
        assert a.buf.dim(1).stride == dense.shape[-1] + lin.cols and o.buf.dim(1).stride == want.shape[-1] + lout.cols
        _run_on(hl, p, dense, want, a, o, f"{name} {size} {lin} -> {lout}")


# ---------------------------------------------------------------------------------------------------- stencil_chain: <first, pin, pout>
SC_FUSE, SC_LAUNCHES = K("stencil_chain.hip", "FUSE"), K("stencil_chain.hip", "STENCILS") // K("stencil_chain.hip", "FUSE")


def _sc_variants(a, o):
    """stencil_chain.hip's choice of stencil_fused8r<first, pin, pout> for its first and its last launch, restated: the
    intermediates are dense planes of the output's width plus a multiple of 4 * FUSE on aligned addresses, so between launches the
    width's parity decides; the user's buffers are checked for stride, address and (the input) the parity of the origins' distance"""
    W, even = o.buf.dim(0).extent, o.buf.dim(0).extent % 2 == 0
    dx0 = o.buf.dim(0).min - 2 * SC_FUSE * (SC_LAUNCHES - 1)
    pin = a.buf.dim(1).stride % 2 == 0 and a.buf.raw.device % 4 == 0 and (dx0 - 2 * SC_FUSE - a.buf.dim(0).min) % 2 == 0
    pout = o.buf.dim(1).stride % 2 == 0 and o.buf.raw.device % 4 == 0
    assert W > 0 and SC_LAUNCHES > 1
    return (True, pin, even), (False, even, pout)


T, F = True, False
SC_CASES = {   # (output w, h, x0, y0, row stride, byte offset), (input w, h, row stride, byte offset), first and last variant
    "dense_even_width": ((66, 12, 0, 0, 66, 0), (66, 12, 66, 0), (T, T, T), (F, T, T)),
    "dense_odd_width": ((67, 12, 0, 0, 67, 0), (67, 12, 67, 0), (T, F, F), (F, F, F)),
    "even_width_odd_input_stride": ((66, 12, 0, 0, 66, 0), (66, 12, 67, 0), (T, F, T), (F, T, T)),
    "odd_width_in_wider_even_input_even_origin": ((67, 12, 6, 4, 67, 0), (80, 20, 80, 0), (T, T, F), (F, F, F)),
    "even_width_odd_origin_difference": ((66, 12, 7, 3, 66, 0), (80, 20, 80, 0), (T, F, T), (F, T, T)),
    "input_two_bytes_off": ((66, 12, 0, 0, 66, 0), (66, 12, 66, 2), (T, F, T), (F, T, T)),
    "output_two_bytes_off": ((66, 12, 0, 0, 66, 2), (66, 12, 66, 0), (T, T, T), (F, T, F)),
    "output_rows_of_odd_stride": ((66, 12, 0, 0, 67, 0), (66, 12, 66, 0), (T, T, T), (F, T, F)),
    "odd_width_output_rows_of_even_stride": ((67, 12, 0, 0, 68, 0), (67, 12, 67, 0), (T, F, F), (F, F, T)),
}


def test_stencil_chain_cases_name_all_eight_variants():
    assert {v for c in SC_CASES.values() for v in c[2:]} == {(f, i, o) for f in (T, F) for i in (T, F) for o in (T, F)}


@functools.lru_cache(maxsize=None)
def _sc_full(iw, ih):
    import oracle_lib
    inp = _ints(65536, u16)((ih, iw), seed=iw * ih)
    return inp, oracle_lib.stencil_chain(inp)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SC_CASES)
def test_hip_stencil_chain_every_variant(hl, case):
    (w, h, x0, y0, osy, ooff), (iw, ih, isy, ioff), first, last = SC_CASES[case]
    inp, full = _sc_full(iw, ih)
    want = np.ascontiguousarray(full[y0:y0 + h, x0:x0 + w])
    a = ph.DevArray(hl, (ih, iw), u16, isy, offset=ioff, fill=inp)
    o = ph.DevArray(hl, (h, w), u16, osy, offset=ooff, mins=(x0, y0))
    assert (a.buf.raw.device % 4, a.buf.dim(1).stride, o.buf.raw.device % 4, o.buf.dim(1).stride, o.buf.dim(0).extent) == (ioff, isy, ooff, osy, w)
    assert _sc_variants(a, o) == (first, last)
    _run_on(hl, PIPES["stencil_chain"], inp, want, a, o, f"stencil_chain {case}")


# ---------------------------------------------------------------------------------------------------- hist: hist_count<vec>, hist_apply<vec>
def _hist_variants(a, o):
    """hist.hip's two choices restated (the input's mins are 0: its address is that of element (0, 0, 0))"""
    vec_in = a.buf.raw.device % 4 == 0 and a.buf.dim(1).stride % 4 == 0 and a.buf.dim(2).stride % 4 == 0
    count = vec_in and a.buf.dim(0).extent % 4 == 0
    apply = (vec_in and o.buf.dim(0).min % 4 == 0 and o.buf.dim(0).extent % 4 == 0 and o.buf.raw.device % 4 == 0 and o.buf.dim(1).stride % 4 == 0 and
             o.buf.dim(2).stride % 4 == 0)
    return count, apply


HIST_H = 12
HIST_CASES = {   # input (w, row stride, plane stride, byte offset), output (w, x0, row stride, plane stride, byte offset), (count, apply) vector
    "dense": ((64, 64, 64 * HIST_H, 0), (64, 0, 64, 64 * HIST_H, 0), (T, T)),
    "input_row_stride_65": ((64, 65, 65 * HIST_H, 0), (64, 0, 64, 64 * HIST_H, 0), (F, F)),
    "output_one_byte_off": ((64, 64, 64 * HIST_H, 0), (64, 0, 64, 64 * HIST_H, 1), (T, F)),
    "input_planes_2_mod_4": ((64, 64, 64 * HIST_H + 2, 0), (64, 0, 64, 64 * HIST_H, 0), (F, F)),
    "output_planes_2_mod_4": ((64, 64, 64 * HIST_H, 0), (64, 0, 64, 64 * HIST_H + 2, 0), (T, F)),
    "crop_off_the_word_grid": ((64, 64, 64 * HIST_H, 0), (56, 2, 56, 56 * HIST_H, 0), (T, F)),
    "width_66_cropped_to_64": ((66, 68, 68 * HIST_H, 0), (64, 0, 64, 64 * HIST_H, 0), (F, T)),
}


def test_hist_cases_name_all_four_combinations():
    assert {c[2] for c in HIST_CASES.values()} == {(c, a) for c in (T, F) for a in (T, F)}


@pytest.mark.gpu
@pytest.mark.parametrize("case", HIST_CASES)
def test_hip_hist_every_count_and_apply_variant(hl, oracle, case):
    (iw, isy, isc, ioff), (ow, x0, osy, osc, ooff), variants = HIST_CASES[case]
    inp = _ints(256, u8)((3, HIST_H, iw), seed=iw)
    want = oracle.hist(inp, out_origin=(x0, 0), out_size=(ow, HIST_H))
    a = ph.DevArray(hl, inp.shape, u8, isy, isc, ioff, fill=inp)
    o = ph.DevArray(hl, want.shape, u8, osy, osc, ooff, mins=(x0, 0, 0))
    assert (a.buf.raw.device % 4, a.buf.dim(1).stride, a.buf.dim(2).stride % 4) == (ioff, isy, isc % 4)
    assert (o.buf.raw.device % 4, o.buf.dim(1).stride, o.buf.dim(2).stride % 4, o.buf.dim(0).min) == (ooff, osy, osc % 4, x0)
    assert _hist_variants(a, o) == variants
    _run_on(hl, PIPES["hist"], inp, want, a, o, f"hist {case}")


# ---------------------------------------------------------------------------------------------------- camera_pipe: one launch or two
def _cp_variant(a, o):
    """camera_pipe.hip's choices restated: cp_fused_tile with or without dword stores, or cp_demosaic<aligned> and one of the two
    sharpen kernels.  The first raw sample a call reads is input(ox + 16, oy + 12)."""
    W, in_sy = o.buf.dim(0).extent, a.buf.dim(1).stride
    raw = a.buf.raw.device + 2 * ((o.buf.dim(1).min + 12 - a.buf.dim(1).min) * in_sy + o.buf.dim(0).min + 16 - a.buf.dim(0).min)
    aligned = in_sy % 2 == 0 and raw % 4 == 0
    dwords = o.buf.dim(1).stride % 4 == 0 and o.buf.dim(2).stride % 4 == 0 and o.buf.raw.device % 4 == 0
    if aligned and W % 2 == 0:
        return "cp_fused", dwords
    return "cp_demosaic", aligned, "cp_sharpen4" if W % 4 == 0 and dwords else "cp_sharpen"


CP_H = 28
CP_CASES = {   # output (w, row stride, byte offset), input (row stride, byte offset), the variant
    "dense_40": ((40, 40, 0), (72, 0), ("cp_fused", T)),
    "dense_42_rows_2_mod_4": ((42, 42, 0), (74, 0), ("cp_fused", F)),
    "width_42_rows_of_44": ((42, 44, 0), (74, 0), ("cp_fused", T)),
    "width_40_rows_of_42": ((40, 42, 0), (72, 0), ("cp_fused", F)),
    "output_one_byte_off": ((40, 40, 1), (72, 0), ("cp_fused", F)),
    "odd_raw_stride_40": ((40, 40, 0), (73, 0), ("cp_demosaic", F, "cp_sharpen4")),
    "odd_raw_stride_42": ((42, 42, 0), (75, 0), ("cp_demosaic", F, "cp_sharpen")),
    "raw_two_bytes_off_40": ((40, 40, 0), (72, 2), ("cp_demosaic", F, "cp_sharpen4")),
    "raw_two_bytes_off_42": ((42, 42, 0), (74, 2), ("cp_demosaic", F, "cp_sharpen")),
    "raw_two_bytes_off_40_output_rows_of_42": ((40, 42, 0), (72, 2), ("cp_demosaic", F, "cp_sharpen")),
    "odd_width_41_aligned_even_raw_stride": ((41, 41, 0), (74, 0), ("cp_demosaic", T, "cp_sharpen")),
    "odd_width_41_odd_raw_stride": ((41, 41, 0), (73, 0), ("cp_demosaic", F, "cp_sharpen")),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CP_CASES)
def test_hip_camera_pipe_every_path_and_variant(hl, oracle, case):
    (w, osy, ooff), (isy, ioff), variant = CP_CASES[case]
    raw = _ints(1024, u16)((CP_H + 24, w + 32), seed=w)
    want = _camera_pipe_want(oracle, raw)
    a = ph.DevArray(hl, raw.shape, u16, isy, offset=ioff, fill=raw)
    o = ph.DevArray(hl, want.shape, u8, osy, osy * CP_H, ooff)
    assert (a.buf.raw.device % 4, a.buf.dim(1).stride, o.buf.raw.device % 4, o.buf.dim(1).stride, o.buf.dim(0).extent) == (ioff, isy, ooff, osy, w)
    assert _cp_variant(a, o) == variant
    try:
        names = ph.launches(hl, lambda: _camera_pipe(hl, a.buf, o.buf))   # the path, at least, shows in the launch names
        assert [n for n in names if n != "cp_setup"] == (["cp_fused"] if variant[0] == "cp_fused" else ["cp_demosaic", "cp_sharpen"])
        ph.same_bits(o.result(), want, f"camera_pipe {case}")
        ph.same_bits(a.result(), raw, f"camera_pipe {case}: the input")
    finally:
        a.free(), o.free()


# ---------------------------------------------------------------------------------------------------- bilateral_grid: float4 staging or not
# bg_histogram_blurz_par<12> stages HTH / 12 grid cells of S pixels per workgroup, the first workgroup of a grid row from two
# cells and half a cell left of the output; it moves float4 only when `vec` holds AND all those columns exist.  At the widths of
# the table above no workgroup lies inside the image, so the input here reaches that far left of a 64-column output and the
# first workgroup of every row is an interior one.
BG_S, BG_SPAN = K("bilateral_grid.hip", "S"), (K("bilateral_grid.hip", "HTH") // 12) * K("bilateral_grid.hip", "S")
BG_XLO = -2 * BG_S - BG_S // 2
BG_CASES = {   # input (min x, width, row stride, byte offset), staged as float4
    "aligned": ((BG_XLO, 172, 172, 0), T),
    "input_row_stride_173": ((BG_XLO, 172, 173, 0), F),
    "input_row_stride_174": ((BG_XLO, 172, 174, 0), F),
    "input_4_bytes_off": ((BG_XLO, 172, 172, 4), F),
    "input_8_bytes_off": ((BG_XLO, 172, 172, 8), F),
    "input_12_bytes_off": ((BG_XLO, 172, 172, 12), F),
    "input_min_2_mod_4": ((BG_XLO - 2, 174, 176, 0), F),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", BG_CASES)
def test_hip_bilateral_grid_vector_and_scalar_staging(hl, oracle, case):
    (x0, iw, isy, ioff), vec = BG_CASES[case]
    w, h = 64, 40
    inp = ph.noise((h, iw), seed=3)
    want = np.ascontiguousarray(oracle.bilateral_grid(inp, 0.1, origin=(x0, 0))[:, -x0:-x0 + w])
    a = ph.DevArray(hl, inp.shape, f32, isy, offset=ioff, mins=(x0, 0), fill=inp)
    o = ph.DevArray(hl, (h, w), f32)
    assert (a.buf.raw.device % 16, a.buf.dim(1).stride, a.buf.dim(0).min) == (ioff, isy, x0)
    assert BG_XLO % 4 == 0 and int(1 / 0.1 + 0.5) + 2 <= 12            # the case table's premises: an aligned first column, the 12-plane kernel
    assert x0 <= BG_XLO and BG_XLO + BG_SPAN - 1 <= x0 + iw - 1        # the first workgroup of a grid row is an interior one
    assert (a.buf.raw.device % 16 == 0 and a.buf.dim(1).stride % 4 == 0 and a.buf.dim(0).min % 4 == 0) == vec   # bilateral_grid.hip's `vec`
    _run_on(hl, PIPES["bilateral_grid"], inp, want, a, o, f"bilateral_grid {case}")


# ---------------------------------------------------------------------------------------------------- halide_blur: 8-byte or per-element stores
@pytest.mark.gpu
@pytest.mark.parametrize("osy,ooff", [(64, 0), (64, 2), (64, 4), (64, 6), (65, 0), (66, 0)])
def test_hip_halide_blur_wide_and_narrow_stores(hl, oracle, osy, ooff):
    """blur3x3_u16 stores four outputs as 8 bytes where their address allows it, element by element elsewhere: with the output 2,
    4 or 6 bytes past an 8-byte address no store is wide, with rows of 65 one row in four, with rows of 66 every other row."""
    w, h = PIPES["halide_blur"].sizes[0]
    inp = _ints(65536, u16)((h + 2, w + 2), seed=9)
    a = ph.DevArray(hl, inp.shape, u16, fill=inp)
    o = ph.DevArray(hl, (h, w), u16, osy, offset=ooff)
    wide = sum((o.buf.raw.device + 2 * y * o.buf.dim(1).stride) % 8 == 0 for y in range(h))
    assert w % 4 == 0 and o.buf.raw.device % 8 == ooff and o.buf.dim(1).stride == osy
    assert wide == {(64, 0): h, (65, 0): (h + 3) // 4, (66, 0): (h + 1) // 2}.get((osy, ooff), 0)
    _run_on(hl, PIPES["halide_blur"], inp, oracle.blur(inp), a, o, f"halide_blur rows of {osy} at byte {ooff}")
