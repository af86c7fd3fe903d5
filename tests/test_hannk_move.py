"""hannk's data movement (halide_amd/csrc/hannk_move.hip): hlmi_hannk_copy_from and hlmi_hannk_gather.

CPU: the plan function on a table of layouts, the LDS layout of the transposing kernel under the bank model, the entry protocol.
GPU (-m gpu): copy_from and gather bit for bit against numpy, every copy once by the plan's choice and once under hlmi_hannk_general,
destinations inside sentinel bytes that must survive."""
from __future__ import annotations

import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

from parity_helpers import DevTensor, launches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts", "model"))
import lds_banks as lb  # noqa: E402

gpu = pytest.mark.gpu
DTYPES = (np.uint8, np.int16, np.float32, np.float64)   # element sizes 1, 2, 4, 8
TILE = {2: 64, 4: 64, 8: 32}   # the transposing kernel takes elements of 2, 4 and 8 bytes
PAD = {2: 2, 4: 1, 8: 1}


def data(shape, dtype, seed):
    """distinct bit patterns, no NaN payload games: small integers in every type"""
    r = np.random.default_rng(seed)
    return r.integers(0, 120, shape).astype(dtype)


def elem_strides(view):
    return tuple(s // view.itemsize for s in view.strides)


def shaped(hl, dtype, extents, strides, mins=None):
    """a buffer that has a shape and no memory, Halide order: all the plan function reads"""
    b = hl.Buffer.bounds_query(dtype, len(extents), mins, extents)
    for i, s in enumerate(strides):
        b._dims[i].stride = int(s)
    return b


# ------------------------------------------------------------------------------------------------------------------ CPU: the plan
PLAN_TABLE = [
    # what, dtype, extents, src strides, dst strides (Halide order) -> kernel, merged rank
    ("dense 3-D copy merges into one row", np.uint8, (24, 10, 10), (1, 24, 240), (1, 24, 240), "rows", 1),
    ("padded rows stay two dimensions", np.uint8, (24, 10, 10), (1, 32, 320), (1, 24, 240), "rows", 2),
    ("a row shorter than 16 bytes", np.uint8, (6, 10), (1, 8), (1, 6), "general", 2),
    ("the same row in 4-byte elements is 24 bytes", np.float32, (6, 10), (1, 8), (1, 6), "rows", 2),
    ("2-D transpose", np.int16, (64, 64), (64, 1), (1, 64), "transposing", 2),
    ("2-D transpose of bytes: the tile did not beat the general kernel", np.uint8, (64, 64), (64, 1), (1, 64), "general", 2),
    ("2-D transpose, one side below the tile threshold", np.float32, (15, 64), (64, 1), (1, 15), "general", 2),
    ("2-D transpose at the threshold", np.int16, (16, 16), (16, 1), (1, 16), "transposing", 2),
    ("TRANSPOSE fixture [384, 28, 16] -> [384, 16, 28]: channel rows", np.uint8, (384, 28, 16), (1, 384, 384 * 28), (1, 384 * 16, 384), "rows", 3),
    # c and bx merge into rows of 6 bytes; by, x' and y' follow each other in dst only
    ("space-to-depth 224^2 x 3, block 2", np.uint8, (3, 2, 112, 2, 112, 1), (1, 3, 6, 672, 1344, 0), (1, 3, 12, 6, 1344, 0), "general", 4),
    ("extent-1 dimensions drop", np.float64, (1, 64, 1, 64), (7, 64, 9, 1), (5, 1, 3, 64), "transposing", 2),
    ("dst's innermost stride is 2 (both dimensions merge: 128 = 2 * 64)", np.uint8, (64, 64), (1, 64), (2, 128), "general", 1),
    ("one element", np.float64, (1, 1), (1, 1), (1, 1), "general", 0),
    ("a negative dst stride is walked from its other end", np.uint8, (64, 4), (1, 64), (1, -64), "rows", 2),
    ("broadcast source", np.uint8, (64, 4), (1, 0), (1, 64), "rows", 2),
    ("rank 3 with the source's rows in the middle", np.float32, (20, 3, 20), (60, 20, 1), (1, 20, 60), "transposing", 3),
]


@pytest.mark.parametrize("case", PLAN_TABLE, ids=[c[0] for c in PLAN_TABLE])
def test_move_plan_table(hl, case):
    _, dtype, ext, ss, ds, kernel, rank = case
    src, dst = shaped(hl, dtype, ext, ss), shaped(hl, dtype, ext, ds)
    assert hl.debug_hannk_move_plan(src, dst) == {"kernel": kernel, "rank": rank}
    assert hl.debug_hannk_move_plan(src, dst, general=True) == {"kernel": "general", "rank": rank}


def test_move_plan_boxes(hl):
    # the intersection is what is planned: [4, 68) x [0, 64) of a transpose
    src, dst = shaped(hl, np.int16, (100, 64), (64, 1), (4, 0)), shaped(hl, np.int16, (68, 64), (1, 68), (0, 0))
    assert hl.debug_hannk_move_plan(src, dst) == {"kernel": "transposing", "rank": 2}
    # boxes that do not meet, and an extent of 0
    assert hl.debug_hannk_move_plan(shaped(hl, np.uint8, (8, 8), (1, 8), (0, 0)), shaped(hl, np.uint8, (8, 8), (1, 8), (8, 0)))["kernel"] == "none"
    assert hl.debug_hannk_move_plan(shaped(hl, np.uint8, (8, 0), (1, 8)), shaped(hl, np.uint8, (8, 0), (1, 8)))["kernel"] == "none"
    # a dst whose indices alias
    with pytest.raises(ValueError, match="aliases"):
        hl.debug_hannk_move_plan(shaped(hl, np.uint8, (8, 8), (1, 8)), shaped(hl, np.uint8, (8, 8), (1, 0)))
    # ... but not where the aliasing dimension has one element inside the box
    assert hl.debug_hannk_move_plan(shaped(hl, np.uint8, (32, 1), (1, 32)), shaped(hl, np.uint8, (32, 8), (1, 0)))["kernel"] == "rows"


@pytest.mark.parametrize("es", (2, 4, 8))
def test_transposing_tile_is_conflict_free_in_the_bank_model(es):
    """hannk_cf_transpose's tile[TILE][TILE + PAD]: a wave stores rows and loads columns; both cost the ideal cycles of their instruction"""
    with open(os.path.join(ROOT, "halide_amd", "csrc", "hannk_move.hip")) as fh:
        assert "constexpr int TILE = sizeof(T) == 8 ? 32 : 64, PAD = sizeof(T) == 2 ? 2 : 1;" in fh.read()
    tile, pad = TILE[es], PAD[es]
    lane = np.arange(64)
    tx, ty = lane % tile, lane // tile
    read, write = ("r64", "w64") if es == 8 else ("r32", "w32")   # sub-dword accesses bank like the dword that holds them
    for j in range(0, tile, 256 // tile):
        assert lb.cycles((tx * (tile + pad) + j + ty) * es, read) == lb.ideal(read), (es, j)
        assert lb.cycles(((j + ty) * (tile + pad) + tx) * es, write) <= lb.ideal(write), (es, j)
    # without the padding the column read is a full conflict: the padding is what the layout needs
    assert lb.cycles((tx * tile + ty) * es, read) >= 8 * lb.ideal(read)


def test_protocol_codes_and_order(hl):
    q = lambda dtype, n: hl.Buffer.bounds_query(dtype, n, None, [4] * n)   # noqa: E731
    real = lambda dtype, n: hl.Buffer(np.zeros((4,) * n, dtype))           # noqa: E731

    def code(fn, *a):
        with pytest.raises(hl.HalideError) as e:
            fn(*a)
        return e.value.code

    for general in (False, True):
        cf = lambda s, d: hl.hannk_copy_from(s, d, general)   # noqa: E731
        assert code(cf, None, real(np.uint8, 2)) == -12
        assert code(cf, real(np.uint8, 2), None) == -12
        assert code(cf, real(np.uint8, 3), real(np.int16, 2)) == -3       # the element size before the rank
        assert code(cf, real(np.uint8, 3), real(np.uint8, 2)) == -43
        assert code(cf, real(np.uint8, 9), real(np.uint8, 9)) == -43
        aliased = real(np.uint8, 2)
        aliased._dims[1].stride = 0
        assert code(cf, real(np.uint8, 2), aliased) == -8
        assert code(cf, real(np.uint8, 2), q(np.uint8, 2)) == -34
        # equal sizes of different type codes pass the type check (the float SPLIT copies f32): the next check answers
        assert code(cf, real(np.float32, 2), q(np.int32, 2)) == -34
    g = hl.hannk_gather_buffers
    idx = hl.Buffer(np.zeros(3, np.int32))
    assert code(g, None, idx, 0, real(np.uint8, 2)) == -12
    assert code(g, real(np.uint8, 2), idx, 0, real(np.int16, 2)) == -3
    assert code(g, real(np.uint8, 2), hl.Buffer(np.zeros(3, np.float32)), 0, real(np.uint8, 2)) == -3
    assert code(g, real(np.uint8, 2), idx, 0, real(np.uint8, 3)) == -43
    assert code(g, real(np.uint8, 2), hl.Buffer(np.zeros((1, 1, 1), np.int32)), 0, real(np.uint8, 4)) == -43
    assert code(g, real(np.uint8, 2), idx, 2, real(np.uint8, 2)) == -8
    assert code(g, real(np.uint8, 2), idx, 0, real(np.uint8, 2)) == -8    # dst's extent along the axis is 4, not 3


# ------------------------------------------------------------------------------------------------------------------ GPU: copy_from
class DevSource:
    """`view`, a numpy view of `flat` with any strides (negative and 0 included), as a device-only buffer over an upload of `flat`"""

    def __init__(self, hl, flat, view, mins=None):
        self.hip = hl.hip_runtime()
        self.p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), C.c_size_t(flat.nbytes)) == 0
        assert self.hip.hipMemcpy(self.p, C.c_void_p(flat.ctypes.data), C.c_size_t(flat.nbytes), 1) == 0
        off = view.__array_interface__["data"][0] - flat.__array_interface__["data"][0]
        assert 0 <= off < flat.nbytes
        self.buf = hl.Buffer.wrap_device(self.p.value + off, view.dtype, view.shape[::-1], elem_strides(view)[::-1], mins)

    def free(self):
        self.buf.device_detach()
        assert self.hip.hipFree(self.p) == 0


def check_copy(hl, src_view, src_flat, dst: DevTensor, want, kernels=None):
    """src (a view of src_flat) into dst, by the plan's choice and under hlmi_hannk_general; dst must end as `want`, its surroundings untouched"""
    before = dst.flat.copy()
    src = src_view if isinstance(src_view, (DevTensor, DevSource)) else DevSource(hl, src_flat, src_view)
    try:
        for general in (False, True):
            assert dst.hip.hipMemcpy(dst.p, C.c_void_p(before.ctypes.data), C.c_size_t(before.nbytes), 1) == 0
            names = launches(hl, lambda: hl.hannk_copy_from(src.buf, dst.buf, general))
            got = dst.result()
            assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), ("general" if general else "plan", names)
            if general:
                assert names in ([], ["hannk_cf_general"])
            elif kernels is not None:
                assert names == kernels
    finally:
        src.free()


SIZES_2D = [(1, 1), (3, 5), (31, 33), (32, 32), (63, 65), (64, 64), (65, 130)]


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("layout", ["dense", "padded_src", "padded_dst", "offset1", "offset2", "offset3"])
def test_hip_copy_from_2d_transposes(hl, dtype, layout):
    es = np.dtype(dtype).itemsize
    for k, (h, w) in enumerate(SIZES_2D):
        a = data((h, w), dtype, 100 * k + es)
        spad = 5 if layout == "padded_src" else 0
        dpad = 3 if layout == "padded_dst" else 0
        off = {"offset1": es, "offset2": 2 * es, "offset3": 3 * es}.get(layout, 0)
        src = DevTensor(hl, (h, w), (w + spad, 1), offset=off, fill=a, dtype=dtype)
        # dst is (w, h) in memory; its view in the source's order has the strides (1, h + dpad)
        dst = DevTensor(hl, (h, w), (1, h + dpad), offset=off, fill=7, dtype=dtype)
        want = "hannk_cf_transpose" if min(h, w) >= 16 and es >= 2 else "hannk_cf_general"
        try:
            check_copy(hl, src, None, dst, a, [want])
        finally:
            dst.free()


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", [(5, 7, 9), (17, 18, 19)], ids=["5x7x9", "17x18x19"])
def test_hip_copy_from_rank3_permutations(hl, dtype, shape):
    a = data(shape, dtype, 3)
    for perm in itertools.permutations(range(3)):
        out_shape = tuple(shape[p] for p in perm)
        dense = np.zeros(out_shape, dtype)
        view = dense.transpose(np.argsort(perm))   # the output in the input's order
        dst = DevTensor(hl, shape, elem_strides(view), fill=1, dtype=dtype)
        src = DevTensor(hl, shape, fill=a, dtype=dtype)
        try:
            check_copy(hl, src, None, dst, a)
            # what the device holds, read in the output's own order, is np.transpose
            back = np.empty_like(dst.flat)
            assert dst.hip.hipMemcpy(C.c_void_p(back.ctypes.data), dst.p, C.c_size_t(back.nbytes), 2) == 0
            assert np.array_equal(back[:dense.nbytes].view(dtype).reshape(out_shape), np.transpose(a, perm))
        finally:
            dst.free()


def space_to_depth_numpy(x, block):
    b, h, w, c = x.shape
    return x.reshape(b, h // block, block, w // block, block, c).transpose(0, 1, 3, 2, 4, 5).reshape(b, h // block, w // block, block * block * c)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape,block", [((3, 8, 6, 2), 2), ((1, 8, 8, 1), 4), ((1, 32, 64, 17), 2)], ids=["3x8x6x2_b2", "c1_b4", "32x64x17_b2"])
def test_hip_space_to_depth_rank6_views(hl, dtype, shape, block):
    x = data(shape, dtype, 11)
    want = space_to_depth_numpy(x, block)
    b, h, w, c = shape
    s6 = x.reshape(b, h // block, block, w // block, block, c)
    d6 = np.zeros(want.shape, dtype).reshape(b, h // block, w // block, block, block, c).transpose(0, 1, 3, 2, 4, 5)
    src = DevTensor(hl, s6.shape, elem_strides(s6), fill=s6, dtype=dtype)
    dst = DevTensor(hl, d6.shape, elem_strides(d6), fill=9, dtype=dtype)
    try:
        check_copy(hl, src, None, dst, s6)
        back = np.empty_like(dst.flat)
        assert dst.hip.hipMemcpy(C.c_void_p(back.ctypes.data), dst.p, C.c_size_t(back.nbytes), 2) == 0
        assert np.array_equal(back[:want.nbytes].view(dtype).reshape(want.shape), want)
    finally:
        dst.free()
    # the op-level wrappers on host arrays: the same views built by the package, and the inverse
    for general in (False, True):
        got = hl.hannk_space_to_depth(x, block, general)
        assert np.array_equal(got, want)
        assert np.array_equal(hl.hannk_depth_to_space(got, block, general), x)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_hip_copy_from_boxes(hl, dtype):
    # src covers [2, 42) x [-3, 27), dst [0, 37) x [5, 45) (Halide order x, y): the intersection [2, 37) x [5, 27) is a strict sub-box of both
    a = data((30, 40), dtype, 5)
    for transposed in (False, True):
        src = DevTensor(hl, (30, 40), mins=(2, -3), fill=a, dtype=dtype)
        dst = DevTensor(hl, (40, 37), (1, 40) if transposed else None, mins=(0, 5), fill=3, dtype=dtype)
        want = np.full((40, 37), 3, dtype)
        want[0:22, 2:37] = a[8:30, 0:35]
        try:
            check_copy(hl, src, None, dst, want, [("hannk_cf_transpose" if np.dtype(dtype).itemsize >= 2 else "hannk_cf_general") if transposed else "hannk_cf_rows"])
        finally:
            dst.free()
    # boxes that do not meet, and an extent of 0: nothing is launched, nothing written, the call returns 0
    for smins, shape in (((100, 0), (30, 40)), ((0, 0), (0, 40))):
        src = DevTensor(hl, shape, mins=smins, dtype=dtype)
        dst = DevTensor(hl, (30, 40) if shape[0] else shape, fill=3, dtype=dtype)
        try:
            check_copy(hl, src, None, dst, np.full(dst.shape, 3, dtype), [])
        finally:
            dst.free()


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_hip_copy_from_broadcast_and_negative_strides(hl, dtype):
    flat = data((70 * 40,), dtype, 8)
    a = flat.reshape(70, 40)
    it = a.itemsize
    cases = {
        "broadcast rows": (np.lib.stride_tricks.as_strided(a, (33, 40), (0, it)), None),
        "broadcast elements": (np.lib.stride_tricks.as_strided(a, (33, 40), (40 * it, 0)), None),
        "rows upside down": (a[::-1], None),
        "rows right to left": (a[:, ::-1], None),
        "both, transposed": (a[::-1, ::-1].T, None),
        "every other row": (a[::2], None),
    }
    for what, (view, _) in cases.items():
        dst = DevTensor(hl, view.shape, fill=2, dtype=dtype)
        try:
            check_copy(hl, view, flat, dst, view)
        finally:
            dst.free()
    # a dst with a negative stride: its buffer's first element is the last row of the memory
    rows = DevTensor(hl, (20, 32), fill=2, dtype=dtype)
    try:
        flipped = hl.Buffer.wrap_device(rows.buf.raw.device + 19 * 32 * it, dtype, (32, 20), (1, -32))
        src = DevTensor(hl, (20, 32), fill=a[:20, :32], dtype=dtype)
        for general in (False, True):
            hl.hannk_copy_from(src.buf, flipped, general)
            assert np.array_equal(rows.result(), a[:20, :32][::-1])
        flipped.device_detach()
        src.free()
    finally:
        rows.free()


@gpu
def test_hip_copy_from_host_buffers_keep_what_is_not_written(hl):
    a = data((12, 40), np.uint8, 1)
    dst = np.full((12, 40), 77, np.uint8)
    d = hl.Buffer(dst)
    hl.hannk_copy_from(hl.Buffer(a[:5], mins=(0, 3)), d)   # rows 3 .. 7 of dst
    want = np.full((12, 40), 77, np.uint8)
    want[3:8] = a[:5]
    assert np.array_equal(d.numpy(), want)
    for perm in itertools.permutations(range(3)):
        x = data((6, 20, 33), np.int16, 2)
        for general in (False, True):
            assert np.array_equal(hl.hannk_transpose(x, perm, general), np.transpose(x, perm))
    parts = [data((2, 3, n), np.float32, n) for n in (36, 5, 7)]
    whole = hl.hannk_concatenation(parts, -1)
    assert np.array_equal(whole, np.concatenate(parts, -1))
    for got, want in zip(hl.hannk_split(whole, [36, 5, 7], 2), parts):
        assert np.array_equal(got, want)
    assert all(np.array_equal(g, w) for g, w in zip(hl.hannk_split(whole, 3, 1), np.split(whole, 3, 1)))


@gpu
def test_hip_quantised_concatenation_and_split_go_through_the_add_kernel(hl):
    """inception_v4's 015.CONCATENATION: two inputs of different scales into one output; every piece is add_uint8(in * 1 + in * 0) with its
    own multiplier (requantize_or_copy), checked against the plain-C add checker"""
    import hannk_nn_checker as hn
    from halide_amd import tflite_reader as tfl
    g = tfl.read(os.path.join(ROOT, "tests", "golden", "hannk", "inception_v4_299_quant", "015.CONCATENATION.tflite"))
    op = g.ops[0]
    q = [(g.tensors[i].scale[0], g.tensors[i].zero[0]) for i in op.inputs + op.outputs]
    r = np.random.RandomState(15)
    parts = [r.randint(0, 256, (1, 5, 7, 19)).astype(np.uint8) for _ in op.inputs]
    mults = [hl.hannk_add_multipliers(qi[0], qi[0], q[-1][0], 0) for qi in q[:-1]]
    assert mults[0] != mults[1] and all(m[1] == 0 for m in mults)
    want = []
    for a, qi, m in zip(parts, q, mults):
        flat = a.reshape(-1, a.shape[-1])
        want.append(hn.add(flat, qi[1], m[0], flat, qi[1], 0, q[-1][1], 0, 255, [flat.shape[1], flat.shape[0]]).reshape(a.shape))
        assert np.array_equal(hl.hannk_requantize(a, qi, q[-1]), want[-1])
    got = hl.hannk_concatenation(parts, -1, quantization=q)
    assert np.array_equal(got, np.concatenate(want, -1))
    assert not np.array_equal(got, np.concatenate(parts, -1))        # the first input's scale differs from the output's
    back = hl.hannk_split(got, 2, -1, quantization=[q[-1], q[-1], q[-1]])
    flat = got.reshape(-1, got.shape[-1])
    m = hl.hannk_add_multipliers(q[-1][0], q[-1][0], q[-1][0], 0)
    same = hn.add(flat, q[-1][1], m[0], flat, q[-1][1], 0, q[-1][1], 0, 255, [flat.shape[1], flat.shape[0]]).reshape(got.shape)
    assert all(np.array_equal(b, w) for b, w in zip(back, np.split(same, 2, -1)))


# ------------------------------------------------------------------------------------------------------------------ GPU: gather
GATHER_INDICES = {"scalar": np.int32(3), "rank1": np.array([2, 0, 2, 3, 3, 1, 0], np.int32), "rank2": np.array([[1, 3, 1], [0, 0, 2]], np.int32)}


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("axis", (0, 1, 2))
@pytest.mark.parametrize("which", sorted(GATHER_INDICES))
def test_hip_gather_is_numpy_take(hl, dtype, axis, which):
    x = data((4, 5, 6), dtype, 21)
    idx = np.asarray(GATHER_INDICES[which])
    want = np.take(x, idx, axis)
    src = DevTensor(hl, x.shape, fill=x, dtype=dtype)
    ind = DevTensor(hl, idx.shape, fill=idx, dtype=np.int32)     # indices on the device: the kernel's flag is read back
    dst = DevTensor(hl, want.shape, offset=np.dtype(dtype).itemsize, fill=5, dtype=dtype)
    try:
        assert launches(hl, lambda: hl.hannk_gather_buffers(src.buf, ind.buf, x.ndim - 1 - axis, dst.buf)) == ["hannk_gather"]
        assert np.array_equal(dst.result(), want)
    finally:
        for t in (src, ind, dst):
            t.free()
    assert np.array_equal(hl.hannk_gather(x, idx, axis), want)   # host arrays: the indices are checked before the launch


@gpu
@pytest.mark.parametrize("where", ("device", "host"))
@pytest.mark.parametrize("bad", (4, -1))
def test_hip_gather_index_out_of_range_is_an_error_return(hl, where, bad):
    x = data((4, 5, 6), np.uint8, 22)
    idx = np.array([1, bad, 3], np.int32)
    want = np.full((3, 5, 6), 5, np.uint8)
    want[0], want[2] = x[1], x[3]      # the slice of the bad index keeps what dst held
    src = DevTensor(hl, x.shape, fill=x)
    ind = DevTensor(hl, idx.shape, fill=idx, dtype=np.int32) if where == "device" else None
    dst = DevTensor(hl, want.shape, fill=5)
    try:
        with pytest.raises(hl.HalideError) as e:
            hl.hannk_gather_buffers(src.buf, ind.buf if ind else hl.Buffer(idx), 2, dst.buf)
        assert e.value.code == -8
        assert np.array_equal(dst.result(), want)
    finally:
        for t in (src, ind, dst):
            if t:
                t.free()


# ------------------------------------------------------------------------------------------------------------------ GPU: torch ops
@gpu
def test_hip_torch_ops_equal_the_wrappers(hl):
    import torch
    import halide_amd.torch_ops  # noqa: F401
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    ops = torch.ops.hlmi
    x = data((2, 8, 6, 17), np.uint8, 31)
    for perm in ([0, 2, 1, 3], [3, 0, 1, 2], [1, 3, 0, 2]):
        got = ops.hannk_transpose(dev(x), perm).cpu().numpy()
        assert np.array_equal(got, hl.hannk_transpose(x, perm)) and np.array_equal(got, np.transpose(x, perm))
    f = data((20, 40), np.float32, 32)
    assert np.array_equal(ops.hannk_transpose(dev(f), [1, 0]).cpu().numpy(), f.T)
    s2d = ops.hannk_space_to_depth(dev(x), 2)
    assert np.array_equal(s2d.cpu().numpy(), hl.hannk_space_to_depth(x, 2)) and np.array_equal(s2d.cpu().numpy(), space_to_depth_numpy(x, 2))
    assert np.array_equal(ops.hannk_depth_to_space(s2d, 2).cpu().numpy(), x)
    idx = np.array([[1, 5, 1], [0, 0, 4]], np.int32)
    for axis in (0, 1, 2, 3, -1):
        i = idx % x.shape[axis]
        got = ops.hannk_gather(dev(x), dev(i), axis).cpu().numpy()
        assert np.array_equal(got, hl.hannk_gather(x, i, axis)) and np.array_equal(got, np.take(x, i, axis))
    with pytest.raises(Exception, match="-8"):
        ops.hannk_gather(dev(x), dev(np.array([8], np.int32)), 1)
    parts = [data((2, 3, n), np.int16, n) for n in (36, 5, 7)]
    got = ops.hannk_concatenation([dev(p) for p in parts], 2).cpu().numpy()
    assert np.array_equal(got, hl.hannk_concatenation(parts, 2)) and np.array_equal(got, np.concatenate(parts, 2))
    w, bias = data((3, 10), np.uint8, 33), np.array([100, -200, 300], np.int32)
    fc_in = data((4, 1, 5, 1), np.uint8, 34)       # bad_fully_connected's shapes: [4, 1, 5, 1] flattened to [2, 10]
    got = ops.hannk_fully_connected(dev(fc_in), dev(w), dev(bias), 3, 139, 1 << 30, 4, 132, 132, 255).cpu().numpy()
    assert got.shape == (2, 3) and np.array_equal(got, hl.hannk_fully_connected(fc_in, w, bias, 3, 139, 1 << 30, 4, 132, 132, 255))
    acc = (fc_in.reshape(2, 10).astype(np.int64) - 3) @ (w.astype(np.int64) - 139).T + bias
    assert np.array_equal(got, hl.debug_hannk_quantize("u8", acc.astype(np.int32), 1 << 30, 4, 132, 132, 255))
    for op, args in ((ops.hannk_transpose, (dev(x), [0, 2, 1, 3])), (ops.hannk_space_to_depth, (dev(x), 2)), (ops.hannk_depth_to_space, (s2d, 2)),
                     (ops.hannk_gather, (dev(x), dev(idx), 2)), (ops.hannk_concatenation, ([dev(p) for p in parts], 2)),
                     (ops.hannk_fully_connected, (dev(fc_in), dev(w), dev(bias), 3, 139, 1 << 30, 4, 132, 132, 255))):
        torch.library.opcheck(op, args, test_utils=("test_schema", "test_faketensor"))
