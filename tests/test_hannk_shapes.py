"""The shape rules of halide_amd/hannk.py: pure functions on tuples of ints that the numpy drivers, the torch ops with their register_fake
twins and hannk_model.py all read.  CPU only, nothing is built and no array leaves the host.

1. every .tflite fixture's declared output shapes are what the rule of its op kind gives for its input shapes and attributes;
2. the boxes of PadOp's walk tile the output, the copy last;  3. the rank-2 operand rule;  4. the rank-6 block views;
5. the torch ops' register_fake twins (run on meta tensors) return the rules' shapes."""
from __future__ import annotations

import glob
import math
import os

import numpy as np
import pytest

from halide_amd import tflite_reader as tfl

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hannk")


# ------------------------------------------------------------------------------------------------------------------ 1. the fixtures
def _elementwise(hl, ins, outs, a):
    return [tuple(np.broadcast_shapes(*ins))], outs


def _conv(hl, ins, outs, a):
    return [hl.hannk_conv_shape(ins[0], ins[1], a["stride"], a["dilation"], a["padding"])[2]], outs


def _depthwise(hl, ins, outs, a):
    x, f = ins[0], ins[1]      # the file's filter is (1, FH, FW, C * depth_multiplier); any multiplier but the broadcast one upsamples the input first
    if x[3] != 1:
        x = x[:3] + (x[3] * a["depth_multiplier"],)
    return [hl.hannk_conv_shape(x, f[1:], a["stride"], a["dilation"], a["padding"], depthwise=True)[2]], outs


def _pool(hl, ins, outs, a):
    return [hl.hannk_pool_shape(ins[0], a["filter"], a["stride"], a["padding"])], outs


def _fully_connected(hl, ins, outs, a):
    co, ci = ins[1]      # the conv op on a 1 x 1 image: (N, CO)
    n, _, _, c = hl.hannk_conv_shape((math.prod(ins[0]) // ci, 1, 1, ci), (co, 1, 1, ci), 1, 1, "valid")[2]
    return [(n, c)], outs


def _numpy_axis(a, rank):      # the reader keeps axes as Halide dimensions
    return rank - 1 - a["axis"]


def _concatenation(hl, ins, outs, a):
    return [hl.hannk_concat_shape(ins, _numpy_axis(a, len(ins[0])))[1]], outs


def _split(hl, ins, outs, a):
    x, axis = ins[0], _numpy_axis(a, len(ins[0]))
    sizes = hl.hannk_split_sizes(x[axis], a["size_splits"] if "size_splits" in a else len(outs))
    return [x[:axis] + (s,) + x[axis + 1:] for s in sizes], outs


def _transpose(hl, ins, outs, a):
    inverse = hl.hannk_inverse_perm(a["perm"], len(ins[0]))
    got = tuple(ins[0][p] for p in a["perm"])
    assert tuple(got[i] for i in inverse) == ins[0]
    return [got], outs


RULES = {
    "ADD": _elementwise, "SUB": _elementwise, "MUL": _elementwise, "LOGISTIC": _elementwise, "SOFTMAX": _elementwise, "L2_NORMALIZATION": _elementwise,
    "CONV_2D": _conv, "DEPTHWISE_CONV_2D": _depthwise, "AVERAGE_POOL_2D": _pool, "MAX_POOL_2D": _pool, "FULLY_CONNECTED": _fully_connected,
    "SPACE_TO_DEPTH": lambda hl, ins, outs, a: ([hl.hannk_block_shape(ins[0], a["block_size"], True)], outs),
    "CONCATENATION": _concatenation, "SPLIT": _split, "SPLIT_V": _split, "TRANSPOSE": _transpose,
    "RESHAPE": lambda hl, ins, outs, a: ([math.prod(ins[0])], [math.prod(outs[0])]),      # the element count
}


def test_every_fixture_declares_the_shape_its_rule_gives(hl):
    on_disk = sum(name.endswith(".tflite") for _, _, names in os.walk(GOLDEN) for name in names)
    checked = 0
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*", "*.tflite"))):
        g = tfl.read(path)
        for op in g.ops:
            assert op.kind in RULES, f"{path}: no shape rule in the table for {op.kind}"
            ins = [g.tensors[i].tfl_shape for i in op.inputs if i >= 0]
            outs = [g.tensors[i].tfl_shape for i in op.outputs]
            got, want = RULES[op.kind](hl, ins, outs, op.attrs)
            assert [tuple(s) if isinstance(s, tuple) else s for s in got] == want, (os.path.relpath(path, GOLDEN), op.kind, got, want)
        checked += 1
    assert checked == on_disk and checked >= 38


def test_out_extent_modes(hl):
    assert hl.hannk_out_extent(128, 3, 2, "same") == 64 and hl.hannk_out_extent(5, 3, 2, "same") == 3
    assert hl.hannk_out_extent(5, 3, 2, "valid") == 2 and hl.hannk_out_extent(7, (3 - 1) * 2 + 1, 1, "valid") == 3
    with pytest.raises(ValueError):
        hl.hannk_out_extent(5, 3, 2, "full")
    # explicit pixels: the positions whose window lies inside the padded input
    assert hl.hannk_conv_shape((2, 9, 11, 8), (24, 3, 5, 8), (2, 1), (1, 2), (2, 1)) == (False, hl.HANNK_VECTOR_REDUCTION, (2, 7, 6, 24))
    assert hl.hannk_conv_shape((1, 4, 5, 1), (3, 3, 17), 1, 1, 1, depthwise=True) == (True, 1, (1, 4, 5, 17))
    assert hl.hannk_conv_shape((1, 4, 5, 17), (3, 3, 17), 1, 1, 1, depthwise=True) == (False, hl.HANNK_DEPTHWISE_VECTOR, (1, 4, 5, 17))
    for depthwise, filt in ((False, (24, 3, 3, 16)), (True, (3, 3, 16))):
        with pytest.raises(ValueError, match="channels"):
            hl.hannk_conv_shape((1, 4, 5, 17), filt, 1, 1, 0, depthwise=depthwise)


# ------------------------------------------------------------------------------------------------------------------ 2. pad boxes
def test_pad_boxes_tile_the_output_and_the_copy_is_last(hl):
    shape, imin, boxes = hl.hannk_pad_boxes((1, 4, 5, 17), ((0, 0), (2, 1), (1, 2), (0, 0)))
    assert shape == (1, 7, 8, 17) and imin == (0, 1, 2, 0)      # Halide order: c, x, y, b
    count = np.zeros(shape, np.int32)
    for _, omin, omax in boxes:
        count[hl.hannk_box_slices(omin, omax)] += 1
    assert np.all(count == 1)
    assert [k for k, _, _ in boxes] == ["fill"] * (len(boxes) - 1) + ["copy"] and len(boxes) == 5
    inside = np.zeros(shape, bool)
    inside[hl.hannk_box_slices(*boxes[-1][1:])] = True
    want = np.zeros(shape, bool)
    want[:, 2:6, 1:6, :] = True
    assert np.array_equal(inside, want)      # the copy's box is the input translated by the padding in front

    # 3 channels to 4: the copy pads the channel itself
    shape, imin, boxes = hl.hannk_pad_boxes((1, 4, 5, 3), ((0, 0), (0, 0), (0, 0), (0, 1)))
    assert shape == (1, 4, 5, 4) and boxes == [("copy", (0, 0, 0, 0), (3, 4, 3, 0))]
    # any other channel padding is filled
    assert [k for k, _, _ in hl.hannk_pad_boxes((1, 4, 5, 3), ((0, 0), (0, 0), (0, 0), (0, 2)))[2]] == ["fill", "copy"]
    # nothing to pad
    shape, imin, boxes = hl.hannk_pad_boxes((1, 4, 5, 17), ((0, 0),) * 4)
    assert shape == (1, 4, 5, 17) and imin == (0, 0, 0, 0) and boxes == [("copy", (0, 0, 0, 0), (16, 4, 3, 0))]
    with pytest.raises(ValueError):
        hl.hannk_pad_boxes((1, 4, 5, 17), ((0, 0), (0, -1), (0, 0), (0, 0)))
    with pytest.raises(ValueError):
        hl.hannk_pad_boxes((4, 5, 17), ((0, 0),) * 3)


# ------------------------------------------------------------------------------------------------------------------ 3. rank-2 operands
def test_rank2_rule(hl):
    assert hl.hannk_rank2_rule((2, 3, 5), (2, 3, 5)) == (6, 5, 1, 5)            # the full shape: dense rows
    assert hl.hannk_rank2_rule((2, 1), (2, 2)) == (2, 2, 0, 1)                  # bad_broadcast_*.tflite: one element along the innermost axis
    assert hl.hannk_rank2_rule((1, 1, 5), (2, 3, 5)) == (6, 5, 1, 0)            # all outer extents 1: every row is the one row
    assert hl.hannk_rank2_rule((5,), (2, 3, 5)) == (6, 5, 1, 0)
    assert hl.hannk_rank2_rule((1,), (2, 3, 5)) == (6, 5, 0, 0) and hl.hannk_rank2_rule((), (2, 3, 5)) == (6, 5, 0, 0)
    assert hl.hannk_rank2_rule((1, 3, 5), (2, 3, 5)) is None                    # some but not all outer extents: to be materialised
    assert hl.hannk_rank2_rule((2, 1, 1), (2, 3, 5)) is None
    assert hl.hannk_rank2_rule((), ()) == (1, 1, 1, 1) and hl.hannk_rank2_rule((7,), (7,)) == (1, 7, 1, 7)
    with pytest.raises(ValueError):
        hl.hannk_rank2_rule((2, 3, 4), (2, 3, 5))
    # the strides describe the broadcast: a strided view of the dense operand is the broadcast operand
    r = np.random.RandomState(0)
    for shape, full in (((2, 3, 5), (2, 3, 5)), ((2, 3, 1), (2, 3, 5)), ((1, 1, 5), (2, 3, 5)), ((1,), (2, 3, 5))):
        a = r.randint(0, 256, shape).astype(np.uint8)
        rows, n, s0, s1 = hl.hannk_rank2_rule(shape, full)
        view = np.lib.stride_tricks.as_strided(a.reshape(-1), (rows, n), (s1, s0), writeable=False)
        assert np.array_equal(view, np.broadcast_to(a, full).reshape(rows, n)), (shape, full)


def test_the_model_reads_the_rank2_rule(hl):
    from halide_amd import hannk_model as hm
    m = hm.HannkModel.from_tflite(os.path.join(GOLDEN, "misc", "bad_broadcast_add.tflite"))
    a, b, out = (m.plan[0].args[i] for i in (0, 3, 9))
    shapes = [m.tensors[v.tensor].shape[::-1] for v in (a, b, out)]
    for v, shape in zip((a, b, out), shapes):
        rows, n, s0, s1 = hl.hannk_rank2_rule(shape, shapes[2])
        assert (v.extents, v.strides) == ((n, rows), (s0, s1))
    assert a.strides == (0, 1)


# ------------------------------------------------------------------------------------------------------------------ 4. block views
@pytest.mark.parametrize("k", [1, 2])
def test_block_views_are_the_numpy_restatement(hl, k):
    shape = (1, 4, 6, 5)
    b, h, w, c = shape
    x = np.arange(math.prod(shape)).reshape(shape)
    dshape = hl.hannk_block_shape(shape, k, True)
    assert dshape == (b, h // k, w // k, k * k * c)
    want = x.reshape(b, h // k, k, w // k, k, c).transpose(0, 1, 3, 2, 4, 5).reshape(dshape)
    space6, depth6, perm = hl.hannk_block_views(shape, k)
    assert perm == (0, 1, 3, 2, 4, 5)
    depth = np.full(dshape, -1)
    depth.reshape(depth6).transpose(perm)[...] = x.reshape(space6)      # space_to_depth: one copy between the two views
    assert np.array_equal(depth, want)
    # depth_to_space of the result gives the input back
    assert hl.hannk_block_shape(dshape, k, False) == shape and hl.hannk_block_views(hl.hannk_block_shape(dshape, k, False), k) == (space6, depth6, perm)
    space = np.full(shape, -1)
    space.reshape(space6)[...] = depth.reshape(depth6).transpose(perm)
    assert np.array_equal(space, x)


def test_block_refusals(hl):
    with pytest.raises(ValueError):
        hl.hannk_block_shape((1, 4, 6, 5), 4, True)      # 4 divides the height, not the width
    with pytest.raises(ValueError):
        hl.hannk_block_views((1, 4, 6, 5), 4)
    with pytest.raises(ValueError):
        hl.hannk_block_shape((1, 4, 6, 5), 2, False)     # 5 channels are no multiple of 4
    with pytest.raises(ValueError):
        hl.hannk_block_shape((1, 4, 6, 5), 0, True)
    with pytest.raises(ValueError):
        hl.hannk_block_shape((4, 6, 5), 2, True)


def test_model_block_views_are_the_rule(hl):
    """the plan's rank-6 views carry the strides of numpy views built from the same rule"""
    from halide_amd import hannk_model as hm
    m = hm.HannkModel.from_tflite(os.path.join(GOLDEN, "misc", "SPACE_TO_DEPTH.2.tflite"))
    s, d = m.plan[0].args
    shape = m.tensors[s.tensor].shape[::-1]
    space6, depth6, perm = hl.hannk_block_views(shape, 2)
    sv = np.empty(shape, np.uint8).reshape(space6)
    dv = np.empty(hl.hannk_block_shape(shape, 2, True), np.uint8).reshape(depth6).transpose(perm)
    assert (s.extents, s.strides) == (sv.shape[::-1], sv.strides[::-1]) and (d.extents, d.strides) == (dv.shape[::-1], dv.strides[::-1])


# ------------------------------------------------------------------------------------------------------------------ the small rules
def test_mean_gather_concat_split_transpose(hl):
    assert hl.hannk_mean_shapes((1, 4, 5, 17), [1, 2]) == ((1, 4, 5, 17), ([0] * 4, [1, 5, 4, 1]), (1, 1, 1, 17), (1, 1, 1, 17), (1, 17))
    assert hl.hannk_mean_shapes((4, 5, 17), [-1, 0, 2]) == ((1, 4, 5, 17), ([0] * 4, [17, 1, 4, 1]), (1, 1, 5, 1), (1, 5, 1), (5,))
    assert hl.hannk_mean_shapes((5,), 0)[1:] == (([0] * 4, [5, 1, 1, 1]), (1, 1, 1, 1), (1,), ())
    with pytest.raises(ValueError):
        hl.hannk_mean_shapes((1, 2, 3, 4, 5), [0])
    assert hl.hannk_gather_shape((1, 4, 5, 17), (2, 2), 2) == (2, (1, 4, 2, 2, 17)) and hl.hannk_gather_shape((4, 5), (), -1) == (1, (4,))
    for bad in (((), (2,), 0), ((4, 5), (1, 1, 1), 0), ((4, 5), (2,), 2), ((4, 5), (2,), -3)):
        with pytest.raises(ValueError):
            hl.hannk_gather_shape(*bad)
    assert hl.hannk_concat_shape([(2, 3, 5), (2, 3, 7)], -1) == (2, (2, 3, 12)) and hl.hannk_concat_shape([(2, 3, 5)], 0) == (0, (2, 3, 5))
    for bad in (([], 0), ([(2, 3, 5), (2, 4, 7)], 2), ([(2, 3, 5), (3, 5)], 2), ([(2, 3)], 2)):
        with pytest.raises(ValueError):
            hl.hannk_concat_shape(*bad)
    assert hl.hannk_split_sizes(48, 3) == [16, 16, 16] and hl.hannk_split_sizes(48, [36, 5, 7]) == [36, 5, 7] and hl.hannk_split_sizes(4, [4, 0]) == [4, 0]
    for bad in ((48, 5), (48, 0), (48, [36, 5]), (4, [5, -1])):
        with pytest.raises(ValueError):
            hl.hannk_split_sizes(*bad)
    assert hl.hannk_inverse_perm((2, 0, 1), 3) == (1, 2, 0) and hl.hannk_inverse_perm([], 0) == ()
    for bad in (((0, 0, 1), 3), ((0, 1), 3), ((0, 1, 3), 3)):
        with pytest.raises(ValueError):
            hl.hannk_inverse_perm(*bad)


# ------------------------------------------------------------------------------------------------------------------ 5. the torch twins
def test_register_fake_twins_return_the_rules_shapes(hl):
    """each torch op on meta tensors (its register_fake, no device) at 17 channels and width 5 against the rule the numpy driver reads"""
    import torch
    from halide_amd import torch_ops  # noqa: F401  (registers torch.ops.hlmi)
    ops = torch.ops.hlmi

    def meta(shape, dtype=torch.uint8):
        return torch.empty(shape, dtype=dtype, device="meta")

    x = (1, 4, 5, 17)
    for padding in ("same", "valid"):
        for kind in ("average", "max"):
            got = ops.hannk_pool2d(meta(x), kind, [3, 2], [2, 1], padding, 0, 255)
            assert tuple(got.shape) == hl.hannk_pool_shape(x, (3, 2), (2, 1), padding) == {"same": (1, 4, 3, 17), "valid": (1, 3, 2, 17)}[padding]
    assert tuple(ops.hannk_mean(meta(x), [1, 2]).shape) == hl.hannk_mean_shapes(x, [1, 2])[3] == (1, 1, 1, 17)
    pads = ((0, 0), (2, 1), (1, 2), (0, 0))
    assert tuple(ops.hannk_pad(meta(x), [v for p in pads for v in p], 128).shape) == hl.hannk_pad_boxes(x, pads)[0] == (1, 7, 8, 17)
    space, depth = (1, 6, 10, 17), (1, 3, 5, 68)
    assert tuple(ops.hannk_space_to_depth(meta(space), 2).shape) == hl.hannk_block_shape(space, 2, True) == depth
    assert tuple(ops.hannk_depth_to_space(meta(depth), 2).shape) == hl.hannk_block_shape(depth, 2, False) == space
    assert tuple(ops.hannk_gather(meta(x), meta((2, 2), torch.int32), 2).shape) == hl.hannk_gather_shape(x, (2, 2), 2)[1] == (1, 4, 2, 2, 17)
    y = (1, 4, 5, 3)
    assert tuple(ops.hannk_concatenation([meta(x), meta(y)], -1).shape) == hl.hannk_concat_shape([x, y], -1)[1] == (1, 4, 5, 20)
    perm = [0, 3, 1, 2]
    assert tuple(ops.hannk_transpose(meta(x), perm).shape) == tuple(x[p] for p in perm) and hl.hannk_inverse_perm(perm, 4) == (0, 2, 3, 1)
    conv = ops.hannk_conv2d(meta(x), meta((24, 3, 3, 17)), meta((24,), torch.int32), 3, 5, [2, 1], [1, 2], [1, 2], 1 << 30, 8, 0, 0, 255, False)
    assert tuple(conv.shape) == hl.hannk_conv_shape(x, (24, 3, 3, 17), (2, 1), (1, 2), (1, 2))[2] == (1, 4, 3, 24) and conv.dtype == torch.uint8
    dw = ops.hannk_depthwise_conv2d(meta(x), meta((3, 3, 17)), meta((17,), torch.int32), 3, 5, [2, 1], [1, 2], [1, 2], 1 << 30, 8, 0, 0, 255)
    assert tuple(dw.shape) == hl.hannk_conv_shape(x, (3, 3, 17), (2, 1), (1, 2), (1, 2), depthwise=True)[2] == (1, 4, 3, 17)
    # a rule's refusal reaches the caller as the RuntimeError torch ops raise, with the op's name in front
    with pytest.raises(RuntimeError, match="hannk_space_to_depth"):
        ops.hannk_space_to_depth(meta(x), 2)
    with pytest.raises(RuntimeError, match="hannk_conv2d"):
        ops.hannk_conv2d(meta(x), meta((24, 3, 3, 16)), meta((24,), torch.int32), 3, 5, [2, 1], [1, 2], [1, 2], 1 << 30, 8, 0, 0, 255, False)
