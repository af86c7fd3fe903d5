"""apps/hannk's op library from Python: the raw entry-point calls, the interpreter's parameter derivations, every op's
shape rule, the elementwise assembler with its programs, the numpy drivers `hannk_*` and the debug hooks.  `halide_amd` re-exports the
names of `__all__`; `torch_ops.py` and `hannk_model.py` take their shapes and parameters from here.  Arrays are the Halide dimensions
reversed: an activation [c, x, y, b] is an array of shape (B, H, W, C) — NHWC —, the tiled filter [4, 16, ci / 4, co / 16, fx, fy] one of
shape (FH, FW, CO16, CQ, 16, 4), a depthwise filter [c, fx, fy] one of shape (FH, FW, C)."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _BP, _HANNK_ALL_PARAMS, _SCALAR_CTYPES, _TYPE_OF, Buffer, HalideError, _as_ptr, _check, _fn, aligned_array, lib, metadata

HANNK_VECTOR_REDUCTION, HANNK_ACCUM_VECTOR_SIZE, HANNK_DEPTHWISE_VECTOR = 4, 16, 16
HANNK_MOVE_KERNELS = ("none", "rows", "transposing", "general")


# raw entry-point calls, arguments as in the C signature (include/aot/halide/<name>.h); stride, dilation and filter are (x, y) pairs
def tile_conv_filter_uint8(input, input_zero, output_zero, output) -> int:
    """u8 [ci, x, y, co] -> the u8 [4, 16, ci / 4, co / 16, x, y] filter conv_u8_u8_* reads; entries outside the input are output_zero."""
    return _check(_fn["tile_conv_filter_uint8"](_as_ptr(input), int(input_zero), int(output_zero), _as_ptr(output)))


def _hannk_conv_args(input, input_zero, filter, filter_zero, bias, stride, dilation, extra, multiplier, shift, output_zero, output_min, output_max,
                     output):
    return ([_as_ptr(input), int(input_zero), _as_ptr(filter), int(filter_zero), _as_ptr(bias), int(stride[0]), int(stride[1]), int(dilation[0]),
             int(dilation[1])] + extra + [int(multiplier), int(shift), int(output_zero), int(output_min), int(output_max), _as_ptr(output)])


def conv_u8_u8_u8(input, input_zero, filter, filter_zero, bias, stride, dilation, multiplier, shift, output_zero, output_min, output_max, output) -> int:
    """input u8 [c, x, y, b], tiled filter, bias i32 [c] -> u8 [c, x, y, b]; stride and dilation are (x, y) pairs."""
    return _check(_fn["conv_u8_u8_u8"](*_hannk_conv_args(input, input_zero, filter, filter_zero, bias, stride, dilation, [], multiplier, shift,
                                                         output_zero, output_min, output_max, output)))


def conv_u8_u8_i16(input, input_zero, filter, filter_zero, bias, stride, dilation, multiplier, shift, output_zero, output_min, output_max, output) -> int:
    """conv_u8_u8_u8 with an int16 output: quantize_i16 only, output_zero / min / max are not read."""
    return _check(_fn["conv_u8_u8_i16"](*_hannk_conv_args(input, input_zero, filter, filter_zero, bias, stride, dilation, [], multiplier, shift,
                                                          output_zero, output_min, output_max, output)))


def depthwise_conv_uint8(input, input_zero, filter, filter_zero, bias, stride, dilation, multiplier, shift, output_zero, output_min, output_max, output,
                         input_stride_x=0) -> int:
    """input u8 [c, x, y, b] (channels padded to a multiple of 16), filter u8 [c, fx, fy], bias i32 [c] -> u8 [c, x, y, b]."""
    return _check(_fn["depthwise_conv_uint8"](*_hannk_conv_args(input, input_zero, filter, filter_zero, bias, stride, dilation, [int(input_stride_x)],
                                                                multiplier, shift, output_zero, output_min, output_max, output)))


def depthwise_conv_broadcast_uint8(input, input_zero, filter, filter_zero, bias, stride, dilation, multiplier, shift, output_zero, output_min,
                                   output_max, output, input_stride_x=0) -> int:
    """depthwise_conv_uint8 with the input's one channel feeding every output channel."""
    return _check(_fn["depthwise_conv_broadcast_uint8"](*_hannk_conv_args(input, input_zero, filter, filter_zero, bias, stride, dilation,
                                                                          [int(input_stride_x)], multiplier, shift, output_zero, output_min, output_max,
                                                                          output)))


def depthwise_conv_shallow_uint8(input, input_zero, filter, filter_zero, bias, stride, dilation, input_stride_x, multiplier, shift, output_zero,
                                 output_min, output_max, output) -> int:
    """depthwise_conv_uint8 with c and x fused into dimension 0: input u8 [c, 1, y, b], filter u8 [D, fx, fy], bias i32 [D] -> u8 [c, 1, y, b];
    the tap rx reads the input at c + rx * dilation_x * input_stride_x; filter and bias are read at (c % 16) % D."""
    return _check(_fn["depthwise_conv_shallow_uint8"](*_hannk_conv_args(input, input_zero, filter, filter_zero, bias, stride, dilation,
                                                                        [int(input_stride_x)], multiplier, shift, output_zero, output_min, output_max,
                                                                        output)))


def average_pool_uint8(input, stride, filter, output_min, output_max, output) -> int:
    """u8 [c, x, y, b] -> u8 [c, x, y, b]; stride and filter are (x, y) pairs; taps outside the input do not count."""
    return _check(_fn["average_pool_uint8"](_as_ptr(input), int(stride[0]), int(stride[1]), int(filter[0]), int(filter[1]), int(output_min),
                                            int(output_max), _as_ptr(output)))


def max_pool_uint8(input, stride, filter, output_min, output_max, output) -> int:
    return _check(_fn["max_pool_uint8"](_as_ptr(input), int(stride[0]), int(stride[1]), int(filter[0]), int(filter[1]), int(output_min),
                                        int(output_max), _as_ptr(output)))


def mean_uint8(input, mins, extents, output) -> int:
    """u8 [c, x, y, b] -> u8 [c, x, y, b]: output(p) = the rounded mean of input over p + [mins, mins + extents), Halide order (c first)."""
    a = [int(v) for pair in zip(mins, extents) for v in pair]
    return _check(_fn["mean_uint8"](_as_ptr(input), *a, _as_ptr(output)))


def add_uint8_uint8(input1, input1_zero, input1_multiplier, input2, input2_zero, input2_multiplier, output_zero, output_min, output_max, output) -> int:
    return _check(_fn["add_uint8_uint8"](_as_ptr(input1), int(input1_zero), int(input1_multiplier), _as_ptr(input2), int(input2_zero),
                                         int(input2_multiplier), int(output_zero), int(output_min), int(output_max), _as_ptr(output)))


def mul_uint8_uint8_uint8(input1, input1_zero, input2, input2_zero, output_zero, output_multiplier, output_shift, output_min, output_max, output) -> int:
    return _check(_fn["mul_uint8_uint8_uint8"](_as_ptr(input1), int(input1_zero), _as_ptr(input2), int(input2_zero), int(output_zero),
                                               int(output_multiplier), int(output_shift), int(output_min), int(output_max), _as_ptr(output)))


def softmax_uint8(input, beta_multiplier, beta_shift, output_zero, output_multiplier, output_shift, output) -> int:
    return _check(_fn["softmax_uint8"](_as_ptr(input), int(beta_multiplier), int(beta_shift), int(output_zero), int(output_multiplier),
                                       int(output_shift), _as_ptr(output)))


def l2_normalization_uint8(input, input_zero, output) -> int:
    return _check(_fn["l2_normalization_uint8"](_as_ptr(input), int(input_zero), _as_ptr(output)))


def elementwise_5xuint8_1xuint8(inputs_0, inputs_1, inputs_2, inputs_3, inputs_4, program, output) -> int:
    """five u8 [x, y] inputs (dimension 0 stride 1 or 0), program i16 [5, n], n <= 20 -> u8 [x, y]: u8_sat of the last slot"""
    return _check(_fn["elementwise_5xuint8_1xuint8"](_as_ptr(inputs_0), _as_ptr(inputs_1), _as_ptr(inputs_2), _as_ptr(inputs_3), _as_ptr(inputs_4),
                                                     _as_ptr(program), _as_ptr(output)))


def elementwise_5xint16_1xuint8int16(inputs_0, inputs_1, inputs_2, inputs_3, inputs_4, program, output_0, output_1) -> int:
    """five i16 [x, y] inputs -> output_0 u8 = u8_sat(the last slot but one), output_1 i16 = the last slot"""
    return _check(_fn["elementwise_5xint16_1xuint8int16"](_as_ptr(inputs_0), _as_ptr(inputs_1), _as_ptr(inputs_2), _as_ptr(inputs_3), _as_ptr(inputs_4),
                                                          _as_ptr(program), _as_ptr(output_0), _as_ptr(output_1)))


def copy_uint8_uint8(input, pad_value, output) -> int:
    """u8 [c, x, y, b] -> u8 [c, x, y, b]; channels outside the input's dimension 0 are uint8(pad_value)"""
    return _check(_fn["copy_uint8_uint8"](_as_ptr(input), int(pad_value), _as_ptr(output)))


def fill_uint8(value, output) -> int:
    return _check(_fn["fill_uint8"](int(value), _as_ptr(output)))


def upsample_channels_uint8(input, factor, output) -> int:
    """output(c, x, y, b) = input(c / factor, x, y, b), Halide's division (c / 0 == 0)"""
    return _check(_fn["upsample_channels_uint8"](_as_ptr(input), int(factor), _as_ptr(output)))


def _hannk_general(name, argv) -> int:
    """hlmi_hannk_general(name, argv): the entry point `name` with one thread per output running the contract's loops as written"""
    fn = lib.hlmi_hannk_general
    fn.restype, fn.argtypes = C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]
    return _check(fn(name.encode(), argv))


# the data movers: Buffer::copy_from on re-viewed buffers, and GatherOp; library extensions without metadata
def hannk_copy_from(src, dst, general=False) -> int:
    """Halide::Runtime::Buffer::copy_from: dst's elements inside src's box take src's values.  Two Buffers of the same rank (<= 8) and element
    size (1, 2, 4, 8 bytes), any strides; `general` forces the one-thread-per-element kernel (hlmi_hannk_general)."""
    if general:
        return _hannk_general("hannk_copy_from", (C.c_void_p * 2)(C.cast(_as_ptr(src), C.c_void_p), C.cast(_as_ptr(dst), C.c_void_p)))
    fn = lib.hlmi_hannk_copy_from
    fn.restype, fn.argtypes = C.c_int, [_BP, _BP]
    return _check(fn(_as_ptr(src), _as_ptr(dst)))


def hannk_gather_buffers(src, indices, axis, dst) -> int:
    """GatherOp::execute with batch_dims == 0 on Buffers: `axis` is a Halide dimension of src, indices int32 of rank 0 .. 2, dst of rank
    src.rank + indices.rank - 1.  An index outside src's dimension leaves its slice of dst unwritten and raises HalideError -8."""
    fn = lib.hlmi_hannk_gather
    fn.restype, fn.argtypes = C.c_int, [_BP, _BP, C.c_int, _BP]
    return _check(fn(_as_ptr(src), _as_ptr(indices), int(axis), _as_ptr(dst)))


# parameter derivations: what the interpreter's ops.cpp computes from float scales before it calls an op
def hannk_int_float(x, bits):
    """ops.cpp's IntFloat<intN_t>(x): x = mantissa * 2^exponent / 2^(bits - 1) -> (mantissa(), exponent()) as its accessors return them."""
    log2_one = bits - 1
    m, e = math.frexp(float(np.float32(x)))
    ml = int(math.floor(abs(m) * (1 << log2_one) + 0.5)) * (1 if m >= 0 else -1)   # std::round
    if ml == 1 << log2_one:
        ml, e = ml >> 1, e + 1
    return ml, e


def _int_float_scaled(x, bits, power):
    log2_one = bits - 1
    m, e = hannk_int_float(x, bits)
    e += power
    return (0 if e < -log2_one else m), max(-log2_one, min(log2_one, e))


def hannk_output_range(activation, zero, scale):
    """ops.cpp's get_quantized_min_max: activation None / "relu" / "relu6" / "relu_n1_to_1" -> (min, max)"""
    lo, hi = 0, 255
    rnd = lambda v: int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)
    if activation in (None, "none"):
        pass
    elif activation == "relu":
        lo = int(zero)
    elif activation == "relu6":
        lo, hi = int(zero), int(zero) + rnd(6.0 / scale)
    elif activation == "relu_n1_to_1":
        lo, hi = int(zero) + rnd(-1.0 / scale), int(zero) + rnd(1.0 / scale)
    else:
        raise ValueError(f"unsupported activation {activation}")
    return max(lo, 0), min(hi, 255)


def hannk_compute_padding(stride, in_size, filter_size, out_size) -> int:
    return max(0, (out_size - 1) * stride + filter_size - in_size) // 2


def hannk_add_multipliers(scale1, scale2, out_scale, sign2=1):
    """add_uint8's (input1_multiplier, input2_multiplier): lround(scale * 2^16 / (out_scale * 2^6)), the second times sign2"""
    f32 = np.float32
    lround = lambda v: int(math.floor(abs(float(v)) + 0.5)) * (1 if v >= 0 else -1)
    so = f32(out_scale) * f32(1 << 6)
    return lround(f32(scale1) * f32(1 << 16) / so), lround(f32(scale2) * f32(1 << 16) / so) * int(sign2)


def hannk_mul_params(scale1, scale2, out_scale):
    """mul_uint8's (output_multiplier, output_shift): IntFloat<int32_t>(scale1 * scale2 / out_scale) * 2^-12"""
    f32 = np.float32
    m, e = _int_float_scaled(f32(scale1) * f32(scale2) / f32(out_scale), 32, -12)
    return m, -e


def hannk_softmax_params(in_scale, beta, out_scale):
    """SoftmaxOp::execute: (beta_multiplier, beta_shift, output_multiplier, output_shift), the extra factor of two on the output included"""
    f32 = np.float32
    beta2 = f32(beta) * f32(np.log2(np.exp(f32(1.0))))
    bm, be = _int_float_scaled(beta2 * f32(in_scale), 16, -6)
    om, oe = _int_float_scaled(f32(out_scale), 16, 1)
    return bm, -be, om, -oe


def hannk_can_be_shallow(channels, width, stride_x=1) -> bool:
    """ops.cpp:931-939, :1012: the channel vector is a multiple of the channel count, the fused row is at least one vector wide, stride_x is 1"""
    return int(stride_x) == 1 and channels > 0 and HANNK_DEPTHWISE_VECTOR % channels == 0 and channels * width >= HANNK_DEPTHWISE_VECTOR


# shape rules: each op's shape arithmetic, once.  Pure functions on tuples of ints in numpy (NHWC) order, no arrays and no library calls;
# a shape that the op refuses raises ValueError.  The numpy drivers below, the torch ops with their register_fake twins and hannk_model.py
# all read their shapes here.
def _pair(v):
    return (int(v[0]), int(v[1])) if hasattr(v, "__len__") else (int(v), int(v))


def hannk_conv_out_extent(size, filt, stride, dilation, padding) -> int:
    """outputs along one axis: the positions x with x * stride + (filt - 1) * dilation inside the padded input"""
    return (int(size) + 2 * int(padding) - (int(filt) - 1) * int(dilation) - 1) // int(stride) + 1


def hannk_out_extent(size, effective_filter, stride, padding) -> int:
    """outputs along one axis under the interpreter's padding modes: "same" ceil(size / stride), "valid" the windows inside the input"""
    if padding == "same":
        return -(-size // stride)
    if padding == "valid":
        return (size - effective_filter) // stride + 1
    raise ValueError("padding is 'same' or 'valid'")


def hannk_conv_shape(input_shape, filter_shape, stride, dilation, padding, depthwise=False):
    """conv (filter (CO, FH, FW, CI)) or depthwise conv (filter (FH, FW, C)) of a (B, H, W, C) input; stride and dilation are (x, y) pairs,
    padding (x, y) pixels on every side or "same" / "valid" -> (broadcast, channel multiple, output shape): one input channel under a
    depthwise filter of several is broadcast; the interpreter pads the input's channels to the channel multiple."""
    b, h, w, c = input_shape
    co, fh, fw, ci = (*filter_shape[2:], *filter_shape) if depthwise else filter_shape      # depthwise: C outputs of one input channel each
    broadcast = bool(depthwise) and c == 1 and co > 1
    if not broadcast and c != ci:
        raise ValueError(f"the input has {c} channels, the filter {ci}")
    (sx, sy), (dx, dy) = _pair(stride), _pair(dilation)
    if isinstance(padding, str):
        oh, ow = hannk_out_extent(h, (fh - 1) * dy + 1, sy, padding), hannk_out_extent(w, (fw - 1) * dx + 1, sx, padding)
    else:
        px, py = _pair(padding)
        oh, ow = hannk_conv_out_extent(h, fh, sy, dy, py), hannk_conv_out_extent(w, fw, sx, dx, px)
    return broadcast, 1 if broadcast else HANNK_DEPTHWISE_VECTOR if depthwise else HANNK_VECTOR_REDUCTION, (b, oh, ow, co)


def hannk_pool_shape(input_shape, filter, stride, padding):
    """Pool2DOp: (B, H, W, C), filter and stride (x, y) pairs, padding "same" or "valid" -> (B, OH, OW, C)"""
    b, h, w, c = input_shape
    (fw, fh), (sx, sy) = _pair(filter), _pair(stride)
    return (b, hannk_out_extent(h, fh, sy, padding), hannk_out_extent(w, fw, sx, padding), c)


def hannk_mean_shapes(shape, axes):
    """ReductionOp (Mean) over the numpy `axes` of a shape of rank <= 4 -> (the shape padded to rank 4 in front, mean_uint8's (mins, extents)
    in Halide order, the rank-4 output shape, the output shape with the reduced axes kept as 1, the one without them)"""
    nd = len(shape)
    if nd > 4:
        raise ValueError("mean takes a rank of 4 at the most")
    axes = sorted({int(a) % nd for a in (axes if hasattr(axes, "__iter__") else (axes,))})
    in4 = (1,) * (4 - nd) + tuple(shape)
    red4 = [a + 4 - nd for a in axes]
    extents = [in4[3 - d] if 3 - d in red4 else 1 for d in range(4)]
    out4 = tuple(1 if a in red4 else in4[a] for a in range(4))
    return in4, ([0] * 4, extents), out4, out4[4 - nd:], tuple(shape[a] for a in range(nd) if a not in axes)


def hannk_pad_boxes(shape, pads):
    """PadOp::execute's walk over a rank-4 shape with one (before, after) pair per axis -> (output shape, the input's mins, the boxes): a box is
    ("fill" | "copy", omin, omax), inclusive corners of a crop of the output; mins and corners are in Halide order.  The borders are filled
    dimension by dimension, outermost first; the last box is the copy, which pads the channel itself where 3 become 4 (ops.cpp:1266-1271)."""
    if len(shape) != 4 or len(pads) != 4:
        raise ValueError("a rank-4 shape and four (before, after) pairs")
    pads = [(int(b), int(a)) for b, a in pads]
    if any(b < 0 or a < 0 for b, a in pads):
        raise ValueError("paddings are not negative")
    out = tuple(s + b + a for s, (b, a) in zip(shape, pads))
    # Halide dimension d is numpy axis 3 - d; the input is translated by the padding in front of it
    imin = [pads[3 - d][0] for d in range(4)]
    imax = [imin[d] + shape[3 - d] - 1 for d in range(4)]
    omin, omax = [0] * 4, [out[3 - d] - 1 for d in range(4)]
    boxes = []
    fill_min_dim = 1 if shape[3] == 3 and out[3] == 4 else 0
    for d in range(3, fill_min_dim - 1, -1):
        lo, hi = omin[d], omax[d]
        if lo < imin[d]:
            omin[d], omax[d] = lo, imin[d] - 1
            boxes.append(("fill", tuple(omin), tuple(omax)))
        if hi > imax[d]:
            omin[d], omax[d] = imax[d] + 1, hi
            boxes.append(("fill", tuple(omin), tuple(omax)))
        omin[d], omax[d] = max(lo, imin[d]), min(hi, imax[d])
    boxes.append(("copy", tuple(omin), tuple(omax)))
    return out, tuple(imin), boxes


def hannk_box_slices(omin, omax):
    """the numpy (or torch) index of a box of hannk_pad_boxes"""
    return tuple(slice(lo, hi + 1) for lo, hi in zip(reversed(omin), reversed(omax)))


def hannk_block_shape(shape, block, to_depth):
    """space_to_depth: (B, H, W, C) -> (B, H / block, W / block, block^2 * C); depth_to_space: the other way"""
    if len(shape) != 4 or block < 1:
        raise ValueError("a (B, H, W, C) shape and a block size >= 1")
    b, h, w, c = shape
    if to_depth:
        if h % block or w % block:
            raise ValueError(f"the block size {block} does not divide both {h} and {w}")
        return (b, h // block, w // block, c * block * block)
    if c % (block * block):
        raise ValueError(f"{block}^2 does not divide {c} channels")
    return (b, h * block, w * block, c // (block * block))


def hannk_block_views(space_shape, block):
    """(space6, depth6, perm): the space tensor reshaped to space6 and the depth tensor reshaped to depth6 with its axes permuted by perm are
    two rank-6 views of one shape (ops.cpp:1607-1625); one copy between them is either op"""
    b, hb, wb, _ = hannk_block_shape(space_shape, block, True)
    c = space_shape[3]
    return (b, hb, block, wb, block, c), (b, hb, wb, block, block, c), (0, 1, 3, 2, 4, 5)


def hannk_gather_shape(shape, index_shape, axis):
    """GatherOp with batch_dims == 0 -> (the axis from the front, the result's shape)"""
    nd = len(shape)
    if nd < 1 or len(index_shape) > 2 or not -nd <= axis < nd:
        raise ValueError("indices of rank 0 .. 2 and an axis of the input")
    axis %= nd
    return axis, tuple(shape[:axis]) + tuple(index_shape) + tuple(shape[axis + 1:])


def hannk_concat_shape(shapes, axis):
    """ConcatenationOp -> (the axis from the front, the result's shape)"""
    if not shapes or not -len(shapes[0]) <= axis < len(shapes[0]):
        raise ValueError("at least one input and an axis of it")
    first, nd = shapes[0], len(shapes[0])
    axis %= nd
    if any(len(s) != nd or any(s[d] != first[d] for d in range(nd) if d != axis) for s in shapes):
        raise ValueError("the inputs share rank and every extent but the axis'")
    return axis, tuple(sum(s[axis] for s in shapes) if d == axis else first[d] for d in range(nd))


def hannk_split_sizes(n, sizes):
    """SplitOp: the pieces' extents along an axis of `n` elements, `sizes` an int (that many equal pieces) or the extents themselves"""
    if not hasattr(sizes, "__len__"):
        if int(sizes) < 1 or n % int(sizes):
            raise ValueError(f"{n} elements do not split into {sizes} equal pieces")
        return [n // int(sizes)] * int(sizes)
    sizes = [int(v) for v in sizes]
    if sum(sizes) != n or any(v < 0 for v in sizes):
        raise ValueError(f"pieces of {sizes} do not add up to {n}")
    return sizes


def hannk_inverse_perm(perm, rank):
    """TransposeOp: the inverse of `perm`, which the output viewed in the input's order is transposed by"""
    perm = [int(p) for p in perm]
    if sorted(perm) != list(range(rank)):
        raise ValueError(f"{perm} is no permutation of {rank} axes")
    return tuple(perm.index(a) for a in range(rank))


def hannk_rank2_rule(shape, full):
    """An operand of `shape` broadcast against `full` as the [x, y] buffer of the elementwise ops (dimension 0 the innermost axis, dimension 1
    everything outside it) -> (rows, n, stride0, stride1) in elements of the dense operand: stride0 is 0 where it has one element along the
    innermost axis, stride1 is 0 where all its outer extents are 1; None where it has some but not all of them: to be materialised."""
    full = tuple(full)
    a = (1,) * (len(full) - len(shape)) + tuple(shape)
    n = full[-1] if full else 1
    inner = a[-1] if a else 1
    if len(a) != len(full) or inner not in (1, n):
        raise ValueError(f"an operand of shape {tuple(shape)} does not broadcast to {full}")
    stride0 = 1 if inner == n else 0
    if a[:-1] == full[:-1]:
        stride1 = inner
    elif all(e == 1 for e in a[:-1]):
        stride1 = 0
    else:
        return None
    return math.prod(full[:-1]), n, stride0, stride1


# the elementwise assembler and the programs the interpreter builds with it
class ElementwiseAssembler:
    """interpreter/elementwise_program.{h,cpp}: builds the [n, 5] int16 program (rows of op, arg1, arg2, arg3, arg4) the elementwise entry
    points run.  Methods return Slot objects; an int where the reference has an int16_t overload is an immediate."""
    Noop, Add, Sub, MulAdd, MulShift, Shift, Min, Max, Clamp, Logistic, Tanh = range(11)
    InstructionSize = 5

    class Slot:
        def __init__(self, index):
            self.index = int(index)

    def __init__(self, capacity=None):
        self.rows = []
        self.capacity = capacity

    def _instruction(self, op, a, b, arg3=0, arg4=0):
        if self.capacity is not None and len(self.rows) >= self.capacity:
            raise ValueError("the program buffer is full")
        for v in (arg3, arg4):
            if not -32768 <= int(v) <= 32767:
                raise ValueError(f"immediate {v} is no int16")
        self.rows.append((op, a.index, b.index, int(arg3), int(arg4)))
        return self.Slot(len(self.rows))

    def _binary(self, op, a, b, imm=0, arg4=0):      # the second operand: a slot (with an immediate beside it) or an immediate alone
        if isinstance(b, self.Slot):
            return self._instruction(op, a, b, imm, arg4)
        return self._instruction(op, a, self.constant(0), b, arg4)

    def constant(self, value):
        return self.Slot(0) if value == 0 else self._instruction(self.Add, self.Slot(0), self.Slot(0), value)

    def input(self, index):
        return self.Slot(-index - 1)

    def add(self, a, b, add_b=0):
        return self._binary(self.Add, a, b, add_b)

    def sub(self, a, b, add_b=0):
        return self._binary(self.Sub, a, b, add_b)

    def mul(self, a, b, add_b=0):
        return self._binary(self.MulAdd, a, b, add_b)

    def mul_add(self, a, b, add):
        return self._binary(self.MulAdd, a, b, 0, add)

    def mul_shift(self, a, b, shift):
        return self._binary(self.MulShift, a, b, 0, shift)

    def shift(self, a, b, extra_shift=0):
        return self._binary(self.Shift, a, b, extra_shift)

    def min(self, a, b, add_b=0):
        return self._binary(self.Min, a, b, add_b)

    def max(self, a, b, add_b=0):
        return self._binary(self.Max, a, b, add_b)

    def clamp(self, x, lo, hi):
        return self._instruction(self.Clamp, x, x, lo, hi)   # op2 is unused: x again, as the reference does

    def logistic(self, q, a, q_a):
        return self._binary(self.Logistic, a, q_a, 0, q)

    def tanh(self, q, a, q_a):
        return self._binary(self.Tanh, a, q_a, 0, q)

    def assemble(self, outputs) -> np.ndarray:
        """The program whose last len(outputs) slots are `outputs`: where they are not there already, each is reloaded by adding 0."""
        needed = len(self.rows) - len(outputs) + 1
        if [o.index for o in outputs] != list(range(needed, needed + len(outputs))):
            for o in outputs:
                self.add(o, 0)
        return np.array(self.rows, np.int16).reshape(-1, 5)


def hannk_logistic_program(in_scale, in_zero) -> np.ndarray:
    """UnaryOp::execute, Logistic (ops.cpp:1797-1813): the output has scale 1 / 256 and zero point 0"""
    m, e = _int_float_scaled(np.float32(in_scale), 16, -6)
    if e > 0:
        raise ValueError("the input scale is too large for the logistic program")
    p = ElementwiseAssembler(64 // 5)
    scaled = p.mul_shift(p.sub(p.input(0), int(in_zero)), m, 15 - 6)
    return p.assemble([p.logistic(8, scaled, -e)])


def hannk_tanh_program(in_scale, in_zero) -> np.ndarray:
    """UnaryOp::execute, Tanh (ops.cpp:1820-1833): the output has scale 1 / 128 and zero point 128"""
    m, e = _int_float_scaled(np.float32(in_scale), 16, -6)
    if e > 0:
        raise ValueError("the input scale is too large for the tanh program")
    p = ElementwiseAssembler(64 // 5)
    scaled = p.mul_shift(p.sub(p.input(0), int(in_zero)), m, 15 - 6)
    return p.assemble([p.add(p.tanh(7, scaled, -e), 128)])


def hannk_lstm_program() -> np.ndarray:
    """The elementwise part of the LSTM cell (lower.cpp:44-69) on inputs (input gate, input modulation gate, forget gate, output gate,
    previous state), all int16 -> the outputs (activation u8, state i16)"""
    p = ElementwiseAssembler(256 // 5)
    q = 15
    input_gate = p.logistic(q, p.input(0), q - 3)
    input_modulation_gate = p.tanh(q, p.input(1), q - 3)
    forget_gate = p.logistic(q, p.input(2), q - 3)
    output_gate = p.logistic(q, p.input(3), q - 3)
    input_times_input_modulation = p.mul_shift(input_gate, input_modulation_gate, q + 4)
    prev_state_times_forget_state = p.mul(forget_gate, p.input(4))
    state = p.add(input_times_input_modulation, prev_state_times_forget_state)
    activation = p.mul_add(output_gate, p.tanh(7, state, q - 4), 128)
    state = p.add(state, 0)
    return p.assemble([activation, state])


# numpy drivers: what the interpreter's ops.cpp / lower.cpp do around each op, on host arrays.  Shapes come from the rules above; what is
# left here is array handling.
def hannk_pad_input(input, input_zero, channel_multiple, padding) -> np.ndarray:
    """What the interpreter does to an activation before a conv op: (B, H, W, C) u8 -> a 64-byte aligned array with the channel axis
    padded to `channel_multiple` and `padding` = (x, y) pixels on each side of W and H, every new element input_zero."""
    input = np.asarray(input)
    b, h, w, c = input.shape
    px, py = _pair(padding)
    cp = -(-c // channel_multiple) * channel_multiple
    out = aligned_array((b, h + 2 * py, w + 2 * px, cp), np.uint8, 64, 1)
    out[...] = np.uint8(input_zero)
    out[:, py:py + h, px:px + w, :c] = input
    return out


def hannk_tile_filter(filter, filter_zero) -> "Buffer":
    """(CO, FH, FW, CI) u8 (Halide [ci, fx, fy, co]) -> the tiled filter as a Buffer, padded entries filter_zero: one
    tile_conv_filter_uint8 call, the re-tiling a model pays once."""
    filter = np.ascontiguousarray(filter, np.uint8)
    co, fh, fw, ci = filter.shape
    tiled = Buffer(aligned_array((fh, fw, -(-co // 16), -(-ci // 4), 16, 4), np.uint8, 64, 1))
    tile_conv_filter_uint8(Buffer(filter), filter_zero, filter_zero, tiled)
    return tiled


def hannk_conv2d(input, filter, bias, input_zero, filter_zero, stride, dilation, padding, multiplier, shift, output_zero=0, output_min=0,
                 output_max=255, out_dtype=np.uint8, tiled_filter=None) -> np.ndarray:
    """A quantised 2-D convolution as the interpreter runs one: input (B, H, W, C) u8, filter (CO, FH, FW, CI) u8, bias int32 (CO,) ->
    (B, OH, OW, CO) u8 or int16.  The channel axis is padded to a multiple of 4 and the image by `padding` with input_zero, the
    filter is tiled (or `tiled_filter` of hannk_tile_filter is used), then conv_u8_u8_u8 / conv_u8_u8_i16 runs."""
    filter = np.asarray(filter)
    _, multiple, shape = hannk_conv_shape(np.shape(input), filter.shape, stride, dilation, padding)
    if np.dtype(out_dtype) not in (np.dtype(np.uint8), np.dtype(np.int16)):
        raise TypeError("out_dtype is uint8 or int16")
    padded = hannk_pad_input(input, input_zero, multiple, padding)
    tiled = hannk_tile_filter(filter, filter_zero) if tiled_filter is None else tiled_filter
    out = Buffer(np.zeros(shape, out_dtype))
    fn = conv_u8_u8_u8 if np.dtype(out_dtype) == np.dtype(np.uint8) else conv_u8_u8_i16
    fn(Buffer(padded), input_zero, tiled, filter_zero, Buffer(np.ascontiguousarray(bias, np.int32)), _pair(stride), _pair(dilation), multiplier, shift,
       output_zero, output_min, output_max, out)
    return out.numpy()


def hannk_depthwise_conv2d(input, filter, bias, input_zero, filter_zero, stride, dilation, padding, multiplier, shift, output_zero=0, output_min=0,
                           output_max=255) -> np.ndarray:
    """A quantised depthwise convolution: input (B, H, W, C) u8, filter (FH, FW, C) u8, bias int32 (C,) -> (B, OH, OW, C) u8.  The
    channel axis is padded to a multiple of 16 and the image by `padding` with input_zero; an input of ONE channel under a filter of
    several runs the broadcast variant."""
    filter = np.ascontiguousarray(filter, np.uint8)
    broadcast, multiple, shape = hannk_conv_shape(np.shape(input), filter.shape, stride, dilation, padding, depthwise=True)
    padded = hannk_pad_input(input, input_zero, multiple, padding)
    out = Buffer(np.zeros(shape, np.uint8))
    fn = depthwise_conv_broadcast_uint8 if broadcast else depthwise_conv_uint8
    fn(Buffer(padded), input_zero, Buffer(filter), filter_zero, Buffer(np.ascontiguousarray(bias, np.int32)), _pair(stride), _pair(dilation), multiplier,
       shift, output_zero, output_min, output_max, out)
    return out.numpy()


def hannk_depthwise_conv2d_shallow(input, filter, bias, input_zero, filter_zero, stride, dilation, padding, multiplier, shift, output_zero=0,
                                   output_min=0, output_max=255) -> np.ndarray:
    """hannk_depthwise_conv2d through the shallow variant, as DepthwiseConv2DOp::execute takes it (ops.cpp:1007-1023): the image is padded
    with input_zero but its channels are not; c and x of input and output are fused in place.  Refuses (ValueError) what can_be_shallow
    refuses."""
    (sx, sy), (dx, dy), (px, py) = _pair(stride), _pair(dilation), _pair(padding)
    filter = np.ascontiguousarray(filter, np.uint8)
    b, h, w, _ = np.shape(input)
    broadcast, _, (_, oh, ow, c) = hannk_conv_shape(np.shape(input), filter.shape, (sx, sy), (dx, dy), (px, py), depthwise=True)
    if broadcast or not hannk_can_be_shallow(c, w + 2 * px, sx):
        raise ValueError("not shallow: stride_x is 1, the channel count is the filter's and divides 16, and channels * padded width >= 16")
    padded = hannk_pad_input(input, input_zero, 1, (px, py))
    out = np.zeros((b, oh, 1, ow * c), np.uint8)
    fused = padded.reshape(b, h + 2 * py, 1, (w + 2 * px) * c)
    ob = Buffer(out)
    depthwise_conv_shallow_uint8(Buffer(fused), input_zero, Buffer(filter), filter_zero, Buffer(np.ascontiguousarray(bias, np.int32)), (1, sy), (dx, dy),
                                 c, multiplier, shift, output_zero, output_min, output_max, ob)
    return ob.numpy().reshape(b, oh, ow, c)


def hannk_fully_connected(input, weights, bias, input_zero, filter_zero, multiplier, shift, output_zero=0, output_min=0, output_max=255) -> np.ndarray:
    """lower_tflite_fullyconnected: input of any rank flattened to (N, CI), weights (CO, CI) u8, bias int32 (CO,) -> (N, CO): the conv op on
    a 1 x 1 image"""
    weights = np.ascontiguousarray(weights, np.uint8)
    co, ci = weights.shape
    flat = np.ascontiguousarray(input, np.uint8).reshape(-1, ci)
    out = hannk_conv2d(flat.reshape(-1, 1, 1, ci), weights.reshape(co, 1, 1, ci), bias, input_zero, filter_zero, 1, 1, 0, multiplier, shift, output_zero,
                       output_min, output_max)
    return out.reshape(-1, co)


def hannk_pool2d(kind, input, filter, stride, padding="same", output_min=0, output_max=255) -> np.ndarray:
    """Pool2DOp::execute: input (B, H, W, C) u8 -> (B, OH, OW, C) u8, kind "average" or "max", padding "same" or "valid".  Nothing is
    padded: the input is translated by compute_padding and the op leaves the taps outside it out."""
    input = np.ascontiguousarray(input, np.uint8)
    (fw, fh), (sx, sy) = _pair(filter), _pair(stride)
    _, h, w, _ = input.shape
    shape = hannk_pool_shape(input.shape, (fw, fh), (sx, sy), padding)
    inb = Buffer(input, mins=(0, hannk_compute_padding(sx, w, fw, shape[2]), hannk_compute_padding(sy, h, fh, shape[1]), 0))
    out = Buffer(np.zeros(shape, np.uint8))
    {"average": average_pool_uint8, "max": max_pool_uint8}[kind](inb, (sx, sy), (fw, fh), output_min, output_max, out)
    return out.numpy()


def hannk_mean(input, axes, keepdims=True) -> np.ndarray:
    """ReductionOp::execute (Mean): input u8 of rank <= 4 (numpy order, padded to rank 4 in front), `axes` numpy axes to reduce."""
    input = np.ascontiguousarray(input, np.uint8)
    in4, box, out4, kept, dropped = hannk_mean_shapes(input.shape, np.atleast_1d(axes).tolist())
    out = Buffer(np.zeros(out4, np.uint8))
    mean_uint8(Buffer(input.reshape(in4)), *box, out)
    return out.numpy().reshape(kept if keepdims else dropped)


def _hannk_rank2(a, shape, dtype=np.uint8):
    """`a` as the [x, y] operand of hannk_rank2_rule against `shape`.  An operand with one element along the innermost axis is passed with a
    stride of 0 there; every other broadcast is expanded, the one over all outer axes included: the drivers launch what they always have."""
    a = np.asarray(a, dtype)
    rule = hannk_rank2_rule(a.shape, shape)
    if rule is None or rule[3] == 0:
        return np.ascontiguousarray(np.broadcast_to(a, tuple(shape))).reshape(-1, shape[-1] if len(shape) else 1)
    rows, n, stride0, stride1 = rule
    flat = np.ascontiguousarray(a).reshape(-1)
    return np.lib.stride_tricks.as_strided(flat, shape=(rows, n), strides=(stride1 * flat.itemsize, stride0 * flat.itemsize), writeable=False)


def hannk_add(in1, q1, in2, q2, qout, activation=None, sign2=1) -> np.ndarray:
    """ops.cpp's add_uint8: q = (scale, zero) of each tensor; sign2 = -1 subtracts.  An operand with one element along the innermost
    axis is passed with a stride of 0, not expanded."""
    shape = np.broadcast_shapes(np.shape(in1), np.shape(in2))
    m1, m2 = hannk_add_multipliers(q1[0], q2[0], qout[0], sign2)
    lo, hi = hannk_output_range(activation, qout[1], qout[0])
    a, b = _hannk_rank2(in1, shape), _hannk_rank2(in2, shape)
    out = Buffer(np.zeros(a.shape, np.uint8))
    add_uint8_uint8(Buffer(a), q1[1], m1, Buffer(b), q2[1], m2, qout[1], lo, hi, out)
    return out.numpy().reshape(shape)


def hannk_mul(in1, q1, in2, q2, qout, activation=None) -> np.ndarray:
    """ops.cpp's mul_uint8: the multiplier is IntFloat<int32_t>(s1 * s2 / sout) * 2^-12."""
    shape = np.broadcast_shapes(np.shape(in1), np.shape(in2))
    m, shift = hannk_mul_params(q1[0], q2[0], qout[0])
    lo, hi = hannk_output_range(activation, qout[1], qout[0])
    a, b = _hannk_rank2(in1, shape), _hannk_rank2(in2, shape)
    out = Buffer(np.zeros(a.shape, np.uint8))
    mul_uint8_uint8_uint8(Buffer(a), q1[1], Buffer(b), q2[1], qout[1], m, shift, lo, hi, out)
    return out.numpy().reshape(shape)


def hannk_requantize(input, q_in, q_out, activation=None) -> np.ndarray:
    """try_requantize (ops.cpp:487-504) on a uint8 array: add_uint8(in * 1 + in * 0) from q_in = (scale, zero) to q_out"""
    input = np.ascontiguousarray(input, np.uint8)
    return hannk_add(input, q_in, input, q_in, q_out, activation, sign2=0)


def _hannk_rows(fn, input, axis):
    """input of any rank, the op over numpy `axis`: rank 2 keeps the caller's memory and transposes the buffers as ops.cpp does (dimension
    0 then has the row stride); other ranks are brought to (rows, n)"""
    input = np.asarray(input, np.uint8)
    axis %= input.ndim
    if input.ndim == 2:
        src = np.ascontiguousarray(input)
        dst = np.zeros(src.shape, np.uint8)
        view = (lambda a: a) if axis == 1 else (lambda a: a.T)
        out = Buffer(view(dst))
        fn(Buffer(view(src)), out)
        out.numpy()
        return dst
    moved = np.ascontiguousarray(np.moveaxis(input, axis, -1))
    out = Buffer(np.zeros((moved.size // moved.shape[-1], moved.shape[-1]), np.uint8))
    fn(Buffer(moved.reshape(out.array.shape)), out)
    return np.moveaxis(out.numpy().reshape(moved.shape), -1, axis)


def hannk_softmax(input, in_scale, beta=1.0, out_scale=1.0 / 256, out_zero=0, axis=-1) -> np.ndarray:
    bm, bs, om, osh = hannk_softmax_params(in_scale, beta, out_scale)
    return _hannk_rows(lambda i, o: softmax_uint8(i, bm, bs, out_zero, om, osh, o), input, axis)


def hannk_l2_normalization(input, input_zero, axis=-1) -> np.ndarray:
    """L2NormalizationOp::execute: the output has scale 1 / 128 and zero point 128"""
    return _hannk_rows(lambda i, o: l2_normalization_uint8(i, input_zero, o), input, axis)


def hannk_elementwise(inputs, program, outputs=1):
    """ElementwiseProgramOp::execute: one to five inputs of one dtype, uint8 or int16 (the last is repeated up to five, as ops.cpp:1080-1084
    does), broadcast against each other; program an [n, 5] int16 array.  uint8 inputs -> the uint8 result (outputs = 1); int16 inputs ->
    the pair (uint8, int16) (outputs = 2): the two variants the library has."""
    if not 1 <= len(inputs) <= 5:
        raise ValueError("one to five inputs")
    dtype = np.asarray(inputs[0]).dtype
    want = {np.dtype(np.uint8): 1, np.dtype(np.int16): 2}.get(dtype)
    if want is None:
        raise TypeError("the inputs are uint8 or int16")
    if outputs != want:
        raise ValueError(f"{dtype} inputs have {want} output(s)")
    shape = np.broadcast_shapes(*[np.shape(a) for a in inputs])
    arrs = [_hannk_rank2(a, shape, dtype) for a in inputs]
    bufs = [Buffer(a) for a in arrs]
    bufs += [bufs[-1]] * (5 - len(bufs))
    prog = Buffer(np.ascontiguousarray(program, np.int16).reshape(-1, 5))
    out0 = Buffer(np.zeros(arrs[0].shape, np.uint8))
    if want == 1:
        elementwise_5xuint8_1xuint8(*bufs, prog, out0)
        return out0.numpy().reshape(shape)
    out1 = Buffer(np.zeros(arrs[0].shape, np.int16))
    elementwise_5xint16_1xuint8int16(*bufs, prog, out0, out1)
    return out0.numpy().reshape(shape), out1.numpy().reshape(shape)


def hannk_logistic(x, in_scale, in_zero) -> np.ndarray:
    """UnaryOp Logistic on a uint8 array of any shape: the result has scale 1 / 256 and zero point 0"""
    return hannk_elementwise([np.asarray(x, np.uint8)], hannk_logistic_program(in_scale, in_zero))


def hannk_tanh(x, in_scale, in_zero) -> np.ndarray:
    """UnaryOp Tanh: the result has scale 1 / 128 and zero point 128"""
    return hannk_elementwise([np.asarray(x, np.uint8)], hannk_tanh_program(in_scale, in_zero))


def hannk_lstm_elementwise(input_gate, input_modulation_gate, forget_gate, output_gate, prev_state):
    """The LSTM cell's elementwise program on five int16 arrays -> (activation uint8, state int16)"""
    return hannk_elementwise([np.asarray(a, np.int16) for a in (input_gate, input_modulation_gate, forget_gate, output_gate, prev_state)],
                             hannk_lstm_program(), outputs=2)


def hannk_pad(input, padding, pad_value) -> np.ndarray:
    """PadOp::execute on a uint8 array of rank <= 4 (numpy order, padded to rank 4 in front): `padding` is one (before, after) pair per numpy
    axis.  One fill_uint8 or copy_uint8_uint8 per box of hannk_pad_boxes."""
    input = np.ascontiguousarray(input, np.uint8)
    nd = input.ndim
    if nd > 4 or len(padding) != nd:
        raise ValueError("rank <= 4 and one (before, after) pair per axis")
    in4 = input.reshape((1,) * (4 - nd) + input.shape)
    shape, imin, boxes = hannk_pad_boxes(in4.shape, [(0, 0)] * (4 - nd) + list(padding))
    out = np.zeros(shape, np.uint8)
    for kind, omin, omax in boxes:
        b = Buffer(out[hannk_box_slices(omin, omax)], mins=omin)
        if kind == "fill":
            fill_uint8(pad_value, b)
        else:
            copy_uint8_uint8(Buffer(in4, mins=imin), pad_value, b)
        b.numpy()
    return out.reshape(shape[4 - nd:])


def hannk_upsample_channels(input, factor) -> np.ndarray:
    """(B, H, W, C) uint8 -> (B, H, W, C * factor): channel c of the result is channel c // factor of the input (depth multiplier > 1)"""
    input = np.ascontiguousarray(input, np.uint8)
    if input.ndim != 4 or int(factor) < 1:
        raise ValueError("a (B, H, W, C) array and a factor >= 1")
    out = Buffer(np.zeros(input.shape[:3] + (input.shape[3] * int(factor),), np.uint8))
    upsample_channels_uint8(Buffer(input), factor, out)
    return out.numpy()


def _hannk_movable(a):
    a = np.ascontiguousarray(a)
    if a.dtype not in _TYPE_OF:
        raise TypeError(f"unsupported dtype {a.dtype}")
    return a


def _hannk_copy_views(src_view, dst_view, general=False):
    d = Buffer(dst_view)
    hannk_copy_from(Buffer(src_view), d, general)
    d.numpy()


def hannk_transpose(input, perm, general=False) -> np.ndarray:
    """TransposeOp::execute: np.transpose(input, perm) as one copy_from into the output re-viewed in the input's order"""
    input = _hannk_movable(input)
    inverse = hannk_inverse_perm(perm, input.ndim)
    out = np.zeros(tuple(input.shape[p] for p in perm), input.dtype)
    _hannk_copy_views(input, out.transpose(inverse), general)
    return out


def hannk_space_to_depth(input, block_size, general=False) -> np.ndarray:
    """SpaceToDepth: (B, H, W, C) -> (B, H / block, W / block, block^2 * C), one copy_from over rank-6 views"""
    input = _hannk_movable(input)
    out = np.zeros(hannk_block_shape(input.shape, int(block_size), True), input.dtype)
    space6, depth6, perm = hannk_block_views(input.shape, int(block_size))
    _hannk_copy_views(input.reshape(space6), out.reshape(depth6).transpose(perm), general)
    return out


def hannk_depth_to_space(input, block_size, general=False) -> np.ndarray:
    """DepthToSpace: (B, H, W, block^2 * C) -> (B, H * block, W * block, C)"""
    input = _hannk_movable(input)
    out = np.zeros(hannk_block_shape(input.shape, int(block_size), False), input.dtype)
    space6, depth6, perm = hannk_block_views(out.shape, int(block_size))
    _hannk_copy_views(input.reshape(depth6).transpose(perm), out.reshape(space6), general)
    return out


def hannk_concatenation(inputs, axis, quantization=None, general=False) -> np.ndarray:
    """ConcatenationOp::execute: every input goes into its crop of the output through requantize_or_copy.  `quantization` = [(scale, zero) of
    each input ..., (scale, zero) of the output] sends uint8 pieces through the add kernel, equal scales or not, as the reference does;
    without it the pieces are copied."""
    inputs = [_hannk_movable(a) for a in inputs]
    axis, shape = hannk_concat_shape([a.shape for a in inputs], int(axis))
    out = np.zeros(shape, inputs[0].dtype)
    if any(a.dtype != out.dtype for a in inputs):
        raise ValueError("the inputs share dtype and every extent but the axis'")
    at = 0
    for i, a in enumerate(inputs):
        piece = out[(slice(None),) * axis + (slice(at, at + a.shape[axis]),)]
        if quantization is not None and out.dtype == np.dtype(np.uint8):
            piece[...] = hannk_requantize(a, quantization[i], quantization[-1])
        else:
            _hannk_copy_views(a, piece, general)
        at += a.shape[axis]
    return out


def hannk_split(input, sizes, axis, quantization=None, general=False) -> list:
    """SplitOp::execute: `sizes` an int (that many equal pieces) or the pieces' extents along `axis`; `quantization` = [(scale, zero) of the
    input, (scale, zero) of each output ...] as for hannk_concatenation."""
    input = _hannk_movable(input)
    axis = int(axis) % input.ndim
    outs, at = [], 0
    for i, size in enumerate(hannk_split_sizes(input.shape[axis], sizes)):
        piece = input[(slice(None),) * axis + (slice(at, at + size),)]
        if quantization is not None and input.dtype == np.dtype(np.uint8):
            outs.append(hannk_requantize(piece, quantization[0], quantization[1 + i]))
        else:
            out = np.zeros(piece.shape, input.dtype)
            _hannk_copy_views(piece, out, general)
            outs.append(out)
        at += size
    return outs


def hannk_gather(input, indices, axis=0) -> np.ndarray:
    """GatherOp::execute: np.take(input, indices, axis) for int32 indices of rank 0 .. 2 in one launch"""
    input = _hannk_movable(input)
    indices = np.require(indices, np.int32, "C")   # (ascontiguousarray would make a scalar index a vector)
    axis, shape = hannk_gather_shape(input.shape, indices.shape, int(axis))
    out = Buffer(np.zeros(shape, input.dtype))
    hannk_gather_buffers(Buffer(input), Buffer(indices), input.ndim - 1 - axis, out)
    return out.numpy()


# debug hooks: test and measurement only
def debug_hannk_general(name: str, *args) -> int:
    """Test and measurement hook: the entry point `name` of HANNK_OPS, HANNK_NN_OPS or HANNK_PROGRAM_OPS, with the arguments of its C signature in order
    (stride and dilation as four scalars), with one thread per output running the contract's loops as written."""
    if name not in _HANNK_ALL_PARAMS:
        raise ValueError(f"no hannk entry point named {name}")
    md = metadata(name)
    if len(args) != md.num_arguments:
        raise TypeError(f"{name} takes {md.num_arguments} arguments, not {len(args)}")
    keep, argv = [], (C.c_void_p * md.num_arguments)()
    for j, v in enumerate(args):
        a = md.arguments[j]
        box = _SCALAR_CTYPES[(a.type.code, a.type.bits)](int(v)) if a.kind == 0 else (v.raw if isinstance(v, Buffer) else v.contents)
        keep.append(box)
        argv[j] = C.cast(C.pointer(box), C.c_void_p)
    return _hannk_general(name, argv)


def debug_hannk_quantize(fn, acc, multiplier, shift, zero=0, lo=0, hi=255) -> np.ndarray:
    """Test hook: the device's epilogue alone on an int32 array: fn 0 or "i16" = quantize_i16 (int16 result), fn 1 or "u8" =
    quantize_and_relu_u8 (uint8 result)."""
    fn = {"i16": 0, "u8": 1}.get(fn, fn)
    acc = np.ascontiguousarray(acc, np.int32)
    out = np.zeros(acc.shape, np.int16 if fn == 0 else np.uint8)
    f = lib.hlmi_debug_hannk_quantize
    f.restype, f.argtypes = C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.c_uint8, C.c_uint8, C.c_uint8, C.c_void_p]
    rc = f(int(fn), acc.ctypes.data, acc.size, int(multiplier), int(shift), int(zero), int(lo), int(hi), out.ctypes.data)
    if rc != 0:
        raise HalideError(-1, f"hlmi_debug_hannk_quantize failed ({rc})")
    return out


def debug_hannk_conv_plan(npix, channels, quads, cus=256) -> dict:
    """What conv_u8_u8_*'s plan chooses for `npix` output pixels, `channels` output channels and `quads` = fw * fh * ci / 4 on `cus`
    compute units (aligned operands; HLMI_HANNK_SPLIT_K is read as in a call)."""
    out = (C.c_int32 * 3)()
    f = lib.hlmi_debug_hannk_conv_plan
    f.restype, f.argtypes = C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    if f(int(npix), int(channels), int(quads), int(cus), out) != 0:
        raise ValueError("hlmi_debug_hannk_conv_plan: sizes must be positive")
    return {"mfma": bool(out[0]), "splits": int(out[1]), "wave_tiles": int(out[2])}


def debug_hannk_approx(fn, q, x, q_x=0, bits=32) -> np.ndarray:
    """Test hook: the device's approx_log2 / approx_exp2 / approx_reciprocal / approx_reciprocal_sqrt (fn 0 .. 3 or the name) of
    common_halide.cpp in Int(bits), over an int32 array."""
    fn = {"approx_log2": 0, "approx_exp2": 1, "approx_reciprocal": 2, "approx_reciprocal_sqrt": 3}.get(fn, fn)
    x = np.ascontiguousarray(x, np.int32)
    out = np.zeros(x.shape, np.int32)
    f = lib.hlmi_debug_hannk_approx
    f.restype, f.argtypes = C.c_int, [C.c_int, C.c_int32, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.c_void_p]
    rc = f(int(fn), int(q), x.ctypes.data, x.size, int(q_x), int(bits), out.ctypes.data)
    if rc != 0:
        raise HalideError(-1, f"hlmi_debug_hannk_approx failed ({rc})")
    return out


def debug_hannk_program_approx(fn, x, q, q_x, width=16) -> np.ndarray:
    """Test hook: the device's approx_log2p1_exp2 / approx_log2m1_exp2 / approx_logistic / approx_tanh (fn 0 .. 3 or the name) in Int(16):
    x the i16 argument, q the result's precision, q_x the argument's (each 0 .. 15), broadcast against each other; `width` (16 or 32) is
    the width of the count q_x."""
    fn = {"approx_log2p1_exp2": 0, "approx_log2m1_exp2": 1, "approx_logistic": 2, "approx_tanh": 3}.get(fn, fn)
    shape = np.broadcast_shapes(np.shape(x), np.shape(q), np.shape(q_x))
    x, q, q_x = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.int32), shape)) for v in (x, q, q_x))
    out = np.zeros(shape, np.int32)
    f = lib.hlmi_debug_hannk_program_approx
    f.restype, f.argtypes = C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p]
    rc = f(int(fn), x.ctypes.data, q.ctypes.data, q_x.ctypes.data, x.size, int(width), out.ctypes.data)
    if rc != 0:
        raise HalideError(-1, f"hlmi_debug_hannk_program_approx failed ({rc})")
    return out


def debug_hannk_move_plan(src, dst, general=False) -> dict:
    """What hannk_copy_from's plan chooses for two Buffers (only their types and dimensions are read; no device is needed): the kernel, one
    of HANNK_MOVE_KERNELS, and the number of dimensions left after dropping extent-1 dimensions and merging."""
    out = (C.c_int32 * 2)()
    f = lib.hlmi_debug_hannk_move_plan
    f.restype, f.argtypes = C.c_int, [_BP, _BP, C.c_int32, C.POINTER(C.c_int32)]
    rc = f(_as_ptr(src), _as_ptr(dst), int(bool(general)), out)
    if rc != 0:
        raise ValueError(f"hlmi_debug_hannk_move_plan: {'dst aliases itself' if rc == -8 else 'bad arguments'}")
    return {"kernel": HANNK_MOVE_KERNELS[out[0]], "rank": int(out[1])}


# what the package re-exports: every public name DEFINED above (constants, functions, the assembler), none of the imports
__all__ = [n for n, v in list(globals().items()) if not n.startswith("_") and not isinstance(v, type(np)) and getattr(v, "__module__", __name__) == __name__]
