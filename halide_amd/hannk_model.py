"""apps/hannk's interpreter as a plan over this library's entry points: HannkModel.from_tflite(path_or_bytes), or
HannkModel(graph) for a tflite_reader.Graph built in Python.

`model.plan` is a list of Steps: the name of one entry point, and its arguments in the order of its C signature, each an int or a View
(tensor id, element offset, mins, extents, strides in Halide order).  `model.setup` holds the steps that run once (filter tiling).  The plan
is backend-neutral: prepare() / run() issue it on the device, tests/hannk_model_checker.py walks the same plan on numpy arrays through the
plain-C checkers.  `model.tensors` lists the graph's tensors followed by the ones the lowering adds (padded conv inputs, tiled filters,
programs); one allocation per tensor, no planner, no aliasing except RESHAPE of a dense tensor, which is a view.

Lowering follows interpreter/ops.cpp and lower.cpp; the parameter derivations are the hannk.hannk_* helpers'.  Of ConvOp::execute's
reshapes (the x/y fusion of 1 x 1 filters and the x/y swap, ops.cpp:879-898) none is kept: the conv kernels here tile output pixels
as one flat index, so neither changes which kernel runs.  The shallow depthwise variant is not chosen by the lowering."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

import halide_amd as hl
from halide_amd import hannk
from halide_amd import tflite_reader as tfl

View = namedtuple("View", "tensor offset mins extents strides")
Step = namedtuple("Step", "name args")
Slot = namedtuple("Slot", "shape dtype data alias")   # shape: Halide extents; data: a constant in numpy order; alias: the tensor whose memory it shares

_f32 = np.float32


def _dense(shape):
    out, s = [], 1
    for e in shape:
        out.append(s)
        s *= max(int(e), 1)
    return out


def _round_up(v, m):
    return -(-v // m) * m


class HannkModel:
    def __init__(self, graph):
        self.graph = graph
        self.tensors = [Slot(tuple(t.shape), np.dtype(t.dtype), t.data, None) for t in graph.tensors]
        self.setup, self.plan = [], []
        self._device = None
        for op in graph.ops:
            lower = getattr(self, "_lower_" + op.kind.lower(), None)
            if lower is None:
                raise NotImplementedError(f"hannk_model: operator {op.kind} has no lowering")
            lower(op)

    @classmethod
    def from_tflite(cls, source):
        return cls(tfl.read(source))

    # ------------------------------------------------------------------------------------------------------------ views
    def _q(self, i):
        t = self.graph.tensors[i]
        if len(t.scale) != 1 or len(t.zero) != 1:
            raise NotImplementedError("hannk_model: a quantised op needs one scale and one zero point per tensor")
        return float(t.scale[0]), int(t.zero[0])

    def _new(self, shape, dtype=np.uint8, data=None):
        self.tensors.append(Slot(tuple(int(e) for e in shape), np.dtype(dtype), data, None))
        return len(self.tensors) - 1

    def _whole(self, i, rank=None):
        shape = list(self.tensors[i].shape)
        strides = _dense(shape)
        total = int(np.prod(shape, dtype=np.int64)) if shape else 1
        while rank is not None and len(shape) < rank:
            shape.append(1)
            strides.append(total)
        if rank is not None and len(shape) > rank:
            raise NotImplementedError(f"hannk_model: a tensor of rank {len(shape)} where rank {rank} is the most")
        return View(i, 0, (0,) * len(shape), tuple(shape), tuple(strides))

    def _rank2(self, i, like=None):
        """tensor i as an [x, y] operand: dimension 0 and everything outside it; against `like` (the full shape) extent-1 dimensions
        are broadcast with a stride of 0, as elementwise_loop_nest<2> does"""
        shape = self.tensors[i].shape[::-1]
        try:
            rule = hannk.hannk_rank2_rule(shape, shape if like is None else tuple(like)[::-1])
        except ValueError:
            raise NotImplementedError("hannk_model: operands that do not broadcast") from None
        if rule is None:
            raise NotImplementedError("hannk_model: broadcasting of some but not all outer dimensions")
        rows, n, s0, s1 = rule
        return View(i, 0, (0, 0), (n, rows), (s0, s1))

    def _piece(self, i, axis, at, size):
        """the crop [at, at + size) of tensor i along Halide dimension `axis`, as an [x, y] view: the dimensions up to the axis are one row"""
        shape = self.tensors[i].shape
        inner = int(np.prod(shape[:axis], dtype=np.int64)) if axis else 1
        outer = int(np.prod(shape[axis + 1:], dtype=np.int64)) if axis + 1 < len(shape) else 1
        return View(i, at * inner, (0, 0), (inner * size, outer), (1, inner * shape[axis]))

    # ------------------------------------------------------------------------------------------------------------ shared pieces
    def _requant(self, src, qin, dst, qout, activation=None):
        """requantize_or_copy's quantised branch: add_uint8(in * 1 + in * 0)"""
        m1, m2 = hannk.hannk_add_multipliers(qin[0], qin[0], qout[0], 0)
        lo, hi = hannk.hannk_output_range(activation, qout[1], qout[0])
        self.plan.append(Step("add_uint8_uint8", (src, qin[1], m1, src, qin[1], m2, qout[1], lo, hi, dst)))

    def _move(self, i_src, src, i_dst, dst):
        """requantize_or_copy: quantised uint8 always goes through the add kernel, anything else through copy_from"""
        a, b = self.graph.tensors[i_src], self.graph.tensors[i_dst]
        if a.dtype != b.dtype:
            raise ValueError("hannk_model: input and output types must match")
        if a.dtype == np.uint8 and a.quantized and b.quantized:
            self._requant(src, self._q(i_src), dst, self._q(i_dst))
        else:
            self.plan.append(Step("hannk_copy_from", (src, dst)))

    def _padded(self, x, zero, channel_multiple, before, need):
        """tensor x ([c, w, h, b]) inside a tensor of [round_up(c), need_w, need_h, b] filled with `zero`, x at (before_x, before_y): the PAD
        step of a conv op, written on the device; x itself where nothing is to pad"""
        c, w, h, b = self._whole(x, 4).extents
        cp = _round_up(c, channel_multiple)
        (px, py), (nw, nh) = before, (max(need[0], w + before[0]), max(need[1], h + before[1]))
        if (cp, nw, nh) == (c, w, h):
            return self._whole(x, 4)
        p = self._new((cp, nw, nh, b))
        whole = self._whole(p)
        self.plan.append(Step("fill_uint8", (zero, whole)))
        src = self._whole(x, 4)._replace(mins=(0, px, py, 0))
        crop = View(p, px * whole.strides[1] + py * whole.strides[2], (0, px, py, 0), (cp, w, h, b), whole.strides)
        self.plan.append(Step("copy_uint8_uint8", (src, zero, crop)))
        return whole

    def _window(self, attrs, size, filt, out, dilation=(1, 1)):
        """(padding in front, input extent the op reads) along x and y"""
        before, need = [], []
        for k in range(2):
            eff = (filt[k] - 1) * dilation[k] + 1
            before.append(hannk.hannk_compute_padding(attrs["stride"][k], size[k], eff, out[k]) if attrs["padding"] == "same" else 0)
            need.append((out[k] - 1) * attrs["stride"][k] + eff)
        return tuple(before), tuple(need)

    def _multiply_params(self, a, b, c):
        m, e = hannk.hannk_int_float(_f32(a) * _f32(b) / _f32(c), 32)
        return m, -e

    # ------------------------------------------------------------------------------------------------------------ lowerings
    def _lower_conv_2d(self, op, flat=False):
        x, f, bias = op.inputs[:3]
        out = op.outputs[0]
        (si, zi), (sf, zf), (so, zo) = self._q(x), self._q(f), self._q(out)
        filt = self.graph.tensors[f].data
        if filt is None or self.graph.tensors[bias].data is None:
            raise NotImplementedError("hannk_model: conv filters and biases are constants")
        a = op.attrs
        if flat:      # lower_tflite_fullyconnected: the input flattened to [ci, n], the conv on a 1 x 1 image
            co, ci = filt.shape
            n = int(np.prod(self.tensors[x].shape, dtype=np.int64)) // ci
            f = self._new((ci, 1, 1, co), np.uint8, np.ascontiguousarray(filt).reshape(co, 1, 1, ci))
            xin = View(x, 0, (0, 0, 0, 0), (ci, 1, 1, n), (1, ci, ci, ci))
            oview = View(out, 0, (0, 0, 0, 0), (co, 1, 1, n), (1, co, co, co))
            a = {"stride": (1, 1), "dilation": (1, 1), "padding": "valid", "activation": a["activation"]}
            if ci % hannk.HANNK_VECTOR_REDUCTION:
                p = self._new((_round_up(ci, hannk.HANNK_VECTOR_REDUCTION), 1, 1, n))
                whole = self._whole(p)
                self.plan.append(Step("fill_uint8", (zi, whole)))
                self.plan.append(Step("copy_uint8_uint8", (xin, zi, whole)))
                xin = whole
            fh = fw = 1
        else:
            co, fh, fw, ci = filt.shape
            oview = self._whole(out, 4)
            _, w, h, _ = self._whole(x, 4).extents
            before, need = self._window(a, (w, h), (fw, fh), oview.extents[1:3], a["dilation"])
            xin = self._padded(x, zi, hannk.HANNK_VECTOR_REDUCTION, before, need)
        tiled = self._new((4, 16, -(-ci // 4), -(-co // 16), fw, fh))
        self.setup.append(Step("tile_conv_filter_uint8", (self._whole(f, 4), zf, zf, self._whole(tiled))))
        m, shift = self._multiply_params(si, sf, so)
        lo, hi = hannk.hannk_output_range(a["activation"], zo, so)
        self.plan.append(Step("conv_u8_u8_u8", (xin, zi, self._whole(tiled), zf, self._whole(bias), a["stride"][0], a["stride"][1], a["dilation"][0],
                                                a["dilation"][1], m, shift, zo, lo, hi, oview)))

    def _lower_fully_connected(self, op):
        self._lower_conv_2d(op, flat=True)

    def _lower_depthwise_conv_2d(self, op):
        x, f, bias = op.inputs[:3]
        out = op.outputs[0]
        (si, zi), (sf, zf), (so, zo) = self._q(x), self._q(f), self._q(out)
        filt = self.graph.tensors[f].data
        if filt is None or self.graph.tensors[bias].data is None:
            raise NotImplementedError("hannk_model: depthwise filters and biases are constants")
        a = op.attrs
        _, fh, fw, co = filt.shape
        f3 = self._new((co, fw, fh), np.uint8, np.ascontiguousarray(filt).reshape(fh, fw, co))
        c, w, h, b = self._whole(x, 4).extents
        mult = int(a["depth_multiplier"])
        broadcast = c == 1 and mult > 1
        if mult > 1 and not broadcast:      # any other multiplier: upsample_channels first
            up = self._new((c * mult, w, h, b))
            self.plan.append(Step("upsample_channels_uint8", (self._whole(x, 4), mult, self._whole(up))))
            x = up
        oview = self._whole(out, 4)
        before, need = self._window(a, (w, h), (fw, fh), oview.extents[1:3], a["dilation"])
        xin = self._padded(x, zi, 1 if broadcast else hannk.HANNK_DEPTHWISE_VECTOR, before, need)
        m, shift = self._multiply_params(si, sf, so)
        lo, hi = hannk.hannk_output_range(a["activation"], zo, so)
        name = "depthwise_conv_broadcast_uint8" if broadcast else "depthwise_conv_uint8"
        self.plan.append(Step(name, (xin, zi, self._whole(f3), zf, self._whole(bias), a["stride"][0], a["stride"][1], a["dilation"][0], a["dilation"][1],
                                     0, m, shift, zo, lo, hi, oview)))

    def _pool(self, op, name):
        x, out = op.inputs[0], op.outputs[0]
        a = op.attrs
        so, zo = self._q(out)
        _, w, h, _ = self._whole(x, 4).extents
        oview = self._whole(out, 4)
        before, _ = self._window(a, (w, h), a["filter"], oview.extents[1:3])
        lo, hi = hannk.hannk_output_range(a["activation"], zo, so)
        xin = self._whole(x, 4)._replace(mins=(0, before[0], before[1], 0))
        self.plan.append(Step(name, (xin, a["stride"][0], a["stride"][1], a["filter"][0], a["filter"][1], lo, hi, oview)))

    def _lower_average_pool_2d(self, op):
        self._pool(op, "average_pool_uint8")

    def _lower_max_pool_2d(self, op):
        self._pool(op, "max_pool_uint8")

    def _binary(self, op, sign2=1, mul=False):
        i1, i2 = op.inputs[:2]
        out = op.outputs[0]
        (s1, z1), (s2, z2), (so, zo) = self._q(i1), self._q(i2), self._q(out)
        full = self.tensors[out].shape
        a, b, o = self._rank2(i1, full), self._rank2(i2, full), self._rank2(out)
        lo, hi = hannk.hannk_output_range(op.attrs.get("activation"), zo, so)
        if mul:
            m, shift = hannk.hannk_mul_params(s1, s2, so)
            self.plan.append(Step("mul_uint8_uint8_uint8", (a, z1, b, z2, zo, m, shift, lo, hi, o)))
        else:
            m1, m2 = hannk.hannk_add_multipliers(s1, s2, so, sign2)
            self.plan.append(Step("add_uint8_uint8", (a, z1, m1, b, z2, m2, zo, lo, hi, o)))

    def _lower_add(self, op):
        self._binary(op)

    def _lower_sub(self, op):
        self._binary(op, sign2=-1)

    def _lower_mul(self, op):
        self._binary(op, mul=True)

    def _activation(self, op, activation):      # try_requantize with the activation's range
        x, out = op.inputs[0], op.outputs[0]
        m1, m2 = hannk.hannk_add_multipliers(self._q(x)[0], self._q(x)[0], self._q(out)[0], 0)
        lo, hi = hannk.hannk_output_range(activation, self._q(out)[1], self._q(out)[0])
        v = self._rank2(x)
        self.plan.append(Step("add_uint8_uint8", (v, self._q(x)[1], m1, v, self._q(x)[1], m2, self._q(out)[1], lo, hi, self._rank2(out))))

    def _lower_relu(self, op):
        self._activation(op, "relu")

    def _lower_relu6(self, op):
        self._activation(op, "relu6")

    def _lower_relu_n1_to_1(self, op):
        self._activation(op, "relu_n1_to_1")

    def _program(self, op, program):
        x, out = op.inputs[0], op.outputs[0]
        p = self._new((5, program.shape[0]), np.int16, np.ascontiguousarray(program, np.int16))
        v = self._rank2(x)
        self.plan.append(Step("elementwise_5xuint8_1xuint8", (v, v, v, v, v, self._whole(p), self._rank2(out))))

    def _lower_logistic(self, op):
        self._program(op, hannk.hannk_logistic_program(*self._q(op.inputs[0])))

    def _lower_tanh(self, op):
        self._program(op, hannk.hannk_tanh_program(*self._q(op.inputs[0])))

    def _lower_softmax(self, op):
        x, out = op.inputs[0], op.outputs[0]
        bm, bs, om, osh = hannk.hannk_softmax_params(self._q(x)[0], op.attrs["beta"], self._q(out)[0])
        self.plan.append(Step("softmax_uint8", (self._rank2(x), bm, bs, self._q(out)[1], om, osh, self._rank2(out))))

    def _lower_l2_normalization(self, op):
        x, out = op.inputs[0], op.outputs[0]
        self.plan.append(Step("l2_normalization_uint8", (self._rank2(x), self._q(x)[1], self._rank2(out))))

    def _lower_mean(self, op):
        x, out = op.inputs[0], op.outputs[0]
        xin = self._whole(x, 4)
        red = [xin.extents[d] if d in op.attrs["axes"] else 1 for d in range(4)]
        oshape = [1 if d in op.attrs["axes"] else xin.extents[d] for d in range(4)]
        oview = View(out, 0, (0, 0, 0, 0), tuple(oshape), tuple(_dense(oshape)))
        self.plan.append(Step("mean_uint8", (xin, 0, red[0], 0, red[1], 0, red[2], 0, red[3], oview)))

    def _lower_pad(self, op):
        x, out = op.inputs[0], op.outputs[0]
        zero = self._q(out)[1]
        before = [b for b, _ in op.attrs["padding"]] + [0] * (4 - len(op.attrs["padding"]))
        xin, whole = self._whole(x, 4), self._whole(out, 4)
        self.plan.append(Step("fill_uint8", (zero, whole)))
        off = sum(b * st for b, st in zip(before[1:], whole.strides[1:]))
        crop = View(out, off, (0,) + tuple(before[1:]), (whole.extents[0],) + tuple(xin.extents[1:]), whole.strides)
        self.plan.append(Step("copy_uint8_uint8", (xin._replace(mins=tuple(before)), zero, crop)))      # channels outside the input: the pad value

    def _lower_reshape(self, op):
        x, out = op.inputs[0], op.outputs[0]
        if int(np.prod(self.tensors[x].shape, dtype=np.int64)) != int(np.prod(self.tensors[out].shape, dtype=np.int64)):
            raise ValueError("hannk_model: RESHAPE changes the number of elements")
        root = x if self.tensors[x].alias is None else self.tensors[x].alias
        self.tensors[out] = self.tensors[out]._replace(alias=root)      # every tensor here is dense: a view

    def _lower_concatenation(self, op):
        out, axis, at = op.outputs[0], op.attrs["axis"], 0
        for i in op.inputs:
            size = self.tensors[i].shape[axis]
            self._move(i, self._piece(i, axis, 0, size), out, self._piece(out, axis, at, size))
            at += size

    def _split(self, op, sizes):
        x, axis, at = op.inputs[0], op.attrs["axis"], 0
        for i, size in zip(op.outputs, sizes):
            self._move(x, self._piece(x, axis, at, size), i, self._piece(i, axis, 0, size))
            at += size

    def _lower_split(self, op):
        n = self.tensors[op.inputs[0]].shape[op.attrs["axis"]]
        self._split(op, [n // len(op.outputs)] * len(op.outputs))

    def _lower_split_v(self, op):
        self._split(op, op.attrs["size_splits"])

    def _lower_transpose(self, op):
        x, out = op.inputs[0], op.outputs[0]
        r, perm = len(self.tensors[x].shape), op.attrs["perm"]
        ostr = _dense(self.tensors[out].shape)
        strides = [0] * r
        for i, p in enumerate(perm):      # numpy axis i of the output is numpy axis p of the input: Halide r-1-i and r-1-p
            strides[r - 1 - p] = ostr[r - 1 - i]
        self.plan.append(Step("hannk_copy_from", (self._whole(x), View(out, 0, (0,) * r, self.tensors[x].shape, tuple(strides)))))

    def _block_views(self, space, depth, block):
        """the two rank-6 views of hannk_block_views in Halide order: the space tensor dense, the depth tensor's dense strides permuted"""
        space6, depth6, perm = hannk.hannk_block_views(self.tensors[space].shape[::-1], block)
        dstr = _dense(depth6[::-1])[::-1]
        return (View(space, 0, (0,) * 6, space6[::-1], tuple(_dense(space6[::-1]))),
                View(depth, 0, (0,) * 6, tuple(depth6[p] for p in perm)[::-1], tuple(dstr[p] for p in perm)[::-1]))

    def _lower_space_to_depth(self, op):
        s6, d6 = self._block_views(op.inputs[0], op.outputs[0], op.attrs["block_size"])
        self.plan.append(Step("hannk_copy_from", (s6, d6)))

    def _lower_depth_to_space(self, op):
        s6, d6 = self._block_views(op.outputs[0], op.inputs[0], op.attrs["block_size"])
        self.plan.append(Step("hannk_copy_from", (d6, s6)))

    def _lower_gather(self, op):
        x, idx = op.inputs[:2]
        self.plan.append(Step("hannk_gather", (self._whole(x), self._whole(idx), op.attrs["axis"], self._whole(op.outputs[0]))))

    # ------------------------------------------------------------------------------------------------------------ the executor
    def _root(self, i):
        a = self.tensors[i].alias
        return i if a is None else a

    def prepare(self, device=0):
        """once: one 256-byte aligned allocation per tensor, constants uploaded, filters tiled, every view wrapped"""
        self._device = int(device)
        hl.set_gpu_device(self._device)
        hip = hl.hip_runtime()
        self._mem = {}
        for i, t in enumerate(self.tensors):
            if t.alias is not None:
                continue
            n = max(int(np.prod(t.shape, dtype=np.int64)) * t.dtype.itemsize, 1)
            p = C.c_void_p()
            if hip.hipMalloc(C.byref(p), C.c_size_t(n + 64)) != 0 or p.value % 64:
                raise MemoryError(f"hannk_model: a device allocation of {n} bytes failed")
            self._mem[i] = (p, n)
            if t.data is not None:
                host = np.ascontiguousarray(t.data, t.dtype)
                _hip_memcpy(p, C.c_void_p(host.ctypes.data), host.nbytes, 1)
        self._bufs = []
        self._calls = [self._bind(s) for s in self.plan]
        for call in [self._bind(s) for s in self.setup]:
            call()
        _hip_device_synchronize()
        return self

    def _buffer(self, v):
        t = self.tensors[v.tensor]
        p, _ = self._mem[self._root(v.tensor)]
        b = hl.Buffer.wrap_device(p.value + v.offset * t.dtype.itemsize, t.dtype, list(v.extents), list(v.strides), list(v.mins))
        self._bufs.append(b)
        return b

    def _bind(self, step):
        args = [self._buffer(a) if isinstance(a, View) else int(a) for a in step.args]
        if step.name == "hannk_copy_from":
            return lambda: hannk.hannk_copy_from(args[0], args[1])
        if step.name == "hannk_gather":
            return lambda: hannk.hannk_gather_buffers(*args)
        fn = hl._fn[step.name]
        cargs = [a.ptr if isinstance(a, hl.Buffer) else a for a in args]
        return lambda: hl._check(fn(*cargs))

    def run(self, *inputs):
        """inputs in the file's order and shape (NHWC): torch tensors on the model's device or numpy arrays (uploaded before the first launch);
        returns device tensors.  Every step goes to torch's current stream; nothing between the first and the last launch waits for the device
        (a GATHER step reads its out-of-range flag back: the one exception)."""
        import torch
        if self._device is None:
            self.prepare()
        if len(inputs) != len(self._activation_inputs()):
            raise TypeError(f"the model takes {len(self._activation_inputs())} inputs, not {len(inputs)}")
        dev = torch.device("cuda", self._device)
        stream = torch.cuda.current_stream(dev).cuda_stream
        for i, x in zip(self._activation_inputs(), inputs):
            t = self.tensors[i]
            p, n = self._mem[self._root(i)]
            if isinstance(x, torch.Tensor):
                if x.device != dev or tuple(x.shape) != tuple(reversed(t.shape)) or x.element_size() != t.dtype.itemsize:
                    raise ValueError(f"input tensor of shape {tuple(x.shape)} on {x.device}; the model wants {tuple(reversed(t.shape))} on {dev}")
                x = x.contiguous()
                _hip_memcpy_async(p, C.c_void_p(x.data_ptr()), n, 3, stream)
            else:
                host = np.ascontiguousarray(x, t.dtype)
                if host.shape != tuple(reversed(t.shape)):
                    raise ValueError(f"input array of shape {host.shape}; the model wants {tuple(reversed(t.shape))}")
                _hip_stream_synchronize(stream)
                _hip_memcpy(p, C.c_void_p(host.ctypes.data), n, 1)
        hl.set_gpu_device(self._device)
        hl.set_stream(stream if stream else 1)
        try:
            for call in self._calls:
                call()
        finally:
            hl.set_stream(None)
        outs = []
        for i in self.graph.outputs:
            t = self.tensors[i]
            o = torch.empty(tuple(reversed(t.shape)), dtype=getattr(torch, t.dtype.name), device=dev)
            if o.numel():
                _hip_memcpy_async(C.c_void_p(o.data_ptr()), self._mem[self._root(i)][0], o.numel() * o.element_size(), 3, stream)
            outs.append(o)
        return outs[0] if len(outs) == 1 else tuple(outs)

    __call__ = run

    def _activation_inputs(self):
        return [i for i in self.graph.inputs if self.graph.tensors[i].data is None]

    def run_host(self, *inputs):
        """run() without torch, for scripts: numpy arrays in, numpy arrays out (waits for the device)"""
        if self._device is None:
            self.prepare()
        for i, x in zip(self._activation_inputs(), inputs):
            host = np.ascontiguousarray(x, self.tensors[i].dtype)
            _hip_memcpy(self._mem[self._root(i)][0], C.c_void_p(host.ctypes.data), host.nbytes, 1)
        self.launch()
        _hip_device_synchronize()
        outs = []
        for i in self.graph.outputs:
            t = self.tensors[i]
            o = np.empty(tuple(reversed(t.shape)), t.dtype)
            if o.nbytes:
                _hip_memcpy(C.c_void_p(o.ctypes.data), self._mem[self._root(i)][0], o.nbytes, 2)
            outs.append(o)
        return outs

    def launch(self):
        """every step of the plan on the library's current stream, nothing else"""
        for call in self._calls:
            call()

    def __del__(self):
        try:
            for b in getattr(self, "_bufs", []):
                b.device_detach()
            hip = hl.hip_runtime()
            for p, _ in getattr(self, "_mem", {}).values():
                hip.hipFree(p)
        except Exception:
            pass


# the HIP calls of this module, one wrapper each: what the tests count around run()
def _hip_memcpy(dst, src, n, kind):
    if hl.hip_runtime().hipMemcpy(dst, src, C.c_size_t(n), int(kind)) != 0:
        raise RuntimeError("hannk_model: hipMemcpy failed")


def _hip_memcpy_async(dst, src, n, kind, stream):
    if hl.hip_runtime().hipMemcpyAsync(dst, src, C.c_size_t(n), int(kind), C.c_void_p(stream or 0)) != 0:
        raise RuntimeError("hannk_model: hipMemcpyAsync failed")


def _hip_stream_synchronize(stream):
    if hl.hip_runtime().hipStreamSynchronize(C.c_void_p(stream or 0)) != 0:
        raise RuntimeError("hannk_model: hipStreamSynchronize failed")


def _hip_device_synchronize():
    if hl.hip_runtime().hipDeviceSynchronize() != 0:
        raise RuntimeError("hannk_model: hipDeviceSynchronize failed")
