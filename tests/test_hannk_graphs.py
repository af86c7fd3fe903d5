"""halide_amd/hannk_model.py against a float64 reading of the graph (tests/hannk_graph_reference.py).

The evaluator of tests/hannk_model_checker.py walks the plan the lowering made, so a wrong padding offset, filter order, multiplier or
activation range is wrong on both sides of test_hannk_model.py.  Here every op faces the definition of the TFLite op: dequantise, compute in
float64, requantise.  Acceptance per element, conditions rather than tolerances:
  move ops and max pool                       exact
  every other linear op                       |got - unrounded| < 1: one of the two integers around the real result
  LOGISTIC, TANH, SOFTMAX, L2_NORMALIZATION   |got - rint(unrounded)| <= 1, the bound of test_hannk_program.py and test_hannk_nn.py
Multi-op graphs list every intermediate tensor as an output and are checked teacher-forced: each op against the float64 result of the inputs
the implementation itself produced, so no error compounds.  No case may pass vacuously: at most half of a checked arithmetic tensor (in the
reference's own output) sits on a clamp limit, and it holds more than 8 distinct values unless it has no more than 8 elements.

CPU: the evaluator over every fixture, the table of one-op graphs, the multi-op graphs and the identities.  `-s` shows the worst distance per
op kind.  GPU (-m gpu): HannkModel.run is the evaluator bit for bit on every returned tensor, and passes the same acceptance."""
from __future__ import annotations

import functools
import glob
import itertools
import os

import numpy as np
import pytest

import hannk_graph_reference as ref
from halide_amd import hannk_model as hm
from halide_amd import tflite_reader as tfl
from hannk_model_checker import Evaluator

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hannk")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "*", "*.tflite")))
gpu = pytest.mark.gpu
XQ = (0.02, 121)      # the activations' usual quantisation: real -2.42 .. 2.68
WORST = {}            # op kind -> the largest distance seen, by rule
SHARES = {}           # case -> the largest share of an arithmetic tensor on a clamp limit


def rel(path):
    return os.path.relpath(path, GOLDEN)


# ------------------------------------------------------------------------------------------------------------------ building graphs
class Build:
    """tensors and ops of one graph; shapes in the file's order (NHWC)"""

    def __init__(self):
        self.tensors, self.ops, self.ranges = [], [], {}

    def t(self, shape, q=XQ, dtype=np.uint8, data=None, values=None):
        """a tensor; `values` = (lo, hi) is the half-open range its test input is drawn from"""
        scale, zero = ((q[0],), (q[1],)) if q is not None and np.dtype(dtype) == np.uint8 else ((), ())
        if data is not None:
            data = np.ascontiguousarray(data, dtype).reshape(shape)
        self.tensors.append(tfl.Tensor(f"t{len(self.tensors)}", tuple(reversed(shape)), np.dtype(dtype), scale, zero, data))
        if values is not None:
            self.ranges[len(self.tensors) - 1] = values
        return len(self.tensors) - 1

    def shape(self, i):
        return self.tensors[i].tfl_shape

    def q(self, i):
        return self.tensors[i].scale[0], self.tensors[i].zero[0]

    def op(self, kind, inputs, outputs, **attrs):
        self.ops.append(tfl.Op(kind, list(inputs), list(outputs), attrs))
        return outputs[0]

    def graph(self, inputs, outputs=None):
        """every tensor an op writes is an output unless `outputs` says otherwise: intermediates come back"""
        if outputs is None:
            outputs = [i for op in self.ops for i in op.outputs]
        g = tfl.Graph(self.tensors, self.ops, list(inputs), list(outputs))
        g.ranges = self.ranges
        return g


def extent(size, taps, stride, dilation, padding):
    span = (taps - 1) * dilation + 1
    return -(-size // stride) if padding == "same" else (size - span) // stride + 1


# the output quantisation of a conv per fused activation, and the real mean and spread its accumulator is steered to: a few per cent
# of the results beyond each limit, so the limits are exercised and no case saturates
CONV_OUT = {None: ((0.05, 128), 0.0, 2.0), "relu": ((0.05, 30), 2.4, 2.0), "relu6": ((0.05, 20), 3.0, 1.5), "relu_n1_to_1": ((0.01, 128), 0.0, 0.4)}


def conv(b, x, co, fh, fw, stride=(1, 1), dilation=(1, 1), padding="valid", act=None, seed=0, kind="CONV_2D", mult=1, rms=0.02 * 74, out=None):
    """a CONV_2D, DEPTHWISE_CONV_2D (co = channels * mult) or FULLY_CONNECTED (fh = fw = 0) on tensor x with a seeded filter and bias; `rms` is
    the root mean square of x's real values, `out` = ((scale, zero), mean, spread) overrides CONV_OUT"""
    r = np.random.RandomState(1000 + seed)
    (qo, mean, spread) = out or CONV_OUT[act]
    si = b.q(x)[0]
    if kind == "FULLY_CONNECTED":
        ci = b.shape(x)[-1]
        k, fshape, oshape = ci, (co, ci), (int(np.prod(b.shape(x))) // ci, co)
    else:
        n, h, w, ci = b.shape(x)
        k = fh * fw * (ci if kind == "CONV_2D" else 1)
        fshape = (co, fh, fw, ci) if kind == "CONV_2D" else (1, fh, fw, co)
        oshape = (n, extent(h, fh, stride[1], dilation[1], padding), extent(w, fw, stride[0], dilation[0], padding), co)
    sf = spread / (np.sqrt(k) * rms * 74)
    f = b.t(fshape, (sf, 128), data=r.randint(0, 256, fshape))
    unit = si * sf
    bias = b.t((co,), None, np.int32, data=np.rint(mean / unit + r.uniform(-0.3, 0.3, co) * spread / unit))
    o = b.t(oshape, qo)
    if kind == "FULLY_CONNECTED":
        return b.op(kind, [x, f, bias], [o], activation=act, weights_format=0, keep_num_dims=False)
    extra = {"depth_multiplier": mult} if kind == "DEPTHWISE_CONV_2D" else {}
    return b.op(kind, [x, f, bias], [o], padding=padding, stride=stride, dilation=dilation, activation=act, **extra)


def pool(b, x, kind, filt, stride, padding, act=None, qo=None):
    n, h, w, c = b.shape(x)
    o = b.t((n, extent(h, filt[1], stride[1], 1, padding), extent(w, filt[0], stride[0], 1, padding), c), qo or b.q(x))
    return b.op(kind, [x], [o], padding=padding, stride=stride, filter=filt, activation=act)


def one(make):
    """a one-op (or few-op) graph from a function that fills a Build and returns its activation inputs"""
    b = Build()
    return b.graph(make(b))


def table():
    x4 = (1, 4, 5, 17)

    def c(shape, *a, q=XQ, **kw):
        def make(b):
            x = b.t(shape, q)
            conv(b, x, *a, **kw)
            return [x]
        return one(make)

    yield "conv dilation 2x2 same", c((1, 9, 11, 5), 17, 3, 3, dilation=(2, 2), padding="same", seed=1)
    yield "conv dilation 2x1 stride 2 same", c((1, 10, 13, 17), 5, 3, 3, stride=(2, 2), dilation=(2, 1), padding="same", seed=2)
    yield "conv stride 2x1 filter 2x2 same", c((1, 8, 7, 19), 33, 2, 2, stride=(2, 1), padding="same", seed=3)
    yield "conv stride 1x3 filter 3x5 valid", c((1, 13, 9, 5), 19, 3, 5, stride=(1, 3), seed=4)
    yield "conv 1x1 valid batch 2", c((2, 4, 5, 17), 33, 1, 1, seed=5)
    for act in (None, "relu", "relu6", "relu_n1_to_1"):
        yield f"conv 3x3 same {act}", c((1, 6, 7, 5), 17, 3, 3, padding="same", act=act, seed=6)
    dw = dict(kind="DEPTHWISE_CONV_2D")
    yield "depthwise multiplier 2 over 5 channels", c((1, 6, 7, 5), 10, 3, 3, padding="same", mult=2, seed=7, **dw)
    yield "depthwise multiplier 3 over 1 channel", c((1, 6, 7, 1), 3, 3, 3, padding="same", mult=3, seed=8, **dw)
    yield "depthwise dilation 2 valid", c((1, 9, 10, 17), 17, 3, 3, dilation=(2, 2), seed=9, **dw)
    yield "depthwise stride 2x1 filter 5x3 same relu6", c((1, 8, 9, 19), 19, 5, 3, stride=(2, 1), padding="same", act="relu6", seed=10, **dw)
    fc = dict(kind="FULLY_CONNECTED")
    yield "fully connected depth 10 batch 3", c((3, 10), 17, 0, 0, seed=11, **fc)
    yield "fully connected depth 16 batch 1", c((1, 16), 19, 0, 0, seed=12, **fc)
    yield "fully connected relu", c((2, 12), 17, 0, 0, act="relu", seed=13, **fc)

    def p(shape, *a, q=XQ, **kw):
        def make(b):
            x = b.t(shape, q)
            pool(b, x, *a, **kw)
            return [x]
        return one(make)

    for kind in ("AVERAGE_POOL_2D", "MAX_POOL_2D"):
        name = kind[:3].lower() + " pool "
        yield name + "same 3x3 stride 2", p((1, 8, 9, 17), kind, (3, 3), (2, 2), "same")
        yield name + "same 2x3 stride 1", p((1, 5, 6, 19), kind, (3, 2), (1, 1), "same")
        yield name + "valid 2x2 stride 2x1", p((2, 6, 7, 5), kind, (2, 2), (2, 1), "valid")
    yield "avg pool same 3x3 stride 2 relu6", p((1, 7, 9, 17), "AVERAGE_POOL_2D", (3, 3), (2, 2), "same", act="relu6", q=(0.04, 10))
    yield "max pool same 3x3 stride 2 relu", p((1, 7, 9, 17), "MAX_POOL_2D", (3, 3), (2, 2), "same", act="relu", q=(0.04, 40))

    def mean(axes, keep):
        def make(b):
            x = b.t((2, 4, 5, 17))
            shape = [1 if 3 - d in axes else e for d, e in enumerate(b.shape(x))]
            if not keep:
                shape = [e for d, e in enumerate(b.shape(x)) if 3 - d not in axes]
            b.op("MEAN", [x], [b.t(tuple(shape))], axes=sorted(axes), keep_dims=keep)
            return [x]
        return one(make)

    for what, axes in (("channel", [0]), ("width", [1]), ("height width batch", [1, 2, 3])):
        for keep in (True, False):
            yield f"mean over {what} keep_dims {keep}", mean(axes, keep)

    def binary(kind, q1, second, q2, qo, act=None, values1=None, values2=None, data=None):
        def make(b):
            x = b.t(x4, q1, values=values1)
            y = b.t(second, q2, data=data, values=values2)
            b.op(kind, [x, y], [b.t(x4, qo)], activation=act)
            return [x] if data is not None else [x, y]
        return one(make)

    per_channel = np.random.RandomState(5).randint(0, 256, 17)
    yield "add same shape ratio 1", binary("ADD", XQ, x4, (0.021, 133), (0.024, 125))
    yield "add per channel ratio 1/25 relu", binary("ADD", (0.025, 90), (17,), (0.001, 100), (0.025, 100), "relu", data=per_channel)
    yield "add scalar relu_n1_to_1", binary("ADD", (0.01, 121), (1,), (0.01, 100), (0.012, 128), "relu_n1_to_1", data=[110])
    yield "sub same shape ratio 1/25 relu6", binary("SUB", (0.035, 60), x4, (0.0016, 133), (0.04, 20), "relu6")
    yield "sub per channel ratio 1", binary("SUB", XQ, (1, 1, 1, 17), (0.021, 133), (0.024, 125), data=per_channel)
    yield "sub scalar", binary("SUB", XQ, (1,), (0.03, 100), (0.022, 140), data=[131])
    yield "mul same shape ratio 1/25", binary("MUL", XQ, x4, (0.03, 133), (0.02 * 0.03 * 25, 128), values1=(71, 172), values2=(83, 184))
    yield "mul per channel ratio 1 relu", binary("MUL", XQ, (17,), (0.03, 133), (0.02 * 0.03 * 1.1, 40), "relu", values1=(115, 136),
                                                 data=np.random.RandomState(6).randint(128, 150, 17))
    yield "mul scalar ratio 1/25", binary("MUL", XQ, (1,), (0.03, 133), (0.02 * 0.03 * 25, 128), data=[142])

    def unary(kind, shape, qi, qo, oshape=None, **attrs):
        def make(b):
            x = b.t(shape, qi)
            b.op(kind, [x], [b.t(oshape or shape, qo)], **attrs)
            return [x]
        return one(make)

    yield "relu", unary("RELU", x4, (0.05, 100), (0.04, 10))
    yield "relu6", unary("RELU6", x4, (0.04, 60), (0.04, 10))
    yield "relu_n1_to_1", unary("RELU_N1_TO_1", x4, (0.01, 121), (0.0085, 128))
    yield "logistic", unary("LOGISTIC", x4, (0.03, 121), (1 / 256, 0))
    yield "tanh", unary("TANH", x4, (0.012, 121), (1 / 128, 128))
    yield "softmax beta 1", unary("SOFTMAX", (3, 17), XQ, (1 / 256, 0), beta=1.0)
    yield "softmax beta 0.5", unary("SOFTMAX", (1, 2, 3, 19), (0.03, 121), (1 / 256, 0), beta=0.5)
    yield "l2 normalization", unary("L2_NORMALIZATION", (2, 3, 17), XQ, (1 / 128, 128))

    three = ((0.02, 120), (0.03, 131), (0.025, 127))

    def concat(axis, sizes, qs, qo):
        def make(b):
            shapes = [tuple(n if 3 - d == axis else e for d, e in enumerate((1, 4, 5, 17))) for n in sizes]
            ins = [b.t(s, q) for s, q in zip(shapes, qs)]
            total = tuple(sum(sizes) if 3 - d == axis else e for d, e in enumerate((1, 4, 5, 17)))
            b.op("CONCATENATION", ins, [b.t(total, qo)], axis=axis, activation=None)
            return ins
        return one(make)

    def split(kind, axis, sizes, qs, qi=XQ):
        def make(b):
            total = tuple(sum(sizes) if 3 - d == axis else e for d, e in enumerate((1, 4, 5, 17)))
            x = b.t(total, qi)
            outs = [b.t(tuple(n if 3 - d == axis else e for d, e in enumerate((1, 4, 5, 17))), q) for n, q in zip(sizes, qs)]
            attrs = {"size_splits": list(sizes)} if kind == "SPLIT_V" else {}
            b.op(kind, [x], outs, axis=axis, num_splits=len(sizes), **attrs)
            return [x]
        return one(make)

    for what, axis in (("channel", 0), ("width", 1)):
        yield f"concatenation along {what} equal", concat(axis, (5, 12), (XQ, XQ), XQ)
        yield f"concatenation along {what} requantised", concat(axis, (5, 12, 7), three, (0.032, 125))
        yield f"split_v along {what} equal", split("SPLIT_V", axis, (5, 12), (XQ, XQ))
        yield f"split_v along {what} requantised", split("SPLIT_V", axis, (5, 12, 7), three, (0.018, 124))
    yield "split along channel equal", split("SPLIT", 0, (5, 5, 5), (XQ,) * 3)
    yield "split along width requantised", split("SPLIT", 1, (6, 6), three[:2], (0.018, 124))

    def pad(shape, pads):
        def make(b):
            x = b.t(shape)
            b.op("PAD", [x], [b.t(tuple(e + lo + hi for e, (lo, hi) in zip(shape, pads[::-1])))], padding=list(pads))
            return [x]
        return one(make)

    yield "pad rank 4", pad(x4, [(1, 2), (2, 1), (1, 2), (0, 0)])      # innermost dimension first
    yield "pad rank 2", pad((5, 17), [(1, 2), (2, 1)])

    def transpose(shape, perm):
        def make(b):
            x = b.t(shape)
            b.op("TRANSPOSE", [x], [b.t(tuple(shape[p] for p in perm))], perm=list(perm))
            return [x]
        return one(make)

    for perm in itertools.permutations(range(3)):
        yield f"transpose {perm}", transpose((5, 7, 17), perm)
    for perm in ((0, 2, 1, 3), (3, 0, 2, 1)):
        yield f"transpose {perm}", transpose((2, 4, 5, 17), perm)

    def gather(axis):
        def make(b):
            x = b.t((4, 5, 17))
            idx = b.t((4,), None, np.int32, data=[3, 0, 3, 2])
            shape = list(b.shape(x))
            shape[2 - axis] = 4
            b.op("GATHER", [x, idx], [b.t(tuple(shape))], axis=axis, batch_dims=0)
            return [x]
        return one(make)

    for axis in range(3):
        yield f"gather axis {axis}", gather(axis)
    yield "space_to_depth block 3", unary("SPACE_TO_DEPTH", (1, 6, 9, 5), XQ, XQ, (1, 2, 3, 45), block_size=3)
    yield "depth_to_space block 3", unary("DEPTH_TO_SPACE", (1, 2, 3, 45), XQ, XQ, (1, 6, 9, 5), block_size=3)


RELU6_RMS = 3.35      # of a tensor steered to mean 3, spread 1.5 and clamped to [0, 6]


def multi():
    def residual(b):
        x = b.t((1, 6, 7, 17))
        e = conv(b, x, 33, 1, 1, act="relu6", seed=20)
        d = conv(b, e, 33, 3, 3, padding="same", act="relu6", seed=21, kind="DEPTHWISE_CONV_2D", rms=RELU6_RMS)
        p = conv(b, d, 17, 1, 1, seed=22, rms=RELU6_RMS, out=((0.03, 125), 0.0, 1.2))
        b.op("ADD", [x, p], [b.t(b.shape(x), (0.035, 122))], activation=None)      # the block's input is read twice
        return [x]

    def inception(b):
        x = b.t((1, 6, 7, 17))
        a = conv(b, x, 5, 1, 1, seed=23)
        c = conv(b, x, 12, 3, 3, padding="same", act="relu", seed=24)
        m = pool(b, x, "MAX_POOL_2D", (3, 3), (1, 1), "same")
        b.op("CONCATENATION", [a, c, m], [b.t((1, 6, 7, 34), (0.055, 90))], axis=0, activation=None)
        return [x]

    def split_unary_concat(b):
        x = b.t((1, 4, 5, 24))
        parts = [b.t((1, 4, 5, n)) for n in (5, 12, 7)]
        b.op("SPLIT_V", [x], parts, axis=0, num_splits=3, size_splits=[5, 12, 7])
        outs = [b.op("RELU6", [parts[0]], [b.t((1, 4, 5, 5), (0.03, 10))]), b.op("LOGISTIC", [parts[1]], [b.t((1, 4, 5, 12), (1 / 256, 0))]),
                b.op("TANH", [parts[2]], [b.t((1, 4, 5, 7), (1 / 128, 128))])]
        b.op("CONCATENATION", outs, [b.t((1, 4, 5, 24), (0.012, 100))], axis=0, activation=None)
        return [x]

    def classifier_tail(b):
        x = b.t((2, 4, 5, 17))
        a = pool(b, x, "AVERAGE_POOL_2D", (5, 4), (1, 1), "valid")
        c = conv(b, a, 19, 1, 1, seed=25, rms=0.36, out=((0.02, 128), 0.0, 1.0))
        r1 = b.op("RESHAPE", [c], [b.t((2, 19), (0.02, 128))], new_shape=[2, 19])
        r2 = b.op("RESHAPE", [r1], [b.t((1, 2, 19), (0.02, 128))], new_shape=[1, 2, 19])      # both alias the conv's allocation
        b.op("SOFTMAX", [r2], [b.t((1, 2, 19), (1 / 256, 0))], beta=1.0)
        return [x]

    def two_paddings(b):
        x = b.t((1, 6, 7, 17))
        conv(b, x, 5, 3, 3, padding="same", seed=26)
        conv(b, x, 12, 5, 5, padding="same", act="relu", seed=27)
        return [x]

    for f in (residual, inception, split_unary_concat, classifier_tail, two_paddings):
        yield f.__name__.replace("_", " "), one(f)


TABLE, MULTI = dict(table()), dict(multi())
CASES = {**TABLE, **MULTI}


# ------------------------------------------------------------------------------------------------------------------ running and judging
def inputs_for(graph, seed):
    """seeded uniform inputs: the full u8 range, or the range the case gives the tensor; f32 inputs in [-1, 1)"""
    r = np.random.RandomState(seed)
    out = []
    for i in graph.inputs:
        t = graph.tensors[i]
        if t.data is None:
            lo, hi = getattr(graph, "ranges", {}).get(i, (0, 256))
            out.append(r.randint(lo, hi, t.tfl_shape).astype(np.uint8) if t.dtype == np.uint8 else (r.random_sample(t.tfl_shape) * 2 - 1).astype(t.dtype))
    return out


def on_evaluator(graph, xs):
    return Evaluator(hm.HannkModel(graph)).run(*xs)


def on_device(model, xs):
    import torch
    got = model.run(*[torch.from_numpy(x.copy()).cuda() for x in xs])      # the shared inputs are read-only
    got = got if isinstance(got, tuple) else (got,)
    assert all(g.is_cuda for g in got)
    return [g.cpu().numpy() for g in got]


def same(got, want, what):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, what
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), (what, int(np.count_nonzero(g != w)), g.size)


def values_of(graph, xs, outs):
    acts = [i for i in graph.inputs if graph.tensors[i].data is None]
    assert len(acts) == len(xs) and len(graph.outputs) == len(outs)
    return {**dict(zip(acts, xs)), **dict(zip(graph.outputs, outs))}


def accept(graph, xs, outs, what, vacuity=True, worst=None):
    """every op of the graph against the float64 reading of the inputs the implementation gave it (teacher-forced); returns the largest share of
    an arithmetic tensor on a clamp limit"""
    values = values_of(graph, xs, outs)
    share = 0.0
    for n, op in enumerate(graph.ops):
        for i, r in zip(op.outputs, ref.run_op(graph, op, values)):
            assert i in values, f"{what}: tensor {i} of {op.kind} is not an output of the graph"
            got, where = values[i], f"{what}, op {n} {op.kind}, tensor {i}"
            assert got.shape == r.rounded.shape and got.dtype == r.rounded.dtype, where
            exact = np.broadcast_to(r.exact, got.shape)
            bad = exact & (got != r.rounded)
            assert not bad.any(), (where, "moved elements differ", int(bad.sum()), np.argwhere(bad)[:4].tolist())
            if op.kind in ref.MOVES or got.dtype != np.uint8:
                continue
            if not exact.all():
                rest = ~exact
                if r.rule == "linear":
                    d = np.abs(got.astype(np.float64) - r.unrounded)
                    ok = d < 1
                else:
                    d = np.abs(got.astype(np.float64) - r.rounded.astype(np.float64))
                    ok = d <= 1
                if worst is not None:
                    key = (op.kind, "to unrounded" if r.rule == "linear" else "to rint")
                    worst[key] = max(worst.get(key, 0.0), float(d[rest].max()))
                bad = rest & ~ok
                assert not bad.any(), (where, r.rule, float(d[rest].max()), int(bad.sum()), np.argwhere(bad)[:4].tolist())
            elif op.kind != "MAX_POOL_2D":
                continue      # a CONCATENATION or SPLIT that only copies
            limits = (r.rounded == np.rint(r.lo)) | (r.rounded == np.rint(r.hi))
            share = max(share, float(limits.mean()))
            if vacuity:
                assert limits.mean() <= 0.5, (where, "share of the reference's output on a clamp limit", float(limits.mean()))
                assert r.rounded.size <= 8 or len(np.unique(r.rounded)) > 8, (where, "distinct values", len(np.unique(r.rounded)))
    return share


@functools.lru_cache(maxsize=None)
def evaluated(name, seed=11):
    """the case's inputs and what the evaluator makes of them: computed once, shared by the CPU and the GPU tests, never written to"""
    g = CASES[name]
    xs = inputs_for(g, seed)
    outs = on_evaluator(g, xs)
    for a in xs + outs:
        a.setflags(write=False)
    return xs, outs


# ------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("path", FILES, ids=rel)
def test_evaluator_on_every_fixture_is_the_float64_graph(path):
    """the fixtures' inputs are what they are (full-range uniform, as in test_hannk_model.py), so the share on a clamp limit is printed, not
    asserted: the table below is what has to keep its cases from saturating"""
    g = tfl.read(path)
    xs = inputs_for(g, FILES.index(path))
    m = hm.HannkModel(g)
    outs = Evaluator(m).run(*xs)
    produced = [i for op in g.ops for i in op.outputs]
    assert sorted(produced) == sorted(g.outputs), rel(path)
    share = accept(g, xs, outs, rel(path), vacuity=False, worst=WORST)
    print(f"{rel(path)}: share on a clamp limit {share:.3f}")


@pytest.mark.parametrize("name", sorted(TABLE))
def test_evaluator_on_the_table_is_the_float64_graph(name):
    xs, outs = evaluated(name)
    SHARES[name] = accept(CASES[name], xs, outs, name, worst=WORST)


@pytest.mark.parametrize("name", sorted(MULTI))
def test_evaluator_on_multi_op_graphs_is_the_float64_graph(name):
    g = CASES[name]
    xs, outs = evaluated(name)
    assert sorted(g.outputs) == sorted(i for op in g.ops for i in op.outputs)      # every intermediate comes back and is judged
    SHARES[name] = accept(g, xs, outs, name, worst=WORST)


def test_the_lowering_shapes_the_multi_op_graphs_as_said():
    m = hm.HannkModel(CASES["two paddings"])
    fills = [s.args[1] for s in m.plan if s.name == "fill_uint8"]
    assert len(fills) == 2 and fills[0].tensor != fills[1].tensor      # one tensor, two padded copies of it
    assert sorted(f.extents for f in fills) == [(20, 9, 8, 1), (20, 11, 10, 1)]
    convs = [s for s in m.plan if s.name == "conv_u8_u8_u8"]
    assert [s.args[0].tensor for s in convs] == [f.tensor for f in fills]
    m = hm.HannkModel(CASES["classifier tail"])
    g = m.graph
    r1, r2 = (op.outputs[0] for op in g.ops if op.kind == "RESHAPE")
    root = g.ops[1].outputs[0]
    assert m.tensors[r1].alias == root and m.tensors[r2].alias == root and r1 in g.outputs and r2 in g.outputs
    m = hm.HannkModel(CASES["residual"])
    assert sum(1 for s in m.plan for a in s.args if isinstance(a, hm.View) and a.tensor == m.graph.inputs[0]) >= 2      # consumed twice
    m = hm.HannkModel(TABLE["depthwise multiplier 2 over 5 channels"])
    assert m.plan[0].name == "upsample_channels_uint8" and m.plan[-1].name == "depthwise_conv_uint8"
    m = hm.HannkModel(TABLE["depthwise multiplier 3 over 1 channel"])
    assert m.plan[-1].name == "depthwise_conv_broadcast_uint8"


def test_constants_the_lowering_adds_have_the_shape_of_their_slot():
    """a Slot's data is "a constant in numpy order": its shape is the slot's extents reversed.  Both executors upload it flat, so a relaid filter
    declared under other axes (a depthwise filter reshaped as (fw, fh, co)) computes the same and would pass everything else"""
    for name, g in [(n, g) for n, g in CASES.items()] + [(rel(p), tfl.read(p)) for p in FILES]:
        for i, t in enumerate(hm.HannkModel(g).tensors):
            assert t.data is None or tuple(t.data.shape) == tuple(reversed(t.shape)), (name, i, t.data.shape, t.shape)


# identities that hold bit for bit, on any implementation: run(graph, inputs) -> the graph's outputs
def pad_then_valid_is_same(run):
    def make(padded):
        def f(b):
            x = b.t((1, 6, 7, 17))
            y = b.op("PAD", [x], [b.t((1, 8, 9, 17))], padding=[(0, 0), (1, 1), (1, 1), (0, 0)]) if padded else x
            conv(b, y, 12, 3, 3, padding="valid" if padded else "same", act="relu6", seed=30)
            return [x]
        return one(f)
    xs = inputs_for(make(True), 3)
    same([run(make(True), xs)[-1]], [run(make(False), xs)[-1]], "PAD by (1, 1) then a VALID 3 x 3 conv against the SAME conv")


def depth_to_space_undoes_space_to_depth(run):
    def f(b):
        x = b.t((2, 6, 9, 5))
        y = b.op("SPACE_TO_DEPTH", [x], [b.t((2, 2, 3, 45))], block_size=3)
        b.op("DEPTH_TO_SPACE", [y], [b.t((2, 6, 9, 5))], block_size=3)
        return [x]
    g = one(f)
    xs = inputs_for(g, 4)
    same([run(g, xs)[-1]], xs, "DEPTH_TO_SPACE of SPACE_TO_DEPTH")


def concat_undoes_split(run):
    for axis in (0, 1):
        def f(b):
            whole = [(1, 4, 5, 24), (1, 4, 24, 5)][axis]
            x = b.t(whole)
            parts = [b.t(tuple(n if e == 24 else e for e in whole)) for n in (5, 12, 7)]
            b.op("SPLIT_V", [x], parts, axis=axis, num_splits=3, size_splits=[5, 12, 7])
            b.op("CONCATENATION", parts, [b.t(whole)], axis=axis, activation=None)
            return [x]
        g = one(f)
        xs = inputs_for(g, 5)
        same([run(g, xs)[-1]], xs, f"CONCATENATION of an equal-quantisation SPLIT_V along {axis}")


def a_reshape_pair_changes_nothing(run):
    def make(reshaped):
        def f(b):
            x = b.t((1, 6, 7, 17))
            y = conv(b, x, 12, 1, 1, act="relu6", seed=31)
            if reshaped:
                y = b.op("RESHAPE", [y], [b.t((42, 12), b.q(y))], new_shape=[42, 12])
                y = b.op("RESHAPE", [y], [b.t((1, 6, 7, 12), b.q(y))], new_shape=[1, 6, 7, 12])
            conv(b, y, 5, 3, 3, padding="same", seed=32, rms=RELU6_RMS)
            return [x]
        return one(f)
    xs = inputs_for(make(True), 6)
    with_pair, without = run(make(True), xs), run(make(False), xs)
    same([with_pair[0], with_pair[-1]], [without[0], without[-1]], "a RESHAPE pair between two convs")
    same(with_pair[1:3], [without[0].reshape(42, 12), without[0]], "the reshaped tensors themselves")


IDENTITIES = [pad_then_valid_is_same, depth_to_space_undoes_space_to_depth, concat_undoes_split, a_reshape_pair_changes_nothing]


@pytest.mark.parametrize("identity", IDENTITIES, ids=lambda f: f.__name__)
def test_identities_on_the_evaluator(identity):
    identity(on_evaluator)


@pytest.mark.parametrize("identity", IDENTITIES, ids=lambda f: f.__name__)
def test_identities_on_the_reference_itself(identity):
    """the float64 graph run freely (each op on the rounded results before it) keeps them too: a check of the reference, not of the package"""
    def run(graph, xs):
        values = ref.run_graph(graph, xs)
        return [values[i] for i in graph.outputs]
    identity(run)


def test_worst_distances_are_printed():
    """last of the CPU tests: what the ones above measured (`-s` shows it; DESIGN.md 5.15 records a run)"""
    for (kind, rule), d in sorted(WORST.items()):
        print(f"worst distance {rule:13s} {kind:20s} {d:.3f}")
    if SHARES:
        name = max(SHARES, key=SHARES.get)
        print(f"largest share of a table case on a clamp limit: {SHARES[name]:.3f} ({name}); cases above 0.25: "
              f"{sorted(n for n, s in SHARES.items() if s > 0.25)}")
    assert all(d < 1 if rule == "to unrounded" else d <= 1 for (_, rule), d in WORST.items())


# ------------------------------------------------------------------------------------------------------------------ GPU
@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_hip_cases_are_the_evaluator_and_the_float64_graph(hl, name):
    g = CASES[name]
    xs, want = evaluated(name)
    got = on_device(hm.HannkModel(g), xs)
    same(got, want, name)
    accept(g, xs, got, name + " on the device")


@gpu
@pytest.mark.parametrize("identity", IDENTITIES, ids=lambda f: f.__name__)
def test_hip_identities(hl, identity):
    identity(lambda graph, xs: on_device(hm.HannkModel(graph), xs))


@gpu
@pytest.mark.parametrize("name", sorted(MULTI))
def test_hip_multi_op_graphs_rerun_fresh_and_on_a_side_stream(hl, name):
    """nothing stale in the padded tensors or the aliased allocation: two runs with different inputs on one prepared model, one on a fresh model
    and one under a side stream, each against the evaluator"""
    import torch
    g = CASES[name]
    (xs1, want1), (xs2, want2) = evaluated(name), evaluated(name, 12)
    m = hm.HannkModel(g).prepare()
    same(on_device(m, xs1), want1, name + ", first run")
    same(on_device(m, xs2), want2, name + ", second run, other inputs")
    same(on_device(hm.HannkModel(g), xs2), want2, name + ", a fresh model")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = on_device(m, xs1)
    side.synchronize()
    same(got, want1, name + ", on a side stream")

