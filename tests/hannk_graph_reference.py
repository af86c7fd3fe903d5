"""A float64 reading of a tflite_reader.Graph, written from the definition of the TFLite ops: dequantise, compute the real-valued op,
requantise.  numpy only.  It takes the Graph / Tensor / Op objects it is handed and nothing else of the package: no plan, no helper of
halide_amd.hannk.  Padding, output extents and activation limits are stated here in its own words, which is the point: the plan evaluator
(tests/hannk_model_checker.py) shares the lowering's numbers with the device, this file shares nothing with either.

Arrays are in the file's order (NHWC), `Tensor.shape` is that reversed; an axis `a` in an Op's attrs counts from the innermost dimension, so it
is numpy axis `rank - 1 - a`.  stride, dilation and a pool's filter are (along the width, along the height).

run_op(graph, op, values) -> one Result per output of `op`, computed from `values[i]` (constants come from the graph).  A Result holds
  unrounded   real / s_out + zero_out in float64, clipped to [0, 255] and to the fused activation's limits (the array itself for a move)
  rounded     rint(unrounded) as the tensor's type
  rule        "exact": an implementation must return `rounded`; "linear": one of the two integers around `unrounded`, |got - unrounded| < 1;
              "nonlinear": |got - rounded| <= 1
  exact       a boolean array (broadcast against the output): the elements that only moved, where `rounded` is due whatever `rule` says
  lo, hi      the clamp limits in quanta that `unrounded` was clipped to
run_graph(graph, inputs) -> {tensor id: array}: every op in turn on the rounded results of the ones before it."""
import numpy as np

F = np.float64
MOVES = ("RESHAPE", "TRANSPOSE", "SPACE_TO_DEPTH", "DEPTH_TO_SPACE", "GATHER", "PAD")
NONLINEAR = ("LOGISTIC", "TANH", "SOFTMAX", "L2_NORMALIZATION")
REAL_LIMITS = {None: (-np.inf, np.inf), "none": (-np.inf, np.inf), "relu": (0.0, np.inf), "relu6": (0.0, 6.0), "relu_n1_to_1": (-1.0, 1.0)}


class Result:
    def __init__(self, unrounded, rounded, rule, exact=None, lo=0.0, hi=255.0):
        self.unrounded, self.rounded, self.rule, self.lo, self.hi = unrounded, rounded, rule, lo, hi
        self.exact = np.bool_(rule == "exact") if exact is None else exact


def scale_of(t):
    assert len(t.scale) == 1 and len(t.zero) == 1, "one scale and one zero point per tensor"
    return F(np.float32(t.scale[0]))


def zero_of(t):
    return F(int(t.zero[0]))


def same_quantisation(a, b):
    return a.dtype == b.dtype and tuple(np.float32(a.scale)) == tuple(np.float32(b.scale)) and tuple(a.zero) == tuple(b.zero)


def real(t, q):
    return (np.asarray(q).astype(F) - zero_of(t)) * scale_of(t)


def quantise(t, r, activation=None, rule="linear"):
    lo_r, hi_r = REAL_LIMITS[activation]
    s, z = scale_of(t), zero_of(t)
    lo, hi = max(0.0, z + lo_r / s), min(255.0, z + hi_r / s)
    u = np.clip(np.asarray(r, F) / s + z, lo, hi)
    return Result(u, np.rint(u).astype(t.dtype), rule, None, lo, hi)


def moved(a):
    return Result(a, a, "exact")


# ---------------------------------------------------------------------------------------------------------------- windows
def window(size, taps, stride, dilation, padding, outputs):
    """one axis of a sliding window: (pixels in front of the image, pixels behind it).  TensorFlow's rule: VALID keeps the windows that
    lie inside the image; SAME makes ceil(size / stride) windows and shares the pixels they lack between the two ends, the odd one behind."""
    span = dilation * (taps - 1) + 1
    if padding == "same":
        count = (size + stride - 1) // stride
        lack = max((count - 1) * stride + span - size, 0)
        front = lack // 2
    else:
        assert padding == "valid", padding
        count = (size - span) // stride + 1
        front = 0
    assert count == outputs, f"the graph says {outputs} windows along an axis of {size}, the definition {count}"
    behind = max((count - 1) * stride + span - size - front, 0)
    return front, behind


def taps_of(x, fh, fw, attrs, oh, ow, fill, dilation=(1, 1)):
    """yields (ky, kx, the (B, OH, OW, C) slice of x that tap multiplies); outside the image x is `fill`"""
    _, h, w, _ = x.shape
    (sw, sh), (dw, dh) = attrs["stride"], dilation
    top, bottom = window(h, fh, sh, dh, attrs["padding"], oh)
    left, right = window(w, fw, sw, dw, attrs["padding"], ow)
    xp = np.pad(x, ((0, 0), (top, bottom), (left, right), (0, 0)), constant_values=fill)
    for ky in range(fh):
        for kx in range(fw):
            y0, x0 = ky * dh, kx * dw
            yield ky, kx, xp[:, y0:y0 + (oh - 1) * sh + 1:sh, x0:x0 + (ow - 1) * sw + 1:sw, :]


# ---------------------------------------------------------------------------------------------------------------- ops
def run_op(graph, op, values):
    T = graph.tensors

    def val(i):
        t = T[i]
        a = t.data if t.data is not None else values[i]
        a = np.asarray(a)
        assert a.shape == t.tfl_shape and a.dtype == t.dtype, (op.kind, i, a.shape, t.tfl_shape)
        return a

    k, a = op.kind, op.attrs
    ins = [i for i in op.inputs if i >= 0]
    x_t, o_t = T[ins[0]], T[op.outputs[0]]
    x = val(ins[0])
    oshape = o_t.tfl_shape

    if k in ("CONV_2D", "DEPTHWISE_CONV_2D", "FULLY_CONNECTED"):
        f_t = T[ins[1]]
        w = real(f_t, val(ins[1]))
        bias = val(ins[2]).astype(F) * scale_of(x_t) * scale_of(f_t) if len(ins) > 2 else 0.0
        xr = real(x_t, x)
        if k == "FULLY_CONNECTED":
            co, ci = w.shape
            acc = xr.reshape(-1, ci) @ w.T
        else:
            assert len(oshape) == 4 and xr.ndim == 4
            _, oh, ow, co = oshape
            acc = np.zeros(oshape, F)
            if k == "CONV_2D":
                assert w.shape[0] == co and w.shape[3] == x.shape[3]
                for ky, kx, tap in taps_of(xr, w.shape[1], w.shape[2], a, oh, ow, 0.0, a["dilation"]):
                    acc += tap @ w[:, ky, kx, :].T
            else:       # output channel c * multiplier + m reads input channel c
                mult = int(a["depth_multiplier"])
                assert w.shape[0] == 1 and w.shape[3] == co == x.shape[3] * mult
                xr = np.repeat(xr, mult, axis=3)
                for ky, kx, tap in taps_of(xr, w.shape[1], w.shape[2], a, oh, ow, 0.0, a["dilation"]):
                    acc += tap * w[0, ky, kx, :]
        return [quantise(o_t, (acc + bias).reshape(oshape), a["activation"])]

    if k in ("AVERAGE_POOL_2D", "MAX_POOL_2D"):
        fw, fh = a["filter"]
        _, oh, ow, c = oshape
        assert c == x.shape[3]
        xr = real(x_t, x)
        if k == "MAX_POOL_2D":
            best = np.full(oshape, -np.inf)
            for _, _, tap in taps_of(xr, fh, fw, a, oh, ow, -np.inf):
                best = np.maximum(best, tap)
            assert np.isfinite(best).all(), "a pool window with no tap inside the image"
            only_picks = same_quantisation(x_t, o_t)
            return [quantise(o_t, best, a["activation"], "exact" if only_picks else "linear")]
        total, count = np.zeros(oshape, F), np.zeros(oshape, F)
        for (_, _, tap), (_, _, inside) in zip(taps_of(xr, fh, fw, a, oh, ow, 0.0), taps_of(np.ones_like(xr), fh, fw, a, oh, ow, 0.0)):
            total += tap
            count += inside
        assert (count > 0).all(), "a pool window with no tap inside the image"
        return [quantise(o_t, total / count, a["activation"])]

    if k == "MEAN":
        axes = tuple(x.ndim - 1 - d for d in a["axes"])
        return [quantise(o_t, real(x_t, x).mean(axis=axes, keepdims=True).reshape(oshape))]

    if k in ("ADD", "SUB", "MUL"):
        p, q = real(x_t, x), real(T[ins[1]], val(ins[1]))
        r = p + q if k == "ADD" else p - q if k == "SUB" else p * q
        assert r.shape == oshape
        return [quantise(o_t, r, a.get("activation"))]

    if k in ("RELU", "RELU6", "RELU_N1_TO_1"):
        return [quantise(o_t, real(x_t, x), k.lower())]

    if k in NONLINEAR:
        r = real(x_t, x)
        if k == "LOGISTIC":
            r = 1.0 / (1.0 + np.exp(-r))
        elif k == "TANH":
            r = np.tanh(r)
        elif k == "SOFTMAX":
            e = np.exp(F(a["beta"]) * (r - r.max(axis=-1, keepdims=True)))
            r = e / e.sum(axis=-1, keepdims=True)
        else:
            norm = np.sqrt((r * r).sum(axis=-1, keepdims=True))
            r = r / np.where(norm > 0, norm, 1.0)
        return [quantise(o_t, r, None, "nonlinear")]

    if k == "CONCATENATION":
        axis = len(oshape) - 1 - a["axis"]
        assert a.get("activation") in (None, "none")
        pieces, exact = [], []
        for i in ins:
            same = not T[i].quantized or same_quantisation(T[i], o_t)
            pieces.append(moved(val(i)) if same else quantise(o_t, real(T[i], val(i))))
            exact.append(np.full(T[i].tfl_shape, same))
        u = np.concatenate([p.unrounded for p in pieces], axis)
        assert u.shape == oshape
        return [Result(u, np.concatenate([p.rounded for p in pieces], axis).astype(o_t.dtype), "linear", np.concatenate(exact, axis))]

    if k in ("SPLIT", "SPLIT_V"):
        axis = x.ndim - 1 - a["axis"]
        sizes = a["size_splits"] if k == "SPLIT_V" else [x.shape[axis] // len(op.outputs)] * len(op.outputs)
        assert sum(sizes) == x.shape[axis] and len(sizes) == len(op.outputs)
        out, at = [], 0
        for i, n in zip(op.outputs, sizes):
            part = np.take(x, np.arange(at, at + n), axis)
            assert part.shape == T[i].tfl_shape
            same = not T[i].quantized or same_quantisation(x_t, T[i])
            out.append(moved(part) if same else quantise(T[i], real(x_t, part)))
            at += n
        return out

    assert k in MOVES, f"no definition of {k} here"
    if k == "RESHAPE":
        r = x.reshape(oshape)
    elif k == "TRANSPOSE":
        r = np.transpose(x, a["perm"])
    elif k == "GATHER":
        r = np.take(x, val(ins[1]), x.ndim - 1 - a["axis"])
    elif k == "PAD":       # the border is real 0, which the output's zero point stands for; the image keeps its quantisation
        assert same_quantisation(x_t, o_t)
        pads = list(a["padding"]) + [(0, 0)] * (x.ndim - len(a["padding"]))
        r = np.pad(x, pads[::-1], constant_values=int(zero_of(o_t)))
    else:
        n = int(a["block_size"])
        if k == "SPACE_TO_DEPTH":      # out[b, y, x, (dy * n + dx) * C + c] = in[b, y * n + dy, x * n + dx, c]
            b, h, w, c = x.shape
            r = x.reshape(b, h // n, n, w // n, n, c).transpose(0, 1, 3, 2, 4, 5).reshape(b, h // n, w // n, n * n * c)
        else:
            b, h, w, c = x.shape
            r = x.reshape(b, h, w, n, n, c // (n * n)).transpose(0, 1, 3, 2, 4, 5).reshape(b, h * n, w * n, c // (n * n))
    assert r.shape == oshape and r.dtype == o_t.dtype, (k, r.shape, oshape)
    return [moved(np.ascontiguousarray(r))]


def run_graph(graph, inputs):
    values = {i: np.asarray(x) for i, x in zip([i for i in graph.inputs if graph.tensors[i].data is None], inputs)}
    for op in graph.ops:
        for i, r in zip(op.outputs, run_op(graph, op, values)):
            values[i] = r.rounded
    return values
