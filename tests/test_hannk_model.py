"""halide_amd/hannk_model.py: the lowering of .tflite graphs to plans over the library's entry points, and the executor.

CPU: the plans' scalar arguments against the hl.hannk_* helpers, the shape of the lowerings the issue names, the evaluator
(tests/hannk_model_checker.py) against direct numpy restatements.
GPU (-m gpu): every fixture, Python-built graphs, a three-op chain, repeated runs and two models at once, all bit for bit against the evaluator;
no host synchronisation inside run()."""
from __future__ import annotations

import glob
import os

import numpy as np
import pytest

from halide_amd import hannk_model as hm
from halide_amd import tflite_reader as tfl
from hannk_model_checker import Evaluator

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hannk")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "*", "*.tflite")))
MOBILENET = os.path.join(GOLDEN, "mobilenet_v1_0.25_128_quant")
gpu = pytest.mark.gpu
Q = ((0.0235, 128),)


def rel(path):
    return os.path.relpath(path, GOLDEN)


def inputs_for(model, seed):
    """seeded uniform inputs over the full u8 range; f32 inputs in [-1, 1)"""
    r = np.random.RandomState(seed)
    out = []
    for i in model._activation_inputs():
        t = model.tensors[i]
        shape = tuple(reversed(t.shape))
        out.append(r.randint(0, 256, shape).astype(np.uint8) if t.dtype == np.uint8 else (r.random_sample(shape) * 2 - 1).astype(t.dtype))
    return out


def tensor(shape_nhwc, dtype=np.uint8, scale=0.0235, zero=128, data=None):
    q = ((scale,), (zero,)) if np.dtype(dtype) == np.uint8 and scale is not None else ((), ())
    return tfl.Tensor("t", tuple(reversed(shape_nhwc)), np.dtype(dtype), q[0], q[1], data)


def graph(tensors, kind, inputs, outputs, attrs, act_inputs=None):
    return tfl.Graph(tensors, [tfl.Op(kind, list(inputs), list(outputs), dict(attrs))], list(inputs if act_inputs is None else act_inputs), list(outputs))


def python_graphs():
    """the ops without a fixture, at 17 channels and width 5: past one 16-byte vector, not a multiple of anything"""
    x = (1, 4, 5, 17)
    idx = np.array([[3, 0], [3, 4]], np.int32)
    yield "DEPTH_TO_SPACE", graph([tensor((1, 3, 5, 68)), tensor((1, 6, 10, 17))], "DEPTH_TO_SPACE", [0], [1], {"block_size": 2})
    yield "GATHER", graph([tensor(x), tensor(idx.shape, np.int32, data=idx), tensor((1, 4, 2, 2, 17))], "GATHER", [0, 1], [2], {"axis": 1, "batch_dims": 0}, [0])
    yield "PAD", graph([tensor(x), tensor((1, 7, 8, 17))], "PAD", [0], [1], {"padding": [(0, 0), (2, 1), (1, 2), (0, 0)]})
    yield "PAD_3_TO_4", graph([tensor((1, 4, 5, 3)), tensor((1, 4, 5, 4))], "PAD", [0], [1], {"padding": [(0, 1), (0, 0), (0, 0), (0, 0)]})
    yield "MEAN", graph([tensor(x), tensor((1, 1, 1, 17))], "MEAN", [0], [1], {"axes": [1, 2], "keep_dims": True})
    yield "TANH", graph([tensor(x, scale=0.05), tensor(x, scale=1 / 128, zero=128)], "TANH", [0], [1], {})
    yield "RELU6", graph([tensor(x, scale=0.05, zero=100), tensor(x, scale=0.04, zero=10)], "RELU6", [0], [1], {})
    yield "CONCATENATION_F32", graph([tensor((2, 3, 5), np.float32), tensor((2, 3, 7), np.float32), tensor((2, 3, 12), np.float32)], "CONCATENATION", [0, 1],
                                     [2], {"axis": 0, "activation": None})


PYTHON_GRAPHS = dict(python_graphs())


def chain(paths):
    """the one-op graphs of `paths` as one graph: each file's output tensor is the next file's input"""
    tensors, ops, prev_out, first_in = [], [], None, None
    for p in paths:
        g = tfl.read(p)
        base = len(tensors)
        tensors += g.tensors
        op = g.ops[0]
        ins = [i + base for i in op.inputs]
        if prev_out is not None:
            a, b = tensors[prev_out], tensors[ins[0]]
            assert (a.shape, a.scale, a.zero) == (b.shape, b.scale, b.zero)
            ins[0] = prev_out
        else:
            first_in = ins[0]
        prev_out = op.outputs[0] + base
        ops.append(tfl.Op(op.kind, ins, [prev_out], dict(op.attrs)))
    return tfl.Graph(tensors, ops, [first_in], [prev_out])


def three_op_chain():
    return hm.HannkModel(chain(sorted(glob.glob(os.path.join(MOBILENET, "00[012].*.tflite")))))


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_every_fixture_lowers(hl):
    for p in FILES:
        m = hm.HannkModel.from_tflite(p)
        assert all(isinstance(s.name, str) and (s.name in hl._fn or s.name in ("hannk_copy_from", "hannk_gather")) for s in m.setup + m.plan), rel(p)


def test_step_scalars_are_the_helpers(hl):
    f32 = np.float32
    m = hm.HannkModel.from_tflite(os.path.join(MOBILENET, "000.CONV_2D.tflite"))
    g = m.graph
    x, f, _ = (g.tensors[i] for i in g.ops[0].inputs)
    o = g.tensors[g.ops[0].outputs[0]]
    assert [s.name for s in m.setup] == ["tile_conv_filter_uint8"] and [s.name for s in m.plan] == ["fill_uint8", "copy_uint8_uint8", "conv_u8_u8_u8"]
    a = m.plan[2].args
    mant, exp = hl.hannk_int_float(f32(x.scale[0]) * f32(f.scale[0]) / f32(o.scale[0]), 32)
    assert a[1] == x.zero[0] and a[3] == f.zero[0] and a[5:9] == (2, 2, 1, 1) and a[9:11] == (mant, -exp) and a[11] == o.zero[0]
    assert a[12:14] == hl.hannk_output_range(None, o.zero[0], o.scale[0])
    # SAME padding of 128 -> 64 at stride 2 under 3 x 3: nothing in front, one pixel behind; channels 3 -> 4: written by the PAD steps
    assert a[0].extents == (4, 129, 129, 1) and m.plan[0].args[0] == x.zero[0] and m.plan[1].args[2].extents == (4, 128, 128, 1)
    assert m.plan[1].args[2].mins == (0, hl.hannk_compute_padding(2, 128, 3, 64), hl.hannk_compute_padding(2, 128, 3, 64), 0)

    m = hm.HannkModel.from_tflite(os.path.join(MOBILENET, "001.DEPTHWISE_CONV_2D.tflite"))
    g = m.graph
    x, f, _ = (g.tensors[i] for i in g.ops[0].inputs)
    o = g.tensors[g.ops[0].outputs[0]]
    a = m.plan[-1].args
    mant, exp = hl.hannk_int_float(f32(x.scale[0]) * f32(f.scale[0]) / f32(o.scale[0]), 32)
    assert m.plan[-1].name == "depthwise_conv_uint8" and a[9] == 0 and a[10:12] == (mant, -exp) and a[0].extents == (16, 66, 66, 1)

    m = hm.HannkModel.from_tflite(os.path.join(GOLDEN, "mobilenet_v2_1.0_224_quant", "009.ADD.tflite"))
    g = m.graph
    q = [(g.tensors[i].scale[0], g.tensors[i].zero[0]) for i in g.ops[0].inputs + g.ops[0].outputs]
    a = m.plan[0].args
    assert (a[2], a[5]) == hl.hannk_add_multipliers(q[0][0], q[1][0], q[2][0]) and (a[1], a[4], a[6]) == (q[0][1], q[1][1], q[2][1])
    assert a[7:9] == hl.hannk_output_range(None, q[2][1], q[2][0])

    m = hm.HannkModel.from_tflite(os.path.join(MOBILENET, "030.SOFTMAX.tflite"))
    g = m.graph
    bm, bs, om, osh = hl.hannk_softmax_params(g.tensors[g.ops[0].inputs[0]].scale[0], 1.0, g.tensors[g.ops[0].outputs[0]].scale[0])
    assert m.plan[0].args[1:6] == (bm, bs, g.tensors[g.ops[0].outputs[0]].zero[0], om, osh)


def test_lowerings_the_issue_names():
    m = hm.HannkModel.from_tflite(os.path.join(GOLDEN, "inception_v2_224_quant", "000.DEPTHWISE_CONV_2D.tflite"))
    names = [s.name for s in m.plan]
    assert names[0] == "upsample_channels_uint8" and names[-1] == "depthwise_conv_uint8" and m.plan[0].args[1] == 8
    m = hm.HannkModel.from_tflite(os.path.join(GOLDEN, "inception_v4_299_quant", "015.CONCATENATION.tflite"))
    assert [s.name for s in m.plan] == ["add_uint8_uint8"] * 2 and m.plan[0].args[2] != m.plan[1].args[2]
    assert m.plan[0].args[5] == 0 and m.plan[1].args[5] == 0 and m.plan[1].args[9].offset == 192
    m = hm.HannkModel.from_tflite(os.path.join(GOLDEN, "misc", "SPLIT.1_1_1.tflite"))
    assert [s.name for s in m.plan] == ["hannk_copy_from"] * 3
    m = hm.HannkModel.from_tflite(os.path.join(GOLDEN, "misc", "bad_fully_connected.tflite"))
    assert m.plan[-1].name == "conv_u8_u8_u8" and m.plan[-1].args[0].extents == (12, 1, 1, 2) and m.plan[-1].args[14].extents == (3, 1, 1, 2)
    assert m.plan[-1].args[12] == m.graph.tensors[m.graph.ops[0].outputs[0]].zero[0]      # RELU
    m = hm.HannkModel.from_tflite(os.path.join(MOBILENET, "029.RESHAPE.tflite"))
    assert m.plan == []      # dense: a view
    for name in ("bad_broadcast_add", "bad_broadcast_mul", "bad_broadcast_sub"):
        m = hm.HannkModel.from_tflite(os.path.join(GOLDEN, "misc", name + ".tflite"))
        assert m.plan[0].args[0].strides == (0, 1)      # [2, 1] against [2, 2]: a stride of 0
    bad = graph([tensor((1, 2, 2, 4)), tensor((1, 2, 2, 4))], "LOGISTIC", [0], [1], {})
    bad.ops[0].kind = "LSTM"
    with pytest.raises(NotImplementedError, match="LSTM"):
        hm.HannkModel(bad)


def test_evaluator_is_the_numpy_restatement():
    def run(model, seed=1):
        x = inputs_for(model, seed)
        return x, Evaluator(model).run(*x)

    x, out = run(hm.HannkModel.from_tflite(os.path.join(GOLDEN, "misc", "TRANSPOSE.2_0_1.tflite")))
    assert np.array_equal(out[0], np.transpose(x[0], (1, 0, 2)))
    for block in (2, 4):
        x, out = run(hm.HannkModel.from_tflite(os.path.join(GOLDEN, "misc", f"SPACE_TO_DEPTH.{block}.tflite")))
        b, h, w, c = x[0].shape
        want = x[0].reshape(b, h // block, block, w // block, block, c).transpose(0, 1, 3, 2, 4, 5).reshape(b, h // block, w // block, block * block * c)
        assert np.array_equal(out[0], want)
        back = hm.HannkModel(graph([tensor(want.shape), tensor(x[0].shape)], "DEPTH_TO_SPACE", [0], [1], {"block_size": block}))
        assert np.array_equal(Evaluator(back).run(want)[0], x[0])      # depth-to-space of space-to-depth is the identity
    x, out = run(hm.HannkModel.from_tflite(os.path.join(GOLDEN, "misc", "SPLIT_V.36_5_7.tflite")))
    assert all(np.array_equal(o, w) for o, w in zip(out, np.split(x[0], [36, 41], -1)))      # equal scales: the add kernel is the identity
    x, out = run(hm.HannkModel(PYTHON_GRAPHS["DEPTH_TO_SPACE"]))
    b, h, w, c = x[0].shape
    assert np.array_equal(out[0], x[0].reshape(b, h, w, 2, 2, c // 4).transpose(0, 1, 3, 2, 4, 5).reshape(b, 2 * h, 2 * w, c // 4))
    m = hm.HannkModel(PYTHON_GRAPHS["GATHER"])
    x, out = run(m)
    assert np.array_equal(out[0], np.take(x[0], m.graph.tensors[1].data, 2))      # Halide axis 1 of rank 4 is numpy axis 2
    x, out = run(hm.HannkModel(PYTHON_GRAPHS["CONCATENATION_F32"]))
    assert np.array_equal(out[0], np.concatenate(x, -1))
    x, out = run(hm.HannkModel(PYTHON_GRAPHS["PAD"]))
    assert np.array_equal(out[0], np.pad(x[0], ((0, 0), (1, 2), (2, 1), (0, 0)), constant_values=128))
    x, out = run(hm.HannkModel(PYTHON_GRAPHS["PAD_3_TO_4"]))
    assert np.array_equal(out[0], np.pad(x[0], ((0, 0), (0, 0), (0, 0), (0, 1)), constant_values=128))


# ------------------------------------------------------------------------------------------------------------------ GPU
def on_device(model, xs):
    import torch
    got = model.run(*[torch.from_numpy(x).cuda() for x in xs])
    got = got if isinstance(got, tuple) else (got,)
    assert all(g.is_cuda for g in got)
    return [g.cpu().numpy() for g in got]


def same(got, want, what):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, what
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), (what, int(np.count_nonzero(g != w)), g.size)


@gpu
@pytest.mark.parametrize("path", FILES, ids=rel)
def test_hip_every_fixture_is_the_evaluator(hl, path):
    m = hm.HannkModel.from_tflite(path)
    xs = inputs_for(m, FILES.index(path))
    same(on_device(m, xs), Evaluator(m).run(*xs), rel(path))


@gpu
@pytest.mark.parametrize("name", sorted(PYTHON_GRAPHS))
def test_hip_python_graphs_are_the_evaluator(hl, name):
    m = hm.HannkModel(PYTHON_GRAPHS[name])
    xs = inputs_for(m, 7)
    same(on_device(m, xs), Evaluator(m).run(*xs), name)


@gpu
def test_hip_chain_repeated_runs_and_two_models(hl):
    a, b = three_op_chain(), hm.HannkModel.from_tflite(os.path.join(MOBILENET, "003.DEPTHWISE_CONV_2D.tflite"))
    assert [s.name for s in a.plan if "conv" in s.name and "tile" not in s.name] == ["conv_u8_u8_u8", "depthwise_conv_uint8", "conv_u8_u8_u8"]
    a.prepare()
    b.prepare()      # two models prepared at once
    xa1, xa2, xb = inputs_for(a, 1), inputs_for(a, 2), inputs_for(b, 3)
    first = on_device(a, xa1)
    other = on_device(b, xb)
    second = on_device(a, xa2)
    same(first, Evaluator(a).run(*xa1), "chain, first run")
    same(second, Evaluator(a).run(*xa2), "chain, second run")
    same(other, Evaluator(b).run(*xb), "the other model")
    same(second, on_device(three_op_chain(), xa2), "a fresh model")
    # the activation passes from step to step on the device: the chain equals the three files run one after the other
    x = xa1
    for p in sorted(glob.glob(os.path.join(MOBILENET, "00[012].*.tflite"))):
        x = on_device(hm.HannkModel.from_tflite(p), x)
    same(first, x, "the chain against its three files")


@gpu
def test_hip_run_does_not_wait_for_the_device(hl, monkeypatch):
    import torch
    m = three_op_chain().prepare()
    x = torch.from_numpy(inputs_for(m, 4)[0]).cuda()
    m.run(x)
    torch.cuda.synchronize()
    calls = []
    for name in ("_hip_memcpy", "_hip_stream_synchronize", "_hip_device_synchronize"):
        real = getattr(hm, name)
        monkeypatch.setattr(hm, name, lambda *a, _n=name, _r=real: (calls.append(_n), _r(*a))[1])
    asyncs = []
    real_async = hm._hip_memcpy_async
    monkeypatch.setattr(hm, "_hip_memcpy_async", lambda *a: (asyncs.append(a[3]), real_async(*a))[1])
    out = m.run(x)
    assert calls == [] and asyncs == [3, 3]      # one device-to-device copy in, one out, both on the stream; nothing that waits
    same([out.cpu().numpy()], Evaluator(m).run(x.cpu().numpy()), "the counted run")
