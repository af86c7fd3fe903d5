"""halide_amd/tflite_reader.py against the one-op .tflite files of apps/hannk's test set under tests/golden/hannk (byte-for-byte copies):
what each file decodes to, agreement between producer and consumer files, and what the reader does with files it should not trust."""
from __future__ import annotations

import glob
import os
import re
import struct

import numpy as np
import pytest

from halide_amd import tflite_reader as tfl

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hannk")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "*", "*.tflite")))
BAD = {"bad_broadcast_add": "ADD", "bad_broadcast_mul": "MUL", "bad_broadcast_sub": "SUB", "bad_fully_connected": "FULLY_CONNECTED"}
MOBILENET = os.path.join(GOLDEN, "mobilenet_v1_0.25_128_quant")


def rel(path):
    return os.path.relpath(path, GOLDEN)


def named_op(path):
    stem = os.path.basename(path)[:-len(".tflite")]
    return BAD[stem] if stem in BAD else re.sub(r"^\d+\.", "", stem).split(".")[0]


def test_the_fixture_set_is_complete():
    assert len(FILES) == 38
    assert len(glob.glob(os.path.join(MOBILENET, "*.tflite"))) == 21 and len(glob.glob(os.path.join(GOLDEN, "misc", "*.tflite"))) == 12
    assert sum(os.path.getsize(f) for f in FILES) < 200 * 1024 and max(os.path.getsize(f) for f in FILES) <= 18 * 1024


@pytest.mark.parametrize("path", FILES, ids=rel)
def test_every_file_decodes_to_the_op_its_name_carries(path):
    g = tfl.read(path)
    assert [op.kind for op in g.ops] == [named_op(path)]
    assert g.tensors and g.inputs and g.outputs
    op = g.ops[0]
    assert op.inputs and op.outputs
    for i in op.inputs + op.outputs:
        t = g.tensors[i]
        assert isinstance(t.shape, tuple) and t.dtype in (np.dtype(np.uint8), np.dtype(np.int32), np.dtype(np.float32))
        if t.dtype == np.uint8:
            assert len(t.scale) == 1 and len(t.zero) == 1 and t.scale[0] > 0 and 0 <= t.zero[0] <= 255, t
        if t.data is not None:
            assert t.data.dtype == t.dtype and t.data.shape == t.tfl_shape
    # activations are not constants; the tensors the subgraph lists as inputs and outputs exist
    assert all(g.tensors[i].data is None for i in op.outputs)
    assert all(0 <= i < len(g.tensors) for i in g.inputs + g.outputs)
    # bytes and a path read alike
    with open(path, "rb") as fh:
        again = tfl.read(fh.read())
    assert [(t.shape, t.dtype, t.scale, t.zero) for t in again.tensors] == [(t.shape, t.dtype, t.scale, t.zero) for t in g.tensors]


def test_shapes_axes_and_options_of_known_files():
    g = tfl.read(os.path.join(MOBILENET, "000.CONV_2D.tflite"))
    op = g.ops[0]
    assert op.attrs == {"padding": "same", "stride": (2, 2), "activation": None, "dilation": (1, 1)}
    inp, filt, bias = (g.tensors[i] for i in op.inputs)
    assert inp.shape == (3, 128, 128, 1) and inp.tfl_shape == (1, 128, 128, 3)        # Halide order: channel innermost
    assert filt.shape == (3, 3, 3, 8) and filt.data.shape == (8, 3, 3, 3) and bias.data.dtype == np.int32 and bias.shape == (8,)
    assert g.tensors[op.outputs[0]].shape == (8, 64, 64, 1)
    g = tfl.read(os.path.join(GOLDEN, "inception_v2_224_quant", "000.DEPTHWISE_CONV_2D.tflite"))
    assert g.ops[0].attrs["depth_multiplier"] == 8 and g.ops[0].attrs["stride"] == (2, 2)
    g = tfl.read(os.path.join(GOLDEN, "inception_v4_299_quant", "016.AVERAGE_POOL_2D.tflite"))
    assert g.ops[0].attrs == {"padding": "same", "stride": (1, 1), "filter": (3, 3), "activation": None}
    g = tfl.read(os.path.join(GOLDEN, "inception_v4_299_quant", "015.CONCATENATION.tflite"))
    assert g.ops[0].attrs["axis"] == 0                       # the file's axis 3 of rank 4
    assert g.tensors[g.ops[0].inputs[0]].scale != g.tensors[g.ops[0].inputs[1]].scale
    g = tfl.read(os.path.join(GOLDEN, "misc", "TRANSPOSE.2_0_1.tflite"))
    op = g.ops[0]
    assert op.attrs["perm"] == [1, 0, 2] and op.attrs["order"] == [0, 2, 1] and len(op.inputs) == 1
    assert g.tensors[op.inputs[0]].tfl_shape == (16, 28, 384) and g.tensors[op.outputs[0]].tfl_shape == (28, 16, 384)
    g = tfl.read(os.path.join(GOLDEN, "misc", "SPLIT_V.36_5_7.tflite"))
    assert g.ops[0].attrs["size_splits"] == [36, 5, 7] and g.ops[0].attrs["axis"] == 0 and len(g.ops[0].outputs) == 3
    g = tfl.read(os.path.join(GOLDEN, "misc", "SPLIT.1_1_1.tflite"))
    assert g.ops[0].attrs["num_splits"] == 3 and g.ops[0].attrs["axis"] == 0 and g.tensors[g.ops[0].inputs[0]].dtype == np.float32
    g = tfl.read(os.path.join(GOLDEN, "misc", "SPACE_TO_DEPTH.4.tflite"))
    assert g.ops[0].attrs == {"block_size": 4} and g.tensors[g.ops[0].inputs[0]].shape[0] == 1
    g = tfl.read(os.path.join(GOLDEN, "misc", "bad_fully_connected.tflite"))
    assert g.ops[0].attrs["activation"] == "relu" and g.tensors[g.ops[0].inputs[0]].tfl_shape == (4, 1, 5, 1)
    g = tfl.read(os.path.join(MOBILENET, "030.SOFTMAX.tflite"))
    assert g.ops[0].attrs == {"beta": 1.0}
    g = tfl.read(os.path.join(MOBILENET, "029.RESHAPE.tflite"))
    assert g.ops[0].attrs["new_shape"] == [1, 1001] and len(g.ops[0].inputs) == 1


def test_mobilenet_chain_agrees_between_producer_and_consumer():
    chain = [tfl.read(f) for f in sorted(glob.glob(os.path.join(MOBILENET, "*.tflite")))[:15]]
    assert len(chain) == 15
    for a, b in zip(chain, chain[1:]):
        out, inp = a.tensors[a.ops[0].outputs[0]], b.tensors[b.ops[0].inputs[0]]
        assert (out.shape, out.dtype, out.scale, out.zero) == (inp.shape, inp.dtype, inp.scale, inp.zero)


def test_truncated_files_raise_value_error():
    with open(os.path.join(MOBILENET, "000.CONV_2D.tflite"), "rb") as fh:
        whole = fh.read()
    tfl.read(whole)
    for n in range(0, len(whole), 64):
        with pytest.raises(ValueError):
            tfl.read(whole[:n])
    with pytest.raises(ValueError):
        tfl.read(b"\x10\x00\x00\x00TFL2" + whole[8:])


def test_offsets_past_the_end_raise_value_error():
    with open(os.path.join(MOBILENET, "002.CONV_2D.tflite"), "rb") as fh:
        whole = bytearray(fh.read())
    root = struct.unpack_from("<I", whole, 0)[0]
    # the root offset itself
    bad = bytearray(whole)
    struct.pack_into("<I", bad, 0, len(whole) + 64)
    with pytest.raises(ValueError):
        tfl.read(bytes(bad))
    # the model's vtable offset, pointing before the file and past it
    for v in (len(whole) * 2, -len(whole) * 2):
        bad = bytearray(whole)
        struct.pack_into("<i", bad, root, v)
        with pytest.raises(ValueError):
            tfl.read(bytes(bad))
    # every field of the model table in turn (operator codes, subgraphs, buffers ...) sent past the end
    vt = root - struct.unpack_from("<i", whole, root)[0]
    vsize = struct.unpack_from("<H", whole, vt)[0]
    hit = 0
    for slot in range((vsize - 4) // 2):
        rel_off = struct.unpack_from("<H", whole, vt + 4 + 2 * slot)[0]
        if rel_off == 0 or slot == 0:      # slot 0 is the version, a scalar
            continue
        bad = bytearray(whole)
        struct.pack_into("<I", bad, root + rel_off, 0x7FFFFFF0)
        if slot in (1, 2, 4):
            hit += 1
            with pytest.raises(ValueError):
                tfl.read(bytes(bad))
    assert hit == 3
    # any single corrupted dword either reads or raises ValueError / NotImplementedError: never an IndexError or struct.error
    r = np.random.RandomState(0)
    for _ in range(300):
        bad = bytearray(whole)
        at = int(r.randint(0, len(bad) // 4)) * 4
        struct.pack_into("<I", bad, at, int(r.choice([0, 1, 0xFFFFFFFF, 0x7FFFFFFF, len(bad), len(bad) - 1, 0x80000000])))
        try:
            tfl.read(bytes(bad))
        except (ValueError, NotImplementedError):
            pass


def _with_op_code(whole, code):
    """`whole` with every operator code replaced, in the deprecated int8 field and the int32 one where present"""
    out = bytearray(whole)
    root = struct.unpack_from("<I", out, 0)[0]
    vt = root - struct.unpack_from("<i", out, root)[0]
    codes_field = root + struct.unpack_from("<H", out, vt + 4 + 2 * 1)[0]
    vec = codes_field + struct.unpack_from("<I", out, codes_field)[0]
    wrote = False
    for k in range(struct.unpack_from("<I", out, vec)[0]):     # the file lists the codes of its whole model; the one operator names one of them
        oc = vec + 4 + 4 * k + struct.unpack_from("<I", out, vec + 4 + 4 * k)[0]
        ovt = oc - struct.unpack_from("<i", out, oc)[0]
        ovsize = struct.unpack_from("<H", out, ovt)[0]
        for slot, fmt in ((0, "<b"), (3, "<i")):
            if 4 + 2 * slot + 2 <= ovsize:
                r = struct.unpack_from("<H", out, ovt + 4 + 2 * slot)[0]
                if r:
                    struct.pack_into(fmt, out, oc + r, min(code, 127) if fmt == "<b" else code)
                    wrote = True
    assert wrote
    return bytes(out)


def test_unsupported_ops_are_refused_by_name():
    with open(os.path.join(MOBILENET, "030.SOFTMAX.tflite"), "rb") as fh:
        whole = fh.read()
    assert tfl.read(_with_op_code(whole, 25)).ops[0].kind == "SOFTMAX"
    with pytest.raises(NotImplementedError, match="LSTM"):
        tfl.read(_with_op_code(whole, 16))
    with pytest.raises(NotImplementedError, match="NEG"):
        tfl.read(_with_op_code(whole, 59))
    with pytest.raises(NotImplementedError, match="code 6"):       # DEQUANTIZE: unknown to the reader
        tfl.read(_with_op_code(whole, 6))


def test_float_models_other_than_copies_are_refused():
    with open(os.path.join(GOLDEN, "misc", "SPLIT.1_1_1.tflite"), "rb") as fh:
        whole = fh.read()
    assert tfl.read(whole).ops[0].kind == "SPLIT"
    with pytest.raises((NotImplementedError, ValueError)) as e:
        tfl.read(_with_op_code(whole, 14))                          # LOGISTIC on float tensors
    assert e.type is NotImplementedError and "LOGISTIC" in str(e.value)


def test_reshape_takes_its_shape_from_the_options_or_the_operand():
    def convert(new_shape, operand, out_shape=(1, 1001)):
        tensors = [tfl.Tensor("in", (1001, 1, 1, 1), np.dtype(np.uint8)), tfl.Tensor("out", tuple(reversed(out_shape)), np.dtype(np.uint8)),
                   tfl.Tensor("shape", (2,), np.dtype(np.int32), data=operand)]
        op = tfl.Op("RESHAPE", [0, 2], [1], {"new_shape": list(new_shape)})
        tfl._convert_axes(op, tensors)
        return op

    for new_shape, operand in (([1, 1001], None), ([], np.array([1, 1001], np.int32)), ([1, -1], None), ([], np.array([-1, 1001], np.int32)), ([], None)):
        op = convert(new_shape, operand)
        assert op.attrs["new_shape"] == [1, 1001] and op.inputs == [0]
    with pytest.raises(ValueError, match="RESHAPE"):
        convert([], np.array([7, 143], np.int32))
    with pytest.raises(ValueError, match="RESHAPE"):
        convert([1, 1000], None)
