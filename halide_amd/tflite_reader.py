"""A reader for .tflite files (the FlatBuffers schema of TensorFlow Lite, identifier TFL3) in plain Python: `struct` and numpy only.

read(path_or_bytes) -> Graph.  Conventions follow apps/hannk's tflite/tflite_parser.cpp: `Tensor.shape` is in Halide order (the file's
shape reversed, channel innermost), an axis `a` of a rank-`r` tensor becomes `r - 1 - a` once its negative form is resolved, and
TRANSPOSE's permutation is converted as interpreter/ops.cpp:1752-1755 does.  Constants stay numpy arrays in the file's own order
(NHWC), which is the order halide_amd.Buffer takes (numpy axes are the Halide dimensions reversed).

The reader does not trust the file: every offset and length that leaves the file raises ValueError.  Table offsets only point forward and
the schema bounds the nesting, so no walk can cycle.  An operator outside the supported set raises NotImplementedError with its name.
"""
import struct
from dataclasses import dataclass, field

import numpy as np

# builtin operator codes.  FIXTURE: decoded from the one-op files under tests/golden/hannk; SCHEMA: taken from the public schema, no file
# to check them against
_OPS_FIXTURE = {0: "ADD", 1: "AVERAGE_POOL_2D", 2: "CONCATENATION", 3: "CONV_2D", 4: "DEPTHWISE_CONV_2D", 9: "FULLY_CONNECTED",
                11: "L2_NORMALIZATION", 14: "LOGISTIC", 17: "MAX_POOL_2D", 18: "MUL", 22: "RESHAPE", 25: "SOFTMAX", 26: "SPACE_TO_DEPTH",
                39: "TRANSPOSE", 41: "SUB", 49: "SPLIT", 102: "SPLIT_V"}
_OPS_SCHEMA = {5: "DEPTH_TO_SPACE", 19: "RELU", 20: "RELU_N1_TO_1", 21: "RELU6", 28: "TANH", 34: "PAD", 36: "GATHER", 40: "MEAN"}
OPS = {**_OPS_FIXTURE, **_OPS_SCHEMA}
# refused by name: the reference runs them as scalar host loops "only intended to support scalar operations"
_OPS_REFUSED = {16: "LSTM", 59: "NEG", 92: "SQUARE", 77: "SHAPE", 107: "GATHER_ND", 61: "GREATER", 62: "GREATER_EQUAL", 58: "LESS",
                63: "LESS_EQUAL", 71: "EQUAL", 72: "NOT_EQUAL"}
# ops that only move elements: the ones a float model may hold
COPY_OPS = ("TRANSPOSE", "SPACE_TO_DEPTH", "DEPTH_TO_SPACE", "GATHER", "CONCATENATION", "SPLIT", "SPLIT_V", "RESHAPE")
ACTIVATIONS = {0: None, 1: "relu", 2: "relu_n1_to_1", 3: "relu6", 4: "tanh"}
_DTYPES = {0: np.float32, 2: np.int32, 3: np.uint8, 4: np.int64, 6: np.bool_, 7: np.int16, 9: np.int8}


@dataclass
class Tensor:
    name: str
    shape: tuple          # Halide order: the file's shape reversed
    dtype: np.dtype
    scale: tuple = ()     # quantization: one entry for a per-tensor scale
    zero: tuple = ()
    data: np.ndarray | None = None   # a constant, in the file's order (numpy axes = Halide dimensions reversed)

    @property
    def tfl_shape(self):
        return tuple(reversed(self.shape))

    @property
    def quantized(self):
        return len(self.scale) > 0


@dataclass
class Op:
    kind: str
    inputs: list          # tensor ids; -1 = an optional input left out
    outputs: list
    attrs: dict = field(default_factory=dict)


@dataclass
class Graph:
    tensors: list
    ops: list
    inputs: list
    outputs: list
    name: str = ""
    version: int = 0


class _File:
    def __init__(self, data):
        self.b = bytes(data)
        self.n = len(self.b)

    def get(self, fmt, off):
        size = struct.calcsize(fmt)
        if not isinstance(off, int) or off < 0 or off + size > self.n:
            raise ValueError(f"tflite: a {size}-byte field at offset {off} leaves the file of {self.n} bytes")
        return struct.unpack_from(fmt, self.b, off)[0]

    def indirect(self, off):
        """the position a uoffset_t at `off` points to: always forward"""
        rel = self.get("<I", off)
        if rel == 0:
            raise ValueError(f"tflite: a null offset at {off}")
        return off + rel

    def table(self, pos):
        return _Table(self, pos)


class _Table:
    def __init__(self, f, pos):
        self.f, self.pos = f, pos
        self.vt = pos - f.get("<i", pos)
        self.vsize = f.get("<H", self.vt)
        self.tsize = f.get("<H", self.vt + 2)
        if self.vsize < 4 or self.vsize % 2 or self.vt + self.vsize > f.n or self.pos + self.tsize > f.n:
            raise ValueError(f"tflite: the table at {pos} has a vtable that leaves the file")

    def _field(self, slot):
        at = 4 + 2 * slot
        if at + 2 > self.vsize:
            return None
        rel = self.f.get("<H", self.vt + at)
        if rel == 0:
            return None
        if rel >= max(self.tsize, 4) and self.tsize:
            raise ValueError(f"tflite: field {slot} of the table at {self.pos} lies outside the table")
        return self.pos + rel

    def scalar(self, slot, fmt, default=0):
        at = self._field(slot)
        return default if at is None else self.f.get(fmt, at)

    def sub(self, slot):
        at = self._field(slot)
        return None if at is None else self.f.table(self.f.indirect(at))

    def _vector(self, slot, item):
        at = self._field(slot)
        if at is None:
            return None, 0
        start = self.f.indirect(at)
        count = self.f.get("<I", start)
        if start + 4 + count * item > self.f.n:
            raise ValueError(f"tflite: a vector of {count} items at {start} leaves the file")
        return start + 4, count

    def array(self, slot, dtype):
        dtype = np.dtype(dtype)
        start, count = self._vector(slot, dtype.itemsize)
        if start is None:
            return None
        return np.frombuffer(self.f.b, dtype.newbyteorder("<"), count, start).astype(dtype)

    def string(self, slot):
        start, count = self._vector(slot, 1)
        return "" if start is None else self.f.b[start:start + count].decode("utf-8", "replace")

    def tables(self, slot):
        start, count = self._vector(slot, 4)
        return [] if start is None else [self.f.table(self.f.indirect(start + 4 * i)) for i in range(count)]


def _ints(a):
    return [] if a is None else [int(v) for v in a]


def _options(kind, opt, tag):
    """the builtin_options table of one operator, by its union tag"""
    want = {"CONV_2D": 1, "DEPTHWISE_CONV_2D": 2, "AVERAGE_POOL_2D": 5, "MAX_POOL_2D": 5, "FULLY_CONNECTED": 8, "SOFTMAX": 9, "CONCATENATION": 10,
            "ADD": 11, "L2_NORMALIZATION": 12, "RESHAPE": 17, "SPACE_TO_DEPTH": 19, "MUL": 21, "SUB": 28, "SPLIT": 35,
            "SPLIT_V": 79}.get(kind)   # the ops without a fixture take whatever table they carry
    if opt is None or tag == 0:
        if kind in ("CONV_2D", "DEPTHWISE_CONV_2D", "AVERAGE_POOL_2D", "MAX_POOL_2D", "SPACE_TO_DEPTH", "DEPTH_TO_SPACE"):
            raise ValueError(f"tflite: {kind} without its options table")
        opt = None
    elif want is not None and tag != want:
        raise ValueError(f"tflite: {kind} carries options of union type {tag}, not {want}")
    a = {}

    def get(slot, fmt, default=0):
        return default if opt is None else opt.scalar(slot, fmt, default)

    def act(slot):
        code = get(slot, "<b")
        if code not in ACTIVATIONS:
            raise NotImplementedError(f"tflite: fused activation {code} of {kind}")
        return ACTIVATIONS[code]

    if kind == "CONV_2D":
        a.update(padding=("same", "valid")[get(0, "<b") & 1], stride=(get(1, "<i"), get(2, "<i")), activation=act(3),
                 dilation=(get(4, "<i", 1), get(5, "<i", 1)))
    elif kind == "DEPTHWISE_CONV_2D":
        a.update(padding=("same", "valid")[get(0, "<b") & 1], stride=(get(1, "<i"), get(2, "<i")), depth_multiplier=get(3, "<i"), activation=act(4),
                 dilation=(get(5, "<i", 1), get(6, "<i", 1)))
    elif kind in ("AVERAGE_POOL_2D", "MAX_POOL_2D"):
        a.update(padding=("same", "valid")[get(0, "<b") & 1], stride=(get(1, "<i"), get(2, "<i")), filter=(get(3, "<i"), get(4, "<i")), activation=act(5))
    elif kind == "FULLY_CONNECTED":
        a.update(activation=act(0), weights_format=get(1, "<b"), keep_num_dims=bool(get(2, "<b")))
    elif kind == "SOFTMAX":
        a.update(beta=float(get(0, "<f", 0.0)))
    elif kind == "CONCATENATION":
        a.update(axis=get(0, "<i"), activation=act(1))
    elif kind in ("ADD", "MUL", "SUB", "L2_NORMALIZATION"):
        a.update(activation=act(0))
    elif kind == "RESHAPE":
        a.update(new_shape=_ints(None if opt is None else opt.array(0, np.int32)))
    elif kind in ("SPACE_TO_DEPTH", "DEPTH_TO_SPACE"):
        a.update(block_size=get(0, "<i"))
    elif kind in ("SPLIT", "SPLIT_V"):
        a.update(num_splits=get(0, "<i"))
    elif kind == "GATHER":
        a.update(axis=get(0, "<i"), batch_dims=get(1, "<i"))
    elif kind == "MEAN":
        a.update(keep_dims=bool(get(0, "<b")))
    return a


def _axis(a, rank, what):
    a = int(a)
    if a < 0:
        a += rank
    if not 0 <= a < rank:
        raise ValueError(f"tflite: axis {a} of {what} is not a dimension of a rank-{rank} tensor")
    return rank - 1 - a


def _constant(tensors, i, what):
    if not 0 <= i < len(tensors) or tensors[i].data is None:
        raise ValueError(f"tflite: {what} must be a constant tensor")
    return tensors[i].data


def _convert_axes(op, tensors):
    """axes and permutations into Halide order; the operands that only carried them leave `inputs`"""
    k, a = op.kind, op.attrs

    def rank(i):
        if not 0 <= i < len(tensors):
            raise ValueError(f"tflite: {k} names tensor {i} of {len(tensors)}")
        return len(tensors[i].shape)

    if k == "CONCATENATION":
        a["axis"] = _axis(a["axis"], rank(op.outputs[0]), k)
    elif k == "SPLIT":      # inputs: axis, value
        a["axis"] = _axis(_constant(tensors, op.inputs[0], "SPLIT's axis").reshape(-1)[0], rank(op.inputs[1]), k)
        op.inputs = [op.inputs[1]]
    elif k == "SPLIT_V":    # inputs: value, size_splits, axis
        a["size_splits"] = _ints(_constant(tensors, op.inputs[1], "SPLIT_V's sizes").reshape(-1))
        a["axis"] = _axis(_constant(tensors, op.inputs[2], "SPLIT_V's axis").reshape(-1)[0], rank(op.inputs[0]), k)
        op.inputs = [op.inputs[0]]
    elif k == "GATHER":
        if a["batch_dims"] != 0:
            raise NotImplementedError("tflite: GATHER with batch_dims != 0")
        a["axis"] = _axis(a["axis"], rank(op.inputs[0]), k)
    elif k == "MEAN":
        r = rank(op.inputs[0])
        a["axes"] = sorted(_axis(v, r, k) for v in _constant(tensors, op.inputs[1], "MEAN's axes").reshape(-1))
        op.inputs = [op.inputs[0]]
    elif k == "TRANSPOSE":
        r = rank(op.inputs[0])
        perm = _ints(_constant(tensors, op.inputs[1], "TRANSPOSE's permutation").reshape(-1))
        if sorted(perm) != list(range(r)):
            raise ValueError(f"tflite: {perm} is no permutation of a rank-{r} tensor")
        order = [0] * r
        for i, p in enumerate(perm):
            order[r - 1 - i] = r - 1 - p
        a["perm"], a["order"] = perm, order
        op.inputs = [op.inputs[0]]
    elif k == "PAD":
        r = rank(op.inputs[0])
        pads = _constant(tensors, op.inputs[1], "PAD's paddings").reshape(-1, 2)
        if len(pads) != r:
            raise ValueError(f"tflite: PAD has {len(pads)} padding pairs for a rank-{r} tensor")
        a["padding"] = [(int(b), int(e)) for b, e in pads[::-1]]   # Halide order
        op.inputs = [op.inputs[0]]
    elif k == "RESHAPE":
        # the shape comes in the options table, as a constant second operand, or both: either form must describe the output tensor
        if not a["new_shape"] and len(op.inputs) > 1 and 0 <= op.inputs[1] < len(tensors) and tensors[op.inputs[1]].data is not None:
            a["new_shape"] = _ints(tensors[op.inputs[1]].data.reshape(-1))
        out = tensors[op.outputs[0]].shape[::-1] if 0 <= op.outputs[0] < len(tensors) else ()
        want = int(np.prod(out, dtype=np.int64))
        if a["new_shape"]:
            shape = list(a["new_shape"])
            if shape.count(-1) == 1:
                known = -int(np.prod(shape, dtype=np.int64))
                shape[shape.index(-1)] = want // known if known > 0 and want % known == 0 else -1
            if tuple(shape) != tuple(out):
                raise ValueError(f"tflite: RESHAPE to {a['new_shape']} but the output tensor has shape {list(out)}")
        a["new_shape"] = list(out)
        op.inputs = [op.inputs[0]]


def read(source) -> Graph:
    """The first subgraph of a .tflite file (a path, bytes or a bytes-like object)."""
    if isinstance(source, (bytes, bytearray, memoryview)):
        data = bytes(source)
    else:
        with open(source, "rb") as fh:
            data = fh.read()
    try:
        return _read(_File(data))
    except (IndexError, struct.error, OverflowError) as e:   # nothing below should get here; a ValueError all the same
        raise ValueError(f"tflite: malformed file ({e})") from e


def _read(f):
    if f.n < 8 or f.b[4:8] != b"TFL3":
        raise ValueError("tflite: not a TFL3 file")
    model = f.table(f.indirect(0))
    version = model.scalar(0, "<I")
    codes = []
    for oc in model.tables(1):
        code = max(oc.scalar(0, "<b"), oc.scalar(3, "<i"))   # the older files leave builtin_code at 0
        codes.append((code, oc.string(1)))
    buffers = model.tables(4)
    subgraphs = model.tables(2)
    if not subgraphs:
        raise ValueError("tflite: no subgraph")
    sg = subgraphs[0]
    tensors = []
    for t in sg.tables(0):
        shape = _ints(t.array(0, np.int32))
        code = t.scalar(1, "<b")
        if code not in _DTYPES:
            raise NotImplementedError(f"tflite: tensor type {code}")
        dtype = np.dtype(_DTYPES[code])
        if any(e < 0 for e in shape):
            raise ValueError(f"tflite: tensor shape {shape}")
        bi = t.scalar(2, "<I")
        data = None
        if bi:
            if bi >= len(buffers):
                raise ValueError(f"tflite: tensor names buffer {bi} of {len(buffers)}")
            raw = buffers[bi].array(0, np.uint8)
            if raw is not None and raw.size:
                want = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
                if raw.size != want:
                    raise ValueError(f"tflite: a constant of {raw.size} bytes for a tensor of {want}")
                data = raw.view(dtype.newbyteorder("<")).astype(dtype).reshape(shape)
        scale, zero = (), ()
        q = t.sub(4)
        if q is not None:
            s, z = q.array(2, np.float32), q.array(3, np.int64)
            scale = () if s is None else tuple(float(v) for v in s)
            zero = () if z is None else tuple(int(v) for v in z)
        tensors.append(Tensor(t.string(3), tuple(reversed(shape)), dtype, scale, zero, data))

    def ids(a, what, optional=False):
        out = _ints(a)
        for i in out:
            if not (0 <= i < len(tensors) or (optional and i == -1)):
                raise ValueError(f"tflite: {what} names tensor {i} of {len(tensors)}")
        return out

    ops = []
    for o in sg.tables(3):
        ci = o.scalar(0, "<I")
        if ci >= len(codes):
            raise ValueError(f"tflite: operator names code {ci} of {len(codes)}")
        code, custom = codes[ci]
        if code in _OPS_REFUSED:
            raise NotImplementedError(f"tflite: operator {_OPS_REFUSED[code]} ({code}) is not supported")
        if code not in OPS:
            raise NotImplementedError(f"tflite: operator code {code}{' (' + custom + ')' if custom else ''} is not supported")
        kind = OPS[code]
        op = Op(kind, ids(o.array(1, np.int32), kind, True), ids(o.array(2, np.int32), kind))
        if not op.inputs or not op.outputs or op.inputs[0] < 0:
            raise ValueError(f"tflite: {kind} without operands")
        op.attrs = _options(kind, o.sub(4), o.scalar(3, "<B"))
        need = {"SPLIT": 2, "SPLIT_V": 3, "MEAN": 2, "TRANSPOSE": 2, "PAD": 2, "GATHER": 2, "CONV_2D": 2, "DEPTHWISE_CONV_2D": 2, "FULLY_CONNECTED": 2,
                "ADD": 2, "SUB": 2, "MUL": 2}.get(kind, 1)
        if len(op.inputs) < need or any(i < 0 for i in op.inputs[:need]):
            raise ValueError(f"tflite: {kind} with {len(op.inputs)} operands")
        _convert_axes(op, tensors)
        used = [tensors[i] for i in op.inputs + op.outputs if i >= 0]
        if kind not in COPY_OPS and any(t.dtype == np.float32 for t in used):
            raise NotImplementedError(f"tflite: operator {kind} on float tensors is not supported (only the quantized form)")
        ops.append(op)
    return Graph(tensors, ops, ids(sg.array(1, np.int32), "the subgraph's inputs"), ids(sg.array(2, np.int32), "the subgraph's outputs"), sg.string(4),
                 version)
