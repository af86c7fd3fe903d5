"""compositing: Porter-Duff blending of six RGBA layers by five run-time op codes (apps/compositing).

The contract is the generator's INTEGER form (uint16 colour, uint8 alpha; include/hlmi_pipelines.h).  The checker is
tests/cpp/compositing_check.c, a plain C restatement of apps/compositing/compositing_generator.cpp:25-154, built and driven through
ctypes by tests/compositing_checker.py.  The CPU tests hold the checker to an independent numpy evaluation (int64 with explicit
masks, `//` with the zero and one denominators written out) and the entry point to its contract; the GPU tests hold the library to
the checker bit for bit, on the default path and on the one-thread-per-pixel path.  No float operation is involved, so the same
bytes are expected of both library builds."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import compositing_checker as cc
from parity_helpers import ROOT, RUNGEN, call_argv, call_direct, load_fuzz_parity
from parity_helpers import gpu_present as _gpu_present, launches as _launches, same_bits as _same

u8, i32, i64 = np.uint8, np.int32, np.int64
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
OUT_OF_RANGE = [-1, 5, INT32_MIN, INT32_MAX]
VALS = np.array([0, 1, 127, 128, 254, 255], u8)
NAME = "compositing"


# ---------------------------------------------------------------------------------------------------- the independent evaluation
def _np_scale16(a, s):
    c = a * s
    c = c + ((c + 128) >> 8)
    return ((c + 128) >> 8) & 0xffff


def _np_scale8(a, s):
    c = (a * s) & 0xffff
    c = (c + (((c + 128) & 0xffff) >> 8)) & 0xffff
    return (((c + 128) & 0xffff) >> 8) & 0xff


def _np_eval(layers, ops, raw=False):
    """the operator table of include/hlmi_pipelines.h in int64; raw: the three quotients before the saturation as well"""
    L = [np.asarray(l).astype(i64) for l in layers]
    Cs, A = [L[0][i] * L[0][3] for i in range(3)], L[0][3].copy()
    for k in range(1, 6):
        op, B3 = int(ops[k - 1]), L[k][3]
        Bc = [L[k][i] * B3 for i in range(3)]
        nb, na = 255 - B3, 255 - A
        if op == 0:
            Cs, A = [(Bc[i] + _np_scale16(Cs[i], nb)) & 0xffff for i in range(3)], (B3 + _np_scale8(A, nb)) & 0xff
        elif op == 1:
            Cs = [(_np_scale16(Bc[i], A) + _np_scale16(Cs[i], nb)) & 0xffff for i in range(3)]
        elif op == 2:
            Cs, A = [(_np_scale16(Bc[i], na) + _np_scale16(Cs[i], nb)) & 0xffff for i in range(3)], (_np_scale8(B3, na) + _np_scale8(A, nb)) & 0xff
        elif op == 3:
            Cs, A = [_np_scale16(Cs[i], B3) for i in range(3)], _np_scale8(A, B3)
        elif op == 4:
            Cs, A = [_np_scale16(Cs[i], nb) for i in range(3)], _np_scale8(A, nb)
    q = []
    for i in range(3):
        n = (Cs[i] + A // 2) & 0xffff
        q.append(np.where(A == 0, 0, np.where(A == 1, n, n // np.maximum(A, 1))))
    out = np.stack([np.minimum(x, 255) for x in q] + [A]).astype(u8)
    return (out, np.stack(q)) if raw else out


def _noise_layers(w, h, seed, n=6):
    """n (4, h, w) uint8 layers of noise whose alpha planes hold 0, 1 and 255 often"""
    rng = np.random.default_rng(seed)
    layers = []
    for _ in range(n):
        l = rng.integers(0, 256, (4, h, w), dtype=u8)
        pick = rng.integers(0, 8, (h, w))
        l[3] = np.where(pick == 0, 0, np.where(pick == 1, 255, np.where(pick == 2, 1, l[3])))
        layers.append(l)
    return layers


@pytest.fixture(scope="module")
def alpha_pairs():
    """256 x 256, the state's alpha A along x and the incoming layer's B3 along y: every pair.  The colour planes of both layers
    take 0, 1, 127, 128, 254 and 255.  With the operator first and the other four codes out of range, layers 2 .. 5 (noise) are not
    folded.  Returns (layers, {op: the checker's output}), computed once and never written to."""
    x, y = np.meshgrid(np.arange(256), np.arange(256))
    l0 = np.stack([VALS[(7 * x + 3 * y + c) % 6] for c in range(3)] + [x.astype(u8)])
    l1 = np.stack([VALS[(5 * x + y + 2 * c + 1) % 6] for c in range(3)] + [y.astype(u8)])
    layers = [l0, l1] + _noise_layers(256, 256, 3, 4)
    for l in layers:
        l.setflags(write=False)
    want = {op: cc.run(layers, [op] + OUT_OF_RANGE) for op in range(5)}
    for v in want.values():
        v.setflags(write=False)
    return layers, want


def _driver_scene(w, h, seed=1):
    """apps/compositing/process.cpp:33-51 on a w x h image: the input (here noise, alpha included) under a ring of five coloured blobs,
    op codes {4, 3, 2, 1, 0}.  The ring's radius (300) and the blobs' half width (500) scale with w / 1536; the alpha ramp is
    steepened by 1536 // w so that a small scene keeps what the driver's has: opaque cores, ramps and transparent ground."""
    k = max(1536 // w, 1)
    layers = [np.random.default_rng(seed).integers(0, 256, (4, h, w), dtype=u8)]
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    for i in range(5):
        cx, cy = int(np.cos(i * 2 * np.pi / 5) * 300 / k + w // 2), int(np.sin(i * 2 * np.pi / 5) * 300 / k + h // 2)
        alpha = np.minimum(255, k * np.minimum(np.maximum(0, 500 // k - np.abs(x - cx)), np.maximum(0, 500 // k - np.abs(y - cy))))
        b = np.zeros((4, h, w), u8)
        b[0], b[1], b[3] = 255, ((255 // 3) * i) & 255, alpha   # the driver stores 85 i into a uint8: 340 wraps to 84
        b[2] = 255 - b[1]
        layers.append(b)
    return layers, np.array([4, 3, 2, 1, 0], i32)


# ---------------------------------------------------------------------------------------------------- CPU: checker vs numpy
@pytest.mark.parametrize("op", range(5), ids=cc.OPS)
def test_checker_equals_numpy_on_every_alpha_pair(alpha_pairs, op):
    layers, want = alpha_pairs
    assert sorted(set(layers[0][:3].ravel())) == sorted(VALS) and sorted(set(layers[1][:3].ravel())) == sorted(VALS)
    assert np.array_equal(layers[0][3][0], np.arange(256)) and np.array_equal(layers[1][3][:, 0], np.arange(256))
    _same(want[op], _np_eval(layers, [op] + OUT_OF_RANGE), cc.OPS[op])
    if op != 1:   # every operator but atop changes alpha somewhere, and all change a colour
        assert not np.array_equal(want[op][3], layers[0][3])
    assert not np.array_equal(want[op][:3], cc.run(layers, OUT_OF_RANGE + [7])[:3])


def test_the_trap_scale16_is_the_two_shift_form_not_a_division_by_255():
    """The generator's comment (:64) says scale is (c + 127) / 255.  For a uint16 `a` it is not: over the reachable pairs a <= 65025,
    s <= 255 the two-shift form is one lower on 4 096 162 of 16 646 656, first at c = 65663, and never differs otherwise.  For a
    uint8 `a` (c <= 65025) the comment holds on all 65536 pairs."""
    a, s = np.meshgrid(np.arange(65026, dtype=np.uint16), np.arange(256, dtype=u8), indexing="ij")
    two, div = cc.scale16_sweep(a, s)
    c = a.astype(i64) * s.astype(i64)
    t = c + ((c + 128) >> 8)
    assert np.array_equal(two, ((t + 128) >> 8).astype(np.uint16))
    assert np.array_equal(div, ((c + 127) // 255).astype(np.uint16))
    d = two.astype(i64) - div.astype(i64)
    assert a.size == 16646656 and np.count_nonzero(d) == 4096162
    assert d.min() == -1 and d.max() == 0
    assert int(c[d != 0].min()) == 65663
    a8, s8 = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    got8 = np.array([[cc.scale8(p, q) for q in range(256)] for p in range(256)])
    assert np.array_equal(got8, (a8 * s8 + 127) // 255) and np.array_equal(got8, _np_scale8(a8.astype(i64), s8.astype(i64)))
    assert np.array_equal(got8, two[:256])   # scale16 on a uint8 value is scale8


def test_the_division_is_total():
    """fast_integer_divide: 0 for a zero denominator, the numerator for 1, the floor quotient otherwise"""
    for n in (0, 1, 254, 255, 256, 32767, 32768, 65534, 65535):
        assert cc.divide(n, 0) == 0 and cc.divide(n, 1) == n
        for d in (2, 3, 127, 128, 254, 255):
            assert cc.divide(n, d) == n // d


def test_alpha_0_gives_colour_0_and_alpha_1_the_numerator():
    layers = _noise_layers(64, 4, 9)
    layers[0][3, :, :32], layers[0][3, :, 32:] = 0, 1
    out = cc.run(layers, OUT_OF_RANGE + [-7])
    assert not out[:, :, :32].any()                       # colour 0, alpha 0
    assert np.array_equal(out[:3, :, 32:], layers[0][:3, :, 32:]) and (out[3, :, 32:] == 1).all()   # (v * 1 + 0) / 1
    # `out` under an opaque layer (the driver's first step) zeroes alpha, and whatever follows an `in` keeps it there
    layers[1][3] = 255
    out = cc.run(layers, [4, 3, -1, 5, 9])
    assert not out.any()
    _same(out, _np_eval(layers, [4, 3, -1, 5, 9]), "alpha 0")


def test_a_quotient_above_255_saturates(alpha_pairs):
    """255 * round(q / 255) can be below q: after `over` a colour can exceed 255 * A, by 127 at the most"""
    layers, want = alpha_pairs
    out, q = _np_eval(layers, [0] + OUT_OF_RANGE, raw=True)
    over = q > 255
    assert over.any() and (out[:3][over] == 255).all() and (want[0][:3][over] == 255).all()
    # one such pixel by hand: state (255, A = 8) over (255, B3 = 16): C = 255 * 16 + scale16(255 * 8, 239) = 4080 + 1912 = 5992,
    # A = 16 + scale8(8, 239) = 16 + 7 = 23; 255 * 23 = 5865 is 127 below C, and (5992 + 11) / 23 = 261
    assert cc.scale16(255 * 8, 239) == 1912 and cc.scale8(8, 239) == 7 and (5992 + 23 // 2) // 23 == 261
    px = lambda v, a: np.array([v, v, v, a], u8).reshape(4, 1, 1)
    one = [px(255, 8), px(255, 16)] + [px(9, 9)] * 4
    assert cc.run(one, [0] + OUT_OF_RANGE).ravel().tolist() == [255, 255, 255, 23]
    assert _np_eval(one, [0] + OUT_OF_RANGE, raw=True)[1].ravel().tolist() == [261, 261, 261]
    assert 256 <= q.max() <= 255 + 128   # C <= 255 A + 127, so the quotient stays below 255 + 127 / A + 1


@pytest.mark.parametrize("code", OUT_OF_RANGE + [6, -5, 1 << 20], ids=str)
def test_an_op_code_outside_0_to_4_leaves_the_state_alone(code):
    layers = _noise_layers(37, 5, 11)
    base = cc.run(layers, [2, 0, 1, 4, 3])
    for k in range(5):   # replacing operator k by the code == dropping layer k + 1
        ops = [2, 0, 1, 4, 3]
        ops[k] = code
        other = list(layers)
        other[k + 1] = np.zeros_like(layers[0])   # what the skipped layer holds does not matter
        got = cc.run(layers, ops)
        _same(got, cc.run(other, ops), f"code {code} at {k}")
        _same(got, _np_eval(layers, ops), f"code {code} at {k}")
        assert not np.array_equal(got, base)


def test_five_out_of_range_codes_give_layer_0_premultiplied_and_normalised():
    layers = _noise_layers(67, 9, 12)
    out = cc.run(layers, OUT_OF_RANGE + [5])
    a = layers[0][3]
    # (v * a + a / 2) / a == v for every a >= 1, colour 0 at alpha 0
    _same(out, np.concatenate([np.where(a > 0, layers[0][:3], 0).astype(u8), a[None]]), "layer 0")
    _same(out, _np_eval(layers, OUT_OF_RANGE + [5]), "layer 0 vs numpy")


def test_checker_equals_numpy_on_random_op_sequences():
    layers = _noise_layers(67, 9, 13)
    rng = np.random.default_rng(5)
    for _ in range(64):
        ops = rng.integers(-1, 6, 5)
        _same(cc.run(layers, ops), _np_eval(layers, ops), str(ops))


def test_every_result_is_formed_from_the_old_state():
    """a tuple assignment: xor's alpha uses the old alpha on both sides, atop's colours the old alpha although alpha stays"""
    px = lambda v, a: np.array([v, v // 2, 255 - v, a], u8).reshape(4, 1, 1)
    for a, b3 in ((200, 100), (1, 255), (255, 1), (77, 77)):
        layers = [px(250, a), px(90, b3)] + [px(0, 0)] * 4
        for op in range(5):
            _same(cc.run(layers, [op] + OUT_OF_RANGE), _np_eval(layers, [op] + OUT_OF_RANGE), f"{cc.OPS[op]} {a} {b3}")


# ---------------------------------------------------------------------------------------------------- CPU: the library's surface
ARG_NAMES = [f"layer_rgba_{i}" for i in range(6)] + ["ops", "output"]


def test_the_entry_point_is_exported_with_argv_and_metadata(hl):
    lib = C.CDLL(hl.LIB_PATH)
    for suffix in ("", "_argv", "_metadata"):
        assert hasattr(lib, NAME + suffix), NAME + suffix
    assert not hasattr(lib, NAME + "_auto_schedule")
    assert hasattr(lib, "hlmi_compositing_general") and hasattr(lib, "hlmi_debug_compositing")
    assert hl._fn[NAME] is not None and callable(hl.compositing) and callable(hl.debug_compositing_general)


def test_metadata_states_the_eight_arguments(hl):
    md = hl.metadata(NAME)
    assert md.version == 1 and md.num_arguments == 8 and md.name.decode() == NAME and b"hip" in md.target
    a = [md.arguments[i] for i in range(8)]
    assert [x.name.decode() for x in a] == ARG_NAMES
    assert [x.kind for x in a] == [1] * 7 + [2]
    assert [(x.type.code, x.type.bits) for x in a] == [(1, 8)] * 6 + [(0, 32), (1, 8)]
    assert [x.dimensions for x in a] == [3] * 6 + [1, 3]
    est = lambda x: [x.buffer_estimates[i][0] for i in range(2 * x.dimensions)]
    for x in a[:6] + a[7:]:
        assert est(x) == [0, 1536, 0, 2560, 0, 4], x.name
    assert est(a[6]) == [0, 5]
    for x in a:
        assert not x.scalar_def and not x.scalar_min and not x.scalar_max and not x.scalar_estimate


def test_the_aot_header_compiles_as_c(tmp_path):
    decl = " ".join(open(os.path.join(ROOT, "include", "hlmi_pipelines.h")).read().split())
    B = "struct halide_buffer_t *"
    assert "int compositing(" + ", ".join(B + n for n in ARG_NAMES) + ");" in decl
    src = tmp_path / "c.c"
    sig = ", ".join([B.strip()] * 8)
    src.write_text(f'#include "aot/compositing.h"\nint (*const f)({sig}) = compositing;\nint (*const a)(void **) = compositing_argv;\n'
                   "const struct halide_filter_metadata_t *(*const m)(void) = compositing_metadata;\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "c.o")], check=True)


def test_runner_describes_it_by_name():
    out = subprocess.run([RUNGEN, f"--name={NAME}", "--describe"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    for i in range(6):
        assert f'Input "layer_rgba_{i}" is of type Buffer<uint8> with 3 dimensions' in out.stdout
    assert 'Input "ops" is of type Buffer<int32> with 1 dimensions' in out.stdout
    assert 'Output "output" is of type Buffer<uint8> with 3 dimensions' in out.stdout


# ---------------------------------------------------------------------------------------------------- CPU: the entry protocol
HOW = pytest.mark.parametrize("how", [call_direct, call_argv], ids=["direct_call", "argv"])
W0, H0 = 20, 6


def _mk(hl, shape=(4, H0, W0), dtype=u8, mins=None):
    return hl.Buffer(np.zeros(shape, dtype), mins=mins)


def _call(hl, how, **over):
    """the entry point on six W0 x H0 layers, five codes and a W0 x H0 output, with the named arguments replaced"""
    args = {n: _mk(hl) for n in ARG_NAMES}
    args["ops"] = _mk(hl, (5,), i32)
    args.update(over)
    return how(hl, NAME, *[args[n] for n in ARG_NAMES])


@HOW
def test_entry_protocol(hl, how):
    ok = 0 if _gpu_present() else -29   # with everything in order only the device can be missing
    call = lambda **over: _call(hl, how, **over)
    assert call() == ok
    for n in ARG_NAMES:
        assert call(**{n: None}) == -12 and n in hl.last_error()
    for n in ARG_NAMES:
        assert call(**{n: _mk(hl, (4, H0, W0) if n != "ops" else (5,), np.uint16)}) == -3 and n in hl.last_error()
    assert call(ops=_mk(hl, (5,), np.float32)) == -3 and call(ops=_mk(hl, (5,), np.uint32)) == -3
    for n in ARG_NAMES:
        assert call(**{n: _mk(hl, (H0, W0) if n != "ops" else (1, 5), i32 if n == "ops" else u8)}) == -43 and n in hl.last_error()
    # order: null, then a buffer's type, then its dimensionality, then the constraint, then sizes and coverage
    assert call(layer_rgba_2=None, output=_mk(hl, dtype=np.uint16)) == -12
    assert call(layer_rgba_1=_mk(hl, (H0, W0), np.uint16)) == -3
    assert call(layer_rgba_1=_mk(hl, (H0, W0)), output=_mk(hl, (3, H0, W0))) == -43
    assert call(layer_rgba_1=_mk(hl, (4, H0, W0 - 1)), output=_mk(hl, (3, H0, W0))) == -8 and "output.extent.2" in hl.last_error()
    strided = lambda: hl.Buffer(np.zeros((4, H0, 2 * W0), u8)[..., ::2])   # stride.0 == 2
    assert call(layer_rgba_3=strided()) == -8 and "layer_rgba_3.stride.0" in hl.last_error()
    assert call(output=strided()) == -8 and "output.stride.0" in hl.last_error()
    assert call(layer_rgba_3=strided(), layer_rgba_0=_mk(hl, (4, H0, W0 - 1))) == -8   # a constraint before coverage
    # nothing is clamped: each layer covers the output's x, y box and channels [0, 4), ops covers [0, 5)
    for n in ARG_NAMES[:6]:
        for bad in (_mk(hl, (4, H0, W0 - 1)), _mk(hl, (4, H0 - 1, W0)), _mk(hl, (3, H0, W0)), _mk(hl, mins=(1, 0, 0)), _mk(hl, mins=(0, -1, 0)),
                    _mk(hl, mins=(0, 0, 1)), _mk(hl, (5, H0, W0), mins=(0, 0, -2))):
            assert call(**{n: bad}) == -4 and n in hl.last_error(), n
    assert call(ops=_mk(hl, (4,), i32)) == -4 and "ops" in hl.last_error()
    assert call(ops=_mk(hl, (5,), i32, mins=(1,))) == -4 and call(ops=_mk(hl, (5,), i32, mins=(-1,))) == -4
    # larger layers with their own mins, a longer ops, an output at a non-zero min: in order
    assert call(layer_rgba_4=_mk(hl, (6, H0 + 5, W0 + 9), mins=(2, -1, -1)), output=_mk(hl, mins=(7, 1, 0)),
                **{n: _mk(hl, (4, H0 + 3, W0 + 9)) for n in ARG_NAMES[:4]}, layer_rgba_5=_mk(hl, (4, H0 + 1, W0 + 7)),
                ops=_mk(hl, (9,), i32, mins=(-3,))) == ok
    # nothing is read where the output is empty in x or y
    tiny = {n: _mk(hl, (4, 1, 1), mins=(50, 50, 0)) for n in ARG_NAMES[:6]}
    sliced = lambda shape, dtype, cut: hl.Buffer(np.zeros(shape, dtype)[cut])   # an empty view: the strides stay
    assert call(output=sliced((4, H0, W0), u8, np.s_[:, :, :0]), ops=sliced((5,), i32, np.s_[:0]), **tiny) == ok
    assert call(output=sliced((4, H0, W0), u8, np.s_[:, :0]), **tiny) == ok


@HOW
def test_the_output_holds_channels_0_to_4(hl, how):
    """bound(c, 0, 4): all four channels are produced together, anything else is -8"""
    call = lambda **over: _call(hl, how, **over)
    wide = {n: _mk(hl, (8, H0, W0), mins=(0, 0, -2)) for n in ARG_NAMES[:6]}
    for shape, mins, what in (((3, H0, W0), None, "output.extent.2"), ((5, H0, W0), None, "output.extent.2"), ((1, H0, W0), (0, 0, 3), "output.min.2"),
                              ((4, H0, W0), (0, 0, 1), "output.min.2"), ((4, H0, W0), (0, 0, -1), "output.min.2"), ((0, H0, W0), None, "output.extent.2")):
        assert call(output=_mk(hl, shape, mins=mins), **wide) == -8, (shape, mins)
        assert what in hl.last_error()
    # held in a bounds query too: the constraint comes first
    q = hl.Buffer.bounds_query(u8, 3, extents=(W0, H0, 3))
    assert call(output=q) == -8


@HOW
def test_bounds_queries_answer_the_boxes_that_are_read(hl, how):
    dims = lambda b: [(b.raw.dim[i].min, b.raw.dim[i].extent) for i in range(b.raw.dimensions)]
    query = lambda n=3, dtype=u8: hl.Buffer.bounds_query(dtype, n, mins=(11, 12, 13)[:n], extents=(14, 15, 16)[:n])
    box = [(-3, W0), (2, H0), (0, 4)]
    out = lambda: _mk(hl, mins=(-3, 2, 0))
    for n in ARG_NAMES[:6]:   # one layer asked for
        q, o, other = query(), out(), _mk(hl, (4, 2, 2))
        assert _call(hl, how, output=o, **{n: q}, **{m: other for m in ARG_NAMES[:6] if m != n}) == 0
        assert dims(q) == box and dims(o) == box and dims(other) == [(0, 2), (0, 2), (0, 4)]
        assert [q.raw.dim[i].stride for i in range(3)] == [1, W0, W0 * H0]
    q, o = query(1, i32), out()
    assert _call(hl, how, ops=q, output=o) == 0 and dims(q) == [(0, 5)] and dims(o) == box
    # everything a query, the output shaped (RunGen's way): every input answered, the output as passed; a wrong type is rewritten
    qs = {n: query() for n in ARG_NAMES[:6]}
    qs["layer_rgba_2"] = query(3, np.float32)
    qo, qops = hl.Buffer.bounds_query(u8, 3, mins=(5, 6, 0), extents=(30, 40, 4)), query(1, np.uint16)
    assert _call(hl, how, output=qo, ops=qops, **qs) == 0
    assert all(dims(q) == [(5, 30), (6, 40), (0, 4)] for q in qs.values()) and dims(qops) == [(0, 5)] and dims(qo) == [(5, 30), (6, 40), (0, 4)]
    assert (qs["layer_rgba_2"].raw.type.code, qs["layer_rgba_2"].raw.type.bits) == (1, 8) and (qops.raw.type.code, qops.raw.type.bits) == (0, 32)
    # a query with the wrong dimensionality stays an error
    assert _call(hl, how, layer_rgba_0=query(2)) == -43


def test_without_a_gpu_the_python_calls_refuse_to_run(hl):
    layers, ops, o = [_mk(hl) for _ in range(6)], _mk(hl, (5,), i32), _mk(hl)
    with pytest.raises(ValueError):
        hl.compositing(layers[:5], ops, o)
    if _gpu_present():
        return   # what follows is the statement about a machine without one
    for fn in (hl.compositing, hl.debug_compositing_general):
        with pytest.raises(hl.HalideError) as e:
            fn(layers, ops, o)
        assert e.value.code == -29


def test_torch_op_shape_function_and_refusals():
    import torch
    import halide_amd.torch_ops  # noqa: F401
    op = torch.ops.hlmi.compositing
    meta = [torch.empty((4, 45, 70), dtype=torch.uint8, device="meta") for _ in range(6)]
    out = op(meta, torch.empty((5,), dtype=torch.int32, device="meta"))
    assert out.shape == (4, 45, 70) and out.dtype == torch.uint8
    layers, ops = [torch.zeros((4, 8, 8), dtype=torch.uint8) for _ in range(6)], torch.zeros(5, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU"):
        op(layers, ops)
    for bad_layers, bad_ops in ((layers[:5], ops), (layers, torch.zeros(5, dtype=torch.int64)), (layers, torch.zeros(4, dtype=torch.int32)),
                                (layers[:5] + [torch.zeros((4, 8, 9), dtype=torch.uint8)], ops), ([t.float() for t in layers], ops),
                                ([torch.zeros((3, 8, 8), dtype=torch.uint8) for _ in range(6)], ops)):
        with pytest.raises(TypeError):
            op(bad_layers, bad_ops)


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(params=["default", "general"])
def general(request):
    """Both implementations (halide_amd/csrc/compositing.hip): the one launch every shape takes, and one thread per pixel through
    the hook."""
    return request.param == "general"


def _place(shape, row_pad=0, plane_pad=0, x0=0):
    """a zeroed uint8 array of `shape` ((4, H, W) or larger) inside one allocation: rows row_pad longer than W, planes plane_pad bytes
    apart beyond their rows, the first element x0 bytes into the allocation"""
    c, h, w = shape
    rs = w + row_pad
    cs = rs * h + plane_pad
    flat = np.zeros(x0 + c * cs + 8, u8)
    return np.lib.stride_tricks.as_strided(flat[x0:], shape, (cs, rs, 1))


def _run(hl, bufs, ops, o, general):
    (hl.debug_compositing_general if general else hl.compositing)(bufs, ops, o)


def _gpu(hl, layers, ops, general=False, layout=(0, 0, 0), out_layout=None):
    """the call on host buffers of the given layout (row_pad, plane_pad, x0), everything at min 0; returns the output, contiguous"""
    bufs = []
    for l in layers:
        a = _place(l.shape, *layout)
        a[...] = l
        bufs.append(hl.Buffer(a))
    o = hl.Buffer(_place(layers[0].shape, *(layout if out_layout is None else out_layout)))
    _run(hl, bufs, hl.Buffer(np.ascontiguousarray(ops, i32)), o, general)
    return np.ascontiguousarray(o.numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("op", range(5), ids=cc.OPS)
def test_every_alpha_pair_on_the_gpu(hl, alpha_pairs, on_stream, general, op):
    layers, want = alpha_pairs
    _same(_gpu(hl, layers, [op] + OUT_OF_RANGE, general), want[op], cc.OPS[op])


@pytest.mark.gpu
def test_the_drivers_sequence_on_the_drivers_blobs(hl, on_stream, general):
    layers, ops = _driver_scene(160, 96)
    assert ops.tolist() == [4, 3, 2, 1, 0]
    for b in layers[1:]:   # opaque cores, ramps and transparent ground
        assert (b[3] == 255).any() and (b[3] == 0).any() and ((b[3] > 0) & (b[3] < 255)).any()
    want = cc.run(layers, ops)
    assert (want[3] == 0).any()   # `out` first zeroes alpha under the first blob's core: the float form's 0 * inf
    _same(_gpu(hl, layers, ops, general), want, "driver")


@pytest.mark.gpu
def test_64_random_op_sequences(hl, general):
    layers = _noise_layers(67, 9, 21)
    bufs = [hl.Buffer(l.copy()) for l in layers]
    rng = np.random.default_rng(64)
    seen = set()
    for _ in range(64):
        ops = rng.integers(-1, 6, 5).astype(i32)
        seen.update(ops.tolist())
        o = hl.Buffer(np.zeros_like(layers[0]))
        _run(hl, bufs, hl.Buffer(ops), o, general)
        _same(o.numpy(), cc.run(layers, ops), str(ops))
    assert seen == set(range(-1, 6))


# A wave owns 512 pixels of one row, a lane 8, a workgroup 4 rows.  1 .. 257: the per-byte path, one lane, lanes whose run crosses the
# row's end, several lanes; 512, 513 and 1029: one whole wave on the 8-byte path, one beside a single pixel, two beside a partial third.
# Heights 1, 2, 9: one wave, two, three workgroups in y.
WIDTHS = [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257, 512, 513, 1029]
HEIGHTS = [1, 2, 9]
# (row_pad, plane_pad, x0): dense; rows of width + 1 and width + 3 (rows start unaligned, 8-byte accesses are legal on some rows only),
# channel strides that are no multiple of 4, a first element off the 8-byte grid
LAYOUTS = [(0, 0, 0), (1, 0, 0), (3, 1, 0), (0, 2, 0), (0, 0, 3), (3, 5, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("w", WIDTHS)
def test_widths_heights_and_strides(hl, general, w):
    for h in HEIGHTS:
        layers = _noise_layers(w, h, 100 * w + h)
        ops = [(w + h + k) % 5 for k in range(5)]
        want = cc.run(layers, ops)
        for layout in LAYOUTS:
            if (h * (w + layout[0]) + layout[1]) % 4 == 0 and layout[1]:
                layout = (layout[0], layout[1] + 1, layout[2])
            _same(_gpu(hl, layers, ops, general, layout), want, f"{w} x {h} layout {layout}")
        # the inputs on the 8-byte grid and the output off it, and the reverse
        _same(_gpu(hl, layers, ops, general, (0, 0, 0), (1, 3, 0)), want, f"{w} x {h} output unaligned")
        _same(_gpu(hl, layers, ops, general, (3, 1, 0), (0, 0, 0)), want, f"{w} x {h} inputs unaligned")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(67, 9), (1040, 5)], ids=["67x9", "1040x5"])
def test_every_layer_its_own_box_and_strides(hl, on_stream, general, w, h):
    """the output at a non-zero min; every layer larger than it, each with other mins, extents, row and channel strides (one with
    channels [-1, 5)); ops longer than five with a negative min"""
    ox, oy = 8, -3
    rng = np.random.default_rng(w)
    bufs, crops = [], []
    for k in range(6):
        mx, my, mc = ox - 8 * (k % 3), oy - k, (-1 if k == 4 else 0)
        ew, eh, ec = w + (ox - mx) + 8 * (k % 2) + (k == 5), h + (oy - my) + k % 2, (6 if k == 4 else 4)
        a = _place((ec, eh, ew), row_pad=(0, 0, 3, 8, 1, 0)[k], plane_pad=(0, 8, 1, 0, 2, 16)[k], x0=(0, 8, 0, 0, 5, 16)[k])
        a[...] = rng.integers(0, 256, a.shape, dtype=u8)
        bufs.append(hl.Buffer(a, mins=(mx, my, mc)))
        crops.append(a[0 - mc:4 - mc, oy - my:oy - my + h, ox - mx:ox - mx + w].copy())
    opsa = rng.integers(-9, 9, 9).astype(i32)
    opsa[3:8] = [0, 2, 1, 4, 3]
    ops = hl.Buffer(opsa, mins=(-3,))
    for pad in (0, 5):
        o = hl.Buffer(_place((4, h, w), row_pad=pad), mins=(ox, oy, 0))
        _run(hl, bufs, ops, o, general)
        _same(np.ascontiguousarray(o.numpy()), cc.run(crops, opsa[3:8]), f"pad {pad}")


@pytest.mark.gpu
def test_one_buffer_as_all_six_layers(hl, general):
    for w, h in ((67, 9), (520, 3)):
        l = _noise_layers(w, h, 31, 1)[0]
        a = hl.Buffer(l.copy())
        for ops in ([0, 1, 2, 3, 4], [2, 2, 0, 4, 1]):
            o = hl.Buffer(np.zeros_like(l))
            _run(hl, [a] * 6, hl.Buffer(np.array(ops, i32)), o, general)
            _same(o.numpy(), cc.run([l] * 6, ops), f"{w} x {h} {ops}")


@pytest.mark.gpu
def test_default_equals_general_and_both_launch_what_they_say(hl):
    for w, h in ((1029, 9), (3, 1)):   # one launch for every shape
        layers = _noise_layers(w, h, 41)
        outs = {}
        for general, kernel in ((False, "comp_blend"), (True, "comp_general")):
            assert _launches(hl, lambda: outs.__setitem__(general, _gpu(hl, layers, [0, 1, 2, 3, 4], general))) == [kernel]
        _same(outs[False], outs[True], f"{w} x {h}")


@pytest.mark.gpu
def test_an_empty_output_launches_nothing(hl, general):
    layers = [hl.Buffer(np.zeros((4, 1, 1), u8)) for _ in range(6)]
    for cut in (np.s_[:, :, :0], np.s_[:, :0]):
        o = hl.Buffer(np.zeros((4, 5, 5), u8)[cut])   # an empty view: the strides stay
        assert _launches(hl, lambda: _run(hl, layers, hl.Buffer(np.zeros(5, i32)), o, general)) == []


@pytest.mark.gpu
def test_argv_equals_the_direct_call(hl, on_stream):
    layers, ops = _driver_scene(160, 24)
    outs = []
    for how in (call_direct, call_argv):
        o = hl.Buffer(np.zeros_like(layers[0]))
        assert how(hl, NAME, *[hl.Buffer(l.copy()) for l in layers], hl.Buffer(ops.copy()), o) == 0
        outs.append(np.ascontiguousarray(o.numpy()))
    _same(outs[1], outs[0], "argv")
    _same(outs[0], cc.run(layers, ops), "direct")


@pytest.mark.gpu
def test_torch_op_equals_the_checker(hl):
    import torch
    import halide_amd.torch_ops  # noqa: F401
    for w, h in ((160, 24), (1029, 5)):
        layers, ops = _noise_layers(w, h, 51), np.array([1, 0, 7, 2, 4], i32)
        ts = [torch.from_numpy(l).cuda() for l in layers]
        out = torch.ops.hlmi.compositing(ts, torch.from_numpy(ops).cuda())
        torch.cuda.synchronize()
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (4, h, w)
        _same(out.cpu().contiguous().numpy(), cc.run(layers, ops), f"torch {w} x {h}")
        assert all(np.array_equal(t.cpu().numpy(), l) for t, l in zip(ts, layers))


@pytest.mark.gpu
def test_calls_from_8_host_threads(hl):
    """eight threads on the library's shared stream, each with its own layers, op codes and size"""
    rng = np.random.default_rng(8)
    jobs = []
    for i in range(8):
        layers, ops = _noise_layers(500 + 9 * i, 6 + i, 60 + i), rng.integers(-1, 6, 5).astype(i32)
        jobs.append((layers, ops, cc.run(layers, ops)))
    errors = []

    def worker(i):
        try:
            layers, ops, want = jobs[i]
            for rep in range(4):
                o = hl.Buffer(np.zeros_like(layers[0]))
                _run(hl, [hl.Buffer(l.copy()) for l in layers], hl.Buffer(ops.copy()), o, rep % 2 == 1)
                if not np.array_equal(o.numpy(), want):
                    errors.append(f"thread {i} rep {rep}: differs")
        except Exception as e:  # noqa: BLE001
            errors.append(f"thread {i}: {e!r}")

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


# ---------------------------------------------------------------------------------------------------- GPU: the debug hook
def _device_math(hl, fn, a, b):
    f = hl.lib.hlmi_debug_compositing
    f.restype, f.argtypes = C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    a, b = np.ascontiguousarray(a, np.uint16), np.ascontiguousarray(b, u8)
    out = np.zeros(a.shape, np.uint16)
    assert f(fn, a.ctypes.data, b.ctypes.data, out.ctypes.data, a.size) == 0
    return out


@pytest.fixture(scope="module")
def all_pairs():
    """every (uint16, uint8) pair, 65536 x 256"""
    a, b = np.meshgrid(np.arange(65536, dtype=np.uint16), np.arange(256, dtype=u8), indexing="ij")
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


@pytest.mark.gpu
def test_the_devices_division_is_exact_on_every_pair(hl, all_pairs):
    """the reciprocal multiply of the normalise step against numpy's floor division: every numerator, every alpha, one launch"""
    n, d = all_pairs
    got = _device_math(hl, 0, n, d)
    n32, d32 = n.astype(np.uint32), d.astype(np.uint32)
    want = np.where(d32 == 0, 0, np.where(d32 == 1, n32, n32 // np.maximum(d32, 1))).astype(np.uint16)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} pairs differ, first (n, d) = {tuple(bad[0])}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


@pytest.mark.gpu
def test_the_devices_scale16_is_the_two_shift_form_on_every_pair(hl, all_pairs):
    a, s = all_pairs
    got = _device_math(hl, 1, a, s)
    c = a.astype(np.uint32) * s.astype(np.uint32)
    c += (c + 128) >> 8
    want = ((c + 128) >> 8).astype(np.uint16)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} pairs differ, first (a, s) = {tuple(bad[0])}"
    two, _ = cc.scale16_sweep(a[:65026], s[:65026])
    assert np.array_equal(got[:65026], two)   # and the checker's, over the reachable pairs


# ---------------------------------------------------------------------------------------------------- a seeded slice of the fuzzer
@pytest.mark.gpu
def test_seeded_fuzz_slice_of_compositing(on_stream):
    """scripts/fuzz_parity.py's compositing case, a fixed number of cases from a fixed seed"""
    mod = load_fuzz_parity()
    rng = np.random.default_rng(20261018)
    for i in range(40):
        desc, ok = mod.CASES["compositing"](rng)
        assert ok, f"case {i}: {desc}"
