"""resnet50_batch: N images per call, column n bit for bit what resnet50 writes for image n (a library extension: the reference's
generator has no batch dimension).

The contract is "per image, the bits of resnet50", so the checker is the one of tests/test_resnet50.py, tests/cpp/resnet50_check.c,
used per image; shapes, inputs and the network are that module's, imported, not restated.  The CPU tests hold the entry point to its
protocol, its metadata and its plan; the GPU tests hold the three batched hooks (every variant: the plan's choice, the general kernel and
each MFMA tile instance forced) and the whole call to the checker, image by image, bit for bit and NaN for NaN, at the smallest shapes
at which the batched indexing can go wrong: tiles that lie across images, images whose exterior taps fall on a neighbour's rows."""
import ctypes as C
import functools
import os
import subprocess
import threading

import numpy as np
import pytest

import resnet50_checker as rn
import test_resnet50 as base
from parity_helpers import ROOT, DevTensor, call_argv, call_direct, kernel_const
from parity_helpers import gpu_present as _gpu_present, launches as _launches, same_bits as _same, same_bits_or_nan as _same_or_nan

f32, u32 = np.float32, np.uint32
PAD_OF = base.PAD_OF

# the plan's constants, read from the source
KC, TILE, SHORT_K, SHORT_K_IMAGES, WIDE, WIDE_MIN_TILES, WIDE_ROUND, BATCH_CHUNK, FC_GROUP = (
    kernel_const("resnet50.hip", n) for n in ("KC", "TILE", "SHORT_K", "SHORT_K_IMAGES", "WIDE", "WIDE_MIN_TILES", "WIDE_ROUND", "BATCH_CHUNK", "FC_GROUP"))
MFMA, GENERAL, MFMA_WIDE = "resnet50_conv_mfma", "resnet50_conv_general", "resnet50_conv_mfma_wide"
OTHERS = ("resnet50_maxpool", "resnet50_avgpool", "resnet50_fc", "resnet50_softmax")
VARIANTS = (0, 1, 2, 3)   # the plan's choice, the general kernel, the 64 x 64 tile, the 64 x WIDE tile
NAME = "resnet50_batch"


@pytest.fixture(autouse=True)
def _checker_follows_the_library(hl):
    rn.set_canon(hl.canon_fma())
    yield


def _ceil(a, b):
    return -(-a // b)


def _expected_launch(hl, variant, co, K, pixels, images):
    """conv_plan() of resnet50.hip restated for a run over `images` images of `pixels` output pixels each; variant as the layer hook
    takes it"""
    if variant >= 2:
        return (MFMA, MFMA_WIDE)[variant - 2]
    if variant == 1 or not hl.canon_fma():
        return GENERAL
    if K <= SHORT_K and co <= TILE and images < SHORT_K_IMAGES:
        return GENERAL
    tiles = _ceil(co, TILE) * _ceil(images * pixels, WIDE)
    wide = images > 1 and tiles >= WIDE_MIN_TILES and not WIDE_ROUND < tiles < 2 * WIDE_ROUND
    return MFMA_WIDE if wide else MFMA


# ---------------------------------------------------------------------------------------------------- CPU: the library's surface
def test_the_entry_point_is_exported_with_argv_and_metadata(hl):
    lib = C.CDLL(hl.LIB_PATH)
    for sym in ("resnet50_batch", "resnet50_batch_argv", "resnet50_batch_metadata", "hlmi_resnet50_batch_general", "hlmi_debug_resnet50_layer_batch",
                "hlmi_debug_resnet50_maxpool_batch", "hlmi_debug_resnet50_tail_batch", "hlmi_debug_resnet50_batch_plan"):
        assert hasattr(lib, sym), sym
    assert not hasattr(lib, "resnet50_batch_auto_schedule")
    assert hl._fn[NAME] is not None and len(hl._fn[NAME].argtypes) == 269


def test_metadata_states_269_f32_buffers_in_signature_order(hl):
    md, one = hl.metadata(NAME), hl.metadata("resnet50")
    assert md.version == 1 and md.num_arguments == 269 and md.name.decode() == NAME and b"hip" in md.target
    a = [md.arguments[i] for i in range(269)]
    assert [x.name.decode() for x in a] == ["input"] + list(hl.RESNET50_PARAM_NAMES) + ["final_output"]
    assert [x.kind for x in a] == [1] * 268 + [2]
    assert all((x.type.code, x.type.bits) == (2, 32) for x in a)
    assert [x.dimensions for x in a] == [4] + [1] * 212 + [4] * 53 + [2, 1, 2]
    # two buffers differ from resnet50's, and only in their dimension count
    assert [i for i in range(269) if a[i].dimensions != one.arguments[i].dimensions] == [0, 268]
    assert not any(x.buffer_estimates for x in a)


def test_the_aot_header_compiles_as_c(tmp_path):
    src = tmp_path / "c.c"
    ptrs = ", ".join(["struct halide_buffer_t *"] * 269)
    src.write_text(f'#include "aot/resnet50_batch.h"\nint (*const f)({ptrs}) = resnet50_batch;\n'
                   "int (*const a)(void **) = resnet50_batch_argv;\nconst struct halide_filter_metadata_t *(*const m)(void) = resnet50_batch_metadata;\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "c.o")], check=True)


# ---------------------------------------------------------------------------------------------------- CPU: the entry protocol
NB = 2   # images of the protocol tests' buffers


def _box(i, n=NB):
    """numpy shape of argument i's box for a batch of n images"""
    return (n, 224, 224, 3) if i == 0 else (n, 1000) if i == 268 else base._box(i)


@functools.lru_cache(maxsize=None)
def _zero_args():
    """269 buffers over untouched zero pages: resnet50's own parameters, and the two buffers that differ"""
    import halide_amd as hl
    args = list(base._zero_args())
    args[0], args[268] = hl.Buffer(np.zeros(_box(0), f32)), hl.Buffer(np.zeros(_box(268), f32))
    return tuple(args)


def _call(hl, how, over=None):
    args = list(_zero_args())
    for i, v in (over or {}).items():
        args[i] = v
    return how(hl, NAME, *args)


_ok = base._ok
HOW = base.HOW
SAMPLE = base.SAMPLE


@HOW
def test_a_call_in_order_reaches_the_device(hl, how, monkeypatch):
    monkeypatch.delenv("HLMI_RN50_BATCH_CHUNK", raising=False)
    assert _call(hl, how) == _ok()


@HOW
@pytest.mark.parametrize("i", SAMPLE)
def test_a_null_argument_is_refused(hl, how, i):
    name = (["input"] + list(hl.RESNET50_PARAM_NAMES) + ["final_output"])[i]
    assert _call(hl, how, {i: None}) == -12 and name in hl.last_error()


@HOW
@pytest.mark.parametrize("i", SAMPLE)
def test_a_wrong_type_and_a_wrong_dimension_count_are_refused(hl, how, i):
    assert _call(hl, how, {i: hl.Buffer(np.zeros(_box(i), np.float64))}) == -3
    assert _call(hl, how, {i: hl.Buffer(np.zeros(_box(i), np.int32))}) == -3
    assert _call(hl, how, {i: hl.Buffer(np.zeros((1,) + _box(i), f32))}) == -43
    assert _call(hl, how, {7: None, i: hl.Buffer(np.zeros(_box(i), np.uint16))}) == -12   # null before type
    assert _call(hl, how, {i: hl.Buffer(np.zeros((1,) + _box(i), np.uint16))}) == -3    # type before dimension count


@HOW
def test_the_buffers_of_resnet50_itself_are_a_wrong_dimension_count(hl, how):
    assert _call(hl, how, {0: hl.Buffer(np.zeros((224, 224, 3), f32))}) == -43 and "input" in hl.last_error()
    assert _call(hl, how, {268: hl.Buffer(np.zeros(1000, f32))}) == -43 and "final_output" in hl.last_error()


@HOW
@pytest.mark.parametrize("i", SAMPLE[:-1])
def test_an_input_one_short_of_its_box_is_refused_and_a_larger_one_is_not(hl, how, i, monkeypatch):
    monkeypatch.delenv("HLMI_RN50_BATCH_CHUNK", raising=False)
    name = (["input"] + list(hl.RESNET50_PARAM_NAMES))[i]
    box = _box(i)
    for axis in range(len(box)):
        if box[axis] == 1:
            continue
        short = tuple(e - (a == axis) for a, e in enumerate(box))
        # (axis 0 of `input` is its images: one image short of final_output's range)
        assert _call(hl, how, {i: hl.Buffer(np.zeros(short, f32))}) == -4 and name in hl.last_error(), (i, axis)
    shifted = hl.Buffer(np.zeros(box, f32), mins=[1] + [0] * (len(box) - 1))
    assert _call(hl, how, {i: shifted}) == -4
    larger = tuple(e + 1 for e in box)
    assert _call(hl, how, {i: hl.Buffer(np.zeros(larger, f32), mins=[-1] * len(box))}) == _ok()
    padded = np.zeros(box[:-2] + (box[-2] + 1, box[-1] + 3) if len(box) > 1 else (box[0],), f32)
    view = padded[..., :box[-2], :box[-1]] if len(box) > 1 else padded
    assert _call(hl, how, {i: hl.Buffer(view)}) == _ok()


@HOW
def test_the_image_range_comes_from_the_output_and_the_input_must_cover_it(hl, how, monkeypatch):
    monkeypatch.delenv("HLMI_RN50_BATCH_CHUNK", raising=False)
    out = lambda n, bmin=0: hl.Buffer(np.zeros((n, 1000), f32), mins=[0, bmin])
    inp = lambda n, bmin=0: hl.Buffer(np.zeros((n, 224, 224, 3), f32), mins=[0, 0, 0, bmin])
    assert _call(hl, how, {0: inp(3), 268: out(2)}) == _ok()          # a larger input
    assert _call(hl, how, {0: inp(2), 268: out(3)}) == -4 and "input" in hl.last_error()   # one image short
    assert _call(hl, how, {0: inp(1), 268: out(1)}) == _ok()
    # a range with a non-zero min: images [5, 7)
    assert _call(hl, how, {0: inp(2, 5), 268: out(2, 5)}) == _ok()
    assert _call(hl, how, {0: inp(4, 4), 268: out(2, 5)}) == _ok()
    assert _call(hl, how, {0: inp(2, 4), 268: out(2, 5)}) == -4 and "input" in hl.last_error()   # [4, 6) does not cover image 6
    assert _call(hl, how, {0: inp(2, 0), 268: out(2, 5)}) == -4
    assert _call(hl, how, {0: inp(2, -3), 268: out(2, -3)}) == _ok()


@HOW
def test_an_output_box_inside_the_classes_is_taken_and_one_outside_is_refused(hl, how, monkeypatch):
    monkeypatch.delenv("HLMI_RN50_BATCH_CHUNK", raising=False)
    out = lambda n, cmin: hl.Buffer(np.zeros((NB, n), f32), mins=[cmin, 0])
    assert _call(hl, how, {268: out(10, 10)}) == _ok()
    assert _call(hl, how, {268: out(1, 999)}) == _ok()
    for cmin, n in ((991, 10), (-1, 5), (0, 1001), (1000, 1)):
        assert _call(hl, how, {268: out(n, cmin)}) == -4 and "fc1000_bias" in hl.last_error(), (cmin, n)
    b = hl.Buffer(np.zeros((NB, 1000, 2), f32)[:, :, 0])
    assert b.dim(0).stride == 2
    assert _call(hl, how, {268: b}) == -8 and "final_output.stride.0" in hl.last_error()
    # a padded column stride is a layout like any other
    assert _call(hl, how, {268: hl.Buffer(np.zeros((NB, 1003), f32)[:, :1000])}) == _ok()


@HOW
def test_a_bounds_query_answers_every_box_and_the_image_range(hl, how):
    dims = lambda b: [(b.raw.dim[d].min, b.raw.dim[d].extent) for d in range(b.raw.dimensions)]
    nd = lambda i: len(_box(i))
    fixed = lambda i, bmin, n: [(0, e) for e in reversed(_box(i, n))][:-1] + [(bmin, n)] if i in (0, 268) else [(0, e) for e in reversed(_box(i))]
    # the range from neither: [0, 1)
    q = [hl.Buffer.bounds_query(f32, nd(i)) for i in range(269)]
    assert how(hl, NAME, *q) == 0
    for i in range(269):
        assert dims(q[i]) == fixed(i, 0, 1), i
        assert q[i].raw.dim[0].stride == 1
    # from the output: a query with a shape keeps it, and the input follows its images
    q = [hl.Buffer.bounds_query(f32, nd(i)) for i in range(269)]
    q[268] = hl.Buffer.bounds_query(f32, 2, mins=[10, 5], extents=[10, 7])
    assert how(hl, NAME, *q) == 0
    assert dims(q[268]) == [(10, 10), (5, 7)] and dims(q[0]) == [(0, 3), (0, 224), (0, 224), (5, 7)] and dims(q[267]) == [(0, 1000)]
    # ... as it does for a real output
    qi = hl.Buffer.bounds_query(f32, 4)
    assert _call(hl, how, {0: qi, 268: hl.Buffer(np.zeros((3, 1000), f32), mins=[0, 2])}) == 0
    assert dims(qi) == [(0, 3), (0, 224), (0, 224), (2, 3)]
    # from the input: an output without a shape gets the input's images
    qo = hl.Buffer.bounds_query(f32, 2)
    assert _call(hl, how, {0: hl.Buffer(np.zeros((4, 224, 224, 3), f32), mins=[0, 0, 0, 3]), 268: qo}) == 0
    assert dims(qo) == [(0, 1000), (3, 4)]
    # one query buffer among real ones; a query of the wrong rank is refused
    for i in SAMPLE[1:-1]:
        qi = hl.Buffer.bounds_query(np.uint16, nd(i))
        assert _call(hl, how, {i: qi}) == 0
        assert dims(qi) == fixed(i, 0, NB) and (qi.raw.type.code, qi.raw.type.bits) == (2, 32)
        assert _call(hl, how, {i: hl.Buffer.bounds_query(f32, nd(i) + 1)}) == -43


@HOW
@pytest.mark.parametrize("value", ["0", "65", "-1"])
def test_a_chunk_size_outside_1_to_64_is_refused(hl, how, monkeypatch, value):
    monkeypatch.setenv("HLMI_RN50_BATCH_CHUNK", value)
    assert _call(hl, how) == -8 and "HLMI_RN50_BATCH_CHUNK" in hl.last_error()
    with pytest.raises(hl.HalideError) as e:
        hl.debug_resnet50_batch_plan(2)
    assert e.value.code == -8
    # resnet50 itself reads no such switch
    assert base._call(hl, how) == _ok()
    monkeypatch.setenv("HLMI_RN50_BATCH_CHUNK", "64")
    assert _call(hl, how) == _ok()


def test_without_a_gpu_the_python_calls_refuse_to_run(hl, monkeypatch):
    if _gpu_present():
        return   # the statement is about a machine without one
    monkeypatch.delenv("HLMI_RN50_BATCH_CHUNK", raising=False)
    args = _zero_args()
    for fn in (lambda: hl.resnet50_batch(args[0], args[1:-1], args[-1]), lambda: hl.debug_resnet50_batch_general(args[0], args[1:-1], args[-1]),
               lambda: hl.resnet50_batch(args[0], dict(zip(hl.RESNET50_PARAM_NAMES, args[1:-1])), args[-1])):
        with pytest.raises(hl.HalideError) as e:
            fn()
        assert e.value.code == -29
    x, wt, vec, res = base._layer_case(3, 8, 5, 7, 3, 1)
    B = lambda a: hl.Buffer(np.array(a))
    for variant in (0, 1):
        with pytest.raises(hl.HalideError) as e:
            hl.debug_resnet50_layer_batch(B(x[None]), B(wt), *[B(v) for v in vec], None, 1, 1, "scaled", B(np.zeros((1, 7, 5, 8), f32)), variant=variant)
        assert e.value.code == -29
    with pytest.raises(hl.HalideError) as e:
        hl.debug_resnet50_maxpool_batch(B(x[None]), 3, 2, 1, B(np.zeros((1, 4, 3, 3), f32)))
    assert e.value.code == -29
    with pytest.raises(hl.HalideError) as e:
        hl.debug_resnet50_tail_batch(B(x[None]), B(np.zeros((3, 4), f32)), B(np.zeros(4, f32)), B(np.zeros((1, 4), f32)))
    assert e.value.code == -29


def test_the_python_call_counts_and_names_its_parameters(hl):
    args = _zero_args()
    with pytest.raises(ValueError):
        hl.resnet50_batch(args[0], args[1:-2], args[-1])
    named = dict(zip(hl.RESNET50_PARAM_NAMES, args[1:-1]))
    named.pop("br2b_mu_7")
    with pytest.raises(ValueError, match="br2b_mu_7"):
        hl.resnet50_batch(args[0], named, args[-1])


def test_the_batched_hooks_refuse_what_does_not_fit(hl):
    x, wt, vec, res = base._layer_case(3, 8, 5, 7, 3, 1)
    B = lambda a: hl.Buffer(np.array(a))
    fn = hl.lib.hlmi_debug_resnet50_layer_batch
    fn.restype, fn.argtypes = C.c_int, [hl._BP] * 7 + [C.c_int32] * 4 + [hl._BP]
    two = lambda a: np.stack([a, a])
    good = dict(input=B(two(x)), weights=B(wt), gamma=B(vec[0]), beta=B(vec[1]), mu=B(vec[2]), sig=B(vec[3]), residual=None, output=B(np.zeros((2, 7, 5, 8), f32)))

    def run(stride=1, pad=1, mode=1, variant=0, **over):
        a = dict(good, **over)
        return fn(*[None if a[k] is None else a[k].ptr for k in ("input", "weights", "gamma", "beta", "mu", "sig", "residual")], stride, pad, mode, variant, a["output"].ptr)

    assert run() == _ok() and run(variant=1) == _ok()
    # an MFMA step is fused by construction: a forced tile instance exists in the fused build only
    assert run(variant=2) == run(variant=3) == (_ok() if hl.canon_fma() else -8)
    assert run(variant=4) == -8 and run(variant=-1) == -8 and "variant" in hl.last_error()
    assert run(input=B(x)) == -43 and run(output=B(np.zeros((7, 5, 8), f32))) == -43
    assert run(output=B(np.zeros((3, 7, 5, 8), f32))) == -8 and "output.extent.3" in hl.last_error()
    assert run(mode=3) == -12 and run(mode=3, residual=B(two(res))) == _ok() and run(mode=3, residual=B(res[None])) == -8
    assert run(gamma=None) == -12 and run(mode=4) == -8 and run(stride=0) == -8
    with pytest.raises(hl.HalideError) as e:
        hl.debug_resnet50_maxpool_batch(B(two(x)), 3, 2, 1, B(np.zeros((3, 4, 3, 3), f32)))
    assert e.value.code == -8
    with pytest.raises(hl.HalideError) as e:
        hl.debug_resnet50_tail_batch(B(two(x)), B(np.zeros((3, 4), f32)), B(np.zeros(4, f32)), B(np.zeros((3, 4), f32)))
    assert e.value.code == -8


# ---------------------------------------------------------------------------------------------------- CPU: the plan
def _plan_expected(hl, n, general=False):
    """the 57 steps of a run over n images, restated: (name, grid, tile) in launch order"""
    steps = []

    def conv(c):
        ci, co, k, stride, pad, size = base.CONVS[c]
        pixels = rn.out_extent(size, k, stride, pad) ** 2
        name = _expected_launch(hl, 1 if general else 0, co, k * k * ci, pixels, n)
        if name == GENERAL:
            steps.append((name, (_ceil(co * pixels * n, 256), 1), None))
        else:
            px = WIDE if name == MFMA_WIDE else TILE
            steps.append((name, (_ceil(co, TILE), _ceil(n * pixels, px)), (TILE, px)))

    conv(0)
    steps.append(("resnet50_maxpool", (_ceil(64 * 56 * 56 * n, 256), 1), None))
    for b in range(16):
        if b in (0, 3, 7, 13):
            conv(1 + (0, 3, 7, 13).index(b))
        conv(5 + b), conv(21 + b), conv(37 + b)
    steps += [("resnet50_avgpool", (_ceil(2048 * n, 256), 1), None), ("resnet50_fc", (_ceil(1000, 64), _ceil(n, FC_GROUP)), None),
              ("resnet50_softmax", (n, 1), None)]
    return steps


@pytest.mark.parametrize("general", [False, True], ids=["default", "general"])
def test_the_plan_of_a_batch(hl, general, monkeypatch):
    monkeypatch.delenv("HLMI_RN50_BATCH_CHUNK", raising=False)
    assert 1 <= BATCH_CHUNK <= 64
    for n in (1, 2, 3, BATCH_CHUNK, BATCH_CHUNK + 1):
        plan = hl.debug_resnet50_batch_plan(n, general=general)
        assert plan["chunk"] == BATCH_CHUNK
        sizes = [BATCH_CHUNK] * (n // BATCH_CHUNK) + ([n % BATCH_CHUNK] if n % BATCH_CHUNK else [])
        assert len(plan["chunks"]) == len(sizes)
        for steps, size in zip(plan["chunks"], sizes):
            assert len(steps) == 57
            assert [(s["name"], s["grid"], s["tile"]) for s in steps] == _plan_expected(hl, size, general), (n, size)
            if general or not hl.canon_fma():   # on the _nofma build every convolution runs the general kernel
                assert sum(s["name"] == GENERAL for s in steps) == 53
    # at one image: the names conv_plan() gives resnet50 today (tests/test_resnet50.py restates the predicate)
    one = hl.debug_resnet50_batch_plan(1, general=general)["chunks"][0]
    convs = [s["name"] for s in one if s["name"] not in OTHERS]
    order = [0] + sum((([1 + (0, 3, 7, 13).index(b)] if b in (0, 3, 7, 13) else []) + [5 + b, 21 + b, 37 + b] for b in range(16)), [])
    assert convs == [base._expected_launch(hl, base.CONVS[c][1], base.CONVS[c][2] ** 2 * base.CONVS[c][0], general) for c in order]
    assert MFMA_WIDE not in convs
    monkeypatch.setenv("HLMI_RN50_BATCH_CHUNK", "2")
    plan = hl.debug_resnet50_batch_plan(3, general=general)
    assert plan["chunk"] == 2 and [len(c) for c in plan["chunks"]] == [57, 57]
    assert [(s["name"], s["grid"], s["tile"]) for s in plan["chunks"][1]] == _plan_expected(hl, 1, general)


def test_the_plans_rule_on_both_sides_of_its_threshold(hl):
    """the predicate restated and the library's own answer (the plan hook), either side of each threshold: two co tiles and WIDE pixels
    per image make 2 n wide tiles of n images.  One image never runs the wide tile; the GPU tests reach that tile at small shapes by
    forcing it through the layer hook's variant, and the whole-network test by the plan's own choice."""
    if not hl.canon_fma():
        return
    for tiles, name in ((WIDE_MIN_TILES - 2, MFMA), (WIDE_MIN_TILES, MFMA_WIDE), (WIDE_ROUND, MFMA_WIDE), (WIDE_ROUND + 2, MFMA), (2 * WIDE_ROUND - 2, MFMA),
                        (2 * WIDE_ROUND, MFMA_WIDE)):
        assert _expected_launch(hl, 0, TILE + 1, SHORT_K, WIDE, tiles // 2) == name, tiles
    assert _expected_launch(hl, 0, TILE + 1, SHORT_K, WIDE * WIDE_MIN_TILES, 1) == MFMA
    # the short-K rule is a rule for few images: br2a of the first block (64 -> 64 at 56 x 56) is step 3 of the plan
    step = lambda n: hl.debug_resnet50_batch_plan(n)["chunks"][0][3]["name"]
    assert step(1) == step(SHORT_K_IMAGES - 1) == GENERAL and step(SHORT_K_IMAGES) == MFMA_WIDE and step(BATCH_CHUNK) == MFMA_WIDE
    # the network's own layers at three images: the stem has 294 wide tiles, the last stage's 3 x 3 layers 16
    names = [s["name"] for s in hl.debug_resnet50_batch_plan(3)["chunks"][0]]
    assert names[0] == MFMA_WIDE and names[-4] == MFMA and names.count(MFMA_WIDE) >= 5


def test_torch_shape_function_and_refusals(hl):
    import torch
    import halide_amd.torch_ops  # noqa: F401
    op = torch.ops.hlmi.resnet50_batch
    meta = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device="meta")
    params = [meta(base._box(i + 1)) for i in range(267)]
    for n in (1, 5):
        out = op(meta((n, 224, 224, 3)), params)
        assert out.shape == (n, 1000) and out.dtype == torch.float32
    cpu = [torch.zeros(base._box(i + 1)) for i in range(267)]
    with pytest.raises(RuntimeError, match="GPU"):
        op(torch.zeros((2, 224, 224, 3)), cpu)
    with pytest.raises(TypeError):
        op(torch.zeros((2, 224, 224, 3), dtype=torch.float64), cpu)
    with pytest.raises(TypeError):
        op(torch.zeros((2, 224, 224, 3)), cpu[:5] + [cpu[5].double()] + cpu[6:])
    with pytest.raises(TypeError):
        op(torch.zeros((2, 224, 224, 3)), cpu[:-1])
    with pytest.raises(TypeError):
        op(torch.zeros((224, 224, 3)), cpu)
    with pytest.raises(TypeError):
        op(torch.zeros((2, 3, 224, 224)), cpu)


# ---------------------------------------------------------------------------------------------------- GPU: arrays and cases
def _dev4(hl, shape, d, fill=None):
    """a (N, H, W, C) float32 array in a device allocation of the test's own: pixels C + d, rows (C + d) W + 2 d + 1 and images a padded
    plane + 3 d + 5 floats apart, the first element d floats off the 16-byte grid, every byte around it a sentinel (DevTensor.result()
    checks them); d = 0: dense and aligned"""
    n, h, w, c = shape
    if not d:
        return DevTensor(hl, shape, fill=fill, dtype=f32)
    sw = c + d
    sh = sw * w + 2 * d + 1
    sn = sh * h + 3 * d + 5
    return DevTensor(hl, shape, strides=(sn, sh, sw, 1), offset=4 * d, fill=fill, dtype=f32)


@functools.lru_cache(maxsize=None)
def _batch_case(shape, n, kind="noise"):
    """(inputs (N, H, W, CI), weights, vectors, residuals (N, OH, OW, CO)): image i is test_resnet50's layer case of seed 10 i; one set
    of weights and vectors, image 0's"""
    cases = [base._layer_case(*shape, kind=kind, seed=10 * i) for i in range(n)]
    x, res = np.stack([c[0] for c in cases]), np.stack([c[3] for c in cases])
    x.setflags(write=False), res.setflags(write=False)
    return x, cases[0][1], cases[0][2], res


def _conv_each(canon, x, wt, vec, res, stride, pad, mode):
    """the checker, image by image"""
    with rn.canon(canon):
        return np.stack([rn.conv(np.ascontiguousarray(x[i]), wt, *vec, residual=np.ascontiguousarray(res[i]), stride=stride, pad=pad, mode=mode) for i in range(len(x))])


@functools.lru_cache(maxsize=None)
def _batch_want(canon, shape, n, mode, kind="noise"):
    x, wt, vec, res = _batch_case(shape, n, kind)
    out = _conv_each(canon, x, wt, vec, res, shape[5], PAD_OF[shape[4]], mode)
    out.setflags(write=False)
    return out


def _run_layer(hl, x, wt, vec, res, stride, pad, mode, variant, layout=0):
    """one call of the batched layer hook on device arrays of the test's own (layout 0: dense, images back to back; 1 .. 3: padded rows,
    planes and images, each array with an image stride of its own, off the 16-byte grid); asserts the launch name and the sentinels
    around all three arrays; returns the output (N, OH, OW, CO)"""
    n, h, w, ci = x.shape
    co, k = wt.shape[3], wt.shape[1]
    oh, ow = rn.out_extent(h, k, stride, pad), rn.out_extent(w, k, stride, pad)
    if variant >= 2 and not hl.canon_fma():   # an MFMA step is fused by construction: no forced tile in the unfused build
        with pytest.raises(hl.HalideError) as e:
            hl.debug_resnet50_layer_batch(hl.Buffer(np.array(x)), hl.Buffer(np.array(wt)), *[hl.Buffer(np.array(v)) for v in vec], None, stride, pad, "raw",
                                          hl.Buffer(np.zeros((n, oh, ow, co), f32)), variant=variant)
        assert e.value.code == -8
        return None
    xi, ri, oo = _dev4(hl, x.shape, layout, x), _dev4(hl, res.shape, layout and layout + 1, res), _dev4(hl, res.shape, layout and 4 - layout)
    try:
        bufs = [hl.Buffer(np.array(wt))] + [hl.Buffer(np.array(v)) for v in vec]
        ran = _launches(hl, lambda: hl.debug_resnet50_layer_batch(xi.buf, *bufs, ri.buf if mode == "residual_relu" else None, stride, pad, mode, oo.buf,
                                                                 variant=variant))
        assert ran == [_expected_launch(hl, variant, co, k * k * ci, oh * ow, n)], (ran, x.shape, wt.shape, variant)
        got = oo.result()
        xi.result(), ri.result()
        return got
    finally:
        xi.free(), ri.free(), oo.free()


# (ci, co, w, h, k, stride) x images: one pixel per image and five images in one ragged tile; 20 pixels per image, three images inside one
# tile, stride 2 and pad 1 so that exterior taps fall on the neighbour's rows; 72 pixels per image, tiles across images, CO one past a
# tile; the stem's class, K = 147, odd; 510 pixels, a last tile of 62, three co tiles; and totals of 127, 128 and 129 pixels, either
# side of the 128-pixel tile
BATCH_SHAPES = [((1, 1, 1, 1, 1, 1), 5), ((5, 63, 9, 8, 3, 2), 3), ((64, 65, 9, 8, 1, 1), 3), ((3, 65, 17, 15, 7, 2), 2), ((64, 130, 17, 15, 3, 1), 2),
                ((1, 8, 127, 1, 1, 1), 1), ((1, 8, 32, 1, 1, 1), 4), ((1, 8, 43, 1, 1, 1), 3)]
VARIANT = pytest.mark.parametrize("variant", VARIANTS, ids=["plan", "general", "mfma_64x64", "mfma_64x128"])


def test_the_shapes_are_what_their_comment_says():
    pixels = lambda s: rn.out_extent(s[2], s[4], s[5], PAD_OF[s[4]]) * rn.out_extent(s[3], s[4], s[5], PAD_OF[s[4]])
    assert [pixels(s) * n for s, n in BATCH_SHAPES] == [5, 60, 216, 144, 510, 127, 128, 129] and WIDE == 128 and TILE == 64
    assert [pixels(s) for s, n in BATCH_SHAPES[:5]] == [1, 20, 72, 72, 255]


# ---------------------------------------------------------------------------------------------------- GPU: the layer hook
@pytest.mark.gpu
@VARIANT
@pytest.mark.parametrize("mode", rn.MODES)
@pytest.mark.parametrize("case", BATCH_SHAPES, ids=[f"{'x'.join(map(str, s))}x{n}" for s, n in BATCH_SHAPES])
def test_the_batched_layer_hook_equals_the_checker_image_by_image(hl, case, mode, variant):
    shape, n = case
    x, wt, vec, res = _batch_case(shape, n)
    got = _run_layer(hl, x, wt, vec, res, shape[5], PAD_OF[shape[4]], mode, variant, layout=BATCH_SHAPES.index(case) % 4)
    if got is not None:
        _same(got, _batch_want(hl.canon_fma(), shape, n, mode), f"{shape} x {n} {mode} variant {variant}")


@pytest.mark.gpu
@VARIANT
@pytest.mark.parametrize("k, stride", [(3, 1), (7, 2)])
@pytest.mark.parametrize("first", ["ones", "nan"])
def test_an_exterior_tap_never_reads_the_neighbouring_image(hl, variant, k, stride, first):
    """images back to back in one dense allocation: row -1 of image 1 is a real address, the last row of image 0.  Image 1 is all +0, so
    every output of it is a sum of w x 0; one tap taken from image 0 shows."""
    ci, co, w, h = 5, 65, 9, 8
    pad = PAD_OF[k]
    wt, vec = base._layer_case(ci, co, w, h, k, stride)[1:3]
    x = np.zeros((2, h, w, ci), f32)
    x[0] = 1.0 if first == "ones" else np.nan
    ow, oh = rn.out_extent(w, k, stride, pad), rn.out_extent(h, k, stride, pad)
    res = np.zeros((2, oh, ow, co), f32)
    got = _run_layer(hl, x, wt, vec, res, stride, pad, "raw", variant)
    if got is None:
        return
    alone = _run_layer(hl, x[1:], wt, vec, res[1:], stride, pad, "raw", variant)
    _same(got[1], alone[0], "image 1 beside image 0 and alone")
    _same(got[1], _conv_each(hl.canon_fma(), x[1:], wt, vec, res[1:], stride, pad, "raw")[0], "image 1 against the checker")
    assert not np.isnan(got[1]).any() and not got[1].any()   # (sums of w x 0 from +0: zeros of either sign)
    if first == "ones":
        _same(got[0], _conv_each(hl.canon_fma(), x[:1], wt, vec, res[:1], stride, pad, "raw")[0], "image 0")
    else:
        assert np.isnan(got[0]).all()


@pytest.mark.gpu
@VARIANT
def test_a_permuted_batch_gives_permuted_outputs(hl, variant):
    shape = (64, 65, 9, 8, 1, 1)
    x, wt, vec, res = _batch_case(shape, 3)
    order = [2, 0, 1]
    a = _run_layer(hl, x, wt, vec, res, 1, 0, "residual_relu", variant)
    b = _run_layer(hl, x[order], wt, vec, res[order], 1, 0, "residual_relu", variant)
    if a is not None:
        _same(b, a[order], "[C, A, B] against [A, B, C]")


@pytest.mark.gpu
@pytest.mark.parametrize("general", [False, True], ids=["default", "general"])
@pytest.mark.parametrize("shape", [(5, 63, 9, 8, 3, 2), (64, 130, 17, 15, 3, 1)])
def test_one_image_is_the_unbatched_hook(hl, shape, general):
    x, wt, vec, res = base._layer_case(*shape)
    stride, pad = shape[5], PAD_OF[shape[4]]
    B = lambda a: hl.Buffer(np.array(a))
    bufs = [B(wt)] + [B(v) for v in vec]
    o1, o4 = B(np.zeros(res.shape, f32)), B(np.zeros((1,) + res.shape, f32))
    ran1 = _launches(hl, lambda: hl.debug_resnet50_layer(B(x), *bufs, B(res), stride, pad, "residual_relu", o1, general_only=general))
    ran4 = _launches(hl, lambda: hl.debug_resnet50_layer_batch(B(x[None]), *bufs, B(res[None]), stride, pad, "residual_relu", o4, variant=int(general)))
    assert ran1 == ran4 == [base._expected_launch(hl, shape[1], shape[4] ** 2 * shape[0], general)]
    _same(o4.numpy()[0], o1.numpy(), f"{shape} general {general}")


@pytest.mark.gpu
@VARIANT
@pytest.mark.parametrize("layout", [1, 2, 3])
def test_padded_rows_planes_and_images_off_the_16_byte_grid(hl, variant, layout):
    for shape, n in (((5, 63, 9, 8, 3, 2), 3), ((64, 130, 17, 15, 3, 1), 2)):
        x, wt, vec, res = _batch_case(shape, n)
        got = _run_layer(hl, x, wt, vec, res, shape[5], PAD_OF[shape[4]], "residual_relu", variant, layout=layout)
        if got is not None:
            _same(got, _batch_want(hl.canon_fma(), shape, n, "residual_relu"), f"{shape} x {n} layout {layout}")


@pytest.mark.gpu
@VARIANT
@pytest.mark.parametrize("shape", base.ORDER_SHAPES)
def test_the_order_sensitive_input_in_the_last_image(hl, variant, shape):
    noise = _batch_case(shape, 3)
    xo, wt, vec, _ = base._layer_case(*shape, kind="order")
    x = np.concatenate([noise[0][:2], xo[None]])
    got = _run_layer(hl, x, wt, vec, noise[3], shape[5], PAD_OF[shape[4]], "raw", variant)
    if got is not None:
        _same(got[2], base._layer_want(hl.canon_fma(), *shape, "raw", "order"), f"order-sensitive {shape}")
        _same(got, _conv_each(hl.canon_fma(), x, wt, vec, noise[3], shape[5], PAD_OF[shape[4]], "raw"), f"the batch around it {shape}")


@pytest.mark.gpu
@VARIANT
@pytest.mark.parametrize("trap", base.TRAPS[2:])
def test_minus_zero_at_an_odd_k_in_the_last_image(hl, variant, trap):
    ci, co, w, h, k, co0, i0, j0 = trap
    xt, wt = base._minus_zero_trap(*trap)
    x = np.concatenate([base._noise((2, h, w, ci), 3), xt[None]])
    pad = PAD_OF[k]
    ones = tuple(np.ones(co, f32) for _ in range(4))
    res = np.zeros((3, rn.out_extent(h, k, 1, pad), rn.out_extent(w, k, 1, pad), co), f32)
    got = _run_layer(hl, x, wt, ones, res, 1, pad, "raw", variant)
    if got is not None:
        assert got.view(u32)[2, j0, i0, co0] == (0x80000000 if hl.canon_fma() else 0), hex(got.view(u32)[2, j0, i0, co0])
        _same(got, _conv_each(hl.canon_fma(), x, wt, ones, res, 1, pad, "raw"), f"-0 {trap}")


# ---------------------------------------------------------------------------------------------------- GPU: the pool and tail hooks
@pytest.mark.gpu
@pytest.mark.parametrize("shape", base.POOL_SHAPES)
def test_the_batched_max_pool_hook(hl, shape):
    c, w, h, k, stride, pad = shape
    for lo, layout in ((0.0, 0), (-3.0, 2)):
        x = (base._noise((3, h, w, c), 5) + f32(lo)).astype(f32)
        want = np.stack([rn.maxpool(x[i], k, stride, pad) for i in range(3)])
        xi, oo = _dev4(hl, x.shape, layout, x), _dev4(hl, want.shape, layout and 3 - layout)
        try:
            assert _launches(hl, lambda: hl.debug_resnet50_maxpool_batch(xi.buf, k, stride, pad, oo.buf)) == ["resnet50_maxpool"]
            _same(oo.result(), want, f"max pool {shape} {lo}")
            xi.result()
        finally:
            xi.free(), oo.free()


@pytest.mark.gpu
def test_the_max_pool_never_reads_the_neighbouring_image(hl):
    c, w, h = 5, 9, 8
    x = np.zeros((2, h, w, c), f32)
    x[0] = np.inf
    o2, o1 = hl.Buffer(np.full((2, 4, 5, c), 7, f32)), hl.Buffer(np.full((1, 4, 5, c), 7, f32))
    hl.debug_resnet50_maxpool_batch(hl.Buffer(x.copy()), 3, 2, 1, o2)
    hl.debug_resnet50_maxpool_batch(hl.Buffer(x[1:].copy()), 3, 2, 1, o1)
    _same(o2.numpy()[1], o1.numpy()[0], "image 1 beside image 0 and alone")
    _same(o2.numpy()[1], rn.maxpool(x[1], 3, 2, 1), "image 1 against the checker")
    assert np.isinf(o2.numpy()[0]).all() and not o2.numpy()[1].any()


def _tail_batch(shape, n, scale_first=1.0):
    c, w, h, classes = shape
    _, fw, fb = base._tail_case(shape)
    x = np.random.default_rng(50).random((n, h, w, c), dtype=f32)
    x[0] *= f32(scale_first)
    return x, fw, fb


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, FC_GROUP, FC_GROUP + 1])
@pytest.mark.parametrize("shape", base.TAIL_SHAPES)
def test_the_batched_tail_hook(hl, shape, n):
    x, fw, fb = _tail_batch(shape, n)
    want = np.stack([rn.tail(x[i], fw, fb)["out"] for i in range(n)])
    assert np.isfinite(want).all() and FC_GROUP == 8
    layout = base.TAIL_SHAPES.index(shape) % 4
    xi = _dev4(hl, x.shape, layout, x)
    oo = DevTensor(hl, want.shape, strides=(want.shape[1] + layout, 1), offset=4 * layout, dtype=f32)
    try:
        ran = _launches(hl, lambda: hl.debug_resnet50_tail_batch(xi.buf, hl.Buffer(fw), hl.Buffer(fb), oo.buf))
        assert ran == ["resnet50_avgpool", "resnet50_fc", "resnet50_softmax"]
        _same(oo.result(), want, f"tail {shape} x {n}")
    finally:
        xi.free(), oo.free()


@pytest.mark.gpu
def test_the_batched_tail_hook_at_the_networks_size(hl):
    shape = (2048, 7, 7, 1000)
    x, fw, fb = _tail_batch(shape, 3)
    want = np.stack([rn.tail(x[i], fw, fb)["out"] for i in range(3)])
    o = hl.Buffer(np.zeros((3, 1000), f32))
    hl.debug_resnet50_tail_batch(hl.Buffer(x), hl.Buffer(fw), hl.Buffer(fb), o)
    _same(o.numpy(), want, "tail 2048 x 7 x 7 -> 1000, three images")


@pytest.mark.gpu
def test_an_image_with_logits_past_exps_range_beside_an_ordinary_one(hl):
    shape = (64, 7, 7, 10)
    x, fw, fb = _tail_batch(shape, 2, scale_first=4000.0)
    want = [rn.tail(x[i], fw, fb) for i in range(2)]
    assert np.isnan(want[0]["out"]).any() and np.isinf(want[0]["e"]).any() and np.isfinite(want[1]["out"]).all()
    o = hl.Buffer(np.full((2, 10), 5, f32))
    hl.debug_resnet50_tail_batch(hl.Buffer(x), hl.Buffer(fw), hl.Buffer(fb), o)
    _same_or_nan(o.numpy(), np.stack([w["out"] for w in want]), "overflowing logits in image 0")
    _same(o.numpy()[1], want[1]["out"], "the ordinary image beside it")


# ---------------------------------------------------------------------------------------------------- GPU: the whole network
N_NET, SEED = 3, 1


@functools.lru_cache(maxsize=None)
def _net_batch():
    """(images (3, 224, 224, 3), parameter list, the checker's probabilities (3, 1000)): image 0 and the parameters are test_resnet50's
    seed-1 case"""
    sd, image, params, want = base._net_case(SEED)
    more = [np.random.default_rng(2000 + i).random((224, 224, 3), dtype=f32) for i in range(1, N_NET)]
    images = np.stack([image] + more)
    outs = np.stack([want["out"]] + [rn.network(m, params)["out"] for m in more])
    assert np.isfinite(outs).all()
    images.setflags(write=False), outs.setflags(write=False)
    return images, params, outs


@pytest.fixture(scope="module")
def net(hl):
    """the images and the parameters as buffers, device-resident after the first call, shared by the whole-network tests"""
    rn.set_canon(hl.canon_fma())
    images, params, outs = _net_batch()
    return hl.Buffer(images.copy()), [hl.Buffer(p.copy()) for p in params], images, outs


def _counts(hl, fn):
    return base._launch_counts(hl, fn)


@pytest.mark.gpu
def test_the_whole_network_on_three_images(hl, net, monkeypatch):
    inp, par, images, want = net
    monkeypatch.delenv("HLMI_RN50_BATCH_CHUNK", raising=False)
    o = hl.Buffer(np.zeros((N_NET, 1000), f32))
    ran = _counts(hl, lambda: hl.resnet50_batch(inp, par, o))
    assert sum(ran.values()) == 57 and {n: ran[n] for n in OTHERS} == dict.fromkeys(OTHERS, 1)
    expect = {}
    for ci, co, k, stride, pad, size in base.CONVS:
        name = _expected_launch(hl, 0, co, k * k * ci, rn.out_extent(size, k, stride, pad) ** 2, N_NET)
        expect[name] = expect.get(name, 0) + 1
    assert {n: c for n, c in ran.items() if n not in OTHERS} == expect
    _same(o.numpy(), want, "default chunk against the checker")
    # three resnet50 calls on the same device-resident parameters
    for i in range(N_NET):
        one = hl.Buffer(np.zeros(1000, f32))
        hl.resnet50(hl.Buffer(images[i].copy()), par, one)
        _same(o.numpy()[i], one.numpy(), f"image {i} against hl.resnet50")
    # chunks of 2 + 1: two runs of the plan
    monkeypatch.setenv("HLMI_RN50_BATCH_CHUNK", "2")
    o = hl.Buffer(np.zeros((N_NET, 1000), f32))
    ran = _counts(hl, lambda: hl.resnet50_batch(inp, dict(zip(hl.RESNET50_PARAM_NAMES, par)), o))
    assert sum(ran.values()) == 114 and {n: ran[n] for n in OTHERS} == dict.fromkeys(OTHERS, 2)
    _same(o.numpy(), want, "chunks of 2 + 1")
    monkeypatch.delenv("HLMI_RN50_BATCH_CHUNK")
    # the general path, and _argv
    o = hl.Buffer(np.zeros((N_NET, 1000), f32))
    ran = _counts(hl, lambda: hl.debug_resnet50_batch_general(inp, par, o))
    assert ran == dict(dict.fromkeys(OTHERS, 1), **{GENERAL: 53})
    _same(o.numpy(), want, "general path")
    o = hl.Buffer(np.zeros((N_NET, 1000), f32))
    assert call_argv(hl, NAME, inp, *par, o) == 0
    _same(o.numpy(), want, "resnet50_batch_argv")


@pytest.mark.gpu
def test_the_whole_network_into_boxes_and_padded_columns(hl, net, monkeypatch):
    inp, par, images, want = net
    monkeypatch.delenv("HLMI_RN50_BATCH_CHUNK", raising=False)
    # classes [10, 20) of images [0, 3) inside a larger device array with sentinels
    box = DevTensor(hl, (N_NET, 10), strides=(17, 1), offset=12, mins=[10, 0], dtype=f32)
    try:
        hl.resnet50_batch(inp, par, box.buf)
        _same(box.result(), want[:, 10:20], "output box [10, 20) x [0, 3)")
    finally:
        box.free()
    # a padded column stride, all classes
    wide = DevTensor(hl, (N_NET, 1000), strides=(1003, 1), offset=4, dtype=f32)
    try:
        hl.resnet50_batch(inp, par, wide.buf)
        _same(wide.result(), want, "padded column stride")
    finally:
        wide.free()
    # images [1, 3) of the same input: the range is the output's
    o = hl.Buffer(np.zeros((2, 1000), f32), mins=[0, 1])
    hl.resnet50_batch(inp, par, o)
    _same(o.numpy(), want[1:], "images [1, 3)")


@pytest.mark.gpu
def test_torch_op_equals_the_python_call_and_leaves_its_input(hl, net):
    import torch
    import halide_amd.torch_ops  # noqa: F401
    inp, par, images, want = net
    _, params, _ = _net_batch()
    ti = torch.from_numpy(images.copy()).cuda()
    tp = [torch.from_numpy(p.copy()).cuda() for p in params]
    out = torch.ops.hlmi.resnet50_batch(ti, tp)
    torch.cuda.synchronize()
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (N_NET, 1000)
    o = hl.Buffer(np.zeros((N_NET, 1000), f32))
    hl.resnet50_batch(inp, par, o)
    _same(out.cpu().numpy(), o.numpy(), "torch op against hl.resnet50_batch")
    _same(out.cpu().numpy(), want, "torch op against the checker")
    assert np.array_equal(ti.cpu().numpy(), images)
    with pytest.raises(TypeError):
        torch.ops.hlmi.resnet50_batch(ti.double(), tp)


@pytest.mark.gpu
def test_two_host_threads_with_a_batch_of_two_each_give_the_bits_of_one(hl, net):
    inp, par, images, want = net
    first, second = hl.Buffer(images[:2].copy()), hl.Buffer(images[1:].copy())
    outs = [hl.Buffer(np.zeros((2, 1000), f32)) for _ in range(4)]
    errors = []

    def work(which):
        try:
            for o in outs[which::2]:
                hl.resnet50_batch(first if which == 0 else second, par, o)
        except Exception as e:   # noqa: BLE001
            errors.append(e)

    hl.resnet50_batch(first, par, hl.Buffer(np.zeros((2, 1000), f32)))   # the parameters are on the device before the threads start
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i, o in enumerate(outs):
        _same(o.numpy(), want[:2] if i % 2 == 0 else want[1:], f"thread {i % 2} call {i // 2}")
