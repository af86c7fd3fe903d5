"""The boundary of every entry point as its callers see it: what `<name>_metadata()` says, and that `<name>_argv` is the direct call.

Each entry point describes its arguments once, in an argument table (csrc/hlmi_internal.h), from which the metadata, the
buffer checks' view of the arguments and the Python caller's argtypes all follow.  tests/golden/metadata.json is the complete
dump of the metadata of all 41 entry points, recorded from the library as it was before the tables existed; run this module
as a script (`python tests/test_metadata_table.py`) to record it again from the library under HLMI_LIB / halide_amd/lib.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "metadata.json")

PIPELINES = ["local_laplacian", "bilateral_grid", "halide_blur", "nl_means", "stencil_chain", "conv_layer", "conv_layer_bf16",
             "depthwise_separable_conv", "unsharp", "max_filter", "hist", "harris", "interpolate", "iir_blur", "lens_blur", "bgu",
             "camera_pipe"]
RESIZES = [f"resize_{k}_{t}_{d}" for k in ("box", "linear", "cubic", "lanczos") for t in ("float32", "uint8", "uint16")
           for d in ("up", "down")]
NAMES = PIPELINES + RESIZES


def _scalar(ptr, t):
    """A scalar pointer of an argument: None, or the value read according to the argument's type."""
    if not ptr:
        return None
    field = {(2, 32): "f32", (2, 64): "f64", (0, 32): "i32", (0, 64): "i64", (1, 64): "u64", (1, 1): "b"}[(t.code, t.bits)]
    return getattr(ptr.contents, field)


def dump(hl, name):
    md = hl.metadata(name)
    args = []
    for i in range(md.num_arguments):
        a = md.arguments[i]
        est = None
        if a.buffer_estimates:
            est = [a.buffer_estimates[j].contents.value if a.buffer_estimates[j] else None for j in range(2 * a.dimensions)]
        args.append(dict(name=a.name.decode(), kind=a.kind, dimensions=a.dimensions,
                         type=dict(code=a.type.code, bits=a.type.bits, lanes=a.type.reserved),
                         scalar_def=_scalar(a.scalar_def, a.type), scalar_min=_scalar(a.scalar_min, a.type),
                         scalar_max=_scalar(a.scalar_max, a.type), scalar_estimate=_scalar(a.scalar_estimate, a.type),
                         buffer_estimates=est))
    return dict(version=md.version, target=md.target.decode(), name=md.name.decode(), arguments=args)


def test_metadata_is_the_recorded_one(hl):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(NAMES) and len(NAMES) == 41
    for name in NAMES:
        assert dump(hl, name) == golden[name], name


# ---- argv == direct call -----------------------------------------------------------------------------------------------------
# Output shapes: SPEC of tests/test_entry_protocol.py; the inputs are sized by the pipeline's own bounds query.  Scalars: valid,
# pairwise distinct within a call and none equal to its estimate, so that two scalars swapped (or one replaced by a default) on
# the argv path would change the output.  resize answers a query with the input's x / y as passed: its input is shaped here.
ARGV_CASES = {
    "local_laplacian": dict(out=(64, 48, 3), scalars=[4, 0.25, 1.5]),
    "bilateral_grid": dict(out=(64, 48), scalars=[0.2]),
    "nl_means": dict(out=(32, 24, 3), scalars=[5, 3, 0.2]),
    "iir_blur": dict(out=(64, 48, 3), scalars=[0.3]),
    "camera_pipe": dict(out=(64, 32, 3), scalars=[4200.0, 1.8, 40.0, 0.7, 20, 900]),
    "lens_blur": dict(out=(48, 40, 3), scalars=[16, 5, 0.25, 8]),
    "bgu": dict(out=(64, 48, 3), scalars=[0.25, 4]),
    "resize_lanczos_float32_up": dict(out=(64, 48, 3), scalars=[2.0], inp=(32, 24, 3)),
    "resize_cubic_uint8_down": dict(out=(32, 24, 3), scalars=[0.5], inp=(64, 48, 3)),
}


def _np_type(t):
    return {(0, 32): np.int32, (1, 8): np.uint8, (1, 16): np.uint16, (2, 32): np.float32}[(t.code, t.bits)]


def _noise(rng, shape, dtype):
    if dtype == np.float32:
        return rng.random(shape, dtype=np.float32)
    return rng.integers(0, 256 if dtype == np.uint8 else 1024, shape).astype(dtype)


def _arguments(hl, name, case):
    """[Buffer | ctypes scalar] in the entry point's order: zeroed output, seeded-noise inputs of the queried shapes."""
    md = hl.metadata(name)
    args = [md.arguments[i] for i in range(md.num_arguments)]
    scalars, values = list(case["scalars"]), []
    for a in args:
        if a.kind == 0:
            v = scalars.pop(0)
            values.append(C.c_float(v) if a.type.code == 2 else C.c_int32(v))
        elif a.kind == 2:
            values.append(hl.Buffer(np.zeros(tuple(reversed(case["out"])), _np_type(a.type))))
        else:
            values.append(hl.Buffer.bounds_query(_np_type(a.type), a.dimensions, extents=case.get("inp")))
    argv = _argv(hl, values)
    fn = getattr(hl.lib, name + "_argv")
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(C.c_void_p)]
    hl._check(fn(argv))                                  # the bounds query
    rng = np.random.default_rng(20261017)
    for i, a in enumerate(args):
        if a.kind == 1:
            q = values[i]
            assert all(e > 0 for e in q.extents), (name, a.name, q.extents)
            values[i] = hl.Buffer(_noise(rng, tuple(reversed(q.extents)), _np_type(a.type))).set_min(*q.mins)
    return args, values, fn


def _argv(hl, values):
    argv = (C.c_void_p * len(values))()
    for i, v in enumerate(values):
        argv[i] = C.cast(C.pointer(v.raw if isinstance(v, hl.Buffer) else v), C.c_void_p)
    return argv


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ARGV_CASES))
def test_argv_is_the_direct_call(hl, name):
    """One call through `<name>_argv`, one through `<name>` itself, on the same inputs: byte-identical outputs."""
    args, values, argv_fn = _arguments(hl, name, ARGV_CASES[name])
    out = next(i for i, a in enumerate(args) if a.kind == 2)

    hl._check(argv_fn(_argv(hl, values)))
    via_argv = values[out].numpy().copy()

    values[out] = hl.Buffer(np.zeros_like(via_argv))
    direct = getattr(hl.lib, name)
    direct.restype = C.c_int
    direct.argtypes = [hl._BP if a.kind else (C.c_float if a.type.code == 2 else C.c_int32) for a in args]
    hl._check(direct(*[v.ptr if isinstance(v, hl.Buffer) else v for v in values]))
    via_direct = values[out].numpy()

    assert via_argv.any(), "an all-zero output would compare equal whatever the scalars were"
    assert via_argv.tobytes() == via_direct.tobytes()


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    import halide_amd
    with open(GOLDEN, "w") as f:
        json.dump({n: dump(halide_amd, n) for n in NAMES}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {GOLDEN}: {len(NAMES)} entry points")
