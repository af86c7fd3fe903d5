"""What the test files of the checker-held pipelines (test_resize.py, test_gaussian_blur.py, test_linear_blur.py) share besides
the checkers themselves (checker_lib.py): bit comparison, launch names, calling an entry point by its metadata, loading the
fuzzer.  Plain functions that take the product module `hl` as an argument; no fixtures."""
import ctypes as C
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNGEN = os.path.join(ROOT, "halide_amd", "bin", "hlmi_rungen")


def noise(shape, seed):
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


def gpu_present():
    import torch
    return torch.cuda.is_available()


def same_bits(got, want, what):
    """bit patterns, not values: -0 is not 0, and a NaN equals itself"""
    assert got.shape == want.shape, what
    bits = {4: np.uint32, 2: np.uint16, 1: np.uint8}[got.itemsize]
    bad = got.view(bits) != want.view(bits)
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} of {got.size} differ, first at {tuple(np.argwhere(bad)[0])}"


def launches(hl, fn):
    """names of the kernels one call launches, sorted, one entry per launch"""
    hl.kernel_timing(True)
    hl.kernel_timing_reset()
    try:
        fn()
        return sorted(e["name"] for e in hl.kernel_timing_report())
    finally:
        hl.kernel_timing(False)
        hl.kernel_timing_reset()


def call_direct(hl, name, *args):
    """The entry point `name` as C calls it, with its own arguments in order: a Buffer or None (a null pointer) for a buffer, a
    number for a scalar (hl._fn holds the argtypes that `<name>_metadata()` states).  Returns the entry point's code."""
    return hl._fn[name](*[a.ptr if isinstance(a, hl.Buffer) else a for a in args])


def call_argv(hl, name, *args):
    """The same call through `<name>_argv`: every scalar boxed by its metadata type, as hl.run_batch boxes a frame"""
    md = hl.metadata(name)
    assert len(args) == md.num_arguments, (name, len(args))
    fn = getattr(hl.lib, name + "_argv")
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(C.c_void_p)]
    argv, keep = (C.c_void_p * len(args))(), []
    for j, v in enumerate(args):
        a = md.arguments[j]
        if a.kind != 0:
            argv[j] = None if v is None else C.cast(v.ptr, C.c_void_p)
        else:
            keep.append({(2, 32): C.c_float, (0, 32): C.c_int32}[(a.type.code, a.type.bits)](v))
            argv[j] = C.cast(C.pointer(keep[-1]), C.c_void_p)
    return fn(argv)


def load_fuzz_parity():
    """scripts/fuzz_parity.py as a module (it imports halide_amd, the product, and oracle_lib; checker_lib on first use)"""
    spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(ROOT, "scripts", "fuzz_parity.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod
