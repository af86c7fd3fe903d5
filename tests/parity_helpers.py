"""What the test files of the checker-held pipelines (test_resize.py, test_gaussian_blur.py, test_linear_blur.py) share besides
the checkers themselves (checker_lib.py): bit comparison, launch names, calling an entry point by its metadata, loading the
fuzzer; and what test_buffer_layouts.py and test_special_values.py add for the older pipelines: arrays with padded rows and planes
in host memory or in a device allocation of the test's own (HostArray, DevArray), NaN-aware bit comparison, kernel constants read
from the source; and what the hannk ops' tests share: DevTensor, a device array of any rank, strides and byte offset.  Plain functions and classes that take the product module `hl` as an argument; no fixtures."""
import ctypes as C
import importlib.util
import os
import re

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
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bits = {8: np.uint64, 4: np.uint32, 2: np.uint16, 1: np.uint8}[got.itemsize]
    bad = got.view(bits) != want.view(bits)
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} of {got.size} differ, first at {tuple(np.argwhere(bad)[0])}"


def same_bits_or_nan(got, want, what):
    """same_bits, except where the oracle has a NaN: there the library must have a NaN, and nothing else is compared (sign and
    payload of a NaN that an operation produces belong to the processor)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype and got.dtype in (np.float32, np.float64), what
    bits = np.uint32 if got.dtype == np.float32 else np.uint64
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), f"{what}: {np.count_nonzero(~np.isnan(got[nan]))} of the oracle's {np.count_nonzero(nan)} NaNs are numbers"
    bad = (got.view(bits) != want.view(bits)) & ~nan
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} of {got.size} differ, first at {tuple(np.argwhere(bad)[0])}"


def kernel_const(hip_file, name):
    """the value of `constexpr int ... <name> = <digits>` in halide_amd/csrc/<hip_file>: tests size their images by the
    kernel's own tile, and a kernel without the constant fails here"""
    src = open(os.path.join(ROOT, "halide_amd", "csrc", hip_file)).read()
    m = re.search(rf"^\s*constexpr int (?:[^;]*[ ,])?{name} = (\d+)\s*[,;]", src, re.M)
    assert m, f"{hip_file} has no constexpr int {name}"
    return int(m.group(1))


SENTINEL = {np.dtype(np.uint8): 0xA5, np.dtype(np.uint16): 0xA5C3, np.dtype(np.float32): np.float32(-1234.5),
            np.dtype(np.float64): np.float64(-1234.5)}


class _Strided:
    """A (H, W) or (C, H, W) array of `dtype` laid out in a flat array of its own: rows `row_stride` and planes `plane_stride`
    elements apart, the first element `offset` bytes (a multiple of the item size) after the flat array's start, eight spare
    elements after the last row.  Every element of the flat array outside the array proper holds SENTINEL[dtype]; `host` is the
    view of the array proper, filled with `fill`."""

    def __init__(self, shape, dtype, row_stride=None, plane_stride=None, offset=0, fill=None):
        dtype = np.dtype(dtype)
        assert len(shape) in (2, 3) and offset % dtype.itemsize == 0
        h, w = shape[-2:]
        rs = w if row_stride is None else row_stride
        ps = rs * h if plane_stride is None else plane_stride
        assert rs >= w and ps >= rs * (h - 1) + w
        n = offset // dtype.itemsize + (ps * shape[0] if len(shape) == 3 else rs * h) + 8
        self.flat = np.full(n, SENTINEL[dtype], dtype)
        self.strides = ((ps,) if len(shape) == 3 else ()) + (rs, 1)          # in elements, numpy order
        self.host = np.lib.stride_tricks.as_strided(self.flat[offset // dtype.itemsize:], shape, tuple(s * dtype.itemsize for s in self.strides))
        self.host[...] = 0 if fill is None else fill
        self.offset = offset

    def _inside(self, flat):
        return np.lib.stride_tricks.as_strided(flat[self.offset // flat.itemsize:], self.host.shape, self.host.strides)

    def _checked(self, back, before):
        """the array proper of `back`, a flat array read after the call, contiguous; every other byte must be as in `before`"""
        view = self._inside(back)
        got = view.copy()   # (ascontiguousarray would alias a dense array)
        view[...] = self._inside(before)
        assert np.array_equal(back.view(np.uint8), before.view(np.uint8)), "bytes outside the array were written"
        return got


class HostArray(_Strided):
    """_Strided in host memory, wrapped as a host buffer: the library gives it a device allocation that mirrors the strides."""

    def __init__(self, hl, shape, dtype, row_stride=None, plane_stride=None, offset=0, mins=None, fill=None):
        super().__init__(shape, dtype, row_stride, plane_stride, offset, fill)
        self.before = self.flat.copy()
        self.buf = hl.Buffer(self.host, mins=mins)

    def result(self):
        """the array as the library left it, contiguous; everything outside it must be as it was"""
        self.buf.numpy()
        return self._checked(self.flat.copy(), self.before)

    def free(self):
        self.buf.device_free()


class DevArray(_Strided):
    """_Strided inside a flat DEVICE allocation of its own (made with the HIP runtime directly, as a caller with device memory
    of its own would; its start is 256-byte aligned), wrapped as a device-only buffer with Buffer.wrap_device: the
    generalisation of hexagon_benchmarks_checker.DevPlane to any element type, planes and sentinel padding."""

    def __init__(self, hl, shape, dtype, row_stride=None, plane_stride=None, offset=0, mins=None, fill=None):
        super().__init__(shape, dtype, row_stride, plane_stride, offset, fill)
        self.hip = hl.hip_runtime()
        self.p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), C.c_size_t(self.flat.nbytes)) == 0
        assert self.p.value % 256 == 0
        assert self.hip.hipMemcpy(self.p, C.c_void_p(self.flat.ctypes.data), C.c_size_t(self.flat.nbytes), 1) == 0   # host to device
        self.buf = hl.Buffer.wrap_device(self.p.value + offset, dtype, shape[::-1], self.strides[::-1], mins)

    def result(self):
        """the array as the device holds it now, contiguous; everything outside it must be as it was"""
        self.buf.device_sync()
        back = np.empty_like(self.flat)
        assert self.hip.hipMemcpy(C.c_void_p(back.ctypes.data), self.p, C.c_size_t(back.nbytes), 2) == 0   # device to host
        return self._checked(back, self.flat)

    def free(self):
        self.buf.device_detach()
        assert self.hip.hipFree(self.p) == 0


class DevTensor:
    """An array of `dtype`, numpy `shape` and element `strides` (any rank, any strides that do not overlap) inside a flat device allocation
    of its own, `offset` BYTES after its 256-byte aligned start, every other byte 0xA5; wrapped as a device-only buffer.  result() reads
    the whole allocation back and checks that no byte outside the array changed: between rows, between pixels, before and after."""
    SENTINEL = 0xA5

    def __init__(self, hl, shape, strides=None, offset=0, mins=None, fill=None, dtype=np.uint8):
        self.hl, self.hip, self.dtype = hl, hl.hip_runtime(), np.dtype(dtype)
        if strides is None:
            strides = [int(np.prod(shape[k + 1:])) for k in range(len(shape))]
        es = self.dtype.itemsize
        n = offset + (sum((e - 1) * s for e, s in zip(shape, strides)) + 1) * es + 16
        self.flat = np.full(n, self.SENTINEL, np.uint8)
        self.shape, self.strides, self.offset = tuple(shape), tuple(strides), offset
        self.view(self.flat)[...] = 0 if fill is None else fill
        self.p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), C.c_size_t(n)) == 0 and self.p.value % 256 == 0
        assert self.hip.hipMemcpy(self.p, C.c_void_p(self.flat.ctypes.data), C.c_size_t(n), 1) == 0
        self.buf = hl.Buffer.wrap_device(self.p.value + offset, self.dtype, shape[::-1], strides[::-1], mins)

    def view(self, flat):
        return np.ndarray(self.shape, self.dtype, buffer=flat, offset=self.offset, strides=tuple(s * self.dtype.itemsize for s in self.strides))

    def result(self):
        self.buf.device_sync()
        back = np.empty_like(self.flat)
        assert self.hip.hipMemcpy(C.c_void_p(back.ctypes.data), self.p, C.c_size_t(back.nbytes), 2) == 0
        got = self.view(back).copy()
        self.view(back)[...] = self.view(self.flat)
        bad = np.flatnonzero(back != self.flat)
        assert bad.size == 0, f"{bad.size} bytes outside the array were written, the first {int(bad[0]) - self.offset} bytes after its first element"
        return got

    def free(self):
        self.buf.device_detach()
        assert self.hip.hipFree(self.p) == 0


def address(arr):
    """the address the kernels see for the first element of a HostArray or DevArray (after the call, for a HostArray)"""
    return arr.buf.raw.device


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
            keep.append({(2, 32): C.c_float, (2, 64): C.c_double, (0, 32): C.c_int32}[(a.type.code, a.type.bits)](v))
            argv[j] = C.cast(C.pointer(keep[-1]), C.c_void_p)
    return fn(argv)


def load_fuzz_parity():
    """scripts/fuzz_parity.py as a module (it imports halide_amd, the product, and oracle_lib; checker_lib on first use)"""
    spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(ROOT, "scripts", "fuzz_parity.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod
