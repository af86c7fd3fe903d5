"""halide_amd — host-side mirror (ctypes) of the C-ABI drop-in library ``libhlmi.so``.

The product is the shared library: hand-written HIP kernels for gfx950 behind the reference's AOT
entry points (``int local_laplacian(halide_buffer_t*, int32_t, float, float, halide_buffer_t*)`` …,
see ``include/hlmi_pipelines.h``).  This package is only the thin Python caller used by the tests and
``bench.py``: a ``Buffer`` that plays the role of ``Halide::Runtime::Buffer`` (reference:
``src/runtime/HalideBuffer.h`` — planar storage, dimension 0 innermost, dirty flags, ``copy_to_host``,
``device_sync``) and one Python function per pipeline with the reference's argument order.

There is deliberately no CPU fallback: if ``libhlmi.so`` is missing the import fails, and if no
gfx950 device is usable every pipeline call raises ``HalideError`` (code -29).
"""
from __future__ import annotations

import ctypes as C
import math
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# HLMI_LIB: an alternative build of the same library (A/B measurements of compile-time switches, csrc/Makefile VARIANT=)
LIB_PATH = os.environ.get("HLMI_LIB") or os.path.join(_HERE, "lib", "libhlmi.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "(or `make -C halide_amd/csrc`). halide_amd has no pure-Python / CPU fallback.")



def _elf_dynamic_strings(path: str, tag: int) -> list:
    """Values of the string-valued entries `tag` (1 = DT_NEEDED, 14 = DT_SONAME) of a little-endian ELF64 shared object's
    dynamic section; [] when the file cannot be parsed."""
    import struct
    try:
        with open(path, "rb") as f:
            data = f.read()
        if data[:4] != b"\x7fELF" or data[4] != 2 or data[5] != 1:
            return []
        shoff, = struct.unpack_from("<Q", data, 0x28)
        shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
        secs = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
        out = []
        for sec in secs:
            if sec[1] != 6:      # SHT_DYNAMIC
                continue
            strtab = secs[sec[6]]
            for off in range(sec[4], sec[4] + sec[5], 16):
                t, v = struct.unpack_from("<qQ", data, off)
                if t == 0:
                    break
                if t == tag:
                    a = strtab[4] + v
                    out.append(data[a:data.index(b"\0", a)].decode())
        return out
    except Exception:  # noqa: BLE001
        return []


def _preload_torch_hip_runtime() -> str | None:
    """One HIP runtime per process.  The torch-ROCm wheel bundles its own libamdhip64.so (same SONAME as the system's): a
    process that loads libhlmi.so first and torch afterwards ends up with TWO runtimes — the system's under libhlmi.so and
    the bundled one under torch — whose streams and events are not interchangeable (torch streams handed to the library,
    tests/test_torch_ops.py, then belong to the other runtime: std::bad_variant_access or a segfault inside HIP).  When
    torch is importable its copy is therefore loaded FIRST, without importing torch, and libhlmi.so binds to it exactly as
    it does when the caller imported torch first.  HLMI_SYSTEM_HIP=1 keeps the system runtime (torch-free processes)."""
    if os.environ.get("HLMI_SYSTEM_HIP"):
        return None
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
    except Exception:  # noqa: BLE001
        return None
    if not spec or not spec.submodule_search_locations:
        return None
    path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if not os.path.exists(path):
        return None
    # libhlmi.so was linked against the system ROCm; torch's copy is only a safe stand-in when it IS the same ABI: its
    # SONAME must be the libamdhip64 name libhlmi.so lists as NEEDED.  On a mismatch the system runtime is kept (a
    # process that then also imports torch has to import torch FIRST) unless HLMI_TORCH_HIP=1 insists.
    import sys
    if "torch" not in sys.modules and os.environ.get("HLMI_TORCH_HIP") != "1":
        needed = [n for n in _elf_dynamic_strings(LIB_PATH, 1) if n.startswith("libamdhip64")]
        soname = _elf_dynamic_strings(path, 14)
        if not needed or not soname or soname[0] != needed[0]:
            import warnings
            warnings.warn(f"halide_amd: torch bundles {soname[0] if soname else 'an unidentified HIP runtime'} but libhlmi.so needs "
                          f"{needed[0] if needed else 'libamdhip64'}: keeping the system HIP runtime — import torch BEFORE halide_amd "
                          "in a process that uses both (INTEGRATION.md), or set HLMI_TORCH_HIP=1", RuntimeWarning, stacklevel=2)
            return None
    try:
        C.CDLL(path, mode=C.RTLD_GLOBAL)
    except OSError:
        return None
    return path


HIP_RUNTIME_PRELOADED = _preload_torch_hip_runtime()
lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)


def hip_runtime() -> C.CDLL:
    """The HIP runtime libhlmi.so is bound to (global symbol scope of the process): callers that create streams or events
    of their own for the library must use THIS runtime, not whatever dlopen("libamdhip64.so") finds."""
    return C.CDLL(None)



# ---------------------------------------------------------------------------------------------------
# ABI structs (include/hlmi_abi.h)
class halide_type_t(C.Structure):
    _fields_ = [("code", C.c_uint8), ("bits", C.c_uint8), ("reserved", C.c_uint16)]


class halide_dimension_t(C.Structure):
    _fields_ = [("min", C.c_int32), ("extent", C.c_int32), ("stride", C.c_int32), ("flags", C.c_uint32)]


class halide_buffer_t(C.Structure):
    _fields_ = [("device", C.c_uint64), ("device_interface", C.c_void_p), ("host", C.c_void_p),
                ("flags", C.c_uint64), ("type", halide_type_t), ("dimensions", C.c_int32),
                ("dim", C.POINTER(halide_dimension_t)), ("padding", C.c_void_p)]


class halide_scalar_value_t(C.Union):
    _fields_ = [("b", C.c_uint8), ("i32", C.c_int32), ("i64", C.c_int64), ("u64", C.c_uint64),
                ("f32", C.c_float), ("f64", C.c_double), ("handle", C.c_void_p)]


class halide_filter_argument_t(C.Structure):
    _fields_ = [("name", C.c_char_p), ("kind", C.c_int32), ("dimensions", C.c_int32), ("type", halide_type_t),
                ("scalar_def", C.POINTER(halide_scalar_value_t)), ("scalar_min", C.POINTER(halide_scalar_value_t)),
                ("scalar_max", C.POINTER(halide_scalar_value_t)),
                ("scalar_estimate", C.POINTER(halide_scalar_value_t)),
                ("buffer_estimates", C.POINTER(C.POINTER(C.c_int64)))]


class halide_filter_metadata_t(C.Structure):
    _fields_ = [("version", C.c_int32), ("num_arguments", C.c_int32),
                ("arguments", C.POINTER(halide_filter_argument_t)), ("target", C.c_char_p), ("name", C.c_char_p)]


assert C.sizeof(halide_buffer_t) == 56 and C.sizeof(halide_dimension_t) == 16 and C.sizeof(halide_type_t) == 4

FLAG_HOST_DIRTY = 1
FLAG_DEVICE_DIRTY = 2

_TYPE_OF = {np.dtype(np.uint8): (1, 8), np.dtype(np.uint16): (1, 16), np.dtype(np.uint32): (1, 32),
            np.dtype(np.int8): (0, 8), np.dtype(np.int16): (0, 16), np.dtype(np.int32): (0, 32),
            np.dtype(np.float32): (2, 32), np.dtype(np.float64): (2, 64)}

ERROR_NAMES = {0: "success", -1: "generic_error", -3: "bad_type", -4: "access_out_of_bounds",
               -5: "buffer_allocation_too_large", -6: "buffer_extents_too_large", -8: "constraint_violated",
               -9: "param_too_small", -10: "param_too_large", -12: "buffer_argument_is_null",
               -14: "copy_to_host_failed", -15: "copy_to_device_failed", -16: "device_malloc_failed",
               -19: "no_device_interface", -20: "unimplemented", -23: "device_run_failed",
               -28: "buffer_extents_negative", -29: "gpu_device_error", -34: "host_is_null",
               -36: "device_interface_no_device", -37: "host_and_device_dirty", -38: "buffer_is_null",
               -42: "incompatible_device_interface", -43: "bad_dimensions",
               -44: "device_dirty_with_no_device_support"}


class HalideError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"halide error {code} ({ERROR_NAMES.get(code, '?')}): {message}")
        self.code = code
        self.message = message


# ---------------------------------------------------------------------------------------------------
# error handler: the library's default prints and abort()s like the reference
# (src/runtime/posix_error_handler.cpp:9-21); under Python we record the message and raise instead.
_ERR_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)
_tls = threading.local()


def _on_error(_uc, msg):
    _tls.last_error = msg.decode("utf-8", "replace") if msg else ""
    if _batch_active[0] and not _batch_error:   # a worker thread of hlmi_run_batch: keep the batch's FIRST message
        _batch_error.append(_tls.last_error)


_error_cb = _ERR_CB(_on_error)
lib.halide_set_error_handler.restype = C.c_void_p
lib.halide_set_error_handler.argtypes = [_ERR_CB]
lib.halide_set_error_handler(_error_cb)


def last_error() -> str:
    return getattr(_tls, "last_error", "")


def _check(code: int) -> int:
    if code != 0:
        msg = last_error()
        _tls.last_error = ""
        raise HalideError(code, msg)
    return code


# ---------------------------------------------------------------------------------------------------
_BP = C.POINTER(halide_buffer_t)
lib.halide_hip_device_interface.restype = C.c_void_p
lib.halide_device_sync.argtypes = [C.c_void_p, _BP]
lib.halide_copy_to_host.argtypes = [C.c_void_p, _BP]
lib.halide_copy_to_device.argtypes = [C.c_void_p, _BP, C.c_void_p]
lib.halide_device_free.argtypes = [C.c_void_p, _BP]
lib.halide_device_malloc.argtypes = [C.c_void_p, _BP, C.c_void_p]
lib.halide_hip_wrap_device_ptr.argtypes = [C.c_void_p, _BP, C.c_uint64]
lib.halide_hip_detach_device_ptr.argtypes = [C.c_void_p, _BP]
lib.halide_hip_get_device_ptr.argtypes = [C.c_void_p, _BP]
lib.halide_hip_get_device_ptr.restype = C.c_size_t
lib.halide_set_gpu_device.argtypes = [C.c_int]
lib.halide_hip_set_stream.argtypes = [C.c_void_p]
lib.halide_hip_get_stream.argtypes = [C.c_void_p]
lib.halide_hip_get_stream.restype = C.c_void_p
lib.halide_device_release.argtypes = [C.c_void_p, C.c_void_p]
lib.halide_reuse_device_allocations.argtypes = [C.c_void_p, C.c_bool]
lib.hlmi_kernel_timing_enable.argtypes = [C.c_int]
lib.hlmi_kernel_timing_report.argtypes = [C.c_char_p, C.c_size_t]
lib.hlmi_kernel_timing_only.argtypes = [C.c_char_p]
lib.hlmi_kernel_timing_report.restype = C.c_size_t
lib.hlmi_version.restype = C.c_char_p
lib.hlmi_canon_fma.restype = C.c_int


def hip_device_interface() -> int:
    return lib.halide_hip_device_interface()


def set_gpu_device(n: int) -> None:
    lib.halide_set_gpu_device(int(n))


def set_stream(stream_ptr: int | None) -> None:
    """Enqueue all subsequent work of this thread on `stream_ptr` (a hipStream_t, e.g.
    torch.cuda.current_stream().cuda_stream); None restores the library's own stream."""
    lib.halide_hip_set_stream(C.c_void_p(stream_ptr or 0))


def partition_stream(part: int, nparts: int, replica: int = 0) -> int | None:
    """hipStream_t of frame queue `part` of `nparts` (a library-owned stream with a hardware queue of its own whose launches are
    sized for `nparts` frames in flight; include/hlmi_runtime.h — the name dates from when its CU mask was believed to confine
    it), or None; `replica` > 0: a further queue of the same kind."""
    lib.halide_hip_partition_stream_replica.restype = C.c_void_p
    lib.halide_hip_partition_stream_replica.argtypes = [C.c_int, C.c_int, C.c_int]
    return lib.halide_hip_partition_stream_replica(int(part), int(nparts), int(replica))


def kernel_timing(enable: bool) -> None:
    lib.hlmi_kernel_timing_enable(1 if enable else 0)


def kernel_timing_only(name) -> None:
    """Measurement only: while `name` is set, every kernel launch with another timing name is skipped (hlmi_runtime.h)."""
    lib.hlmi_kernel_timing_only(name.encode() if name else None)


def kernel_timing_reset() -> None:
    lib.hlmi_kernel_timing_reset()


def kernel_timing_report() -> list:
    import json
    n = lib.hlmi_kernel_timing_report(None, 0)
    buf = C.create_string_buffer(n + 16)
    lib.hlmi_kernel_timing_report(buf, n + 16)
    return json.loads(buf.value.decode())


class Buffer:
    """Caller-side image descriptor, the role Halide::Runtime::Buffer<T> plays for the reference's drivers.

    Storage is a numpy array in C order whose axes are the Halide dimensions REVERSED (the convention of the
    reference's Python bindings, src/PythonExtensionGen.cpp): ``np.zeros((3, H, W))`` is a planar W x H x 3
    image with dimension 0 (x) innermost, exactly ``Buffer<T,3>(W, H, 3)`` (HalideBuffer.h:441-451).
    """

    def __init__(self, array: np.ndarray | None = None, *, dtype=None, shape_xyz=None, mins=None):
        if array is None:
            array = np.zeros(tuple(reversed(shape_xyz)), dtype=dtype)
        self.array = array
        nd = array.ndim
        if array.dtype not in _TYPE_OF:
            raise TypeError(f"unsupported dtype {array.dtype}")
        self._dims = (halide_dimension_t * max(nd, 1))()
        for i in range(nd):
            ax = nd - 1 - i
            st = array.strides[ax]
            assert st % array.itemsize == 0
            self._dims[i] = halide_dimension_t(0 if mins is None else int(mins[i]), array.shape[ax],
                                               st // array.itemsize, 0)
        code, bits = _TYPE_OF[array.dtype]
        self.raw = halide_buffer_t(0, None, array.ctypes.data, FLAG_HOST_DIRTY, halide_type_t(code, bits, 0), nd,
                                   self._dims, None)

    # -- construction helpers --------------------------------------------------------------------
    @classmethod
    def bounds_query(cls, dtype, ndim: int, mins=None, extents=None) -> "Buffer":
        """A buffer with host == NULL and device == 0 (HalideRuntime.h:1851-1853)."""
        b = cls.__new__(cls)
        b.array = None
        b._dims = (halide_dimension_t * max(ndim, 1))()
        stride = 1
        for i in range(ndim):
            e = 0 if extents is None else int(extents[i])
            b._dims[i] = halide_dimension_t(0 if mins is None else int(mins[i]), e, stride, 0)
            stride *= max(e, 1)
        code, bits = _TYPE_OF[np.dtype(dtype)]
        b.raw = halide_buffer_t(0, None, None, 0, halide_type_t(code, bits, 0), ndim, b._dims, None)
        return b

    @classmethod
    def wrap_device(cls, device_ptr: int, dtype, extents, strides=None, mins=None) -> "Buffer":
        """Device-only buffer around an existing allocation (mirrors halide_cuda_wrap_device_ptr)."""
        nd = len(extents)
        b = cls.bounds_query(dtype, nd, mins, extents)
        if strides is not None:
            for i in range(nd):
                b._dims[i].stride = int(strides[i])
        _check(lib.halide_hip_wrap_device_ptr(None, C.byref(b.raw), C.c_uint64(device_ptr)))
        return b

    # -- accessors -----------------------------------------------------------------------------------
    @property
    def ptr(self):
        return C.byref(self.raw)

    def dim(self, i: int) -> halide_dimension_t:
        return self._dims[i]

    @property
    def extents(self):
        return [self._dims[i].extent for i in range(self.raw.dimensions)]

    @property
    def mins(self):
        return [self._dims[i].min for i in range(self.raw.dimensions)]

    def set_min(self, *mins) -> "Buffer":
        for i, m in enumerate(mins):
            self._dims[i].min = int(m)
        return self

    def set_host_dirty(self, v: bool = True) -> None:
        self.raw.flags = (self.raw.flags | FLAG_HOST_DIRTY) if v else (self.raw.flags & ~FLAG_HOST_DIRTY)

    @property
    def host_dirty(self) -> bool:
        return bool(self.raw.flags & FLAG_HOST_DIRTY)

    @property
    def device_dirty(self) -> bool:
        return bool(self.raw.flags & FLAG_DEVICE_DIRTY)

    @property
    def has_device_allocation(self) -> bool:
        return self.raw.device != 0

    # -- device protocol (HalideBuffer.h:1810-1815, :1908) -------------------------------------
    def copy_to_host(self) -> "Buffer":
        _check(lib.halide_copy_to_host(None, self.ptr))
        return self

    def copy_to_device(self) -> "Buffer":
        _check(lib.halide_copy_to_device(None, self.ptr, hip_device_interface()))
        return self

    def device_sync(self) -> "Buffer":
        if self.raw.device_interface:
            _check(lib.halide_device_sync(None, self.ptr))
        return self

    def device_free(self) -> None:
        if self.raw.device:
            _check(lib.halide_device_free(None, self.ptr))

    def device_detach(self) -> None:
        if self.raw.device:
            _check(lib.halide_hip_detach_device_ptr(None, self.ptr))

    def numpy(self) -> np.ndarray:
        """Host array, after bringing device results back if the device copy is newer."""
        if self.device_dirty:
            self.copy_to_host()
        return self.array

    def __del__(self):
        try:
            if getattr(self, "raw", None) is not None and self.raw.device:
                lib.halide_device_free(None, C.byref(self.raw))
        except Exception:
            pass


def _as_ptr(b):
    if b is None:
        return None
    return b.ptr if isinstance(b, Buffer) else b


# ---------------------------------------------------------------------------------------------------
# pipelines — argument order and meaning exactly as in include/hlmi_pipelines.h
# apps/hannk's op library is built with C++ name mangling, every symbol in namespace hannk (include/aot/halide/<name>.h): the
# Itanium names of <name>, <name>_argv and <name>_metadata, the parameter lists spelled as the compiler spells them
# (P15halide_buffer_t the first buffer, S1_ every further one, h uint8_t, i int32_t)
_HANNK_CONV_PARAMS = "P15halide_buffer_thS1_hS1_iiiiiihhhS1_"
_HANNK_DW_PARAMS = "P15halide_buffer_thS1_hS1_iiiiiiihhhS1_"
_HANNK_PARAMS = {"tile_conv_filter_uint8": "P15halide_buffer_thhS1_", "conv_u8_u8_u8": _HANNK_CONV_PARAMS, "conv_u8_u8_i16": _HANNK_CONV_PARAMS,
                 "depthwise_conv_uint8": _HANNK_DW_PARAMS, "depthwise_conv_broadcast_uint8": _HANNK_DW_PARAMS}
HANNK_OPS = tuple(_HANNK_PARAMS)
# the pooling, reduction, elementwise and normalisation ops: s int16_t, t uint16_t, j uint32_t
_HANNK_POOL_PARAMS = "P15halide_buffer_tiiiihhS1_"
_HANNK_NN_PARAMS = {"average_pool_uint8": _HANNK_POOL_PARAMS, "max_pool_uint8": _HANNK_POOL_PARAMS, "mean_uint8": "P15halide_buffer_tiiiiiiiiS1_",
                    "add_uint8_uint8": "P15halide_buffer_thsS1_hshhhS1_", "mul_uint8_uint8_uint8": "P15halide_buffer_thS1_hhijhhS1_",
                    "softmax_uint8": "P15halide_buffer_tsthstS1_", "l2_normalization_uint8": "P15halide_buffer_thS1_"}
HANNK_NN_OPS = tuple(_HANNK_NN_PARAMS)
# the elementwise programs, the data movers and the shallow depthwise variant
_HANNK_PROGRAM_PARAMS = {"elementwise_5xuint8_1xuint8": "P15halide_buffer_t" + "S1_" * 6, "elementwise_5xint16_1xuint8int16": "P15halide_buffer_t" + "S1_" * 7,
                         "depthwise_conv_shallow_uint8": _HANNK_DW_PARAMS, "copy_uint8_uint8": "P15halide_buffer_tiS1_", "fill_uint8": "hP15halide_buffer_t", "upsample_channels_uint8": "P15halide_buffer_tiS1_"}
HANNK_PROGRAM_OPS = tuple(_HANNK_PROGRAM_PARAMS)
_HANNK_ALL_PARAMS = {**_HANNK_PARAMS, **_HANNK_NN_PARAMS, **_HANNK_PROGRAM_PARAMS}
# ctypes of a scalar argument by (halide type code, bits)
_SCALAR_CTYPES = {(2, 32): C.c_float, (2, 64): C.c_double, (0, 32): C.c_int32, (1, 8): C.c_uint8, (0, 16): C.c_int16, (1, 16): C.c_uint16,
                  (1, 32): C.c_uint32}


def _symbol(name, suffix=""):
    """The exported symbol of entry point `name` (+ "_argv" / "_metadata"): the name itself, or hannk's mangled one."""
    if name not in _HANNK_ALL_PARAMS:
        return name + suffix
    full = name + suffix
    return f"_ZN5hannk{len(full)}{full}E" + {"": _HANNK_ALL_PARAMS[name], "_argv": "PPv", "_metadata": "v"}[suffix]


def _bind(name):
    """The entry point `name` with the argtypes its own `<name>_metadata()` states (one table per entry point in the library:
    csrc/hlmi_internal.h); None when the library does not export it."""
    fn = getattr(lib, _symbol(name), None)
    if fn is None or getattr(lib, _symbol(name, "_metadata"), None) is None:
        return None
    md = metadata(name)
    argtypes = []
    for a in (md.arguments[i] for i in range(md.num_arguments)):
        t = _BP if a.kind != 0 else _SCALAR_CTYPES.get((a.type.code, a.type.bits))
        if t is None:
            raise ImportError(f"{name}: no ctypes type for scalar argument {a.name.decode()} (type code {a.type.code}, {a.type.bits} bits)")
        argtypes.append(t)
    fn.argtypes = argtypes
    fn.restype = C.c_int
    return fn


def metadata(name: str) -> halide_filter_metadata_t:
    fn = getattr(lib, _symbol(name, "_metadata"))
    fn.restype = C.POINTER(halide_filter_metadata_t)
    return fn().contents


RESIZE_KERNELS = ("box", "linear", "cubic", "lanczos")
_RESIZE_TYPES = {"float32": "float32", "uint8": "uint8", "uint16": "uint16"}
_fn = {name: _bind(name) for name in
       ["local_laplacian", "bilateral_grid", "halide_blur", "nl_means", "stencil_chain", "conv_layer", "conv_layer_bf16",
        "depthwise_separable_conv", "unsharp", "max_filter", "hist", "harris", "interpolate", "iir_blur", "lens_blur", "bgu",
        "camera_pipe"] + [f"resize_{k}_{t}_{d}" for k in RESIZE_KERNELS for t in _RESIZE_TYPES for d in ("up", "down")]
       + ["gaussian_blur_direct"] + [f"gaussian_blur_{u}_{d}_{f}" for u in (2, 3, 4) for d in (1, 2, 3) for f in (2, 4, 8, 16)]
       + ["linear_blur", "simple_blur"] + ["haar_x", "inverse_haar_x", "daubechies_x", "inverse_daubechies_x"] + ["compositing"]
       + ["conv3x3a16", "conv3x3a32", "dilate3x3", "median3x3", "gaussian5x5", "sobel"] + ["mat_mul"] + ["resnet50"]
       + ["fft_forward_r2c", "fft_inverse_c2r", "fft_forward_c2c", "fft_inverse_c2c"]
       + ["halide_scopy_impl", "halide_sscal_impl", "halide_saxpy_impl", "halide_sdot", "halide_sasum", "halide_sgemv_notrans",
          "halide_sgemv_trans", "halide_sger_impl", "halide_sgemm_notrans", "halide_sgemm_transA", "halide_sgemm_transB",
          "halide_sgemm_transAB"]
       + ["halide_dcopy_impl", "halide_dscal_impl", "halide_daxpy_impl", "halide_ddot", "halide_dasum", "halide_dgemv_notrans",
          "halide_dgemv_trans", "halide_dger_impl", "halide_dgemm_notrans", "halide_dgemm_transA", "halide_dgemm_transB",
          "halide_dgemm_transAB"]
       + list(HANNK_OPS) + list(HANNK_NN_OPS) + list(HANNK_PROGRAM_OPS)}


def local_laplacian(input, levels, alpha, beta, output) -> int:
    """apps/local_laplacian: u16 [W,H,3] -> u16 [W,H,3]; drivers pass alpha/(levels-1) (process.cpp:31)."""
    return _check(_fn["local_laplacian"](_as_ptr(input), int(levels), float(alpha), float(beta), _as_ptr(output)))


def debug_local_laplacian_outg(level: int) -> np.ndarray:
    """Test hook: outGPyramid[level] (restricted to the region R_level) of this thread's last
    local_laplacian call, as an (rh, rw) float32 array."""
    fn = lib.hlmi_debug_local_laplacian_outg
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    rw, rh = C.c_int(0), C.c_int(0)
    if fn(level, None, 0, C.byref(rw), C.byref(rh)) != 0:
        raise HalideError(-1, "no local_laplacian call to inspect")
    out = np.zeros((rh.value, rw.value), np.float32)
    if fn(level, out.ctypes.data_as(C.c_void_p), out.size, None, None) != 0:
        raise HalideError(-1, "debug copy failed")
    return out


def membench_naive(nbytes: int = 1 << 30, iters: int = 10, blocks: int = 0) -> dict:
    """The round-1/2 figure: naive grid-stride float4 copy / read-only / write-only kernels over buffers of `nbytes`."""
    fn = lib.hlmi_membench
    fn.restype = C.c_int
    fn.argtypes = [C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_double)]
    out = (C.c_double * 3)()
    _check(fn(int(nbytes), int(iters), int(blocks), out))
    return {"copy_gbs": out[0], "read_gbs": out[1], "write_gbs": out[2]}


def membench_sweep(nbytes: int = 1 << 30, iters: int = 10) -> dict:
    """Every (loads in flight, workgroups per CU, temporal policy) variant of the streaming kernels + hipMemcpyDtoD
    (csrc/membench.hip); the full table, as the library measured it."""
    import json
    fn = lib.hlmi_membench_sweep
    fn.restype = C.c_long
    fn.argtypes = [C.c_size_t, C.c_int, C.c_char_p, C.c_size_t]
    n = fn(int(nbytes), int(iters), None, 0)
    if n < 0:
        _check(int(n))
    buf = C.create_string_buffer(n + 16)
    fn(int(nbytes), int(iters), buf, n + 16)
    return json.loads(buf.value.decode())


def membench_widths(nbytes: int = 1 << 30, iters: int = 4) -> dict:
    """Read-only kernels that fetch `nbytes` exactly once with 4 / 8 / 16-byte aligned, 8-byte misaligned and overlapping
    8-byte loads: the known-bytes calibration runs for rocprofv3's FETCH_SIZE (csrc/membench.hip)."""
    fn = lib.hlmi_membench_widths
    fn.restype = C.c_int
    fn.argtypes = [C.c_size_t, C.c_int, C.POINTER(C.c_double)]
    out = (C.c_double * 5)()
    _check(fn(int(nbytes), int(iters), out))
    return dict(zip(("ld4_gbs", "ld8_gbs", "ld16_gbs", "ld8u_gbs", "ld8o_gbs"), (round(v, 1) for v in out)))


def membench(nbytes: int = 1 << 30, iters: int = 10, blocks: int = 0) -> dict:
    """Measurement hook: the practical HBM ceiling the pipelines' roofline fractions can be read against — the BEST copy /
    read-only / write-only rate over the sweep of streaming-kernel variants, beside the naive kernel's and hipMemcpyDtoD's."""
    naive = membench_naive(nbytes, iters, blocks)
    sw = membench_sweep(nbytes, iters)
    best = sw["best"]
    return {"copy_gbs": max(best["copy"]["gbs"], naive["copy_gbs"]), "read_gbs": max(best["read"]["gbs"], naive["read_gbs"]),
            "write_gbs": max(best["write"]["gbs"], naive["write_gbs"]), "best_variant": best,
            "naive": {k: round(v, 1) for k, v in naive.items()}, "memcpy_d2d_gbs": sw["memcpy_d2d_gbs"],
            "bytes_per_buffer": sw["bytes"], "guide_copy_gbs": 6290.0}


def bilateral_grid(input, r_sigma, output) -> int:
    return _check(_fn["bilateral_grid"](_as_ptr(input), float(r_sigma), _as_ptr(output)))


def halide_blur(input, blur_y) -> int:
    return _check(_fn["halide_blur"](_as_ptr(input), _as_ptr(blur_y)))


def nl_means(input, patch_size, search_area, sigma, output) -> int:
    return _check(_fn["nl_means"](_as_ptr(input), int(patch_size), int(search_area), float(sigma), _as_ptr(output)))


def stencil_chain(input, output) -> int:
    return _check(_fn["stencil_chain"](_as_ptr(input), _as_ptr(output)))


def conv_layer(input, filter, bias, relu) -> int:
    return _check(_fn["conv_layer"](_as_ptr(input), _as_ptr(filter), _as_ptr(bias), _as_ptr(relu)))


def conv_layer_bf16(input, filter, bias, relu) -> int:
    return _check(_fn["conv_layer_bf16"](_as_ptr(input), _as_ptr(filter), _as_ptr(bias), _as_ptr(relu)))


def depthwise_separable_conv(input, depthwise_filter, pointwise_filter, bias, output) -> int:
    return _check(_fn["depthwise_separable_conv"](_as_ptr(input), _as_ptr(depthwise_filter), _as_ptr(pointwise_filter), _as_ptr(bias), _as_ptr(output)))


def unsharp(input, output) -> int:
    return _check(_fn["unsharp"](_as_ptr(input), _as_ptr(output)))


def max_filter(input, output) -> int:
    return _check(_fn["max_filter"](_as_ptr(input), _as_ptr(output)))


def hist(input, output) -> int:
    return _check(_fn["hist"](_as_ptr(input), _as_ptr(output)))


def harris(input, output) -> int:
    return _check(_fn["harris"](_as_ptr(input), _as_ptr(output)))


def interpolate(input, output) -> int:
    return _check(_fn["interpolate"](_as_ptr(input), _as_ptr(output)))


def iir_blur(input, alpha, output) -> int:
    return _check(_fn["iir_blur"](_as_ptr(input), float(alpha), _as_ptr(output)))


def resize_variant(input, scale_factor, interpolation="cubic", upsample=None) -> str:
    """The AOT variant `resize` calls: element type from the buffer, kernel by name, direction from `upsample` (default:
    scale_factor > 1, the rule of the reference's driver, apps/resize/resize.cpp:126)."""
    if interpolation not in RESIZE_KERNELS:
        raise ValueError(f"interpolation must be one of {RESIZE_KERNELS}, not {interpolation!r}")
    raw = input.raw if isinstance(input, Buffer) else input.contents
    tname = {(2, 32): "float32", (1, 8): "uint8", (1, 16): "uint16"}.get((raw.type.code, raw.type.bits))
    if tname is None:
        raise TypeError("resize takes float32, uint8 or uint16 buffers")
    up = (float(scale_factor) > 1.0) if upsample is None else bool(upsample)
    return f"resize_{interpolation}_{tname}_{'up' if up else 'down'}"


def resize(input, scale_factor, output, interpolation="cubic", upsample=None) -> int:
    """apps/resize: planar [W,H,C] f32 / u8 / u16 -> the same type at the output's size; output x, y are absolute coordinates."""
    fn = _fn[resize_variant(input, scale_factor, interpolation, upsample)]
    return _check(fn(_as_ptr(input), float(scale_factor), _as_ptr(output)))


def debug_resize_general(variant: str, input, scale_factor, output) -> int:
    """Test and measurement hook: the named resize variant on its general two-launch path, whatever the sizes."""
    fn = lib.hlmi_resize_general
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p, _BP, C.c_float, _BP]
    return _check(fn(variant.encode(), _as_ptr(input), float(scale_factor), _as_ptr(output)))


def gaussian_blur_variant(upsample_order=3, downsample_order=2, factor=8) -> str:
    """The AOT variant `gaussian_blur` calls: gaussian_blur_<upsample_order>_<downsample_order>_<factor>, one of the 36 the
    reference's build generates (apps/gaussian_blur/Makefile)."""
    if upsample_order not in (2, 3, 4) or downsample_order not in (1, 2, 3) or factor not in (2, 4, 8, 16):
        raise ValueError(f"no gaussian_blur variant with upsample_order {upsample_order!r}, downsample_order {downsample_order!r}, "
                         f"factor {factor!r}: orders 2..4 and 1..3, factors 2, 4, 8, 16")
    return f"gaussian_blur_{int(upsample_order)}_{int(downsample_order)}_{int(factor)}"


def gaussian_blur_direct(input, sigma, trunc, output) -> int:
    """apps/gaussian_blur: f32 [W,H] -> f32, the separable blur of the edge-clamped input truncated at `trunc` sigmas; any
    output region."""
    return _check(_fn["gaussian_blur_direct"](_as_ptr(input), float(sigma), int(trunc), _as_ptr(output)))


def gaussian_blur(input, sigma, trunc, output, upsample_order=3, downsample_order=2, factor=8) -> int:
    """apps/gaussian_blur: reduce by `factor` (box spline of downsample_order), blur at low resolution, expand (box spline of
    upsample_order).  The output's mins are 0, its row stride a multiple of 16 and its host pointer 64-byte aligned:
    `aligned_array` makes one."""
    fn = _fn[gaussian_blur_variant(upsample_order, downsample_order, factor)]
    return _check(fn(_as_ptr(input), float(sigma), int(trunc), _as_ptr(output)))


def debug_gaussian_blur_general(variant: str, input, sigma, trunc, output) -> int:
    """Test and measurement hook: the named blur with its blur passes on the general path, whatever the sizes."""
    fn = lib.hlmi_gaussian_blur_general
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p, _BP, C.c_float, C.c_int32, _BP]
    return _check(fn(variant.encode(), _as_ptr(input), float(sigma), int(trunc), _as_ptr(output)))


def aligned_array(shape, dtype=np.float32, alignment=64, row_multiple=16) -> np.ndarray:
    """A zeroed C-order array of `shape` whose data pointer is a multiple of `alignment` bytes and whose row stride (the last
    axis but one) is a multiple of `row_multiple` elements: a view into a larger allocation, which `Buffer` wraps as it is.
    numpy's own allocations promise neither."""
    shape = tuple(int(n) for n in shape)
    dtype = np.dtype(dtype)
    row = -(-shape[-1] // row_multiple) * row_multiple
    padded = shape[:-1] + (row,)
    raw = np.zeros(int(np.prod(padded)) * dtype.itemsize + alignment, np.uint8)
    off = -raw.ctypes.data % alignment
    return raw[off:off + int(np.prod(padded)) * dtype.itemsize].view(dtype).reshape(padded)[..., :shape[-1]]


def linear_blur(input, output) -> int:
    """apps/linear_blur: f32 [W,H,C] sRGB -> f32, the 3x3 box blur over x .. x + 2, y .. y + 2 in linear light; the clamp is to the
    input's extents; any output region."""
    return _check(_fn["linear_blur"](_as_ptr(input), _as_ptr(output)))


def simple_blur(input, width, height, output) -> int:
    """apps/linear_blur's simple_blur: f32 [W,H,C] -> f32, the same blur on the values as they are, the input clamped to
    [0, width) x [0, height); any output region."""
    return _check(_fn["simple_blur"](_as_ptr(input), int(width), int(height), _as_ptr(output)))


def debug_linear_blur_general(name: str, input, width, height, output) -> int:
    """Test and measurement hook: "linear_blur" or "simple_blur" as the unfused composition (three launches / one), whatever the
    sizes; linear_blur does not read width and height."""
    fn = lib.hlmi_linear_blur_general
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p, _BP, C.c_int32, C.c_int32, _BP]
    return _check(fn(name.encode(), _as_ptr(input), int(width), int(height), _as_ptr(output)))


def haar_x(input, output) -> int:
    """apps/wavelet: f32 [W,H] -> f32 [W/2,H,c]; plane 0 the pair means, any other plane the half differences; any output region."""
    return _check(_fn["haar_x"](_as_ptr(input), _as_ptr(output)))


def inverse_haar_x(input, output) -> int:
    """apps/wavelet: f32 [W2,H,2] -> f32 [2*W2,H], the inverse of haar_x; reads clamp into the input's own box."""
    return _check(_fn["inverse_haar_x"](_as_ptr(input), _as_ptr(output)))


def daubechies_x(input, output) -> int:
    """apps/wavelet: f32 [W,H] -> f32 [W/2,H,c], the D4 low-pass (plane 0) and high-pass over samples 2x - 1 .. 2x + 2."""
    return _check(_fn["daubechies_x"](_as_ptr(input), _as_ptr(output)))


def inverse_daubechies_x(input, output) -> int:
    """apps/wavelet: f32 [W2,H,2] -> f32 [2*W2,H] from pairs x/2 and x/2 + 1; reconstructs daubechies_x's input one sample on."""
    return _check(_fn["inverse_daubechies_x"](_as_ptr(input), _as_ptr(output)))


def debug_wavelet_general(name: str, input, output) -> int:
    """Test and measurement hook: the named wavelet entry point with one thread per output and clamped scalar taps."""
    fn = lib.hlmi_wavelet_general
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p, _BP, _BP]
    return _check(fn(name.encode(), _as_ptr(input), _as_ptr(output)))


def compositing(layers, ops, output) -> int:
    """apps/compositing: six u8 [W,H,4] layers blended by five int32 op codes (0 over, 1 atop, 2 xor, 3 in, 4 out, anything else
    skips the layer) into u8 [W,H,4]; the generator's integer form (include/hlmi_pipelines.h)."""
    if len(layers) != 6:
        raise ValueError(f"compositing takes six layers, not {len(layers)}")
    return _check(_fn["compositing"](*[_as_ptr(l) for l in layers], _as_ptr(ops), _as_ptr(output)))


def debug_compositing_general(layers, ops, output) -> int:
    """Test and measurement hook: compositing with one thread per pixel and byte loads."""
    if len(layers) != 6:
        raise ValueError(f"compositing takes six layers, not {len(layers)}")
    fn = lib.hlmi_compositing_general
    fn.restype = C.c_int
    fn.argtypes = [_BP] * 8
    return _check(fn(*[_as_ptr(l) for l in layers], _as_ptr(ops), _as_ptr(output)))


HEXAGON_BENCHMARKS = ("conv3x3a16", "conv3x3a32", "dilate3x3", "median3x3", "gaussian5x5", "sobel")


def conv3x3a16(input, mask, output) -> int:
    """apps/hexagon_benchmarks: u8 [W,H] under an int8 3x3 mask, the sum wrapped to int16, u8(clamp(sum >> 4, 0, 255)); the input is
    edge-clamped to its own box (include/hlmi_pipelines.h)."""
    return _check(_fn["conv3x3a16"](_as_ptr(input), _as_ptr(mask), _as_ptr(output)))


def conv3x3a32(input, mask, output) -> int:
    """apps/hexagon_benchmarks: conv3x3a16 with the sum in int32."""
    return _check(_fn["conv3x3a32"](_as_ptr(input), _as_ptr(mask), _as_ptr(output)))


def dilate3x3(input, output) -> int:
    """apps/hexagon_benchmarks: u8 [W,H] -> u8, the maximum of the 3x3 window of the edge-clamped input."""
    return _check(_fn["dilate3x3"](_as_ptr(input), _as_ptr(output)))


def median3x3(input, output) -> int:
    """apps/hexagon_benchmarks: u8 [W,H] -> u8, the median of the 3x3 window of the edge-clamped input."""
    return _check(_fn["median3x3"](_as_ptr(input), _as_ptr(output)))


def gaussian5x5(input, output) -> int:
    """apps/hexagon_benchmarks: u8 [W,H] -> u8, the (1, 4, 6, 4, 1) x (1, 4, 6, 4, 1) window of the edge-clamped input over 256,
    truncated."""
    return _check(_fn["gaussian5x5"](_as_ptr(input), _as_ptr(output)))


def sobel(input, output) -> int:
    """apps/hexagon_benchmarks: u8 [W,H] -> u8, min(|gx| + |gy|, 255) of the edge-clamped input, no square root; the output region
    may lie anywhere."""
    return _check(_fn["sobel"](_as_ptr(input), _as_ptr(output)))


def debug_hexagon_benchmarks_general(name: str, input, mask, output) -> int:
    """Test and measurement hook: the named hexagon_benchmarks entry point with one thread per output pixel and clamped taps from
    global memory; `mask` is None for the four filters that take none."""
    fn = lib.hlmi_hexagon_benchmarks_general
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p, _BP, _BP, _BP]
    return _check(fn(name.encode(), _as_ptr(input), _as_ptr(mask), _as_ptr(output)))


def mat_mul(A, B, out) -> int:
    """apps/cuda_mat_mul at the size the reference builds (1024): f32 [1024, 1024] x 2 -> f32, out(x, y) the k-ordered fmaf chain over
    r of A(x, r) * B(r, y) from +0.  Dimension 0 is innermost: with row-major arrays out = B @ A, not A @ B."""
    return _check(_fn["mat_mul"](_as_ptr(A), _as_ptr(B), _as_ptr(out)))


def _mat_mul_hook(symbol):
    fn = getattr(lib, symbol)
    fn.restype = C.c_int
    fn.argtypes = [C.c_int32, _BP, _BP, _BP]
    return fn


def mat_mul_sized(size, A, B, out) -> int:
    """mat_mul as the generator instantiated at another size, 1 .. 8192: the same shim, plan and rules, every buffer
    [0, size) x [0, size) (csrc/hlmi_internal.h)."""
    return _check(_mat_mul_hook("hlmi_mat_mul_sized")(int(size), _as_ptr(A), _as_ptr(B), _as_ptr(out)))


def debug_mat_mul_general(size, A, B, out) -> int:
    """Test and measurement hook: mat_mul_sized with one thread per output running a plain fmaf loop."""
    return _check(_mat_mul_hook("hlmi_mat_mul_general")(int(size), _as_ptr(A), _as_ptr(B), _as_ptr(out)))


# apps/resnet_50: the f32 ResNet-50 forward pass (include/hlmi_pipelines.h).  Arrays are the Halide dimensions reversed: the image is
# (224, 224, 3), a convolution's weights (CI, KH, KW, CO), fc1000_weights (2048, 1000).
def _resnet50_group(suffix, conv=""):
    return ([f"conv1_{suffix}"] + [f"br1_{conv}{suffix}_{i}" for i in range(4)]
            + [f"{b}_{conv}{suffix}_{i}" for b in ("br2a", "br2b", "br2c") for i in range(16)])


# the 267 arguments between `input` and `final_output`, in signature order (Resnet50Generator.cpp:31-66)
RESNET50_PARAM_NAMES = tuple(sum((_resnet50_group(s) for s in ("gamma", "beta", "mu", "sig")), [])
                             + ["conv1_weights"] + _resnet50_group("weights", "conv_")[1:] + ["fc1000_weights", "fc1000_bias"])
RESNET50_BLOCKS = (3, 4, 6, 3)   # bottleneck blocks per stage; br1 exists in the first block of each


def _resnet50_args(input, params, output):
    if isinstance(params, dict):
        missing = [n for n in RESNET50_PARAM_NAMES if n not in params]
        if missing or len(params) != len(RESNET50_PARAM_NAMES):
            raise ValueError(f"resnet50: parameters missing {missing[:4]}, unknown {[k for k in params if k not in RESNET50_PARAM_NAMES][:4]}")
        params = [params[n] for n in RESNET50_PARAM_NAMES]
    if len(params) != len(RESNET50_PARAM_NAMES):
        raise ValueError(f"resnet50 takes {len(RESNET50_PARAM_NAMES)} parameters, not {len(params)}")
    return [_as_ptr(input)] + [_as_ptr(b) for b in params] + [_as_ptr(output)]


def resnet50(input, params, output) -> int:
    """apps/resnet_50: f32 [3, 224, 224] and the 267 parameters -> the softmax probabilities of the classes in `output`'s box, any box
    inside [0, 1000).  `params`: a sequence in signature order (RESNET50_PARAM_NAMES) or a dict by argument name."""
    return _check(_fn["resnet50"](*_resnet50_args(input, params, output)))


def debug_resnet50_general(input, params, output) -> int:
    """Test and measurement hook: resnet50 with every convolution on the one-thread-per-output kernel."""
    fn = lib.hlmi_resnet50_general
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(C.c_void_p)]
    args = _resnet50_args(input, params, output)
    return _check(fn((C.c_void_p * len(args))(*[None if a is None else C.cast(a, C.c_void_p) for a in args])))


RESNET50_LAYER_MODES = ("raw", "scaled", "scaled_relu", "residual_relu")


def debug_resnet50_layer(input, weights, gamma, beta, mu, sig, residual, stride, pad, mode, output, general_only=False) -> int:
    """Test and measurement hook: ONE convolution layer of any shape through resnet50's plan and kernels.  input [CI, W, H], weights
    [CO, KW, KH, CI], four vectors [CO], output [CO, OW, OH]; mode: an index into or a name of RESNET50_LAYER_MODES; residual is read
    in the last mode only (None otherwise)."""
    fn = lib.hlmi_debug_resnet50_layer
    fn.restype, fn.argtypes = C.c_int, [_BP] * 7 + [C.c_int32] * 4 + [_BP]
    mode = RESNET50_LAYER_MODES.index(mode) if isinstance(mode, str) else int(mode)
    return _check(fn(*[_as_ptr(b) for b in (input, weights, gamma, beta, mu, sig, residual)], int(stride), int(pad), mode, int(bool(general_only)),
                     _as_ptr(output)))


def debug_resnet50_maxpool(input, k, stride, pad, output) -> int:
    """Test hook: resnet50's max pool with a k x k window at any size, [C, W, H] -> [C, OW, OH]."""
    fn = lib.hlmi_debug_resnet50_maxpool
    fn.restype, fn.argtypes = C.c_int, [_BP, C.c_int32, C.c_int32, C.c_int32, _BP]
    return _check(fn(_as_ptr(input), int(k), int(stride), int(pad), _as_ptr(output)))


def debug_resnet50_tail(input, fc_weights, fc_bias, output) -> int:
    """Test hook: resnet50's tail at any size: [C, W, H] -> mean over W x H -> fc (weights [N, C], bias [N]) -> softmax -> [N]."""
    fn = lib.hlmi_debug_resnet50_tail
    fn.restype, fn.argtypes = C.c_int, [_BP] * 4
    return _check(fn(*[_as_ptr(b) for b in (input, fc_weights, fc_bias, output)]))


def _resnet50_keys():
    """{argument name: state-dict key}, the way the reference's process.cpp:143-239 names its files (dots for underscores)"""
    keys = {"conv1_weights": "conv1.weight", "fc1000_weights": "fc.weight", "fc1000_bias": "fc.bias"}
    bn = {"gamma": "weight", "beta": "bias", "mu": "running_mean", "sig": "running_var"}
    for s, k in bn.items():
        keys[f"conv1_{s}"] = f"bn1.{k}"
    block = 0
    for stage, n in enumerate(RESNET50_BLOCKS):
        for i in range(n):
            layer = f"layer{stage + 1}.{i}"
            if i == 0:
                keys[f"br1_conv_weights_{stage}"] = f"{layer}.downsample.0.weight"
                for s, k in bn.items():
                    keys[f"br1_{s}_{stage}"] = f"{layer}.downsample.1.{k}"
            for j, br in enumerate(("br2a", "br2b", "br2c")):
                keys[f"{br}_conv_weights_{block}"] = f"{layer}.conv{j + 1}.weight"
                for s, k in bn.items():
                    keys[f"{br}_{s}_{block}"] = f"{layer}.bn{j + 1}.{k}"
            block += 1
    return keys


RESNET50_STATE_DICT_KEYS = _resnet50_keys()


def resnet50_params_from_state_dict(sd) -> dict:
    """{argument name: float32 array} from a torchvision-style ResNet-50 state dict (tensors or arrays): 4-D weights (co, ci, h, w)
    transposed (1, 2, 3, 0) to Halide's (co, kx, ky, ci) innermost first, fc.weight transposed, as the reference's load_weights.py
    does; keys the network does not read (num_batches_tracked) are ignored."""
    out = {}
    for name in RESNET50_PARAM_NAMES:
        v = sd[RESNET50_STATE_DICT_KEYS[name]]
        a = np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v).astype(np.float32)
        if a.ndim == 4:
            a = a.transpose(1, 2, 3, 0)
        elif a.ndim == 2:
            a = a.transpose(1, 0)
        out[name] = np.ascontiguousarray(a)
    return out


def resnet50_load_weight_dir(path) -> dict:
    """{argument name: float32 array} from a directory of the reference's `<key>.data` + `<key>_shape.data` pairs (process.cpp:45-72;
    `<key>`: the state-dict key with dots replaced by underscores; the shape file: int32 count, then the Halide extents, innermost
    first)."""
    out = {}
    for name in RESNET50_PARAM_NAMES:
        base = os.path.join(path, RESNET50_STATE_DICT_KEYS[name].replace(".", "_"))
        shape = np.fromfile(base + "_shape.data", dtype=np.int32)
        if shape.size < 1 or shape[0] != shape.size - 1:
            raise ValueError(f"{base}_shape.data: not a shape file")
        data = np.fromfile(base + ".data", dtype=np.float32)
        extents = [int(e) for e in shape[1:]]
        if data.size != int(np.prod(extents)):
            raise ValueError(f"{base}.data: {data.size} floats for extents {extents}")
        out[name] = data.reshape(extents[::-1])
    return out


# apps/fft: the four objects the reference builds (16 x 16) and the generator at other sizes and gains (include/hlmi_pipelines.h).  A
# complex array with Halide extents (N0, rows, 2) is a numpy array of shape (rows, N0, 2), a real one (rows, N0, 1).
FFT_KINDS = ("c2c_forward", "c2c_inverse", "r2c", "c2r")


def fft_forward_r2c(input, output) -> int:
    """real [16, 16, 1] -> complex [16, 9, 2], gain 1/256"""
    return _check(_fn["fft_forward_r2c"](_as_ptr(input), _as_ptr(output)))


def fft_inverse_c2r(input, output) -> int:
    """complex [16, >= 9, 2] -> real [16, 16, 1], gain 1"""
    return _check(_fn["fft_inverse_c2r"](_as_ptr(input), _as_ptr(output)))


def fft_forward_c2c(input, output) -> int:
    """complex [16, 16, 2] -> complex [16, 16, 2], sign -1, gain 1/256"""
    return _check(_fn["fft_forward_c2c"](_as_ptr(input), _as_ptr(output)))


def fft_inverse_c2c(input, output) -> int:
    """complex [16, 16, 2] -> complex [16, 16, 2], sign +1, gain 1"""
    return _check(_fn["fft_inverse_c2c"](_as_ptr(input), _as_ptr(output)))


def _fft_hook(symbol):
    fn = getattr(lib, symbol)
    fn.restype = C.c_int
    fn.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_float, _BP, _BP]
    return fn


def fft_buffer(array) -> "Buffer":
    """A numpy array of shape (rows, N0, 2) (complex: re, im), (rows, N0, 1) or (rows, N0) (real) as the generator's buffer: dimension
    0 along N0, dimension 1 the rows, dimension 2 the components with stride 1.  No copy: the rows may be padded."""
    a = array if array.ndim == 3 else array.reshape(array.shape + (1,)) if array.flags.c_contiguous else array[..., None]
    b = Buffer(a)
    d = [(x.min, x.extent, x.stride) for x in (b._dims[1], b._dims[2], b._dims[0])]
    for i, (mn, ext, st) in enumerate(d):
        b._dims[i] = halide_dimension_t(mn, ext, 1 if i == 2 and ext == 1 else st, 0)
    return b


def _fft_sizes(kind, input, output):
    """N0 and N1 from the buffers: N0 is the output's extent 0, N1 the rows of the side that is not halved"""
    full = output if kind == "c2r" else input
    return int(output.dim(0).extent), int(full.dim(1).extent)


def fft2d(kind, input, output, gain=1.0, sizes=None) -> int:
    """The transform `kind` (one of FFT_KINDS) with the sizes taken from the buffers (or given as (N0, N1)): each 2 .. 4096 with
    radix factors 8, 6, 4, 2 only, both even for r2c and c2r."""
    n0, n1 = _fft_sizes(kind, input, output) if sizes is None else sizes
    return _check(_fft_hook("hlmi_fft2d")(FFT_KINDS.index(kind), n0, n1, float(gain), _as_ptr(input), _as_ptr(output)))


def debug_fft2d_general(kind, input, output, gain=1.0, sizes=None) -> int:
    """Test and measurement hook: fft2d with one thread per 1-D line, every pass in full through the scratch arena."""
    n0, n1 = _fft_sizes(kind, input, output) if sizes is None else sizes
    return _check(_fft_hook("hlmi_fft2d_general")(FFT_KINDS.index(kind), n0, n1, float(gain), _as_ptr(input), _as_ptr(output)))


def fft_radix_factor(n):
    """radix_factor(n) as the library holds it"""
    R = (C.c_int32 * 16)()
    lib.hlmi_fft_radix_factor.restype, lib.hlmi_fft_radix_factor.argtypes = C.c_int, [C.c_int32, C.POINTER(C.c_int32)]
    return list(R[:lib.hlmi_fft_radix_factor(int(n), R)])


def fft_size_ok(n) -> bool:
    lib.hlmi_fft_size_ok.restype, lib.hlmi_fft_size_ok.argtypes = C.c_int, [C.c_int32]
    return bool(lib.hlmi_fft_size_ok(int(n)))


def fft_twiddles_address() -> int:
    """the address of hlmi_fft_twiddles, the host function behind every twiddle table (tests/fft_checker.py: use_twiddles)"""
    return C.cast(lib.hlmi_fft_twiddles, C.c_void_p).value


# apps/linear_algebra: the f32 BLAS subset (include/hlmi_pipelines.h, include/hlmi_blas.h).  Vectors are 1-D buffers; a matrix with
# Halide extents (w, h) is column-major, i.e. a numpy array of shape (h, w).  Where `result` / `output` is left out the call is the
# wrapper's of hlmi_blas.h: in place on y (x for sscal, C for sgemm).
LINEAR_ALGEBRA = ("halide_scopy_impl", "halide_sscal_impl", "halide_saxpy_impl", "halide_sdot", "halide_sasum", "halide_sgemv_notrans",
                  "halide_sgemv_trans", "halide_sger_impl", "halide_sgemm_notrans", "halide_sgemm_transA", "halide_sgemm_transB",
                  "halide_sgemm_transAB")


def scopy(x, result) -> int:
    """result(i) = x(i)"""
    return _check(_fn["halide_scopy_impl"](0.0, _as_ptr(x), None, _as_ptr(result)))


def sscal(a, x, result=None) -> int:
    """result(i) = a * x(i); in place on x by default"""
    return _check(_fn["halide_sscal_impl"](float(a), _as_ptr(x), None, _as_ptr(x if result is None else result)))


def saxpy(a, x, y, result=None) -> int:
    """result(i) = a * x(i) + y(i); in place on y by default"""
    return _check(_fn["halide_saxpy_impl"](float(a), _as_ptr(x), _as_ptr(y), _as_ptr(y if result is None else result)))


def sdot(x, y, result) -> int:
    """result() = the V = 8 lane-chain dot product of the contract; result is a 0-dimensional buffer"""
    return _check(_fn["halide_sdot"](_as_ptr(x), _as_ptr(y), _as_ptr(result)))


def sasum(x, result) -> int:
    """result() = the sum of |x(i)| in the contract's order"""
    return _check(_fn["halide_sasum"](_as_ptr(x), _as_ptr(result)))


def sgemv(trans, a, A, x, b, y, output=None) -> int:
    """output = a op(A) x + b y for A of extents (M, N): notrans x[N], y[M]; trans x[M], y[N]; in place on y by default"""
    name = "halide_sgemv_trans" if trans else "halide_sgemv_notrans"
    return _check(_fn[name](float(a), _as_ptr(A), _as_ptr(x), float(b), _as_ptr(y), _as_ptr(y if output is None else output)))


def sger(a, x, y, result) -> int:
    """result(i, j) += (a * y(j)) * x(i), in place"""
    return _check(_fn["halide_sger_impl"](float(a), _as_ptr(x), _as_ptr(y), _as_ptr(result)))


def sgemm_name(transA, transB) -> str:
    return "halide_sgemm_" + ("transAB" if transA and transB else "transA" if transA else "transB" if transB else "notrans")


def sgemm(transA, transB, a, A, B, b, C, result=None) -> int:
    """result = a op(A) op(B) + b C, k upward; a transposed operand must be square; in place on C by default"""
    return _check(_fn[sgemm_name(transA, transB)](float(a), _as_ptr(A), _as_ptr(B), float(b), _as_ptr(C), _as_ptr(C if result is None else result)))


def _linear_algebra_hook():
    fn = lib.hlmi_linear_algebra_general
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p, C.c_float, C.c_float, _BP, _BP, _BP, _BP]
    return fn


def debug_linear_algebra_general(name: str, *args) -> int:
    """Test and measurement hook: the entry point `name` of LINEAR_ALGEBRA, with the arguments of its C signature in order, with one
    thread per output running the chain as written."""
    if name not in LINEAR_ALGEBRA:
        raise ValueError(f"no linear_algebra entry point named {name}")
    md = metadata(name)
    if len(args) != md.num_arguments:
        raise TypeError(f"{name} takes {md.num_arguments} arguments, not {len(args)}")
    scalars = [float(v) for v, i in zip(args, range(md.num_arguments)) if md.arguments[i].kind == 0]
    bufs = [_as_ptr(v) for v, i in zip(args, range(md.num_arguments)) if md.arguments[i].kind != 0]
    if name in ("halide_scopy_impl", "halide_sscal_impl", "halide_saxpy_impl", "halide_sger_impl"):
        a, b = scalars[0], 0.0
    elif name in ("halide_sdot", "halide_sasum"):
        a, b = 0.0, 0.0
    else:
        a, b = scalars
    bufs += [None] * (4 - len(bufs))
    return _check(_linear_algebra_hook()(name.encode(), a, b, *bufs))


def debug_sgemm_general(transA, transB, a, A, B, b, C, result=None) -> int:
    return debug_linear_algebra_general(sgemm_name(transA, transB), a, A, B, b, C, C if result is None else result)


def debug_sgemv_general(trans, a, A, x, b, y, output=None) -> int:
    return debug_linear_algebra_general("halide_sgemv_trans" if trans else "halide_sgemv_notrans", a, A, x, b, y, y if output is None else output)


# apps/linear_algebra, the f64 half: the same calls on float64 buffers with double scalars; the lane width of ddot, dasum and dgemv_trans
# is LINEAR_ALGEBRA_F64_V = 4 (natural_vector_size(double) of the reference's AVX2 build), against 8 for the f32 half.
LINEAR_ALGEBRA_F64 = ("halide_dcopy_impl", "halide_dscal_impl", "halide_daxpy_impl", "halide_ddot", "halide_dasum", "halide_dgemv_notrans",
                      "halide_dgemv_trans", "halide_dger_impl", "halide_dgemm_notrans", "halide_dgemm_transA", "halide_dgemm_transB",
                      "halide_dgemm_transAB")
LINEAR_ALGEBRA_F64_V = 4


def dcopy(x, result) -> int:
    """result(i) = x(i)"""
    return _check(_fn["halide_dcopy_impl"](0.0, _as_ptr(x), None, _as_ptr(result)))


def dscal(a, x, result=None) -> int:
    """result(i) = a * x(i); in place on x by default"""
    return _check(_fn["halide_dscal_impl"](float(a), _as_ptr(x), None, _as_ptr(x if result is None else result)))


def daxpy(a, x, y, result=None) -> int:
    """result(i) = a * x(i) + y(i); in place on y by default"""
    return _check(_fn["halide_daxpy_impl"](float(a), _as_ptr(x), _as_ptr(y), _as_ptr(y if result is None else result)))


def ddot(x, y, result) -> int:
    """result() = the V = 4 lane-chain dot product of the contract; result is a 0-dimensional buffer"""
    return _check(_fn["halide_ddot"](_as_ptr(x), _as_ptr(y), _as_ptr(result)))


def dasum(x, result) -> int:
    """result() = the sum of |x(i)| in the contract's order"""
    return _check(_fn["halide_dasum"](_as_ptr(x), _as_ptr(result)))


def dgemv(trans, a, A, x, b, y, output=None) -> int:
    """output = a op(A) x + b y for A of extents (M, N): notrans x[N], y[M]; trans x[M], y[N]; in place on y by default"""
    name = "halide_dgemv_trans" if trans else "halide_dgemv_notrans"
    return _check(_fn[name](float(a), _as_ptr(A), _as_ptr(x), float(b), _as_ptr(y), _as_ptr(y if output is None else output)))


def dger(a, x, y, result) -> int:
    """result(i, j) += (a * y(j)) * x(i), in place"""
    return _check(_fn["halide_dger_impl"](float(a), _as_ptr(x), _as_ptr(y), _as_ptr(result)))


def dgemm_name(transA, transB) -> str:
    return "halide_dgemm_" + ("transAB" if transA and transB else "transA" if transA else "transB" if transB else "notrans")


def dgemm(transA, transB, a, A, B, b, C, result=None) -> int:
    """result = a op(A) op(B) + b C, k upward; a transposed operand must be square; in place on C by default"""
    return _check(_fn[dgemm_name(transA, transB)](float(a), _as_ptr(A), _as_ptr(B), float(b), _as_ptr(C), _as_ptr(C if result is None else result)))


def debug_linear_algebra_general_f64(name: str, *args) -> int:
    """Test and measurement hook: the entry point `name` of LINEAR_ALGEBRA_F64, with the arguments of its C signature in order, with
    one thread per output running the chain as written."""
    if name not in LINEAR_ALGEBRA_F64:
        raise ValueError(f"no f64 linear_algebra entry point named {name}")
    md = metadata(name)
    if len(args) != md.num_arguments:
        raise TypeError(f"{name} takes {md.num_arguments} arguments, not {len(args)}")
    scalars = [float(v) for v, i in zip(args, range(md.num_arguments)) if md.arguments[i].kind == 0]
    bufs = [_as_ptr(v) for v, i in zip(args, range(md.num_arguments)) if md.arguments[i].kind != 0]
    a, b = (scalars + [0.0, 0.0])[:2]
    bufs += [None] * (4 - len(bufs))
    fn = lib.hlmi_linear_algebra_general_f64
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p, C.c_double, C.c_double, _BP, _BP, _BP, _BP]
    return _check(fn(name.encode(), a, b, *bufs))


# apps/hannk's op library: the quantised convolution pair and the filter re-tiler (include/aot/halide/<name>.h).
# Arrays are the Halide dimensions reversed: an activation [c, x, y, b] is an array of shape (B, H, W, C) — NHWC —, the tiled filter
# [4, 16, ci / 4, co / 16, fx, fy] one of shape (FH, FW, CO16, CQ, 16, 4), a depthwise filter [c, fx, fy] one of shape (FH, FW, C).
HANNK_VECTOR_REDUCTION, HANNK_ACCUM_VECTOR_SIZE, HANNK_DEPTHWISE_VECTOR = 4, 16, 16


def tile_conv_filter_uint8(input, input_zero, output_zero, output) -> int:
    """u8 [ci, x, y, co] -> the u8 [4, 16, ci / 4, co / 16, x, y] filter conv_u8_u8_* reads; entries outside the input are output_zero."""
    return _check(_fn["tile_conv_filter_uint8"](_as_ptr(input), int(input_zero), int(output_zero), _as_ptr(output)))


def _hannk_conv_args(input, input_zero, filter, filter_zero, bias, stride, dilation, extra, multiplier, shift, output_zero, output_min, output_max,
                     output):
    return ([_as_ptr(input), int(input_zero), _as_ptr(filter), int(filter_zero), _as_ptr(bias), int(stride[0]), int(stride[1]), int(dilation[0]),
             int(dilation[1])] + extra + [int(multiplier), int(shift), int(output_zero), int(output_min), int(output_max), _as_ptr(output)])


def conv_u8_u8_u8(input, input_zero, filter, filter_zero, bias, stride, dilation, multiplier, shift, output_zero, output_min, output_max, output) -> int:
    """input u8 [c, x, y, b], tiled filter, bias i32 [c] -> u8 [c, x, y, b]; stride and dilation are (x, y) pairs."""
    return _check(_fn["conv_u8_u8_u8"](*_hannk_conv_args(input, input_zero, filter, filter_zero, bias, stride, dilation, [], multiplier, shift,
                                                         output_zero, output_min, output_max, output)))


def conv_u8_u8_i16(input, input_zero, filter, filter_zero, bias, stride, dilation, multiplier, shift, output_zero, output_min, output_max, output) -> int:
    """conv_u8_u8_u8 with an int16 output: quantize_i16 only, output_zero / min / max are not read."""
    return _check(_fn["conv_u8_u8_i16"](*_hannk_conv_args(input, input_zero, filter, filter_zero, bias, stride, dilation, [], multiplier, shift,
                                                          output_zero, output_min, output_max, output)))


def depthwise_conv_uint8(input, input_zero, filter, filter_zero, bias, stride, dilation, multiplier, shift, output_zero, output_min, output_max, output,
                         input_stride_x=0) -> int:
    """input u8 [c, x, y, b] (channels padded to a multiple of 16), filter u8 [c, fx, fy], bias i32 [c] -> u8 [c, x, y, b]."""
    return _check(_fn["depthwise_conv_uint8"](*_hannk_conv_args(input, input_zero, filter, filter_zero, bias, stride, dilation, [int(input_stride_x)],
                                                                multiplier, shift, output_zero, output_min, output_max, output)))


def depthwise_conv_broadcast_uint8(input, input_zero, filter, filter_zero, bias, stride, dilation, multiplier, shift, output_zero, output_min,
                                   output_max, output, input_stride_x=0) -> int:
    """depthwise_conv_uint8 with the input's one channel feeding every output channel."""
    return _check(_fn["depthwise_conv_broadcast_uint8"](*_hannk_conv_args(input, input_zero, filter, filter_zero, bias, stride, dilation,
                                                                          [int(input_stride_x)], multiplier, shift, output_zero, output_min, output_max,
                                                                          output)))


def debug_hannk_general(name: str, *args) -> int:
    """Test and measurement hook: the entry point `name` of HANNK_OPS, HANNK_NN_OPS or HANNK_PROGRAM_OPS, with the arguments of its C signature in order
    (stride and dilation as four scalars), with one thread per output running the contract's loops as written."""
    if name not in _HANNK_ALL_PARAMS:
        raise ValueError(f"no hannk entry point named {name}")
    md = metadata(name)
    if len(args) != md.num_arguments:
        raise TypeError(f"{name} takes {md.num_arguments} arguments, not {len(args)}")
    keep, argv = [], (C.c_void_p * md.num_arguments)()
    for j, v in enumerate(args):
        a = md.arguments[j]
        box = _SCALAR_CTYPES[(a.type.code, a.type.bits)](int(v)) if a.kind == 0 else (v.raw if isinstance(v, Buffer) else v.contents)
        keep.append(box)
        argv[j] = C.cast(C.pointer(box), C.c_void_p)
    fn = lib.hlmi_hannk_general
    fn.restype, fn.argtypes = C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]
    return _check(fn(name.encode(), argv))


def debug_hannk_quantize(fn, acc, multiplier, shift, zero=0, lo=0, hi=255) -> np.ndarray:
    """Test hook: the device's epilogue alone on an int32 array: fn 0 or "i16" = quantize_i16 (int16 result), fn 1 or "u8" =
    quantize_and_relu_u8 (uint8 result)."""
    fn = {"i16": 0, "u8": 1}.get(fn, fn)
    acc = np.ascontiguousarray(acc, np.int32)
    out = np.zeros(acc.shape, np.int16 if fn == 0 else np.uint8)
    f = lib.hlmi_debug_hannk_quantize
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.c_uint8, C.c_uint8, C.c_uint8, C.c_void_p]
    rc = f(int(fn), acc.ctypes.data, acc.size, int(multiplier), int(shift), int(zero), int(lo), int(hi), out.ctypes.data)
    if rc != 0:
        raise HalideError(-1, f"hlmi_debug_hannk_quantize failed ({rc})")
    return out


def debug_hannk_conv_plan(npix, channels, quads, cus=256) -> dict:
    """What conv_u8_u8_*'s plan chooses for `npix` output pixels, `channels` output channels and `quads` = fw * fh * ci / 4 on `cus`
    compute units (aligned operands; HLMI_HANNK_SPLIT_K is read as in a call)."""
    out = (C.c_int32 * 3)()
    f = lib.hlmi_debug_hannk_conv_plan
    f.restype, f.argtypes = C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    if f(int(npix), int(channels), int(quads), int(cus), out) != 0:
        raise ValueError("hlmi_debug_hannk_conv_plan: sizes must be positive")
    return {"mfma": bool(out[0]), "splits": int(out[1]), "wave_tiles": int(out[2])}


def _pair(v):
    return (int(v), int(v)) if np.isscalar(v) else (int(v[0]), int(v[1]))


def hannk_conv_out_extent(size, filt, stride, dilation, padding) -> int:
    """outputs along one axis: the positions x with x * stride + (filt - 1) * dilation inside the padded input"""
    return (int(size) + 2 * int(padding) - (int(filt) - 1) * int(dilation) - 1) // int(stride) + 1


def hannk_pad_input(input, input_zero, channel_multiple, padding) -> np.ndarray:
    """What the interpreter does to an activation before a conv op: (B, H, W, C) u8 -> a 64-byte aligned array with the channel axis
    padded to `channel_multiple` and `padding` = (x, y) pixels on each side of W and H, every new element input_zero."""
    input = np.asarray(input)
    b, h, w, c = input.shape
    px, py = _pair(padding)
    cp = -(-c // channel_multiple) * channel_multiple
    out = aligned_array((b, h + 2 * py, w + 2 * px, cp), np.uint8, 64, 1)
    out[...] = np.uint8(input_zero)
    out[:, py:py + h, px:px + w, :c] = input
    return out


def hannk_tile_filter(filter, filter_zero) -> "Buffer":
    """(CO, FH, FW, CI) u8 (Halide [ci, fx, fy, co]) -> the tiled filter as a Buffer, padded entries filter_zero: one
    tile_conv_filter_uint8 call, the re-tiling a model pays once."""
    filter = np.ascontiguousarray(filter, np.uint8)
    co, fh, fw, ci = filter.shape
    tiled = Buffer(aligned_array((fh, fw, -(-co // 16), -(-ci // 4), 16, 4), np.uint8, 64, 1))
    tile_conv_filter_uint8(Buffer(filter), filter_zero, filter_zero, tiled)
    return tiled


def hannk_conv2d(input, filter, bias, input_zero, filter_zero, stride, dilation, padding, multiplier, shift, output_zero=0, output_min=0,
                 output_max=255, out_dtype=np.uint8, tiled_filter=None) -> np.ndarray:
    """A quantised 2-D convolution as the interpreter runs one: input (B, H, W, C) u8, filter (CO, FH, FW, CI) u8, bias int32 (CO,) ->
    (B, OH, OW, CO) u8 or int16.  The channel axis is padded to a multiple of 4 and the image by `padding` with input_zero, the
    filter is tiled (or `tiled_filter` of hannk_tile_filter is used), then conv_u8_u8_u8 / conv_u8_u8_i16 runs."""
    (sx, sy), (dx, dy), (px, py) = _pair(stride), _pair(dilation), _pair(padding)
    filter = np.asarray(filter)
    co, fh, fw, ci = filter.shape
    b, h, w, c = np.asarray(input).shape
    if c != ci:
        raise ValueError(f"input has {c} channels, the filter {ci}")
    if np.dtype(out_dtype) not in (np.dtype(np.uint8), np.dtype(np.int16)):
        raise TypeError("out_dtype is uint8 or int16")
    padded = hannk_pad_input(input, input_zero, HANNK_VECTOR_REDUCTION, (px, py))
    tiled = hannk_tile_filter(filter, filter_zero) if tiled_filter is None else tiled_filter
    out = Buffer(np.zeros((b, hannk_conv_out_extent(h, fh, sy, dy, py), hannk_conv_out_extent(w, fw, sx, dx, px), co), out_dtype))
    fn = conv_u8_u8_u8 if np.dtype(out_dtype) == np.dtype(np.uint8) else conv_u8_u8_i16
    fn(Buffer(padded), input_zero, tiled, filter_zero, Buffer(np.ascontiguousarray(bias, np.int32)), (sx, sy), (dx, dy), multiplier, shift,
       output_zero, output_min, output_max, out)
    return out.numpy()


def hannk_depthwise_conv2d(input, filter, bias, input_zero, filter_zero, stride, dilation, padding, multiplier, shift, output_zero=0, output_min=0,
                           output_max=255) -> np.ndarray:
    """A quantised depthwise convolution: input (B, H, W, C) u8, filter (FH, FW, C) u8, bias int32 (C,) -> (B, OH, OW, C) u8.  The
    channel axis is padded to a multiple of 16 and the image by `padding` with input_zero; an input of ONE channel under a filter of
    several runs the broadcast variant."""
    (sx, sy), (dx, dy), (px, py) = _pair(stride), _pair(dilation), _pair(padding)
    filter = np.ascontiguousarray(filter, np.uint8)
    fh, fw, co = filter.shape
    b, h, w, c = np.asarray(input).shape
    broadcast = c == 1 and co > 1
    if not broadcast and c != co:
        raise ValueError(f"input has {c} channels, the filter {co}")
    padded = hannk_pad_input(input, input_zero, 1 if broadcast else HANNK_DEPTHWISE_VECTOR, (px, py))
    out = Buffer(np.zeros((b, hannk_conv_out_extent(h, fh, sy, dy, py), hannk_conv_out_extent(w, fw, sx, dx, px), co), np.uint8))
    fn = depthwise_conv_broadcast_uint8 if broadcast else depthwise_conv_uint8
    fn(Buffer(padded), input_zero, Buffer(filter), filter_zero, Buffer(np.ascontiguousarray(bias, np.int32)), (sx, sy), (dx, dy), multiplier, shift,
       output_zero, output_min, output_max, out)
    return out.numpy()

# apps/hannk's op library, second half: pooling, mean, add, mul, softmax and L2 normalisation (include/aot/halide/<name>.h, DESIGN.md
# 5.13).  Raw calls first, arguments as in the C signature; then what the interpreter's ops.cpp does around each of them.
def average_pool_uint8(input, stride, filter, output_min, output_max, output) -> int:
    """u8 [c, x, y, b] -> u8 [c, x, y, b]; stride and filter are (x, y) pairs; taps outside the input do not count."""
    return _check(_fn["average_pool_uint8"](_as_ptr(input), int(stride[0]), int(stride[1]), int(filter[0]), int(filter[1]), int(output_min),
                                            int(output_max), _as_ptr(output)))


def max_pool_uint8(input, stride, filter, output_min, output_max, output) -> int:
    return _check(_fn["max_pool_uint8"](_as_ptr(input), int(stride[0]), int(stride[1]), int(filter[0]), int(filter[1]), int(output_min),
                                        int(output_max), _as_ptr(output)))


def mean_uint8(input, mins, extents, output) -> int:
    """u8 [c, x, y, b] -> u8 [c, x, y, b]: output(p) = the rounded mean of input over p + [mins, mins + extents), Halide order (c first)."""
    a = [int(v) for pair in zip(mins, extents) for v in pair]
    return _check(_fn["mean_uint8"](_as_ptr(input), *a, _as_ptr(output)))


def add_uint8_uint8(input1, input1_zero, input1_multiplier, input2, input2_zero, input2_multiplier, output_zero, output_min, output_max, output) -> int:
    return _check(_fn["add_uint8_uint8"](_as_ptr(input1), int(input1_zero), int(input1_multiplier), _as_ptr(input2), int(input2_zero),
                                         int(input2_multiplier), int(output_zero), int(output_min), int(output_max), _as_ptr(output)))


def mul_uint8_uint8_uint8(input1, input1_zero, input2, input2_zero, output_zero, output_multiplier, output_shift, output_min, output_max, output) -> int:
    return _check(_fn["mul_uint8_uint8_uint8"](_as_ptr(input1), int(input1_zero), _as_ptr(input2), int(input2_zero), int(output_zero),
                                               int(output_multiplier), int(output_shift), int(output_min), int(output_max), _as_ptr(output)))


def softmax_uint8(input, beta_multiplier, beta_shift, output_zero, output_multiplier, output_shift, output) -> int:
    return _check(_fn["softmax_uint8"](_as_ptr(input), int(beta_multiplier), int(beta_shift), int(output_zero), int(output_multiplier),
                                       int(output_shift), _as_ptr(output)))


def l2_normalization_uint8(input, input_zero, output) -> int:
    return _check(_fn["l2_normalization_uint8"](_as_ptr(input), int(input_zero), _as_ptr(output)))


def debug_hannk_approx(fn, q, x, q_x=0, bits=32) -> np.ndarray:
    """Test hook: the device's approx_log2 / approx_exp2 / approx_reciprocal / approx_reciprocal_sqrt (fn 0 .. 3 or the name) of
    common_halide.cpp in Int(bits), over an int32 array."""
    fn = {"approx_log2": 0, "approx_exp2": 1, "approx_reciprocal": 2, "approx_reciprocal_sqrt": 3}.get(fn, fn)
    x = np.ascontiguousarray(x, np.int32)
    out = np.zeros(x.shape, np.int32)
    f = lib.hlmi_debug_hannk_approx
    f.restype, f.argtypes = C.c_int, [C.c_int, C.c_int32, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.c_void_p]
    rc = f(int(fn), int(q), x.ctypes.data, x.size, int(q_x), int(bits), out.ctypes.data)
    if rc != 0:
        raise HalideError(-1, f"hlmi_debug_hannk_approx failed ({rc})")
    return out


def hannk_int_float(x, bits):
    """ops.cpp's IntFloat<intN_t>(x): x = mantissa * 2^exponent / 2^(bits - 1) -> (mantissa(), exponent()) as its accessors return them."""
    log2_one = bits - 1
    m, e = math.frexp(float(np.float32(x)))
    ml = int(math.floor(abs(m) * (1 << log2_one) + 0.5)) * (1 if m >= 0 else -1)   # std::round
    if ml == 1 << log2_one:
        ml, e = ml >> 1, e + 1
    return ml, e


def _int_float_scaled(x, bits, power):
    log2_one = bits - 1
    m, e = hannk_int_float(x, bits)
    e += power
    return (0 if e < -log2_one else m), max(-log2_one, min(log2_one, e))


def hannk_output_range(activation, zero, scale):
    """ops.cpp's get_quantized_min_max: activation None / "relu" / "relu6" / "relu_n1_to_1" -> (min, max)"""
    lo, hi = 0, 255
    rnd = lambda v: int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)
    if activation in (None, "none"):
        pass
    elif activation == "relu":
        lo = int(zero)
    elif activation == "relu6":
        lo, hi = int(zero), int(zero) + rnd(6.0 / scale)
    elif activation == "relu_n1_to_1":
        lo, hi = int(zero) + rnd(-1.0 / scale), int(zero) + rnd(1.0 / scale)
    else:
        raise ValueError(f"unsupported activation {activation}")
    return max(lo, 0), min(hi, 255)


def hannk_compute_padding(stride, in_size, filter_size, out_size) -> int:
    return max(0, (out_size - 1) * stride + filter_size - in_size) // 2


def hannk_pool2d(kind, input, filter, stride, padding="same", output_min=0, output_max=255) -> np.ndarray:
    """Pool2DOp::execute: input (B, H, W, C) u8 -> (B, OH, OW, C) u8, kind "average" or "max", padding "same" or "valid".  Nothing is
    padded: the input is translated by compute_padding and the op leaves the taps outside it out."""
    input = np.ascontiguousarray(input, np.uint8)
    (fw, fh), (sx, sy) = _pair(filter), _pair(stride)
    b, h, w, c = input.shape
    if padding == "same":
        ow, oh = -(-w // sx), -(-h // sy)
    elif padding == "valid":
        ow, oh = (w - fw) // sx + 1, (h - fh) // sy + 1
    else:
        raise ValueError("padding is 'same' or 'valid'")
    inb = Buffer(input, mins=(0, hannk_compute_padding(sx, w, fw, ow), hannk_compute_padding(sy, h, fh, oh), 0))
    out = Buffer(np.zeros((b, oh, ow, c), np.uint8))
    {"average": average_pool_uint8, "max": max_pool_uint8}[kind](inb, (sx, sy), (fw, fh), output_min, output_max, out)
    return out.numpy()


def hannk_mean(input, axes, keepdims=True) -> np.ndarray:
    """ReductionOp::execute (Mean): input u8 of rank <= 4 (numpy order, padded to rank 4 in front), `axes` numpy axes to reduce."""
    input = np.ascontiguousarray(input, np.uint8)
    nd = input.ndim
    axes = sorted({a % nd for a in np.atleast_1d(axes)})
    in4 = input.reshape((1,) * (4 - nd) + input.shape)
    red4 = [a + 4 - nd for a in axes]
    out_shape = tuple(1 if a in red4 else in4.shape[a] for a in range(4))
    mins, extents = [0] * 4, [1] * 4
    for a in red4:
        extents[3 - a] = in4.shape[a]
    out = Buffer(np.zeros(out_shape, np.uint8))
    mean_uint8(Buffer(in4), mins, extents, out)
    res = out.numpy().reshape(tuple(1 if a in axes else input.shape[a] for a in range(nd)))
    return res if keepdims else res.reshape(tuple(input.shape[a] for a in range(nd) if a not in axes))


def _hannk_rank2(a, shape):
    """`a` broadcast against `shape` as the [x, y] operand of add / mul: the innermost axis is dimension 0 (stride 0 where `a` has one
    element there), everything outside it one dimension 1 (which needs `a` to be the full shape there)"""
    a = np.asarray(a, np.uint8)
    full = tuple(shape)
    if a.shape == full:
        return np.ascontiguousarray(a).reshape(-1, full[-1])
    lead = full[:-1]
    a = a.reshape((1,) * (len(full) - a.ndim) + a.shape)
    if a.shape[-1] == 1 and a.shape[:-1] == lead:
        rows = np.ascontiguousarray(a).reshape(-1, 1)
        return np.lib.stride_tricks.as_strided(rows, shape=(rows.shape[0], full[-1]), strides=(rows.strides[0], 0), writeable=False)
    return np.ascontiguousarray(np.broadcast_to(a, full)).reshape(-1, full[-1])


def hannk_add_multipliers(scale1, scale2, out_scale, sign2=1):
    """add_uint8's (input1_multiplier, input2_multiplier): lround(scale * 2^16 / (out_scale * 2^6)), the second times sign2"""
    f32 = np.float32
    lround = lambda v: int(math.floor(abs(float(v)) + 0.5)) * (1 if v >= 0 else -1)
    so = f32(out_scale) * f32(1 << 6)
    return lround(f32(scale1) * f32(1 << 16) / so), lround(f32(scale2) * f32(1 << 16) / so) * int(sign2)


def hannk_mul_params(scale1, scale2, out_scale):
    """mul_uint8's (output_multiplier, output_shift): IntFloat<int32_t>(scale1 * scale2 / out_scale) * 2^-12"""
    f32 = np.float32
    m, e = _int_float_scaled(f32(scale1) * f32(scale2) / f32(out_scale), 32, -12)
    return m, -e


def hannk_add(in1, q1, in2, q2, qout, activation=None, sign2=1) -> np.ndarray:
    """ops.cpp's add_uint8: q = (scale, zero) of each tensor; sign2 = -1 subtracts.  An operand with one element along the innermost
    axis is passed with a stride of 0, not expanded."""
    shape = np.broadcast_shapes(np.shape(in1), np.shape(in2))
    m1, m2 = hannk_add_multipliers(q1[0], q2[0], qout[0], sign2)
    lo, hi = hannk_output_range(activation, qout[1], qout[0])
    a, b = _hannk_rank2(in1, shape), _hannk_rank2(in2, shape)
    out = Buffer(np.zeros(a.shape, np.uint8))
    add_uint8_uint8(Buffer(a), q1[1], m1, Buffer(b), q2[1], m2, qout[1], lo, hi, out)
    return out.numpy().reshape(shape)


def hannk_mul(in1, q1, in2, q2, qout, activation=None) -> np.ndarray:
    """ops.cpp's mul_uint8: the multiplier is IntFloat<int32_t>(s1 * s2 / sout) * 2^-12."""
    shape = np.broadcast_shapes(np.shape(in1), np.shape(in2))
    m, shift = hannk_mul_params(q1[0], q2[0], qout[0])
    lo, hi = hannk_output_range(activation, qout[1], qout[0])
    a, b = _hannk_rank2(in1, shape), _hannk_rank2(in2, shape)
    out = Buffer(np.zeros(a.shape, np.uint8))
    mul_uint8_uint8_uint8(Buffer(a), q1[1], Buffer(b), q2[1], qout[1], m, shift, lo, hi, out)
    return out.numpy().reshape(shape)


def hannk_softmax_params(in_scale, beta, out_scale):
    """SoftmaxOp::execute: (beta_multiplier, beta_shift, output_multiplier, output_shift), the extra factor of two on the output included"""
    f32 = np.float32
    beta2 = f32(beta) * f32(np.log2(np.exp(f32(1.0))))
    bm, be = _int_float_scaled(beta2 * f32(in_scale), 16, -6)
    om, oe = _int_float_scaled(f32(out_scale), 16, 1)
    return bm, -be, om, -oe


def _hannk_rows(fn, input, axis):
    """input of any rank, the op over numpy `axis`: rank 2 keeps the caller's memory and transposes the buffers as ops.cpp does (dimension
    0 then has the row stride); other ranks are brought to (rows, n)"""
    input = np.asarray(input, np.uint8)
    axis %= input.ndim
    if input.ndim == 2:
        src = np.ascontiguousarray(input)
        dst = np.zeros(src.shape, np.uint8)
        view = (lambda a: a) if axis == 1 else (lambda a: a.T)
        out = Buffer(view(dst))
        fn(Buffer(view(src)), out)
        out.numpy()
        return dst
    moved = np.ascontiguousarray(np.moveaxis(input, axis, -1))
    out = Buffer(np.zeros((moved.size // moved.shape[-1], moved.shape[-1]), np.uint8))
    fn(Buffer(moved.reshape(out.array.shape)), out)
    return np.moveaxis(out.numpy().reshape(moved.shape), -1, axis)


def hannk_softmax(input, in_scale, beta=1.0, out_scale=1.0 / 256, out_zero=0, axis=-1) -> np.ndarray:
    bm, bs, om, osh = hannk_softmax_params(in_scale, beta, out_scale)
    return _hannk_rows(lambda i, o: softmax_uint8(i, bm, bs, out_zero, om, osh, o), input, axis)


def hannk_l2_normalization(input, input_zero, axis=-1) -> np.ndarray:
    """L2NormalizationOp::execute: the output has scale 1 / 128 and zero point 128"""
    return _hannk_rows(lambda i, o: l2_normalization_uint8(i, input_zero, o), input, axis)


# apps/hannk's op library, third part: the elementwise programs, copy, fill and upsample_channels (include/aot/halide/<name>.h, DESIGN.md
# 5.14).  Raw calls first, arguments as in the C signature; then the assembler and what the interpreter's ops.cpp / lower.cpp do around them.
def elementwise_5xuint8_1xuint8(inputs_0, inputs_1, inputs_2, inputs_3, inputs_4, program, output) -> int:
    """five u8 [x, y] inputs (dimension 0 stride 1 or 0), program i16 [5, n], n <= 20 -> u8 [x, y]: u8_sat of the last slot"""
    return _check(_fn["elementwise_5xuint8_1xuint8"](_as_ptr(inputs_0), _as_ptr(inputs_1), _as_ptr(inputs_2), _as_ptr(inputs_3), _as_ptr(inputs_4),
                                                     _as_ptr(program), _as_ptr(output)))


def elementwise_5xint16_1xuint8int16(inputs_0, inputs_1, inputs_2, inputs_3, inputs_4, program, output_0, output_1) -> int:
    """five i16 [x, y] inputs -> output_0 u8 = u8_sat(the last slot but one), output_1 i16 = the last slot"""
    return _check(_fn["elementwise_5xint16_1xuint8int16"](_as_ptr(inputs_0), _as_ptr(inputs_1), _as_ptr(inputs_2), _as_ptr(inputs_3), _as_ptr(inputs_4),
                                                          _as_ptr(program), _as_ptr(output_0), _as_ptr(output_1)))


def copy_uint8_uint8(input, pad_value, output) -> int:
    """u8 [c, x, y, b] -> u8 [c, x, y, b]; channels outside the input's dimension 0 are uint8(pad_value)"""
    return _check(_fn["copy_uint8_uint8"](_as_ptr(input), int(pad_value), _as_ptr(output)))


def fill_uint8(value, output) -> int:
    return _check(_fn["fill_uint8"](int(value), _as_ptr(output)))


def upsample_channels_uint8(input, factor, output) -> int:
    """output(c, x, y, b) = input(c / factor, x, y, b), Halide's division (c / 0 == 0)"""
    return _check(_fn["upsample_channels_uint8"](_as_ptr(input), int(factor), _as_ptr(output)))


def depthwise_conv_shallow_uint8(input, input_zero, filter, filter_zero, bias, stride, dilation, input_stride_x, multiplier, shift, output_zero,
                                 output_min, output_max, output) -> int:
    """depthwise_conv_uint8 with c and x fused into dimension 0: input u8 [c, 1, y, b], filter u8 [D, fx, fy], bias i32 [D] -> u8 [c, 1, y, b];
    the tap rx reads the input at c + rx * dilation_x * input_stride_x; filter and bias are read at (c % 16) % D."""
    return _check(_fn["depthwise_conv_shallow_uint8"](*_hannk_conv_args(input, input_zero, filter, filter_zero, bias, stride, dilation,
                                                                        [int(input_stride_x)], multiplier, shift, output_zero, output_min, output_max,
                                                                        output)))


def hannk_can_be_shallow(channels, width, stride_x=1) -> bool:
    """ops.cpp:931-939, :1012: the channel vector is a multiple of the channel count, the fused row is at least one vector wide, stride_x is 1"""
    return int(stride_x) == 1 and channels > 0 and HANNK_DEPTHWISE_VECTOR % channels == 0 and channels * width >= HANNK_DEPTHWISE_VECTOR


def hannk_depthwise_conv2d_shallow(input, filter, bias, input_zero, filter_zero, stride, dilation, padding, multiplier, shift, output_zero=0,
                                   output_min=0, output_max=255) -> np.ndarray:
    """hannk_depthwise_conv2d through the shallow variant, as DepthwiseConv2DOp::execute takes it (ops.cpp:1007-1023): the image is padded
    with input_zero but its channels are not; c and x of input and output are fused in place.  Refuses (ValueError) what can_be_shallow
    refuses."""
    (sx, sy), (dx, dy), (px, py) = _pair(stride), _pair(dilation), _pair(padding)
    filter = np.ascontiguousarray(filter, np.uint8)
    fh, fw, c = filter.shape
    b, h, w, ci = np.asarray(input).shape
    if ci != c:
        raise ValueError(f"input has {ci} channels, the filter {c}")
    if not hannk_can_be_shallow(c, w + 2 * px, sx):
        raise ValueError("not shallow: stride_x is 1, the channel count divides 16 and channels * padded width >= 16")
    padded = hannk_pad_input(input, input_zero, 1, (px, py))
    oh, ow = hannk_conv_out_extent(h, fh, sy, dy, py), hannk_conv_out_extent(w, fw, 1, dx, px)
    out = np.zeros((b, oh, 1, ow * c), np.uint8)
    fused = padded.reshape(b, h + 2 * py, 1, (w + 2 * px) * c)
    ob = Buffer(out)
    depthwise_conv_shallow_uint8(Buffer(fused), input_zero, Buffer(filter), filter_zero, Buffer(np.ascontiguousarray(bias, np.int32)), (1, sy), (dx, dy),
                                 c, multiplier, shift, output_zero, output_min, output_max, ob)
    return ob.numpy().reshape(b, oh, ow, c)


def debug_hannk_program_approx(fn, x, q, q_x, width=16) -> np.ndarray:
    """Test hook: the device's approx_log2p1_exp2 / approx_log2m1_exp2 / approx_logistic / approx_tanh (fn 0 .. 3 or the name) in Int(16):
    x the i16 argument, q the result's precision, q_x the argument's (each 0 .. 15), broadcast against each other; `width` (16 or 32) is
    the width of the count q_x."""
    fn = {"approx_log2p1_exp2": 0, "approx_log2m1_exp2": 1, "approx_logistic": 2, "approx_tanh": 3}.get(fn, fn)
    shape = np.broadcast_shapes(np.shape(x), np.shape(q), np.shape(q_x))
    x, q, q_x = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.int32), shape)) for v in (x, q, q_x))
    out = np.zeros(shape, np.int32)
    f = lib.hlmi_debug_hannk_program_approx
    f.restype, f.argtypes = C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p]
    rc = f(int(fn), x.ctypes.data, q.ctypes.data, q_x.ctypes.data, x.size, int(width), out.ctypes.data)
    if rc != 0:
        raise HalideError(-1, f"hlmi_debug_hannk_program_approx failed ({rc})")
    return out


class ElementwiseAssembler:
    """interpreter/elementwise_program.{h,cpp}: builds the [n, 5] int16 program (rows of op, arg1, arg2, arg3, arg4) the elementwise entry
    points run.  Methods return Slot objects; an int where the reference has an int16_t overload is an immediate."""
    Noop, Add, Sub, MulAdd, MulShift, Shift, Min, Max, Clamp, Logistic, Tanh = range(11)
    InstructionSize = 5

    class Slot:
        def __init__(self, index):
            self.index = int(index)

    def __init__(self, capacity=None):
        self.rows = []
        self.capacity = capacity

    def _instruction(self, op, a, b, arg3=0, arg4=0):
        if self.capacity is not None and len(self.rows) >= self.capacity:
            raise ValueError("the program buffer is full")
        for v in (arg3, arg4):
            if not -32768 <= int(v) <= 32767:
                raise ValueError(f"immediate {v} is no int16")
        self.rows.append((op, a.index, b.index, int(arg3), int(arg4)))
        return self.Slot(len(self.rows))

    def _binary(self, op, a, b, imm):
        if isinstance(b, self.Slot):
            return self._instruction(op, a, b, imm)
        return self._instruction(op, a, self.constant(0), b)

    def constant(self, value):
        return self.Slot(0) if value == 0 else self._instruction(self.Add, self.Slot(0), self.Slot(0), value)

    def input(self, index):
        return self.Slot(-index - 1)

    def add(self, a, b, add_b=0):
        return self._binary(self.Add, a, b, add_b)

    def sub(self, a, b, add_b=0):
        return self._binary(self.Sub, a, b, add_b)

    def mul(self, a, b, add_b=0):
        return self._binary(self.MulAdd, a, b, add_b)

    def mul_add(self, a, b, add):
        if isinstance(b, self.Slot):
            return self._instruction(self.MulAdd, a, b, 0, add)
        return self._instruction(self.MulAdd, a, self.constant(0), b, add)

    def mul_shift(self, a, b, shift):
        if isinstance(b, self.Slot):
            return self._instruction(self.MulShift, a, b, 0, shift)
        return self._instruction(self.MulShift, a, self.constant(0), b, shift)

    def shift(self, a, b, extra_shift=0):
        return self._binary(self.Shift, a, b, extra_shift)

    def min(self, a, b, add_b=0):
        return self._binary(self.Min, a, b, add_b)

    def max(self, a, b, add_b=0):
        return self._binary(self.Max, a, b, add_b)

    def clamp(self, x, lo, hi):
        return self._instruction(self.Clamp, x, x, lo, hi)   # op2 is unused: x again, as the reference does

    def logistic(self, q, a, q_a):
        if isinstance(q_a, self.Slot):
            return self._instruction(self.Logistic, a, q_a, 0, q)
        return self._instruction(self.Logistic, a, self.constant(0), q_a, q)

    def tanh(self, q, a, q_a):
        if isinstance(q_a, self.Slot):
            return self._instruction(self.Tanh, a, q_a, 0, q)
        return self._instruction(self.Tanh, a, self.constant(0), q_a, q)

    def assemble(self, outputs) -> np.ndarray:
        """The program whose last len(outputs) slots are `outputs`: where they are not there already, each is reloaded by adding 0."""
        needed = len(self.rows) - len(outputs) + 1
        if [o.index for o in outputs] != list(range(needed, needed + len(outputs))):
            for o in outputs:
                self.add(o, 0)
        return np.array(self.rows, np.int16).reshape(-1, 5)


def hannk_logistic_program(in_scale, in_zero) -> np.ndarray:
    """UnaryOp::execute, Logistic (ops.cpp:1797-1813): the output has scale 1 / 256 and zero point 0"""
    m, e = _int_float_scaled(np.float32(in_scale), 16, -6)
    if e > 0:
        raise ValueError("the input scale is too large for the logistic program")
    p = ElementwiseAssembler(64 // 5)
    scaled = p.mul_shift(p.sub(p.input(0), int(in_zero)), m, 15 - 6)
    return p.assemble([p.logistic(8, scaled, -e)])


def hannk_tanh_program(in_scale, in_zero) -> np.ndarray:
    """UnaryOp::execute, Tanh (ops.cpp:1820-1833): the output has scale 1 / 128 and zero point 128"""
    m, e = _int_float_scaled(np.float32(in_scale), 16, -6)
    if e > 0:
        raise ValueError("the input scale is too large for the tanh program")
    p = ElementwiseAssembler(64 // 5)
    scaled = p.mul_shift(p.sub(p.input(0), int(in_zero)), m, 15 - 6)
    return p.assemble([p.add(p.tanh(7, scaled, -e), 128)])


def hannk_lstm_program() -> np.ndarray:
    """The elementwise part of the LSTM cell (lower.cpp:44-69) on inputs (input gate, input modulation gate, forget gate, output gate,
    previous state), all int16 -> the outputs (activation u8, state i16)"""
    p = ElementwiseAssembler(256 // 5)
    q = 15
    input_gate = p.logistic(q, p.input(0), q - 3)
    input_modulation_gate = p.tanh(q, p.input(1), q - 3)
    forget_gate = p.logistic(q, p.input(2), q - 3)
    output_gate = p.logistic(q, p.input(3), q - 3)
    input_times_input_modulation = p.mul_shift(input_gate, input_modulation_gate, q + 4)
    prev_state_times_forget_state = p.mul(forget_gate, p.input(4))
    state = p.add(input_times_input_modulation, prev_state_times_forget_state)
    activation = p.mul_add(output_gate, p.tanh(7, state, q - 4), 128)
    state = p.add(state, 0)
    return p.assemble([activation, state])


def _hannk_program_rank2(a, shape, dtype):
    """`a` broadcast against `shape` as an [x, y] operand: stride 0 along the innermost axis where `a` has one element there"""
    a = np.asarray(a, dtype)
    full = tuple(shape)
    n = full[-1] if full else 1
    a = a.reshape((1,) * (len(full) - a.ndim) + a.shape)
    if a.shape == full:
        return np.ascontiguousarray(a).reshape(-1, n)
    if a.shape[-1] == 1 and a.shape[:-1] == full[:-1]:
        rows = np.ascontiguousarray(a).reshape(-1, 1)
        return np.lib.stride_tricks.as_strided(rows, shape=(rows.shape[0], n), strides=(rows.strides[0], 0), writeable=False)
    return np.ascontiguousarray(np.broadcast_to(a, full)).reshape(-1, n)


def hannk_elementwise(inputs, program, outputs=1):
    """ElementwiseProgramOp::execute: one to five inputs of one dtype, uint8 or int16 (the last is repeated up to five, as ops.cpp:1080-1084
    does), broadcast against each other; program an [n, 5] int16 array.  uint8 inputs -> the uint8 result (outputs = 1); int16 inputs ->
    the pair (uint8, int16) (outputs = 2): the two variants the library has."""
    if not 1 <= len(inputs) <= 5:
        raise ValueError("one to five inputs")
    dtype = np.asarray(inputs[0]).dtype
    if dtype == np.dtype(np.uint8):
        want = 1
    elif dtype == np.dtype(np.int16):
        want = 2
    else:
        raise TypeError("the inputs are uint8 or int16")
    if outputs != want:
        raise ValueError(f"{dtype} inputs have {want} output(s)")
    shape = np.broadcast_shapes(*[np.shape(a) for a in inputs])
    arrs = [_hannk_program_rank2(a, shape, dtype) for a in inputs]
    bufs = [Buffer(a) for a in arrs]
    bufs += [bufs[-1]] * (5 - len(bufs))
    prog = Buffer(np.ascontiguousarray(program, np.int16).reshape(-1, 5))
    out0 = Buffer(np.zeros(arrs[0].shape, np.uint8))
    if want == 1:
        elementwise_5xuint8_1xuint8(*bufs, prog, out0)
        return out0.numpy().reshape(shape)
    out1 = Buffer(np.zeros(arrs[0].shape, np.int16))
    elementwise_5xint16_1xuint8int16(*bufs, prog, out0, out1)
    return out0.numpy().reshape(shape), out1.numpy().reshape(shape)


def hannk_logistic(x, in_scale, in_zero) -> np.ndarray:
    """UnaryOp Logistic on a uint8 array of any shape: the result has scale 1 / 256 and zero point 0"""
    return hannk_elementwise([np.asarray(x, np.uint8)], hannk_logistic_program(in_scale, in_zero))


def hannk_tanh(x, in_scale, in_zero) -> np.ndarray:
    """UnaryOp Tanh: the result has scale 1 / 128 and zero point 128"""
    return hannk_elementwise([np.asarray(x, np.uint8)], hannk_tanh_program(in_scale, in_zero))


def hannk_lstm_elementwise(input_gate, input_modulation_gate, forget_gate, output_gate, prev_state):
    """The LSTM cell's elementwise program on five int16 arrays -> (activation uint8, state int16)"""
    return hannk_elementwise([np.asarray(a, np.int16) for a in (input_gate, input_modulation_gate, forget_gate, output_gate, prev_state)],
                             hannk_lstm_program(), outputs=2)


def hannk_pad(input, padding, pad_value) -> np.ndarray:
    """PadOp::execute on a uint8 array of rank <= 4 (numpy order, padded to rank 4 in front): `padding` is one (before, after) pair per numpy
    axis.  The borders are filled dimension by dimension with fill_uint8, the rest is one copy_uint8_uint8; where 3 channels become 4
    the copy pads the channel itself (ops.cpp:1266-1271)."""
    input = np.ascontiguousarray(input, np.uint8)
    nd = input.ndim
    if nd > 4 or len(padding) != nd:
        raise ValueError("rank <= 4 and one (before, after) pair per axis")
    in4 = input.reshape((1,) * (4 - nd) + input.shape)
    pads = [(0, 0)] * (4 - nd) + [(int(b), int(a)) for b, a in padding]
    if any(b < 0 or a < 0 for b, a in pads):
        raise ValueError("paddings are not negative")
    out = np.zeros(tuple(s + b + a for s, (b, a) in zip(in4.shape, pads)), np.uint8)
    # Halide dimension d is numpy axis 3 - d; the input is translated by the padding in front of it
    imin = [pads[3 - d][0] for d in range(4)]
    imax = [imin[d] + in4.shape[3 - d] - 1 for d in range(4)]
    omin, omax = [0] * 4, [out.shape[3 - d] - 1 for d in range(4)]

    def crop():
        view = out[tuple(slice(omin[3 - ax], omax[3 - ax] + 1) for ax in range(4))]
        return Buffer(view, mins=tuple(omin))

    fill_min_dim = 1 if in4.shape[3] == 3 and out.shape[3] == 4 else 0
    for d in range(3, fill_min_dim - 1, -1):
        lo, hi = omin[d], omax[d]
        if lo < imin[d]:
            omin[d], omax[d] = lo, imin[d] - 1
            b = crop()
            fill_uint8(pad_value, b)
            b.numpy()
        if hi > imax[d]:
            omin[d], omax[d] = imax[d] + 1, hi
            b = crop()
            fill_uint8(pad_value, b)
            b.numpy()
        omin[d], omax[d] = max(lo, imin[d]), min(hi, imax[d])
    b = crop()
    copy_uint8_uint8(Buffer(in4, mins=tuple(imin)), pad_value, b)
    b.numpy()
    return out.reshape(tuple(out.shape[4 - nd:]))


def hannk_upsample_channels(input, factor) -> np.ndarray:
    """(B, H, W, C) uint8 -> (B, H, W, C * factor): channel c of the result is channel c // factor of the input (depth multiplier > 1)"""
    input = np.ascontiguousarray(input, np.uint8)
    if input.ndim != 4 or int(factor) < 1:
        raise ValueError("a (B, H, W, C) array and a factor >= 1")
    out = Buffer(np.zeros(input.shape[:3] + (input.shape[3] * int(factor),), np.uint8))
    upsample_channels_uint8(Buffer(input), factor, out)
    return out.numpy()


# apps/hannk's data movement: what the interpreter does with Buffer::copy_from on re-viewed buffers, and GatherOp.  The two
# entry points are library extensions (no metadata); the ops below build their views with numpy, whose axes are the Halide dimensions reversed.
HANNK_MOVE_KERNELS = ("none", "rows", "transposing", "general")


def hannk_copy_from(src, dst, general=False) -> int:
    """Halide::Runtime::Buffer::copy_from: dst's elements inside src's box take src's values.  Two Buffers of the same rank (<= 8) and element
    size (1, 2, 4, 8 bytes), any strides; `general` forces the one-thread-per-element kernel (hlmi_hannk_general)."""
    if general:
        argv = (C.c_void_p * 2)(C.cast(_as_ptr(src), C.c_void_p), C.cast(_as_ptr(dst), C.c_void_p))
        fn = lib.hlmi_hannk_general
        fn.restype, fn.argtypes = C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]
        return _check(fn(b"hannk_copy_from", argv))
    fn = lib.hlmi_hannk_copy_from
    fn.restype, fn.argtypes = C.c_int, [_BP, _BP]
    return _check(fn(_as_ptr(src), _as_ptr(dst)))


def hannk_gather_buffers(src, indices, axis, dst) -> int:
    """GatherOp::execute with batch_dims == 0 on Buffers: `axis` is a Halide dimension of src, indices int32 of rank 0 .. 2, dst of rank
    src.rank + indices.rank - 1.  An index outside src's dimension leaves its slice of dst unwritten and raises HalideError -8."""
    fn = lib.hlmi_hannk_gather
    fn.restype, fn.argtypes = C.c_int, [_BP, _BP, C.c_int, _BP]
    return _check(fn(_as_ptr(src), _as_ptr(indices), int(axis), _as_ptr(dst)))


def debug_hannk_move_plan(src, dst, general=False) -> dict:
    """What hannk_copy_from's plan chooses for two Buffers (only their types and dimensions are read; no device is needed): the kernel, one
    of HANNK_MOVE_KERNELS, and the number of dimensions left after dropping extent-1 dimensions and merging."""
    out = (C.c_int32 * 2)()
    f = lib.hlmi_debug_hannk_move_plan
    f.restype, f.argtypes = C.c_int, [_BP, _BP, C.c_int32, C.POINTER(C.c_int32)]
    rc = f(_as_ptr(src), _as_ptr(dst), int(bool(general)), out)
    if rc != 0:
        raise ValueError(f"hlmi_debug_hannk_move_plan: {'dst aliases itself' if rc == -8 else 'bad arguments'}")
    return {"kernel": HANNK_MOVE_KERNELS[out[0]], "rank": int(out[1])}


def _hannk_movable(a):
    a = np.ascontiguousarray(a)
    if a.dtype not in _TYPE_OF:
        raise TypeError(f"unsupported dtype {a.dtype}")
    return a


def _hannk_copy_views(src_view, dst_view, general=False):
    d = Buffer(dst_view)
    hannk_copy_from(Buffer(src_view), d, general)
    d.numpy()


def hannk_transpose(input, perm, general=False) -> np.ndarray:
    """TransposeOp::execute: np.transpose(input, perm) as one copy_from into the output re-viewed in the input's order"""
    input = _hannk_movable(input)
    perm = [int(p) for p in perm]
    if sorted(perm) != list(range(input.ndim)):
        raise ValueError(f"{perm} is no permutation of {input.ndim} axes")
    out = np.zeros(tuple(input.shape[p] for p in perm), input.dtype)
    _hannk_copy_views(input, out.transpose(np.argsort(perm)), general)
    return out


def _hannk_block_views(space, depth, block):
    """(B, H, W, C) and (B, H / block, W / block, block * block * C) as two rank-6 views of one shape (ops.cpp:1607-1625)"""
    b, h, w, c = space.shape
    if block < 1 or h % block or w % block or depth.shape != (b, h // block, w // block, block * block * c):
        raise ValueError("the block size divides height and width, and depth = block^2 * channels")
    s6 = space.reshape(b, h // block, block, w // block, block, c)
    d6 = depth.reshape(b, h // block, w // block, block, block, c).transpose(0, 1, 3, 2, 4, 5)
    return s6, d6


def hannk_space_to_depth(input, block_size, general=False) -> np.ndarray:
    """SpaceToDepth: (B, H, W, C) -> (B, H / block, W / block, block^2 * C), one copy_from over rank-6 views"""
    input = _hannk_movable(input)
    block = int(block_size)
    if input.ndim != 4 or block < 1 or input.shape[1] % block or input.shape[2] % block:
        raise ValueError("a (B, H, W, C) array whose height and width the block size divides")
    b, h, w, c = input.shape
    out = np.zeros((b, h // block, w // block, block * block * c), input.dtype)
    s6, d6 = _hannk_block_views(input, out, block)
    _hannk_copy_views(s6, d6, general)
    return out


def hannk_depth_to_space(input, block_size, general=False) -> np.ndarray:
    """DepthToSpace: (B, H, W, block^2 * C) -> (B, H * block, W * block, C)"""
    input = _hannk_movable(input)
    block = int(block_size)
    if input.ndim != 4 or block < 1 or input.shape[3] % (block * block):
        raise ValueError("a (B, H, W, C) array whose channel count the squared block size divides")
    b, h, w, c = input.shape
    out = np.zeros((b, h * block, w * block, c // (block * block)), input.dtype)
    s6, d6 = _hannk_block_views(out, input, block)
    _hannk_copy_views(d6, s6, general)
    return out


def hannk_requantize(input, q_in, q_out, activation=None) -> np.ndarray:
    """try_requantize (ops.cpp:487-504) on a uint8 array: add_uint8(in * 1 + in * 0) from q_in = (scale, zero) to q_out"""
    input = np.ascontiguousarray(input, np.uint8)
    return hannk_add(input, q_in, input, q_in, q_out, activation, sign2=0)


def hannk_concatenation(inputs, axis, quantization=None, general=False) -> np.ndarray:
    """ConcatenationOp::execute: every input goes into its crop of the output through requantize_or_copy.  `quantization` = [(scale, zero) of
    each input ..., (scale, zero) of the output] sends uint8 pieces through the add kernel, equal scales or not, as the reference does;
    without it the pieces are copied."""
    inputs = [_hannk_movable(a) for a in inputs]
    nd = inputs[0].ndim
    axis = int(axis) % nd
    out = np.zeros(tuple(sum(a.shape[d] for a in inputs) if d == axis else inputs[0].shape[d] for d in range(nd)), inputs[0].dtype)
    at = 0
    for i, a in enumerate(inputs):
        if a.dtype != out.dtype or any(a.shape[d] != out.shape[d] for d in range(nd) if d != axis):
            raise ValueError("the inputs share dtype and every extent but the axis'")
        piece = out[tuple(slice(at, at + a.shape[axis]) if d == axis else slice(None) for d in range(nd))]
        if quantization is not None and out.dtype == np.dtype(np.uint8):
            piece[...] = hannk_requantize(a, quantization[i], quantization[-1])
        else:
            _hannk_copy_views(a, piece, general)
        at += a.shape[axis]
    return out


def hannk_split(input, sizes, axis, quantization=None, general=False) -> list:
    """SplitOp::execute: `sizes` an int (that many equal pieces) or the pieces' extents along `axis`; `quantization` = [(scale, zero) of the
    input, (scale, zero) of each output ...] as for hannk_concatenation."""
    input = _hannk_movable(input)
    axis = int(axis) % input.ndim
    n = input.shape[axis]
    if np.isscalar(sizes):
        if int(sizes) < 1 or n % int(sizes):
            raise ValueError(f"{n} elements do not split into {sizes} equal pieces")
        sizes = [n // int(sizes)] * int(sizes)
    sizes = [int(v) for v in sizes]
    if sum(sizes) != n or any(v < 0 for v in sizes):
        raise ValueError(f"pieces of {sizes} do not add up to {n}")
    outs, at = [], 0
    for i, size in enumerate(sizes):
        piece = input[tuple(slice(at, at + size) if d == axis else slice(None) for d in range(input.ndim))]
        if quantization is not None and input.dtype == np.dtype(np.uint8):
            outs.append(hannk_requantize(piece, quantization[0], quantization[1 + i]))
        else:
            out = np.zeros(piece.shape, input.dtype)
            _hannk_copy_views(piece, out, general)
            outs.append(out)
        at += size
    return outs


def hannk_gather(input, indices, axis=0) -> np.ndarray:
    """GatherOp::execute: np.take(input, indices, axis) for int32 indices of rank 0 .. 2 in one launch"""
    input = _hannk_movable(input)
    indices = np.require(indices, np.int32, "C")   # (ascontiguousarray would make a scalar index a vector)
    axis = int(axis) % input.ndim
    out = Buffer(np.zeros(input.shape[:axis] + indices.shape + input.shape[axis + 1:], input.dtype))
    hannk_gather_buffers(Buffer(input), Buffer(indices), input.ndim - 1 - axis, out)
    return out.numpy()


def hannk_fully_connected(input, weights, bias, input_zero, filter_zero, multiplier, shift, output_zero=0, output_min=0, output_max=255) -> np.ndarray:
    """lower_tflite_fullyconnected: input of any rank flattened to (N, CI), weights (CO, CI) u8, bias int32 (CO,) -> (N, CO): the conv op on
    a 1 x 1 image"""
    weights = np.ascontiguousarray(weights, np.uint8)
    co, ci = weights.shape
    flat = np.ascontiguousarray(input, np.uint8).reshape(-1, ci)
    out = hannk_conv2d(flat.reshape(-1, 1, 1, ci), weights.reshape(co, 1, 1, ci), bias, input_zero, filter_zero, 1, 1, 0, multiplier, shift, output_zero,
                       output_min, output_max)
    return out.reshape(-1, co)


def lens_blur(left_im, right_im, slices, focus_depth, blur_radius_scale, aperture_samples, final) -> int:
    return _check(_fn["lens_blur"](_as_ptr(left_im), _as_ptr(right_im), int(slices), int(focus_depth), float(blur_radius_scale),
                        int(aperture_samples), _as_ptr(final)))


def bgu(r_sigma, s_sigma, splat_loc, values, slice_loc, output) -> int:
    """apps/bgu: low-res f32 pair (splat_loc -> values) fitted per bilateral-grid cell, applied to the full-res slice_loc."""
    return _check(_fn["bgu"](float(r_sigma), int(s_sigma), _as_ptr(splat_loc), _as_ptr(values), _as_ptr(slice_loc), _as_ptr(output)))


def camera_pipe(input, matrix_3200, matrix_7000, color_temp, gamma, contrast, sharpen_strength, black_level,
                white_level, processed) -> int:
    return _check(_fn["camera_pipe"](_as_ptr(input), _as_ptr(matrix_3200), _as_ptr(matrix_7000), float(color_temp), float(gamma),
                       float(contrast), float(sharpen_strength), int(black_level), int(white_level),
                       _as_ptr(processed)))


def device_count() -> int:
    """Usable gfx950 devices visible to this process."""
    lib.hlmi_device_count.restype = C.c_int
    return lib.hlmi_device_count()


def run_batch(name: str, frames, devices=None, streams_per_device: int = 1) -> int:
    """The in-process frame sharder (`hlmi_run_batch`, include/hlmi_runtime.h): run pipeline `name` once
    per frame, frames dealt round-robin to one host thread + HIP stream per entry of `devices` (x streams_per_device).

    `frames` is a list of argument tuples in the pipeline's own order (Buffers and Python scalars), exactly what
    `<name>_argv` receives per call.  Outputs are left device-dirty on the device that produced them; `Buffer.numpy()`
    brings them back from there.  Returns 0 or raises HalideError with the first failing frame's code."""
    md = metadata(name)
    n_args = md.num_arguments
    fn = getattr(lib, _symbol(name, "_argv"))
    keep = []          # ctypes objects that must outlive the call
    argvs = (C.POINTER(C.c_void_p) * max(len(frames), 1))()
    for i, frame in enumerate(frames):
        if len(frame) != n_args:
            raise TypeError(f"{name} takes {n_args} arguments, frame {i} has {len(frame)}")
        argv = (C.c_void_p * n_args)()
        for j, v in enumerate(frame):
            a = md.arguments[j]
            if a.kind == 0:
                box = (C.c_double(v) if a.type.bits == 64 else C.c_float(v)) if a.type.code == 2 else (C.c_int32(v) if a.type.bits == 32 else C.c_uint8(v) if a.type.bits == 8 else C.c_int64(v))
                keep.append(box)
                argv[j] = C.cast(C.pointer(box), C.c_void_p)
            else:
                argv[j] = C.cast(C.pointer(v.raw), C.c_void_p)
        keep.append(argv)
        argvs[i] = C.cast(argv, C.POINTER(C.c_void_p))
    if devices is None:
        devices = list(range(max(device_count(), 1)))
    devs = (C.c_int * len(devices))(*devices)
    lib.hlmi_run_batch.restype = C.c_int
    lib.hlmi_run_batch.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_void_p)), C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int]
    with _batch_lock:      # one batch at a time records messages: a HalideError never carries another batch's text
        del _batch_error[:]
        _batch_active[0] = True
        try:
            code = lib.hlmi_run_batch(C.cast(fn, C.c_void_p), argvs, len(frames), devs, len(devices), int(streams_per_device))
        finally:
            _batch_active[0] = False
        msg = _batch_error[0] if _batch_error else ""
    if code != 0:
        raise HalideError(code, msg)
    return 0


# worker threads of hlmi_run_batch report through the same handler but on their own threads; messages are recorded only
# while a batch is running (and cleared when it starts), so unrelated calls on other Python threads leave no stale text
_batch_error: list = []
_batch_active = [False]
_batch_lock = threading.Lock()


def version() -> str:
    return lib.hlmi_version().decode()


def canon_fma() -> int:
    """1: the library's float kernels contract mul+add pairs into fma (the default build), 0: one rounding per operator."""
    return int(lib.hlmi_canon_fma())
