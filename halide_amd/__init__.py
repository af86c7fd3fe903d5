"""halide_amd — host-side mirror (ctypes) of the C-ABI drop-in library ``libhlmi.so``.

The product is the shared library: hand-written HIP kernels for gfx950 behind the reference's AOT
entry points (``int local_laplacian(halide_buffer_t*, int32_t, float, float, halide_buffer_t*)`` …,
see ``include/hlmi_pipelines.h``).  This package is only the thin Python caller used by the tests and
``bench.py``: a ``Buffer`` that plays the role of ``Halide::Runtime::Buffer`` (reference:
``src/runtime/HalideBuffer.h`` — planar storage, dimension 0 innermost, dirty flags, ``copy_to_host``,
``device_sync``) and one Python function per pipeline with the reference's argument order.  apps/hannk's op library, which needs more
than calls (parameter derivations, shape rules, an assembler, numpy drivers), is ``hannk.py``; its public names are re-exported here.

There is deliberately no CPU fallback: if ``libhlmi.so`` is missing the import fails, and if no
gfx950 device is usable every pipeline call raises ``HalideError`` (code -29).
"""
from __future__ import annotations

import ctypes as C
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
# apps/hannk's op library (its Python side is hannk.py: here is only what binding needs) is built with C++ name mangling, every symbol in
# namespace hannk (include/aot/halide/<name>.h): the Itanium names of <name>, <name>_argv and <name>_metadata, the parameter lists spelled
# as the compiler spells them (P15halide_buffer_t the first buffer, S1_ every further one, h uint8_t, i int32_t)
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
       + ["reaction_diffusion_init", "reaction_diffusion_update", "reaction_diffusion_render"]
       + ["conv3x3a16", "conv3x3a32", "dilate3x3", "median3x3", "gaussian5x5", "sobel"] + ["mat_mul"] + ["resnet50", "resnet50_batch"]
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


def reaction_diffusion_init(output) -> int:
    """apps/HelloWasm reaction_diffusion: f32 [W,H,C] = random_float() hashed over the coordinates; any output region."""
    return _check(_fn["reaction_diffusion_init"](_as_ptr(output)))


def reaction_diffusion_update(state, mouse_x, mouse_y, frame, new_state) -> int:
    """apps/HelloWasm reaction_diffusion: one time step, f32 [W,H,3] -> f32 [W,H,3]; new_state must hold the state's edge rows and
    columns and the clobber box around the mouse (include/hlmi_pipelines.h)."""
    return _check(_fn["reaction_diffusion_update"](_as_ptr(state), int(mouse_x), int(mouse_y), int(frame), _as_ptr(new_state)))


def reaction_diffusion_render(state, render) -> int:
    """apps/HelloWasm reaction_diffusion: f32 [W,H,3] -> u32 [W,H], the contour colours packed B | G << 8 | R << 16 | 255 << 24."""
    return _check(_fn["reaction_diffusion_render"](_as_ptr(state), _as_ptr(render)))


def _rd_int32(v):
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


def reaction_diffusion_run(state, mouse_x, mouse_y, frame0, steps, new_state, render=None) -> int:
    """`steps` updates with frames frame0 .. frame0 + steps - 1 from state into new_state and, render given, one render of the final
    state: what that many reaction_diffusion_update calls and one reaction_diffusion_render give, in as few launches as the plan
    allows (the switch HLMI_RD_STEPS_PER_LAUNCH = 1, 2, 4 overrides its steps per launch)."""
    fn = lib.hlmi_reaction_diffusion_run
    fn.restype = C.c_int
    fn.argtypes = [_BP, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _BP, _BP]
    return _check(fn(_as_ptr(state), int(mouse_x), int(mouse_y), _rd_int32(frame0), int(steps), _as_ptr(new_state), None if render is None else _as_ptr(render)))


def debug_reaction_diffusion_general(name: str, state=None, mouse_x=0, mouse_y=0, frame=0, steps=1, out=None, render=None) -> int:
    """Test and measurement hook: "reaction_diffusion_init" (out), "reaction_diffusion_update" (state, mouse_x, mouse_y, frame, out),
    "reaction_diffusion_render" (state, render) or "run" (reaction_diffusion_run's arguments, out = new_state) with one thread per
    output and, for "run", one launch per step."""
    fn = lib.hlmi_reaction_diffusion_general
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p, _BP, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _BP, _BP]
    p = lambda b: None if b is None else _as_ptr(b)
    return _check(fn(name.encode(), p(state), int(mouse_x), int(mouse_y), _rd_int32(frame), int(steps), p(out), p(render)))


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


# resnet50_batch, a library extension (the reference's generator has no batch dimension): N images per call, each bit for bit what
# resnet50 gives it.  Arrays: images (N, 224, 224, 3), output (N, 1000).
def resnet50_batch(input, params, output) -> int:
    """f32 [3, 224, 224, N] and resnet50's 267 parameters -> [<= 1000, N]: column n is what resnet50 writes for image n, bit for bit.
    The image range is `output`'s dimension 1; any N >= 1 runs in chunks of 64 images (HLMI_RN50_BATCH_CHUNK = 1 .. 64 overrides)."""
    return _check(_fn["resnet50_batch"](*_resnet50_args(input, params, output)))


def debug_resnet50_batch_general(input, params, output) -> int:
    """Test and measurement hook: resnet50_batch with every convolution on the one-thread-per-output kernel."""
    fn = lib.hlmi_resnet50_batch_general
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(C.c_void_p)]
    args = _resnet50_args(input, params, output)
    return _check(fn((C.c_void_p * len(args))(*[None if a is None else C.cast(a, C.c_void_p) for a in args])))


# `variant` of the batched layer hook: the plan's choice, the general kernel, then each MFMA tile instance (co x pixels) in turn
RESNET50_LAYER_VARIANTS = ("plan", "general", "mfma_64x64", "mfma_64x128")
RESNET50_LAUNCH_NAMES = ("resnet50_conv_mfma", "resnet50_conv_general", "resnet50_maxpool", "resnet50_avgpool", "resnet50_fc", "resnet50_softmax",
                         "resnet50_conv_mfma_wide")


def debug_resnet50_layer_batch(input, weights, gamma, beta, mu, sig, residual, stride, pad, mode, output, variant=0) -> int:
    """debug_resnet50_layer over N images: input [CI, W, H, N], residual and output [CO, OW, OH, N]; variant: an index into or a name of
    RESNET50_LAYER_VARIANTS (an unknown index is refused with -8)."""
    fn = lib.hlmi_debug_resnet50_layer_batch
    fn.restype, fn.argtypes = C.c_int, [_BP] * 7 + [C.c_int32] * 4 + [_BP]
    mode = RESNET50_LAYER_MODES.index(mode) if isinstance(mode, str) else int(mode)
    variant = RESNET50_LAYER_VARIANTS.index(variant) if isinstance(variant, str) else int(variant)
    return _check(fn(*[_as_ptr(b) for b in (input, weights, gamma, beta, mu, sig, residual)], int(stride), int(pad), mode, variant, _as_ptr(output)))


def debug_resnet50_maxpool_batch(input, k, stride, pad, output) -> int:
    """debug_resnet50_maxpool over N images: [C, W, H, N] -> [C, OW, OH, N]."""
    fn = lib.hlmi_debug_resnet50_maxpool_batch
    fn.restype, fn.argtypes = C.c_int, [_BP, C.c_int32, C.c_int32, C.c_int32, _BP]
    return _check(fn(_as_ptr(input), int(k), int(stride), int(pad), _as_ptr(output)))


def debug_resnet50_tail_batch(input, fc_weights, fc_bias, output) -> int:
    """debug_resnet50_tail over N images: [C, W, H, N] -> [classes, N]."""
    fn = lib.hlmi_debug_resnet50_tail_batch
    fn.restype, fn.argtypes = C.c_int, [_BP] * 4
    return _check(fn(*[_as_ptr(b) for b in (input, fc_weights, fc_bias, output)]))


def debug_resnet50_batch_plan(n, general=False) -> dict:
    """The launch plan of resnet50_batch for n images, without a device: {"chunk": images per run of the plan in force, "chunks": one list
    per run, each of 57 steps {"name", "grid": (x, y), "tile": (co, pixels) or None}}."""
    fn = lib.hlmi_debug_resnet50_batch_plan
    fn.restype, fn.argtypes = C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    if n < 1:
        raise ValueError("debug_resnet50_batch_plan takes n >= 1")
    chunk, steps = C.c_int32(0), (C.c_int32 * (64 * 5))()

    def run(images):
        count = fn(images, int(bool(general)), C.byref(chunk), steps)
        if count < 0:
            _check(count)
        return [{"name": RESNET50_LAUNCH_NAMES[steps[5 * i]], "grid": (steps[5 * i + 1], steps[5 * i + 2]),
                 "tile": (steps[5 * i + 3], steps[5 * i + 4]) if steps[5 * i + 3] else None} for i in range(count)]

    first = run(n)   # the first run of the batch: min(n, chunk) images, and the chunk size in force
    size = chunk.value
    full, rest = divmod(n, size)
    return {"chunk": size, "chunks": [first] * max(full, 1) + ([run(rest)] if full and rest else [])}


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


# apps/hannk's op library lives in hannk.py, which takes lib, _fn, _check, Buffer … from this module: imported last
from .hannk import *      # noqa: E402,F401,F403
