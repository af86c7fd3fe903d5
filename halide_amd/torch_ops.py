"""PyTorch-ROCm operators over libhlmi.so — SURVEY.md §8(f4).

The reference puts AOT pipelines behind torch through generated wrappers that build a ``halide_buffer_t`` around a
tensor's storage with the dimensions reversed (``src/runtime/HalidePyTorchHelpers.h:28-120``, ``apps/HelloPyTorch``).
This module does the same against the C ABI, without a copy: a CUDA(HIP) tensor's ``data_ptr()`` is attached with
``halide_hip_wrap_device_ptr`` (counterpart of ``halide_cuda_wrap_device_ptr``, ``src/runtime/HalideRuntimeCuda.h:44-58``),
the library enqueues on torch's current stream (``halide_hip_set_stream``), the result lands in a tensor allocated by
torch, and the wrapper detaches before returning so the library never owns torch memory.

    import torch, halide_amd.torch_ops          # registers torch.ops.hlmi.*
    out = torch.ops.hlmi.local_laplacian(img_u16_cuda, 8, 1 / 7, 1.0)       # (3, H, W) uint16 -> same

Tensor axes are the Halide dimensions REVERSED (innermost last), as in the reference's Python bindings: an image
``Buffer<uint16_t, 3>(W, H, 3)`` is a tensor of shape ``(3, H, W)``.  There is no CPU fallback: CPU tensors are an error.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

import halide_amd as hl

_NP = {torch.uint8: np.uint8, torch.uint16: np.uint16, torch.int16: np.int16, torch.int32: np.int32, torch.float32: np.float32,
       torch.float64: np.float64}


class _Wrapped:
    """`with _Wrapped(t0, t1, ...) as (b0, b1, ...)`: zero-copy halide buffers on torch's current stream."""

    def __init__(self, *tensors):
        self.tensors, self.bufs = tensors, []

    def __enter__(self):
        for t in self.tensors:
            if not t.is_cuda:
                raise RuntimeError("hlmi ops need tensors on the GPU (there is no CPU implementation)")
            if t.dtype not in _NP:
                raise TypeError(f"unsupported dtype {t.dtype}")
            if t.dim() and t.stride(-1) != 1:
                raise RuntimeError("the innermost dimension must be dense (halide dim[0].stride == 1)")
            self.bufs.append(hl.Buffer.wrap_device(t.data_ptr(), _NP[t.dtype], list(reversed(t.shape)),
                                                   list(reversed(t.stride()))))
        # torch's default stream is the NULL stream (handle 0), which halide_hip_set_stream reads as "the library's own
        # stream": name it by HIP's explicit handle hipStreamLegacy (= 1) instead
        s = torch.cuda.current_stream(self.tensors[0].device).cuda_stream
        hl.set_stream(s if s else 1)
        hl.set_gpu_device(self.tensors[0].device.index or 0)
        return self.bufs

    def __exit__(self, *exc):
        hl.set_stream(None)
        for b in self.bufs:
            b.device_detach()   # the storage belongs to torch
        return False


@torch.library.custom_op("hlmi::local_laplacian", mutates_args=())
def local_laplacian(input: torch.Tensor, levels: int, alpha: float, beta: float) -> torch.Tensor:
    """apps/local_laplacian: (3, H, W) uint16 -> (3, H, W) uint16; `alpha` as the drivers pass it (alpha / (levels - 1))."""
    out = torch.empty_like(input)
    with _Wrapped(input, out) as (a, o):
        hl.local_laplacian(a, levels, alpha, beta, o)
    return out


@torch.library.custom_op("hlmi::bilateral_grid", mutates_args=())
def bilateral_grid(input: torch.Tensor, r_sigma: float) -> torch.Tensor:
    """apps/bilateral_grid: (H, W) float32 -> (H, W) float32, s_sigma = 8."""
    out = torch.empty_like(input)
    with _Wrapped(input, out) as (a, o):
        hl.bilateral_grid(a, r_sigma, o)
    return out


@torch.library.custom_op("hlmi::nl_means", mutates_args=())
def nl_means(input: torch.Tensor, patch_size: int, search_area: int, sigma: float) -> torch.Tensor:
    """apps/nl_means: (3, H, W) float32 -> (3, H, W) float32."""
    out = torch.empty_like(input)
    with _Wrapped(input, out) as (a, o):
        hl.nl_means(a, patch_size, search_area, sigma, o)
    return out


@torch.library.custom_op("hlmi::stencil_chain", mutates_args=())
def stencil_chain(input: torch.Tensor) -> torch.Tensor:
    """apps/stencil_chain: (H, W) uint16 -> (H, W) uint16, 32 stages."""
    out = torch.empty_like(input)
    with _Wrapped(input, out) as (a, o):
        hl.stencil_chain(a, o)
    return out


@torch.library.custom_op("hlmi::blur", mutates_args=())
def blur(input: torch.Tensor) -> torch.Tensor:
    """apps/blur: (H + 2, W + 2) uint16 -> (H, W) uint16."""
    out = torch.empty((input.shape[0] - 2, input.shape[1] - 2), dtype=input.dtype, device=input.device)
    with _Wrapped(input, out) as (a, o):
        hl.halide_blur(a, o)
    return out


def _conv(fn, input, filter, bias):
    n, hp, wp, _ = input.shape
    out = torch.empty((n, hp - 2, wp - 2, bias.shape[0]), dtype=torch.float32, device=input.device)
    with _Wrapped(input, filter, bias, out) as (a, f, b, o):
        fn(a, f, b, o)
    return out


@torch.library.custom_op("hlmi::conv_layer", mutates_args=())
def conv_layer(input: torch.Tensor, filter: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """apps/conv_layer, exact f32: input (N, H+2, W+2, CI), filter (CI, 3, 3, CO), bias (CO,) -> relu (N, H, W, CO)."""
    return _conv(hl.conv_layer, input, filter, bias)


@torch.library.custom_op("hlmi::conv_layer_bf16", mutates_args=())
def conv_layer_bf16(input: torch.Tensor, filter: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """Same buffers as conv_layer; operands rounded to bf16, f32 accumulation on the matrix cores."""
    return _conv(hl.conv_layer_bf16, input, filter, bias)


@torch.library.custom_op("hlmi::depthwise_separable_conv", mutates_args=())
def depthwise_separable_conv(input: torch.Tensor, depthwise_filter: torch.Tensor, pointwise_filter: torch.Tensor,
                             bias: torch.Tensor) -> torch.Tensor:
    """apps/depthwise_separable_conv: input (N, H, W, CI), depthwise (FH, FW, IC, CM), pointwise (IC, CO), bias (CO,)."""
    n, h, w, _ = input.shape
    out = torch.empty((n, h, w, bias.shape[0]), dtype=torch.float32, device=input.device)
    with _Wrapped(input, depthwise_filter, pointwise_filter, bias, out) as (a, d, p, b, o):
        hl.depthwise_separable_conv(a, d, p, b, o)
    return out


@torch.library.custom_op("hlmi::unsharp", mutates_args=())
def unsharp(input: torch.Tensor) -> torch.Tensor:
    """apps/unsharp: (3, H, W) float32 -> (3, H, W) float32, sigma = 1.5."""
    out = torch.empty_like(input)
    with _Wrapped(input, out) as (a, o):
        hl.unsharp(a, o)
    return out


@torch.library.custom_op("hlmi::max_filter", mutates_args=())
def max_filter(input: torch.Tensor) -> torch.Tensor:
    """apps/max_filter: (3, H, W) float32 -> (3, H, W) float32, max over the radius-26 footprint of the edge-clamped input."""
    out = torch.empty_like(input)
    with _Wrapped(input, out) as (a, o):
        hl.max_filter(a, o)
    return out


@torch.library.custom_op("hlmi::hist", mutates_args=())
def hist(input: torch.Tensor) -> torch.Tensor:
    """apps/hist: (3, H, W) uint8 -> (3, H, W) uint8, histogram equalisation of the luma."""
    out = torch.empty_like(input)
    with _Wrapped(input, out) as (a, o):
        hl.hist(a, o)
    return out


@torch.library.custom_op("hlmi::camera_pipe", mutates_args=())
def camera_pipe(input: torch.Tensor, matrix_3200: torch.Tensor, matrix_7000: torch.Tensor, color_temp: float, gamma: float,
                contrast: float, sharpen_strength: float, black_level: int, white_level: int, out_width: int,
                out_height: int) -> torch.Tensor:
    """apps/camera_pipe: raw (IH, IW) uint16 Bayer -> (3, out_height, out_width) uint8."""
    out = torch.empty((3, out_height, out_width), dtype=torch.uint8, device=input.device)
    with _Wrapped(input, matrix_3200, matrix_7000, out) as (a, m3, m7, o):
        hl.camera_pipe(a, m3, m7, color_temp, gamma, contrast, sharpen_strength, black_level, white_level, o)
    return out


@torch.library.custom_op("hlmi::harris", mutates_args=())
def harris(input: torch.Tensor) -> torch.Tensor:
    """apps/harris: (3, H, W) float32 -> (H - 6, W - 6) float32 corner response of the interior (the driver's region:
    output origin (3, 3) in the input's frame, apps/harris/filter.cpp:22-28)."""
    c, h, w = input.shape
    out = torch.empty((h - 6, w - 6), dtype=torch.float32, device=input.device)
    with _Wrapped(input, out) as (a, o):
        o.set_min(3, 3)
        hl.harris(a, o)
    return out


@torch.library.custom_op("hlmi::interpolate", mutates_args=())
def interpolate(input: torch.Tensor) -> torch.Tensor:
    """apps/interpolate: (4, H, W) float32 RGBA -> (3, H, W) float32, alpha-weighted pull-push."""
    out = torch.empty((3,) + tuple(input.shape[1:]), dtype=torch.float32, device=input.device)
    with _Wrapped(input, out) as (a, o):
        hl.interpolate(a, o)
    return out


@torch.library.custom_op("hlmi::iir_blur", mutates_args=())
def iir_blur(input: torch.Tensor, alpha: float) -> torch.Tensor:
    """apps/iir_blur: (C, H, W) float32 -> same, first-order IIR low pass down / up the columns, then along the rows."""
    out = torch.empty_like(input)
    with _Wrapped(input, out) as (a, o):
        hl.iir_blur(a, alpha, o)
    return out


def _resize_shape(input, scale_factor):
    # apps/resize/resize.cpp:77-78: int out_width = in.width() * scale_factor (int * float in f32, truncated)
    w, h = int(np.float32(input.shape[2]) * np.float32(scale_factor)), int(np.float32(input.shape[1]) * np.float32(scale_factor))
    return (input.shape[0], h, w)


@torch.library.custom_op("hlmi::resize", mutates_args=())
def resize(input: torch.Tensor, scale_factor: float, interpolation: str = "cubic", upsample: Optional[bool] = None) -> torch.Tensor:
    """apps/resize: (C, H, W) uint8 / uint16 / float32 -> (C, int(H * scale_factor), int(W * scale_factor)) of the same type;
    interpolation box / linear / cubic / lanczos; `upsample` picks the _up or _down variant (default: scale_factor > 1)."""
    if input.dim() != 3 or input.dtype not in (torch.uint8, torch.uint16, torch.float32):
        raise TypeError("resize takes a (C, H, W) tensor of uint8, uint16 or float32")
    out = torch.empty(_resize_shape(input, scale_factor), dtype=input.dtype, device=input.device)
    with _Wrapped(input, out) as (a, o):
        hl.resize(a, scale_factor, o, interpolation, upsample)
    return out


def _gaussian_blur_out(input):
    # rows padded to a multiple of 16 elements (the resampled variants pin output.stride.1 to one); the result is the view of
    # the image's own columns
    h, w = input.shape
    return input.new_empty((h, -(-w // 16) * 16))[:, :w]


@torch.library.custom_op("hlmi::gaussian_blur", mutates_args=())
def gaussian_blur(input: torch.Tensor, sigma: float, trunc: int = 5, upsample_order: int = 0, downsample_order: int = 0,
                  factor: int = 0) -> torch.Tensor:
    """apps/gaussian_blur: (H, W) float32 -> (H, W) float32 blurred with `sigma`, truncated at `trunc` sigmas.  All three of
    upsample_order, downsample_order and factor 0: the direct blur; otherwise the variant gaussian_blur_<U>_<D>_<F>."""
    if input.dim() != 2 or input.dtype != torch.float32:
        raise TypeError("gaussian_blur takes an (H, W) float32 tensor")
    direct = upsample_order == 0 and downsample_order == 0 and factor == 0
    if not direct:
        hl.gaussian_blur_variant(upsample_order, downsample_order, factor)   # ValueError outside the 36
    out = _gaussian_blur_out(input)
    with _Wrapped(input, out) as (a, o):
        if direct:
            hl.gaussian_blur_direct(a, sigma, trunc, o)
        else:
            hl.gaussian_blur(a, sigma, trunc, o, upsample_order, downsample_order, factor)
    return out


def _blur3_check(name, input):
    if input.dim() != 3 or input.dtype != torch.float32:
        raise TypeError(f"{name} takes a (C, H, W) float32 tensor")


@torch.library.custom_op("hlmi::linear_blur", mutates_args=())
def linear_blur(input: torch.Tensor) -> torch.Tensor:
    """apps/linear_blur: (C, H, W) float32 sRGB -> (C, H, W) float32, the 3x3 box blur over x .. x + 2, y .. y + 2 of the
    edge-clamped image, taken in linear light."""
    _blur3_check("linear_blur", input)
    out = torch.empty(tuple(input.shape), dtype=torch.float32, device=input.device)
    with _Wrapped(input, out) as (a, o):
        hl.linear_blur(a, o)
    return out


@torch.library.custom_op("hlmi::simple_blur", mutates_args=())
def simple_blur(input: torch.Tensor) -> torch.Tensor:
    """apps/linear_blur's simple_blur: (C, H, W) float32 -> (C, H, W) float32, the same blur on the values as they are; width and
    height are the image's (apps/linear_blur/run_linear_blur.cpp:33)."""
    _blur3_check("simple_blur", input)
    out = torch.empty(tuple(input.shape), dtype=torch.float32, device=input.device)
    with _Wrapped(input, out) as (a, o):
        hl.simple_blur(a, input.shape[2], input.shape[1], o)
    return out


def _wavelet_forward(name, fn, input):
    if input.dim() != 2 or input.dtype != torch.float32:
        raise TypeError(f"{name} takes an (H, W) float32 tensor")
    out = torch.empty((2, input.shape[0], input.shape[1] // 2), dtype=torch.float32, device=input.device)
    with _Wrapped(input, out) as (a, o):
        fn(a, o)
    return out


def _wavelet_inverse(name, fn, input):
    if input.dim() != 3 or input.shape[0] != 2 or input.dtype != torch.float32:
        raise TypeError(f"{name} takes a (2, H, W2) float32 tensor")
    out = torch.empty((input.shape[1], 2 * input.shape[2]), dtype=torch.float32, device=input.device)
    with _Wrapped(input, out) as (a, o):
        fn(a, o)
    return out


@torch.library.custom_op("hlmi::haar_x", mutates_args=())
def haar_x(input: torch.Tensor) -> torch.Tensor:
    """apps/wavelet: (H, W) float32 -> (2, H, W // 2) float32, the pair means and half differences, the output the driver allocates
    (apps/wavelet/wavelet.cpp:61)."""
    return _wavelet_forward("haar_x", hl.haar_x, input)


@torch.library.custom_op("hlmi::daubechies_x", mutates_args=())
def daubechies_x(input: torch.Tensor) -> torch.Tensor:
    """apps/wavelet: (H, W) float32 -> (2, H, W // 2) float32, the D4 low-pass and high-pass of the edge-clamped rows."""
    return _wavelet_forward("daubechies_x", hl.daubechies_x, input)


@torch.library.custom_op("hlmi::inverse_haar_x", mutates_args=())
def inverse_haar_x(input: torch.Tensor) -> torch.Tensor:
    """apps/wavelet: (2, H, W2) float32 -> (H, 2 * W2) float32, the inverse of haar_x."""
    return _wavelet_inverse("inverse_haar_x", hl.inverse_haar_x, input)


@torch.library.custom_op("hlmi::inverse_daubechies_x", mutates_args=())
def inverse_daubechies_x(input: torch.Tensor) -> torch.Tensor:
    """apps/wavelet: (2, H, W2) float32 -> (H, 2 * W2) float32, the D4 synthesis from pairs x / 2 and x / 2 + 1 (clamped)."""
    return _wavelet_inverse("inverse_daubechies_x", hl.inverse_daubechies_x, input)


def _rd_state_check(name, state):
    if state.dim() != 3 or state.shape[0] != 3 or state.dtype != torch.float32:
        raise TypeError(f"{name} takes a (3, H, W) float32 tensor")


def _rd_pixels(t):
    """the u32 halide buffer over an int32 tensor of packed pixels (torch has no arithmetic on uint32: the bits are what matters)"""
    return hl.Buffer.wrap_device(t.data_ptr(), np.uint32, list(reversed(t.shape)), list(reversed(t.stride())))


@torch.library.custom_op("hlmi::reaction_diffusion_init", mutates_args=())
def reaction_diffusion_init(height: int, width: int, device: torch.device) -> torch.Tensor:
    """apps/HelloWasm reaction_diffusion: a (3, height, width) float32 state of random_float() hashed over the coordinates."""
    out = torch.empty((3, height, width), dtype=torch.float32, device=device)
    with _Wrapped(out) as (o,):
        hl.reaction_diffusion_init(o)
    return out


@torch.library.custom_op("hlmi::reaction_diffusion_update", mutates_args=())
def reaction_diffusion_update(state: torch.Tensor, mouse_x: int, mouse_y: int, frame: int) -> torch.Tensor:
    """apps/HelloWasm reaction_diffusion: one time step, (3, H, W) float32 -> (3, H, W) float32."""
    _rd_state_check("reaction_diffusion_update", state)
    out = torch.empty(tuple(state.shape), dtype=torch.float32, device=state.device)
    with _Wrapped(state, out) as (a, o):
        hl.reaction_diffusion_update(a, mouse_x, mouse_y, frame, o)
    return out


@torch.library.custom_op("hlmi::reaction_diffusion_render", mutates_args=())
def reaction_diffusion_render(state: torch.Tensor) -> torch.Tensor:
    """apps/HelloWasm reaction_diffusion: (3, H, W) float32 -> (H, W) int32 holding the packed pixels' 32 bits, B | G << 8 | R << 16 |
    255 << 24."""
    _rd_state_check("reaction_diffusion_render", state)
    out = torch.empty(tuple(state.shape[1:]), dtype=torch.int32, device=state.device)
    with _Wrapped(state) as (a,):
        p = _rd_pixels(out)
        try:
            hl.reaction_diffusion_render(a, p)
        finally:
            p.device_detach()
    return out


@torch.library.custom_op("hlmi::reaction_diffusion_run", mutates_args=())
def reaction_diffusion_run(state: torch.Tensor, mouse_x: int, mouse_y: int, frame0: int, steps: int) -> tuple[torch.Tensor, torch.Tensor]:
    """`steps` updates with frames frame0 .. frame0 + steps - 1 and one render of the final state: the new (3, H, W) float32 state and the
    (H, W) int32 packed pixels, in as few launches as the library's plan allows."""
    _rd_state_check("reaction_diffusion_run", state)
    out = torch.empty(tuple(state.shape), dtype=torch.float32, device=state.device)
    pix = torch.empty(tuple(state.shape[1:]), dtype=torch.int32, device=state.device)
    with _Wrapped(state, out) as (a, o):
        p = _rd_pixels(pix)
        try:
            hl.reaction_diffusion_run(a, mouse_x, mouse_y, frame0, steps, o, p)
        finally:
            p.device_detach()
    return out, pix


@torch.library.custom_op("hlmi::compositing", mutates_args=())
def compositing(layers: list[torch.Tensor], ops: torch.Tensor) -> torch.Tensor:
    """apps/compositing: six (4, H, W) uint8 layers and five int32 op codes (0 over, 1 atop, 2 xor, 3 in, 4 out; any other code skips
    its layer) -> (4, H, W) uint8, the generator's integer form.  The op codes are read on the device."""
    if len(layers) != 6 or any(t.dim() != 3 or t.shape != layers[0].shape or t.shape[0] != 4 or t.dtype != torch.uint8 for t in layers):
        raise TypeError("compositing takes six (4, H, W) uint8 tensors of one shape")
    if ops.dim() != 1 or ops.shape[0] != 5 or ops.dtype != torch.int32:
        raise TypeError("compositing takes five int32 op codes")
    out = torch.empty_like(layers[0])
    with _Wrapped(*layers, ops, out) as bufs:
        hl.compositing(bufs[:6], bufs[6], bufs[7])
    return out


def _plane_check(name, input):
    if input.dim() != 2 or input.dtype != torch.uint8:
        raise TypeError(f"{name} takes an (H, W) uint8 tensor")


def _plane_op(name, input):
    _plane_check(name, input)
    out = torch.empty_like(input, memory_format=torch.contiguous_format)
    with _Wrapped(input, out) as (a, o):
        getattr(hl, name)(a, o)
    return out


def _conv3x3(name, input, mask):
    _plane_check(name, input)
    if mask.dim() != 2 or tuple(mask.shape) != (3, 3) or mask.dtype != torch.int8:
        raise TypeError(f"{name} takes a (3, 3) int8 mask")
    out = torch.empty_like(input, memory_format=torch.contiguous_format)
    with _Wrapped(input, out) as (a, o):
        # the entry point reads the nine values on the host: hand them over there
        getattr(hl, name)(a, hl.Buffer(mask.cpu().contiguous().numpy()), o)
    return out


@torch.library.custom_op("hlmi::mat_mul", mutates_args=())
def mat_mul(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """apps/cuda_mat_mul at any size 1 .. 8192: two (n, n) float32 tensors -> (n, n) float32, out[y][x] the k-ordered fmaf chain over
    r of A[r][x] * B[y][r] from +0.  Mathematically this is B @ A, NOT A @ B: tensor axes are the Halide dimensions reversed, and the
    generator writes out(x, y) += A(x, r) * B(r, y)."""
    for t in (A, B):
        if t.dim() != 2 or t.shape[0] != t.shape[1] or t.dtype != torch.float32:
            raise TypeError("mat_mul takes two square float32 tensors")
    if A.shape != B.shape:
        raise TypeError("mat_mul takes two tensors of one size")
    n = A.shape[0]
    if not 1 <= n <= 8192:
        raise TypeError("mat_mul takes sizes 1 .. 8192")
    out = torch.empty((n, n), dtype=torch.float32, device=A.device)
    with _Wrapped(A, B, out) as (a, b, o):
        hl.mat_mul_sized(n, a, b, o)
    return out


@torch.library.custom_op("hlmi::resnet50", mutates_args=())
def resnet50(input: torch.Tensor, params: list[torch.Tensor]) -> torch.Tensor:
    """apps/resnet_50: a (224, 224, 3) float32 image (Halide's (c, x, y) reversed) and the 267 parameters in signature order
    (hl.RESNET50_PARAM_NAMES; convolution weights as (CI, KH, KW, CO), fc1000_weights as (2048, 1000)) -> (1000,) float32
    probabilities.  float32 only."""
    if len(params) != len(hl.RESNET50_PARAM_NAMES):
        raise TypeError(f"resnet50 takes {len(hl.RESNET50_PARAM_NAMES)} parameters, not {len(params)}")
    for t in (input, *params):
        if t.dtype != torch.float32:
            raise TypeError("resnet50 takes float32 tensors only")
    if tuple(input.shape) != (224, 224, 3):
        raise TypeError("resnet50 takes a (224, 224, 3) image")
    out = torch.empty((1000,), dtype=torch.float32, device=input.device)
    with _Wrapped(input, *params, out) as bufs:
        hl.resnet50(bufs[0], bufs[1:-1], bufs[-1])
    return out


@torch.library.custom_op("hlmi::resnet50_batch", mutates_args=())
def resnet50_batch(input: torch.Tensor, params: list[torch.Tensor]) -> torch.Tensor:
    """resnet50 over N images per call (a library extension: the reference's generator has no batch dimension): (N, 224, 224, 3)
    float32 images in the layout resnet50 takes for one, the same 267 parameters -> (N, 1000) float32; row n is bit for bit what
    resnet50 gives image n.  float32 only."""
    if len(params) != len(hl.RESNET50_PARAM_NAMES):
        raise TypeError(f"resnet50_batch takes {len(hl.RESNET50_PARAM_NAMES)} parameters, not {len(params)}")
    for t in (input, *params):
        if t.dtype != torch.float32:
            raise TypeError("resnet50_batch takes float32 tensors only")
    if input.dim() != 4 or tuple(input.shape[1:]) != (224, 224, 3) or input.shape[0] < 1:
        raise TypeError("resnet50_batch takes (N, 224, 224, 3) images, N >= 1")
    out = torch.empty((input.shape[0], 1000), dtype=torch.float32, device=input.device)
    with _Wrapped(input, *params, out) as bufs:
        hl.resnet50_batch(bufs[0], bufs[1:-1], bufs[-1])
    return out


@torch.library.custom_op("hlmi::fft2d", mutates_args=())
def fft2d(input: torch.Tensor, kind: str, gain: float) -> torch.Tensor:
    """apps/fft at any allowed size: kind "c2c_forward" / "c2c_inverse" take and return a complex array, "r2c" takes a real (N1, N0)
    tensor and returns the N1/2 + 1 rows of its spectrum, "c2r" takes those rows and returns the real (N1, N0) array.  A complex
    array is a float32 tensor (rows, N0, 2), the layout of torch.view_as_real and the generator's interleaved one: no copy either way."""
    if kind not in hl.FFT_KINDS:
        raise TypeError(f"fft2d: kind must be one of {hl.FFT_KINDS}")
    real_in = kind == "r2c"
    if input.dtype != torch.float32 or input.dim() != (2 if real_in else 3) or (not real_in and input.shape[2] != 2):
        raise TypeError("fft2d takes a float32 tensor (rows, N0) for r2c and (rows, N0, 2) otherwise")
    if input.stride(-1) != 1 or (not real_in and input.stride(1) != 2):
        raise RuntimeError("fft2d: the components and dimension 0 must be dense")
    rows, n0 = input.shape[0], input.shape[1]
    n1 = 2 * (rows - 1) if kind == "c2r" else rows
    out_shape = {"r2c": (n1 // 2 + 1, n0, 2), "c2r": (n1, n0)}.get(kind, (n1, n0, 2))
    out = torch.empty(out_shape, dtype=torch.float32, device=input.device)
    if not input.is_cuda:
        raise RuntimeError("hlmi ops need tensors on the GPU (there is no CPU implementation)")

    def wrap(t, comps):
        return hl.Buffer.wrap_device(t.data_ptr(), np.float32, [n0, t.shape[0], comps], [comps, t.stride(0), 1])

    a, o = wrap(input, 1 if real_in else 2), wrap(out, 1 if kind == "c2r" else 2)
    s = torch.cuda.current_stream(input.device).cuda_stream
    hl.set_stream(s if s else 1)
    hl.set_gpu_device(input.device.index or 0)
    try:
        hl.fft2d(kind, a, o, gain, sizes=(n0, n1))
    finally:
        hl.set_stream(None)
        a.device_detach()
        o.device_detach()
    return out


# ---- apps/linear_algebra (include/hlmi_blas.h): functional forms, each returns a new tensor and leaves its arguments as they are.
# A matrix with Halide extents (w, h) — column-major in BLAS terms — is a tensor of shape (h, w).
def _la_check(what, *pairs):
    """pairs: (tensor, number of dimensions)"""
    for t, nd in pairs:
        if t.dim() != nd or t.dtype != torch.float32:
            raise TypeError(f"{what} takes float32 tensors of {', '.join(str(n) for _, n in pairs)} dimensions")


@torch.library.custom_op("hlmi::saxpy", mutates_args=())
def saxpy(a: float, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """a * x + y over two float32 vectors of one length"""
    _la_check("saxpy", (x, 1), (y, 1))
    if x.shape != y.shape:
        raise TypeError("saxpy takes two vectors of one length")
    out = torch.empty_like(y, memory_format=torch.contiguous_format)
    with _Wrapped(x, y, out) as (bx, by, bo):
        hl.saxpy(a, bx, by, bo)
    return out


@torch.library.custom_op("hlmi::sdot", mutates_args=())
def sdot(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """the dot product in the contract's order (eight lane chains, their sum, the tail): a 0-dimensional tensor"""
    _la_check("sdot", (x, 1), (y, 1))
    if x.shape != y.shape:
        raise TypeError("sdot takes two vectors of one length")
    out = torch.empty((), dtype=torch.float32, device=x.device)
    with _Wrapped(x, y, out) as (bx, by, bo):
        hl.sdot(bx, by, bo)
    return out


@torch.library.custom_op("hlmi::sasum", mutates_args=())
def sasum(x: torch.Tensor) -> torch.Tensor:
    """the sum of |x| in the contract's order: a 0-dimensional tensor"""
    _la_check("sasum", (x, 1))
    out = torch.empty((), dtype=torch.float32, device=x.device)
    with _Wrapped(x, out) as (bx, bo):
        hl.sasum(bx, bo)
    return out


@torch.library.custom_op("hlmi::sgemv", mutates_args=())
def sgemv(trans: bool, a: float, A: torch.Tensor, x: torch.Tensor, b: float, y: torch.Tensor) -> torch.Tensor:
    """a op(A) x + b y for A of shape (h, w): notrans x[h], y[w]; trans x[w], y[h]"""
    _la_check("sgemv", (A, 2), (x, 1), (y, 1))
    h, w = A.shape
    if (x.shape[0], y.shape[0]) != ((w, h) if trans else (h, w)):
        raise TypeError("sgemv: the vectors do not fit the matrix")
    out = torch.empty_like(y, memory_format=torch.contiguous_format)
    with _Wrapped(A, x, y, out) as (bA, bx, by, bo):
        hl.sgemv(trans, a, bA, bx, b, by, bo)
    return out


@torch.library.custom_op("hlmi::sger", mutates_args=())
def sger(a: float, x: torch.Tensor, y: torch.Tensor, A: torch.Tensor) -> torch.Tensor:
    """A + a x y' for x[m], y[n] and A of shape (n, m)"""
    _la_check("sger", (x, 1), (y, 1), (A, 2))
    if tuple(A.shape) != (y.shape[0], x.shape[0]):
        raise TypeError("sger: the vectors do not fit the matrix")
    out = A.clone(memory_format=torch.contiguous_format)
    with _Wrapped(x, y, out) as (bx, by, bo):
        hl.sger(a, bx, by, bo)
    return out


@torch.library.custom_op("hlmi::sgemm", mutates_args=())
def sgemm(transA: bool, transB: bool, a: float, A: torch.Tensor, B: torch.Tensor, b: float, C: torch.Tensor) -> torch.Tensor:
    """a op(A) op(B) + b C with k upward; A of shape (K, M) as stored, B (N, K), C (N, M); a transposed operand must be square"""
    _la_check("sgemm", (A, 2), (B, 2), (C, 2))
    K, M = A.shape
    N = B.shape[0]
    if B.shape[1] != K or tuple(C.shape) != (N, M) or (transA and M != K) or (transB and N != K):
        raise TypeError("sgemm: the shapes do not fit (A (K, M), B (N, K), C (N, M); a transposed operand is square)")
    out = torch.empty((N, M), dtype=torch.float32, device=C.device)
    with _Wrapped(A, B, C, out) as (bA, bB, bC, bo):
        hl.sgemm(transA, transB, a, bA, bB, b, bC, bo)
    return out


# ---- the f64 half: the same six forms over float64 tensors
def _la_check_f64(what, *pairs):
    """pairs: (tensor, number of dimensions); a float32 tensor is refused, not converted"""
    for t, nd in pairs:
        if t.dim() != nd or t.dtype != torch.float64:
            raise TypeError(f"{what} takes float64 tensors of {', '.join(str(n) for _, n in pairs)} dimensions")


@torch.library.custom_op("hlmi::daxpy", mutates_args=())
def daxpy(a: float, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """a * x + y over two float64 vectors of one length"""
    _la_check_f64("daxpy", (x, 1), (y, 1))
    if x.shape != y.shape:
        raise TypeError("daxpy takes two vectors of one length")
    out = torch.empty_like(y, memory_format=torch.contiguous_format)
    with _Wrapped(x, y, out) as (bx, by, bo):
        hl.daxpy(a, bx, by, bo)
    return out


@torch.library.custom_op("hlmi::ddot", mutates_args=())
def ddot(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """the dot product in the contract's order (four lane chains, their sum, the tail): a 0-dimensional tensor"""
    _la_check_f64("ddot", (x, 1), (y, 1))
    if x.shape != y.shape:
        raise TypeError("ddot takes two vectors of one length")
    out = torch.empty((), dtype=torch.float64, device=x.device)
    with _Wrapped(x, y, out) as (bx, by, bo):
        hl.ddot(bx, by, bo)
    return out


@torch.library.custom_op("hlmi::dasum", mutates_args=())
def dasum(x: torch.Tensor) -> torch.Tensor:
    """the sum of |x| in the contract's order: a 0-dimensional tensor"""
    _la_check_f64("dasum", (x, 1))
    out = torch.empty((), dtype=torch.float64, device=x.device)
    with _Wrapped(x, out) as (bx, bo):
        hl.dasum(bx, bo)
    return out


@torch.library.custom_op("hlmi::dgemv", mutates_args=())
def dgemv(trans: bool, a: float, A: torch.Tensor, x: torch.Tensor, b: float, y: torch.Tensor) -> torch.Tensor:
    """a op(A) x + b y for A of shape (h, w): notrans x[h], y[w]; trans x[w], y[h]"""
    _la_check_f64("dgemv", (A, 2), (x, 1), (y, 1))
    h, w = A.shape
    if (x.shape[0], y.shape[0]) != ((w, h) if trans else (h, w)):
        raise TypeError("dgemv: the vectors do not fit the matrix")
    out = torch.empty_like(y, memory_format=torch.contiguous_format)
    with _Wrapped(A, x, y, out) as (bA, bx, by, bo):
        hl.dgemv(trans, a, bA, bx, b, by, bo)
    return out


@torch.library.custom_op("hlmi::dger", mutates_args=())
def dger(a: float, x: torch.Tensor, y: torch.Tensor, A: torch.Tensor) -> torch.Tensor:
    """A + a x y' for x[m], y[n] and A of shape (n, m)"""
    _la_check_f64("dger", (x, 1), (y, 1), (A, 2))
    if tuple(A.shape) != (y.shape[0], x.shape[0]):
        raise TypeError("dger: the vectors do not fit the matrix")
    out = A.clone(memory_format=torch.contiguous_format)
    with _Wrapped(x, y, out) as (bx, by, bo):
        hl.dger(a, bx, by, bo)
    return out


@torch.library.custom_op("hlmi::dgemm", mutates_args=())
def dgemm(transA: bool, transB: bool, a: float, A: torch.Tensor, B: torch.Tensor, b: float, C: torch.Tensor) -> torch.Tensor:
    """a op(A) op(B) + b C with k upward; A of shape (K, M) as stored, B (N, K), C (N, M); a transposed operand must be square"""
    _la_check_f64("dgemm", (A, 2), (B, 2), (C, 2))
    K, M = A.shape
    N = B.shape[0]
    if B.shape[1] != K or tuple(C.shape) != (N, M) or (transA and M != K) or (transB and N != K):
        raise TypeError("dgemm: the shapes do not fit (A (K, M), B (N, K), C (N, M); a transposed operand is square)")
    out = torch.empty((N, M), dtype=torch.float64, device=C.device)
    with _Wrapped(A, B, C, out) as (bA, bB, bC, bo):
        hl.dgemm(transA, transB, a, bA, bB, b, bC, bo)
    return out


@torch.library.custom_op("hlmi::conv3x3a16", mutates_args=())
def conv3x3a16(input: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """apps/hexagon_benchmarks: (H, W) uint8 under a (3, 3) int8 mask (mask[i][j] multiplies in(x + j - 1, y + i - 1)), the sum wrapped
    to int16 -> (H, W) uint8."""
    return _conv3x3("conv3x3a16", input, mask)


@torch.library.custom_op("hlmi::conv3x3a32", mutates_args=())
def conv3x3a32(input: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """apps/hexagon_benchmarks: conv3x3a16 with the sum in int32."""
    return _conv3x3("conv3x3a32", input, mask)


@torch.library.custom_op("hlmi::dilate3x3", mutates_args=())
def dilate3x3(input: torch.Tensor) -> torch.Tensor:
    """apps/hexagon_benchmarks: (H, W) uint8 -> (H, W) uint8, the 3x3 maximum of the edge-clamped image."""
    return _plane_op("dilate3x3", input)


@torch.library.custom_op("hlmi::median3x3", mutates_args=())
def median3x3(input: torch.Tensor) -> torch.Tensor:
    """apps/hexagon_benchmarks: (H, W) uint8 -> (H, W) uint8, the 3x3 median of the edge-clamped image."""
    return _plane_op("median3x3", input)


@torch.library.custom_op("hlmi::gaussian5x5", mutates_args=())
def gaussian5x5(input: torch.Tensor) -> torch.Tensor:
    """apps/hexagon_benchmarks: (H, W) uint8 -> (H, W) uint8, the 5x5 binomial window over 256, truncated."""
    return _plane_op("gaussian5x5", input)


@torch.library.custom_op("hlmi::sobel", mutates_args=())
def sobel(input: torch.Tensor) -> torch.Tensor:
    """apps/hexagon_benchmarks: (H, W) uint8 -> (H, W) uint8, min(|gx| + |gy|, 255), no square root."""
    return _plane_op("sobel", input)


@torch.library.custom_op("hlmi::lens_blur", mutates_args=())
def lens_blur(left_im: torch.Tensor, right_im: torch.Tensor, slices: int, focus_depth: int, blur_radius_scale: float,
              aperture_samples: int) -> torch.Tensor:
    """apps/lens_blur: two (3, H, W) uint8 views -> (3, H, W) float32 (depth from stereo, depth-dependent bokeh)."""
    out = torch.empty(tuple(left_im.shape), dtype=torch.float32, device=left_im.device)
    with _Wrapped(left_im, right_im, out) as (a, b, o):
        hl.lens_blur(a, b, slices, focus_depth, blur_radius_scale, aperture_samples, o)
    return out


@torch.library.custom_op("hlmi::bgu", mutates_args=())
def bgu(r_sigma: float, s_sigma: int, splat_loc: torch.Tensor, values: torch.Tensor, slice_loc: torch.Tensor) -> torch.Tensor:
    """apps/bgu: low-res (3, h, w) float32 pair splat_loc -> values, applied to the full-res (3, H, W) slice_loc."""
    out = torch.empty_like(slice_loc)
    with _Wrapped(splat_loc, values, slice_loc, out) as (a, b, c, o):
        hl.bgu(r_sigma, s_sigma, a, b, c, o)
    return out


# shape functions for torch.compile / meta tensors
@local_laplacian.register_fake
def _(input, levels, alpha, beta):
    return torch.empty_like(input)


@bilateral_grid.register_fake
def _(input, r_sigma):
    return torch.empty_like(input)


@nl_means.register_fake
def _(input, patch_size, search_area, sigma):
    return torch.empty_like(input)


@stencil_chain.register_fake
def _(input):
    return torch.empty_like(input)


@harris.register_fake
def _(input):
    return input.new_empty((input.shape[1] - 6, input.shape[2] - 6))


@interpolate.register_fake
def _(input):
    return input.new_empty((3,) + tuple(input.shape[1:]))


@iir_blur.register_fake
def _(input, alpha):
    return torch.empty_like(input)


@resize.register_fake
def _(input, scale_factor, interpolation="cubic", upsample=None):
    return input.new_empty(_resize_shape(input, scale_factor))


@gaussian_blur.register_fake
def _(input, sigma, trunc=5, upsample_order=0, downsample_order=0, factor=0):
    return _gaussian_blur_out(input)


@linear_blur.register_fake
def _(input):
    return input.new_empty(tuple(input.shape))


@simple_blur.register_fake
def _(input):
    return input.new_empty(tuple(input.shape))


@haar_x.register_fake
def _(input):
    return input.new_empty((2, input.shape[0], input.shape[1] // 2))


@daubechies_x.register_fake
def _(input):
    return input.new_empty((2, input.shape[0], input.shape[1] // 2))


@inverse_haar_x.register_fake
def _(input):
    return input.new_empty((input.shape[1], 2 * input.shape[2]))


@inverse_daubechies_x.register_fake
def _(input):
    return input.new_empty((input.shape[1], 2 * input.shape[2]))


@reaction_diffusion_init.register_fake
def _(height, width, device):
    return torch.empty((3, height, width), dtype=torch.float32, device=device)


@reaction_diffusion_update.register_fake
def _(state, mouse_x, mouse_y, frame):
    return state.new_empty(tuple(state.shape))


@reaction_diffusion_render.register_fake
def _(state):
    return state.new_empty(tuple(state.shape[1:]), dtype=torch.int32)


@reaction_diffusion_run.register_fake
def _(state, mouse_x, mouse_y, frame0, steps):
    return state.new_empty(tuple(state.shape)), state.new_empty(tuple(state.shape[1:]), dtype=torch.int32)


@compositing.register_fake
def _(layers, ops):
    return layers[0].new_empty(tuple(layers[0].shape))


@mat_mul.register_fake
def _(A, B):
    return A.new_empty(tuple(A.shape))


@resnet50.register_fake
def _(input, params):
    return input.new_empty((1000,))


@resnet50_batch.register_fake
def _(input, params):
    return input.new_empty((input.shape[0], 1000))


@fft2d.register_fake
def _(input, kind, gain):
    rows, n0 = input.shape[0], input.shape[1]
    n1 = 2 * (rows - 1) if kind == "c2r" else rows
    return input.new_empty({"r2c": (n1 // 2 + 1, n0, 2), "c2r": (n1, n0)}.get(kind, (n1, n0, 2)))


@saxpy.register_fake
def _(a, x, y):
    return y.new_empty(tuple(y.shape))


@sdot.register_fake
def _(x, y):
    return x.new_empty(())


@sasum.register_fake
def _(x):
    return x.new_empty(())


@sgemv.register_fake
def _(trans, a, A, x, b, y):
    return y.new_empty(tuple(y.shape))


@sger.register_fake
def _(a, x, y, A):
    return A.new_empty(tuple(A.shape))


@sgemm.register_fake
def _(transA, transB, a, A, B, b, C):
    return C.new_empty(tuple(C.shape))


@daxpy.register_fake
def _(a, x, y):
    return y.new_empty(tuple(y.shape))


@ddot.register_fake
def _(x, y):
    return x.new_empty(())


@dasum.register_fake
def _(x):
    return x.new_empty(())


@dgemv.register_fake
def _(trans, a, A, x, b, y):
    return y.new_empty(tuple(y.shape))


@dger.register_fake
def _(a, x, y, A):
    return A.new_empty(tuple(A.shape))


@dgemm.register_fake
def _(transA, transB, a, A, B, b, C):
    return C.new_empty(tuple(C.shape))


@conv3x3a16.register_fake
@conv3x3a32.register_fake
def _(input, mask):
    return input.new_empty(tuple(input.shape))


@dilate3x3.register_fake
@median3x3.register_fake
@gaussian5x5.register_fake
@sobel.register_fake
def _(input):
    return input.new_empty(tuple(input.shape))


@lens_blur.register_fake
def _(left_im, right_im, slices, focus_depth, blur_radius_scale, aperture_samples):
    return left_im.new_empty(tuple(left_im.shape), dtype=torch.float32)


@bgu.register_fake
def _(r_sigma, s_sigma, splat_loc, values, slice_loc):
    return torch.empty_like(slice_loc)


# apps/hannk's quantised convolutions on NHWC uint8 tensors: the memory order of the ops' [c, x, y, b] buffers.  Padding happens on the
# device with torch (the interpreter's pad op), the filter is tiled by the library's own kernel, and the op runs on torch's stream.
def _hannk_check(name, *tensors):
    for t in tensors:
        if t.dtype != torch.uint8:
            raise TypeError(f"{name}: activations and filters are uint8 tensors, not {t.dtype}")


def _hannk_pad(input, zero, channel_multiple, padding):
    c = input.shape[3]
    cp = -(-c // channel_multiple) * channel_multiple
    if cp == c and padding[0] == 0 and padding[1] == 0:
        return input.contiguous()
    return torch.nn.functional.pad(input, (0, cp - c, padding[0], padding[0], padding[1], padding[1]), value=zero).contiguous()


def _hannk_rule(name, rule, *args, **kwargs):
    """a shape rule of halide_amd/hannk.py for the op `name` and its register_fake twin: its refusal as the RuntimeError torch ops raise"""
    try:
        return rule(*args, **kwargs)
    except ValueError as e:
        raise RuntimeError(f"{name}: {e}") from None


@torch.library.custom_op("hlmi::hannk_conv2d", mutates_args=())
def hannk_conv2d(input: torch.Tensor, filter: torch.Tensor, bias: torch.Tensor, input_zero: int, filter_zero: int, stride: list[int],
                 dilation: list[int], padding: list[int], multiplier: int, shift: int, output_zero: int, output_min: int, output_max: int,
                 out_int16: bool) -> torch.Tensor:
    """apps/hannk conv: input (B, H, W, CI) uint8, filter (CO, FH, FW, CI) uint8, bias (CO,) int32 -> (B, OH, OW, CO) uint8, or int16 with
    out_int16; stride, dilation and padding are (x, y) pairs, the padding is input_zero."""
    _hannk_check("hannk_conv2d", input, filter)
    _, multiple, shape = _hannk_rule("hannk_conv2d", hl.hannk_conv_shape, input.shape, filter.shape, stride, dilation, padding)
    co, fh, fw, ci = filter.shape
    padded = _hannk_pad(input, input_zero, multiple, padding)
    tiled = torch.empty((fh, fw, -(-co // 16), -(-ci // 4), 16, 4), dtype=torch.uint8, device=input.device)
    out = torch.empty(shape, dtype=torch.int16 if out_int16 else torch.uint8, device=input.device)
    with _Wrapped(padded, filter.contiguous(), tiled, bias.contiguous(), out) as (a, f, t, b, o):
        hl.tile_conv_filter_uint8(f, filter_zero, filter_zero, t)
        (hl.conv_u8_u8_i16 if out_int16 else hl.conv_u8_u8_u8)(a, input_zero, t, filter_zero, b, stride, dilation, multiplier, shift, output_zero,
                                                             output_min, output_max, o)
    return out


@torch.library.custom_op("hlmi::hannk_depthwise_conv2d", mutates_args=())
def hannk_depthwise_conv2d(input: torch.Tensor, filter: torch.Tensor, bias: torch.Tensor, input_zero: int, filter_zero: int, stride: list[int],
                           dilation: list[int], padding: list[int], multiplier: int, shift: int, output_zero: int, output_min: int,
                           output_max: int) -> torch.Tensor:
    """apps/hannk depthwise conv: input (B, H, W, C) uint8, filter (FH, FW, C) uint8, bias (C,) int32 -> (B, OH, OW, C) uint8; an input of
    one channel under a filter of several is broadcast."""
    _hannk_check("hannk_depthwise_conv2d", input, filter)
    broadcast, multiple, shape = _hannk_rule("hannk_depthwise_conv2d", hl.hannk_conv_shape, input.shape, filter.shape, stride, dilation, padding,
                                             depthwise=True)
    padded = _hannk_pad(input, input_zero, multiple, padding)
    out = torch.empty(shape, dtype=torch.uint8, device=input.device)
    with _Wrapped(padded, filter.contiguous(), bias.contiguous(), out) as (a, f, b, o):
        (hl.depthwise_conv_broadcast_uint8 if broadcast else hl.depthwise_conv_uint8)(a, input_zero, f, filter_zero, b, stride, dilation, multiplier,
                                                                                     shift, output_zero, output_min, output_max, o)
    return out


@hannk_conv2d.register_fake
def _(input, filter, bias, input_zero, filter_zero, stride, dilation, padding, multiplier, shift, output_zero, output_min, output_max, out_int16):
    shape = _hannk_rule("hannk_conv2d", hl.hannk_conv_shape, input.shape, filter.shape, stride, dilation, padding)[2]
    return input.new_empty(shape, dtype=torch.int16 if out_int16 else torch.uint8)


@hannk_depthwise_conv2d.register_fake
def _(input, filter, bias, input_zero, filter_zero, stride, dilation, padding, multiplier, shift, output_zero, output_min, output_max):
    return input.new_empty(_hannk_rule("hannk_depthwise_conv2d", hl.hannk_conv_shape, input.shape, filter.shape, stride, dilation, padding, depthwise=True)[2])


# apps/hannk's pooling, mean, add, mul, softmax and L2 normalisation on uint8 tensors (NHWC where the op is spatial), parameters derived
# from float scales as the interpreter's ops.cpp derives them (halide_amd/hannk.py has the derivations and every op's shape rule).
@torch.library.custom_op("hlmi::hannk_pool2d", mutates_args=())
def hannk_pool2d(input: torch.Tensor, kind: str, filter: list[int], stride: list[int], padding: str, output_min: int, output_max: int) -> torch.Tensor:
    """Pool2DOp: input (B, H, W, C) uint8 -> (B, OH, OW, C) uint8; kind "average" or "max", filter and stride (x, y) pairs, padding "same" or
    "valid" (nothing is padded: the input is translated and the taps outside it do not count)."""
    _hannk_check("hannk_pool2d", input)
    if kind not in ("average", "max"):
        raise RuntimeError("hannk_pool2d: kind is 'average' or 'max'")
    _, oh, ow, _ = shape = _hannk_rule("hannk_pool2d", hl.hannk_pool_shape, input.shape, filter, stride, padding)
    out = torch.empty(shape, dtype=torch.uint8, device=input.device)
    with _Wrapped(input.contiguous(), out) as (a, o):
        a.set_min(0, hl.hannk_compute_padding(stride[0], input.shape[2], filter[0], ow), hl.hannk_compute_padding(stride[1], input.shape[1], filter[1], oh), 0)
        (hl.average_pool_uint8 if kind == "average" else hl.max_pool_uint8)(a, stride, filter, output_min, output_max, o)
    return out


@torch.library.custom_op("hlmi::hannk_mean", mutates_args=())
def hannk_mean(input: torch.Tensor, axes: list[int]) -> torch.Tensor:
    """ReductionOp (Mean): input uint8 of rank <= 4, the reduced axes kept with extent 1"""
    _hannk_check("hannk_mean", input)
    in4, box, out4, kept, _ = _hannk_rule("hannk_mean", hl.hannk_mean_shapes, input.shape, axes)
    out = torch.empty(out4, dtype=torch.uint8, device=input.device)
    with _Wrapped(input.contiguous().reshape(in4), out) as (a, o):
        hl.mean_uint8(a, *box, o)
    return out.reshape(kept)


def _hannk_rank2_pair(name, in1, in2):
    _hannk_check(name, in1, in2)
    shape = torch.broadcast_shapes(in1.shape, in2.shape)
    n = shape[-1] if len(shape) else 1
    return shape, in1.broadcast_to(shape).contiguous().reshape(-1, n), in2.broadcast_to(shape).contiguous().reshape(-1, n)


@torch.library.custom_op("hlmi::hannk_add", mutates_args=())
def hannk_add(in1: torch.Tensor, scale1: float, zero1: int, in2: torch.Tensor, scale2: float, zero2: int, out_scale: float, out_zero: int,
              activation: str) -> torch.Tensor:
    """add_uint8: activation "none", "relu", "relu6" or "relu_n1_to_1" """
    shape, a2, b2 = _hannk_rank2_pair("hannk_add", in1, in2)
    m1, m2 = hl.hannk_add_multipliers(scale1, scale2, out_scale)
    lo, hi = hl.hannk_output_range(activation, out_zero, out_scale)
    out = torch.empty_like(a2)
    with _Wrapped(a2, b2, out) as (a, b, o):
        hl.add_uint8_uint8(a, zero1, m1, b, zero2, m2, out_zero, lo, hi, o)
    return out.reshape(shape)


@torch.library.custom_op("hlmi::hannk_mul", mutates_args=())
def hannk_mul(in1: torch.Tensor, scale1: float, zero1: int, in2: torch.Tensor, scale2: float, zero2: int, out_scale: float, out_zero: int,
              activation: str) -> torch.Tensor:
    shape, a2, b2 = _hannk_rank2_pair("hannk_mul", in1, in2)
    m, shift = hl.hannk_mul_params(scale1, scale2, out_scale)
    lo, hi = hl.hannk_output_range(activation, out_zero, out_scale)
    out = torch.empty_like(a2)
    with _Wrapped(a2, b2, out) as (a, b, o):
        hl.mul_uint8_uint8_uint8(a, zero1, b, zero2, out_zero, m, shift, lo, hi, o)
    return out.reshape(shape)


def _hannk_rows_op(name, input, axis, call):
    _hannk_check(name, input)
    moved = input.movedim(axis, -1).contiguous()
    rows = moved.reshape(-1, moved.shape[-1])
    out = torch.empty_like(rows)
    with _Wrapped(rows, out) as (a, o):
        call(a, o)
    return out.reshape(moved.shape).movedim(-1, axis).contiguous()


@torch.library.custom_op("hlmi::hannk_softmax", mutates_args=())
def hannk_softmax(input: torch.Tensor, in_scale: float, beta: float, out_scale: float, out_zero: int, axis: int) -> torch.Tensor:
    bm, bs, om, osh = hl.hannk_softmax_params(in_scale, beta, out_scale)
    return _hannk_rows_op("hannk_softmax", input, axis, lambda a, o: hl.softmax_uint8(a, bm, bs, out_zero, om, osh, o))


@torch.library.custom_op("hlmi::hannk_l2_normalization", mutates_args=())
def hannk_l2_normalization(input: torch.Tensor, input_zero: int, axis: int) -> torch.Tensor:
    return _hannk_rows_op("hannk_l2_normalization", input, axis, lambda a, o: hl.l2_normalization_uint8(a, input_zero, o))


@hannk_pool2d.register_fake
def _(input, kind, filter, stride, padding, output_min, output_max):
    return input.new_empty(_hannk_rule("hannk_pool2d", hl.hannk_pool_shape, input.shape, filter, stride, padding))


@hannk_mean.register_fake
def _(input, axes):
    return input.new_empty(_hannk_rule("hannk_mean", hl.hannk_mean_shapes, input.shape, axes)[3])


@hannk_add.register_fake
@hannk_mul.register_fake
def _(in1, scale1, zero1, in2, scale2, zero2, out_scale, out_zero, activation):
    return in1.new_empty(torch.broadcast_shapes(in1.shape, in2.shape))


@hannk_softmax.register_fake
def _(input, in_scale, beta, out_scale, out_zero, axis):
    return torch.empty_like(input)


@hannk_l2_normalization.register_fake
def _(input, input_zero, axis):
    return torch.empty_like(input)


# apps/hannk's elementwise programs, pad and upsample_channels: uint8 (int16 for the LSTM program) tensors, the programs
# built on the host as the interpreter builds them (hl.hannk_*_program, hl.ElementwiseAssembler).
def _hannk_program_call(name, inputs, program):
    if not 1 <= len(inputs) <= 5:
        raise RuntimeError(f"{name}: one to five inputs")
    dtype = inputs[0].dtype
    if dtype not in (torch.uint8, torch.int16) or any(t.dtype != dtype for t in inputs):
        raise TypeError(f"{name}: the inputs are all uint8 or all int16")
    shape = torch.broadcast_shapes(*[t.shape for t in inputs])
    n = shape[-1] if len(shape) else 1
    rows = [t.broadcast_to(shape).contiguous().reshape(-1, n) for t in inputs]
    prog = hl.Buffer(np.ascontiguousarray(program.detach().cpu().numpy(), np.int16).reshape(-1, 5))
    outs = [torch.empty_like(rows[0], dtype=torch.uint8)] + ([torch.empty_like(rows[0])] if dtype == torch.int16 else [])
    with _Wrapped(*rows, *outs) as bufs:
        ins = bufs[:len(rows)] + [bufs[len(rows) - 1]] * (5 - len(rows))
        (hl.elementwise_5xint16_1xuint8int16 if dtype == torch.int16 else hl.elementwise_5xuint8_1xuint8)(*ins, prog, *bufs[len(rows):])
    return [o.reshape(shape) for o in outs]


@torch.library.custom_op("hlmi::hannk_elementwise", mutates_args=())
def hannk_elementwise(inputs: list[torch.Tensor], program: torch.Tensor) -> list[torch.Tensor]:
    """ElementwiseProgramOp: one to five uint8 tensors -> [uint8]; one to five int16 tensors -> [uint8, int16]; program an (n, 5) int16
    tensor (hl.ElementwiseAssembler), read on the host."""
    return _hannk_program_call("hannk_elementwise", inputs, program)


@torch.library.custom_op("hlmi::hannk_logistic", mutates_args=())
def hannk_logistic(input: torch.Tensor, in_scale: float, in_zero: int) -> torch.Tensor:
    """UnaryOp Logistic: uint8 -> uint8 with scale 1 / 256 and zero point 0"""
    _hannk_check("hannk_logistic", input)
    return _hannk_program_call("hannk_logistic", [input], torch.from_numpy(hl.hannk_logistic_program(in_scale, in_zero)))[0]


@torch.library.custom_op("hlmi::hannk_tanh", mutates_args=())
def hannk_tanh(input: torch.Tensor, in_scale: float, in_zero: int) -> torch.Tensor:
    """UnaryOp Tanh: uint8 -> uint8 with scale 1 / 128 and zero point 128"""
    _hannk_check("hannk_tanh", input)
    return _hannk_program_call("hannk_tanh", [input], torch.from_numpy(hl.hannk_tanh_program(in_scale, in_zero)))[0]


def _hannk_pad_boxes(input, padding):
    if len(padding) != 8:
        raise RuntimeError("hannk_pad: eight paddings: (before, after) of B, H, W, C")
    return _hannk_rule("hannk_pad", hl.hannk_pad_boxes, input.shape, list(zip(padding[::2], padding[1::2])))


@torch.library.custom_op("hlmi::hannk_pad", mutates_args=())
def hannk_pad(input: torch.Tensor, padding: list[int], pad_value: int) -> torch.Tensor:
    """PadOp: (B, H, W, C) uint8, `padding` = (before, after) of B, H, W, C: one fill_uint8 or copy_uint8_uint8 per box of hl.hannk_pad_boxes
    (the borders filled, the rest one copy, which pads the channel itself where 3 channels become 4)"""
    _hannk_check("hannk_pad", input)
    shape, imin, boxes = _hannk_pad_boxes(input, padding)
    out = torch.empty(shape, dtype=torch.uint8, device=input.device)
    src = input.contiguous()
    for kind, omin, omax in boxes:
        with _Wrapped(src, out[hl.hannk_box_slices(omin, omax)]) as (a, o):
            a.set_min(*imin)
            o.set_min(*omin)
            if kind == "fill":
                hl.fill_uint8(pad_value, o)
            else:
                hl.copy_uint8_uint8(a, pad_value, o)
    return out


@torch.library.custom_op("hlmi::hannk_upsample_channels", mutates_args=())
def hannk_upsample_channels(input: torch.Tensor, factor: int) -> torch.Tensor:
    """(B, H, W, C) uint8 -> (B, H, W, C * factor): channel c of the result is channel c // factor of the input"""
    _hannk_check("hannk_upsample_channels", input)
    if input.dim() != 4 or factor < 1:
        raise RuntimeError("hannk_upsample_channels: a (B, H, W, C) tensor and a factor >= 1")
    out = torch.empty(tuple(input.shape[:3]) + (input.shape[3] * factor,), dtype=torch.uint8, device=input.device)
    with _Wrapped(input.contiguous(), out) as (a, o):
        hl.upsample_channels_uint8(a, factor, o)
    return out


@hannk_elementwise.register_fake
def _(inputs, program):
    shape = torch.broadcast_shapes(*[t.shape for t in inputs])
    outs = [inputs[0].new_empty(shape, dtype=torch.uint8)]
    return outs + ([inputs[0].new_empty(shape, dtype=torch.int16)] if inputs[0].dtype == torch.int16 else [])


@hannk_logistic.register_fake
@hannk_tanh.register_fake
def _(input, in_scale, in_zero):
    return torch.empty_like(input)


@hannk_pad.register_fake
def _(input, padding, pad_value):
    return input.new_empty(_hannk_pad_boxes(input, padding)[0])


@hannk_upsample_channels.register_fake
def _(input, factor):
    return input.new_empty(tuple(input.shape[:3]) + (input.shape[3] * factor,))


# apps/hannk's data movement: one hlmi_hannk_copy_from over two views of the tensors' memory, or one hlmi_hannk_gather.  Any
# dtype of 1, 2, 4 or 8 bytes this module wraps; nothing is synchronised except by gather, whose indices are device data (its flag is read back).
class _Views:
    """_Wrapped for views: any strides, the innermost included"""

    def __init__(self, *tensors):
        self.tensors, self.bufs = tensors, []

    def __enter__(self):
        for t in self.tensors:      # every tensor is checked before any is wrapped: a refusal leaves nothing to detach
            if not t.is_cuda:
                raise RuntimeError("hlmi ops need tensors on the GPU (there is no CPU implementation)")
            if t.dtype not in _NP:
                raise TypeError(f"unsupported dtype {t.dtype}")
        for t in self.tensors:
            self.bufs.append(hl.Buffer.wrap_device(t.data_ptr(), _NP[t.dtype], list(reversed(t.shape)), list(reversed(t.stride()))))
        s = torch.cuda.current_stream(self.tensors[0].device).cuda_stream
        hl.set_stream(s if s else 1)
        hl.set_gpu_device(self.tensors[0].device.index or 0)
        return self.bufs

    def __exit__(self, *exc):
        hl.set_stream(None)
        for b in self.bufs:
            b.device_detach()
        return False


def _hannk_copy(src_view, dst_view):
    with _Views(src_view, dst_view) as (s, d):
        hl.hannk_copy_from(s, d)


@torch.library.custom_op("hlmi::hannk_transpose", mutates_args=())
def hannk_transpose(input: torch.Tensor, perm: list[int]) -> torch.Tensor:
    """TransposeOp: input.permute(perm) as a dense tensor, one copy_from into the output viewed in the input's order"""
    inverse = _hannk_rule("hannk_transpose", hl.hannk_inverse_perm, perm, input.dim())
    out = torch.empty([input.shape[p] for p in perm], dtype=input.dtype, device=input.device)
    _hannk_copy(input, out.permute(inverse))
    return out


def _hannk_block_views(space, depth, block):
    space6, depth6, perm = hl.hannk_block_views(space.shape, block)
    return space.view(space6), depth.view(depth6).permute(perm)


@torch.library.custom_op("hlmi::hannk_space_to_depth", mutates_args=())
def hannk_space_to_depth(input: torch.Tensor, block_size: int) -> torch.Tensor:
    """(B, H, W, C) -> (B, H / block, W / block, block^2 * C)"""
    out = torch.empty(_hannk_rule("hannk_space_to_depth", hl.hannk_block_shape, input.shape, block_size, True), dtype=input.dtype, device=input.device)
    _hannk_copy(*_hannk_block_views(input.contiguous(), out, block_size))
    return out


@torch.library.custom_op("hlmi::hannk_depth_to_space", mutates_args=())
def hannk_depth_to_space(input: torch.Tensor, block_size: int) -> torch.Tensor:
    """(B, H, W, block^2 * C) -> (B, H * block, W * block, C)"""
    out = torch.empty(_hannk_rule("hannk_depth_to_space", hl.hannk_block_shape, input.shape, block_size, False), dtype=input.dtype, device=input.device)
    s6, d6 = _hannk_block_views(out, input.contiguous(), block_size)
    _hannk_copy(d6, s6)
    return out


@torch.library.custom_op("hlmi::hannk_gather", mutates_args=())
def hannk_gather(input: torch.Tensor, indices: torch.Tensor, axis: int) -> torch.Tensor:
    """GatherOp: torch.index_select generalised to int32 indices of rank 0 .. 2; an index outside the axis raises (HalideError -8) after the
    other slices were written.  The one op here that waits for the device: the kernel's out-of-range flag is read back."""
    if indices.dtype != torch.int32:
        raise TypeError("hannk_gather: indices are int32")
    axis, shape = _hannk_rule("hannk_gather", hl.hannk_gather_shape, input.shape, indices.shape, axis)
    out = torch.zeros(shape, dtype=input.dtype, device=input.device)
    with _Views(input, indices, out) as (a, i, o):
        hl.hannk_gather_buffers(a, i, input.dim() - 1 - axis, o)
    return out


def _hannk_concat_shape(inputs, axis):
    if any(t.dtype != inputs[0].dtype for t in inputs):
        raise RuntimeError("hannk_concatenation: the inputs share dtype and every extent but the axis'")
    return _hannk_rule("hannk_concatenation", hl.hannk_concat_shape, [t.shape for t in inputs], axis)


@torch.library.custom_op("hlmi::hannk_concatenation", mutates_args=())
def hannk_concatenation(inputs: list[torch.Tensor], axis: int) -> torch.Tensor:
    """ConcatenationOp's copying half: every input into its crop of the output, one copy_from each (pieces of different quantisation go
    through hannk_add first, as hl.hannk_concatenation does)"""
    axis, shape = _hannk_concat_shape(inputs, axis)
    out = torch.empty(shape, dtype=inputs[0].dtype, device=inputs[0].device)
    at = 0
    for t in inputs:
        if t.shape[axis]:
            _hannk_copy(t, out.narrow(axis, at, t.shape[axis]))
        at += t.shape[axis]
    return out


@torch.library.custom_op("hlmi::hannk_fully_connected", mutates_args=())
def hannk_fully_connected(input: torch.Tensor, weights: torch.Tensor, bias: torch.Tensor, input_zero: int, filter_zero: int, multiplier: int,
                          shift: int, output_zero: int, output_min: int, output_max: int) -> torch.Tensor:
    """lower_tflite_fullyconnected: input of any rank flattened to (N, CI), weights (CO, CI) uint8, bias (CO,) int32 -> (N, CO) uint8: the conv
    op on a 1 x 1 image"""
    _hannk_check("hannk_fully_connected", input, weights)
    if weights.dim() != 2 or input.numel() % weights.shape[1]:
        raise RuntimeError("hannk_fully_connected: weights are (CO, CI) and CI divides the input")
    co, ci = weights.shape
    out = hannk_conv2d(input.reshape(-1, 1, 1, ci), weights.reshape(co, 1, 1, ci), bias, input_zero, filter_zero, [1, 1], [1, 1], [0, 0], multiplier,
                       shift, output_zero, output_min, output_max, False)
    return out.reshape(-1, co)


@hannk_transpose.register_fake
def _(input, perm):
    _hannk_rule("hannk_transpose", hl.hannk_inverse_perm, perm, input.dim())
    return input.new_empty([input.shape[p] for p in perm])


@hannk_space_to_depth.register_fake
def _(input, block_size):
    return input.new_empty(_hannk_rule("hannk_space_to_depth", hl.hannk_block_shape, input.shape, block_size, True))


@hannk_depth_to_space.register_fake
def _(input, block_size):
    return input.new_empty(_hannk_rule("hannk_depth_to_space", hl.hannk_block_shape, input.shape, block_size, False))


@hannk_gather.register_fake
def _(input, indices, axis):
    return input.new_empty(_hannk_rule("hannk_gather", hl.hannk_gather_shape, input.shape, indices.shape, axis)[1])


@hannk_concatenation.register_fake
def _(inputs, axis):
    return inputs[0].new_empty(_hannk_concat_shape(inputs, axis)[1])


@hannk_fully_connected.register_fake
def _(input, weights, bias, input_zero, filter_zero, multiplier, shift, output_zero, output_min, output_max):
    return input.new_empty((input.numel() // weights.shape[1], weights.shape[0]))
