/* hlmi_pipelines.h — the AOT entry points libhlmi.so exports.
 *
 * Each pipeline keeps the exact C signature the reference's code generator emits for it
 * (src/CodeGen_C.cpp:1085-1112: buffers as `struct halide_buffer_t *`, scalars by value, inputs in
 * declaration order then outputs — src/AbstractGenerator.cpp:41-52), plus the argv-call variant
 * (src/CodeGen_C.cpp:675-705) and the metadata getter (src/CodeGen_C.cpp:707-720), so that the
 * object is a drop-in for `<name>.a` + `<name>.h` of the reference.  Return value: 0 or a negative
 * halide_error_code_t; on error `halide_error()` is called first (default handler aborts).
 *
 * Entry protocol, identical for all pipelines, in the order the reference emits its checks
 * (src/UnpackBuffers.cpp:148; src/AddParameterChecks.cpp; src/AddImageChecks.cpp:315-347, 393-470, 591-671,
 * 716-760; buffers are visited in NAME order within each step; pinned by tests/test_entry_protocol.py):
 *   1. a NULL buffer argument                       -> -12 (buffer_argument_is_null)
 *   2. a scalar parameter outside its range         -> -9 / -10 (param_too_small / param_too_large)
 *   3. any buffer with host==NULL && device==0      -> BOUNDS QUERY: dim[] (and type) of every such buffer is
 *      rewritten to the region the pipeline needs / produces, nothing is computed, return 0
 *   4. per buffer: element type mismatch -> -3, then wrong dimensionality -> -43
 *   5. per buffer and dimension: dim[0].stride != 1 or another pinned stride / min / extent -> -8
 *   6. per buffer and dimension: region required > region supplied -> -4, then a negative extent -> -28
 *   7. per buffer and dimension: |extent * stride| > 2^31-1 -> -5, product of extents > 2^31-1 -> -6; then, where a pipeline sets a
 *      host alignment (the resampled gaussian_blur variants), a host pointer off that grid -> -24
 *   8. with the device: both dirty bits -> -37; device handle without interface -> -19 (and vice versa -36); a
 *      device allocation of another API -> -42; a host-dirty input without host pointer -> -34.  (-44,
 *      device_dirty_with_no_device_support, is what a HOST-only target reports; a GPU target copies instead.)
 * Device protocol (what the reference emits for a GPU target,
 * src/InjectHostDevBufferCopies.cpp:197-217, 285-304): inputs are brought to the device with
 * halide_copy_to_device (allocation is attached to the caller's buffer and stays there), the
 * output gets a device allocation, kernels are ENQUEUED on the HIP stream, the output is marked
 * device_dirty and the call returns; the caller uses halide_device_sync / halide_copy_to_host
 * (Halide::Runtime::Buffer::device_sync()/copy_to_host()) exactly as with the reference's GPU
 * targets.  There is no CPU fallback: without a usable gfx950 device the call fails with -29.
 */
#ifndef HLMI_PIPELINES_H
#define HLMI_PIPELINES_H

#include "hlmi_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HLMI_DECLARE_AUX(name)                                   \
    int name##_argv(void **args);                                \
    const struct halide_filter_metadata_t *name##_metadata(void);

/* apps/local_laplacian/local_laplacian_generator.cpp:12-16,287 — u16 [W,H,3] planar in/out,
 * pyramid_levels J=8 (compile-time GeneratorParam :10), `levels` K >= 2 at run time (no upper bound, as in the reference).
 * Drivers pass alpha/(levels-1) (apps/local_laplacian/process.cpp:31). */
int local_laplacian(struct halide_buffer_t *input, int32_t levels, float alpha, float beta,
                    struct halide_buffer_t *output);
HLMI_DECLARE_AUX(local_laplacian)

/* apps/bilateral_grid/bilateral_grid_generator.cpp:10-12,203 — f32 [W,H]; s_sigma=8 compile-time (:8). */
int bilateral_grid(struct halide_buffer_t *input, float r_sigma, struct halide_buffer_t *bilateral_grid);
HLMI_DECLARE_AUX(bilateral_grid)

/* apps/blur/halide_blur_generator.cpp:31-32,117 — u16 [W+2,H+2] -> u16 [W,H]; no boundary condition. */
int halide_blur(struct halide_buffer_t *input, struct halide_buffer_t *blur_y);
HLMI_DECLARE_AUX(halide_blur)

/* apps/nl_means/nl_means_generator.cpp:9-14,162 — f32 [W,H,3] in/out. */
int nl_means(struct halide_buffer_t *input, int32_t patch_size, int32_t search_area, float sigma,
             struct halide_buffer_t *non_local_means);
HLMI_DECLARE_AUX(nl_means)

/* apps/stencil_chain/stencil_chain_generator.cpp:9-10,150 — u16 [W,H], stencils=32 compile-time (:7). */
int stencil_chain(struct halide_buffer_t *input, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(stencil_chain)

/* apps/conv_layer/conv_layer_generator.cpp:9-12,207 — f32 input [CI,W+2,H+2,N], filter [CO,3,3,CI],
 * bias [CO], relu [CO,W,H,N] (c fastest).  The reference pins N=5, CI=CO=128, W=100, H=80 (:15,35-50);
 * this entry point accepts any N, W, H with CI a multiple of 32 and CO a multiple of 128 (superset), dense
 * strides and zero mins as the generator pins them.  Exact f32: a k-ordered fma chain on the f32 matrix cores. */
int conv_layer(struct halide_buffer_t *input, struct halide_buffer_t *filter, struct halide_buffer_t *bias,
               struct halide_buffer_t *relu);
HLMI_DECLARE_AUX(conv_layer)

/* Same algorithm, buffers and layouts as conv_layer (apps/conv_layer/conv_layer_generator.cpp:9-12, :21-27, :35-50),
 * evaluated on the bf16 matrix cores (BASELINE.json configs[4]): input and filter are rounded to bfloat16
 * (nearest even), products accumulate in f32 from the f32 bias.  CI must be a multiple of 64, CO of 128.
 * Not bit-exact against the f32 reference by construction: tolerance parity (tests/test_conv_layer.py). */
int conv_layer_bf16(struct halide_buffer_t *input, struct halide_buffer_t *filter, struct halide_buffer_t *bias,
                    struct halide_buffer_t *relu);
HLMI_DECLARE_AUX(conv_layer_bf16)

/* apps/depthwise_separable_conv/depthwise_separable_conv_generator.cpp:11-23 — f32 input [CI,W,H,N], depthwise_filter
 * [CM,IC,FW,FH] (stride(1) == CM, :283), pointwise_filter [CO,IC], bias [CO], output [CO,W,H,N]; zero padding,
 * depthwise FWxFH convolution, pointwise 1x1 convolution, bias, ReLU.  Bit-exact fma chains in RDom order. */
int depthwise_separable_conv(struct halide_buffer_t *input, struct halide_buffer_t *depthwise_filter,
                             struct halide_buffer_t *pointwise_filter, struct halide_buffer_t *bias,
                             struct halide_buffer_t *output);
HLMI_DECLARE_AUX(depthwise_separable_conv)

/* apps/unsharp/unsharp_generator.cpp:9-10,113 — f32 [W,H,3] planar in and out, sigma = 1.5 (GeneratorParam :7): gray,
 * separable 7-tap Gaussian, sharpen, ratio, recolour.  An adjacent app with the same boundary. */
int unsharp(struct halide_buffer_t *input, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(unsharp)

/* apps/max_filter/max_filter_generator.cpp:11-12,121 — f32 [W,H,3] planar in and out, radius = 26 (GeneratorParam :10):
 * max over a disc-like footprint of the edge-clamped input.  An adjacent app with the same boundary. */
int max_filter(struct halide_buffer_t *input, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(max_filter)

/* apps/hist/hist_generator.cpp:9-10,215 — u8 [W,H,3] planar in and out: histogram equalisation of the luma (integer
 * histogram over the whole input, cdf, pointwise recolouring).  An adjacent app with the same boundary. */
int hist(struct halide_buffer_t *input, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(hist)

/* apps/harris/harris_generator.cpp:13-15,130 — f32 [W,H,3] planar in, f32 [.,.] out: Harris corner response; no
 * boundary condition (the input must cover the output grown by 2).  Adjacent app, same boundary. */
int harris(struct halide_buffer_t *input, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(harris)

/* apps/interpolate/interpolate_generator.cpp:17-18,215 — f32 [W,H,4] planar in (r, g, b, alpha), f32 [W,H,3] out over
 * the input's extent: alpha-weighted pull-push pyramid, 10 levels.  Adjacent app, same boundary. */
int interpolate(struct halide_buffer_t *input, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(interpolate)

/* apps/iir_blur/iir_blur_generator.cpp:136-144,181 — f32 [W,H,C] planar in and out, `alpha` = weight of the input:
 * first-order IIR low pass down and up the columns, then along the rows.  Adjacent app; the reference
 * pins 1536 x 2560 x 3 (:158-163), this entry point accepts any extents. */
int iir_blur(struct halide_buffer_t *input, float alpha, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(iir_blur)

/* apps/lens_blur/lens_blur_generator.cpp:12-21,301 — u8 [W,H,3] planar stereo pair in, f32 [W,H,3] out: depth from
 * stereo (cost volume of `slices` disparities, confidence-weighted 8-level push-pull), depth-dependent bokeh from
 * `aperture_samples` pseudo-random samples per pixel.  Adjacent app, same boundary.  The sample
 * positions are Halide's random_float(): a fixed hash whose "definition tag" is a counter of the reference's COMPILER that
 * cannot be observed without it — see hlmi_lens_blur_set_random_tag below and oracle/lens_blur_oracle.c.
 * Limit of this implementation: the output plus its blur radius on either side must be narrower than 2^23 columns
 * (halide_error_code_buffer_extents_too_large otherwise). */
int lens_blur(struct halide_buffer_t *left_im, struct halide_buffer_t *right_im, int32_t slices, int32_t focus_depth,
              float blur_radius_scale, int32_t aperture_samples, struct halide_buffer_t *final);
HLMI_DECLARE_AUX(lens_blur)
/* The tag the random_float() calls of lens_blur's sample_locations were lowered with (src/Function.cpp:640-648: the number
 * of pure Func definitions the generator process made before it).  Default 71 = the count derived in
 * oracle/lens_blur_oracle.c; a maintainer who can run the reference's compiler sets the observed value. */
void hlmi_lens_blur_set_random_tag(int tag);
int hlmi_lens_blur_get_random_tag(void);

/* apps/bgu/bgu_generator.cpp:252-266,698 — bilateral-guided upsampling: fits a 3x4 affine colour transform per cell of
 * a bilateral grid (cells of s_sigma x s_sigma low-res pixels x r_sigma of luma) from the low-res pair splat_loc ->
 * values, and applies the trilinearly sliced transforms to the full-res slice_loc.  f32 [W,H,3] planar everywhere; the
 * low-res pair is edge-clamped (:270-271).  Adjacent app, same boundary.  fast_inverse (:170) is the
 * correctly rounded 1/x of the reference's CUDA path (src/runtime/ptx_dev.ll:61-66), not x86's rcpss estimate. */
int bgu(float r_sigma, int32_t s_sigma, struct halide_buffer_t *splat_loc, struct halide_buffer_t *values,
        struct halide_buffer_t *slice_loc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(bgu)

/* apps/resize/resize_generator.cpp:61-63,249 — resampling to another size: planar [x, y, c] input and output of the variant's
 * element type (f32 / u8 / u16), any channel count, any min on every dimension; the output's x, y are absolute coordinates, so
 * an output crop equals that region of the full result.  4 kernels (box 1, linear 2, cubic 4, lanczos 6 taps) x 3 types x
 * `_up` (resample x, then y; kernel unscaled) / `_down` (y, then x; kernel widened by 1 / scale_factor): the NAME decides, not
 * the value of the factor.  Interleaved layouts, which the reference also specialises, are not supported: dim[0].stride != 1
 * returns -8 as everywhere here.  Particular to this pipeline: with taps_f = ceil(T / scale_factor) (`_up`: T), a call with
 * !(taps_f >= 1 && taps_f <= input extent) in x or in y returns -4 (the reference's clamped window would leave the input);
 * this catches a non-finite or non-positive factor on the `_down` variants.  On `_up` variants such a factor reads in bounds
 * and its result is unspecified.  The output's channel range must lie inside the input's (-4).  Bounds query: a query on the
 * output leaves its dim[] as passed and sets its type; a query on the input sets its channels from the output and leaves
 * x / y as passed (the required region is expressed through the input's own extents: the windows are clamped to them).
 * float results are clamped to [0, 1], integer results saturate and truncate toward zero.  sin() of the lanczos kernel is this
 * project's dev::halide_sin (the reference's CPU targets call libm).  No `_auto_schedule` twins: the reference's app has none. */
int resize_box_float32_up(struct halide_buffer_t *input, float scale_factor, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(resize_box_float32_up)
int resize_box_float32_down(struct halide_buffer_t *input, float scale_factor, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(resize_box_float32_down)
int resize_box_uint8_up(struct halide_buffer_t *input, float scale_factor, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(resize_box_uint8_up)
int resize_box_uint8_down(struct halide_buffer_t *input, float scale_factor, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(resize_box_uint8_down)
int resize_box_uint16_up(struct halide_buffer_t *input, float scale_factor, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(resize_box_uint16_up)
int resize_box_uint16_down(struct halide_buffer_t *input, float scale_factor, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(resize_box_uint16_down)
int resize_linear_float32_up(struct halide_buffer_t *input, float scale_factor, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(resize_linear_float32_up)
int resize_linear_float32_down(struct halide_buffer_t *input, float scale_factor, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(resize_linear_float32_down)
int resize_linear_uint8_up(struct halide_buffer_t *input, float scale_factor, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(resize_linear_uint8_up)
int resize_linear_uint8_down(struct halide_buffer_t *input, float scale_factor, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(resize_linear_uint8_down)
int resize_linear_uint16_up(struct halide_buffer_t *input, float scale_factor, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(resize_linear_uint16_up)
int resize_linear_uint16_down(struct halide_buffer_t *input, float scale_factor, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(resize_linear_uint16_down)
int resize_cubic_float32_up(struct halide_buffer_t *input, float scale_factor, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(resize_cubic_float32_up)
int resize_cubic_float32_down(struct halide_buffer_t *input, float scale_factor, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(resize_cubic_float32_down)
int resize_cubic_uint8_up(struct halide_buffer_t *input, float scale_factor, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(resize_cubic_uint8_up)
int resize_cubic_uint8_down(struct halide_buffer_t *input, float scale_factor, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(resize_cubic_uint8_down)
int resize_cubic_uint16_up(struct halide_buffer_t *input, float scale_factor, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(resize_cubic_uint16_up)
int resize_cubic_uint16_down(struct halide_buffer_t *input, float scale_factor, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(resize_cubic_uint16_down)
int resize_lanczos_float32_up(struct halide_buffer_t *input, float scale_factor, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(resize_lanczos_float32_up)
int resize_lanczos_float32_down(struct halide_buffer_t *input, float scale_factor, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(resize_lanczos_float32_down)
int resize_lanczos_uint8_up(struct halide_buffer_t *input, float scale_factor, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(resize_lanczos_uint8_up)
int resize_lanczos_uint8_down(struct halide_buffer_t *input, float scale_factor, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(resize_lanczos_uint8_down)
int resize_lanczos_uint16_up(struct halide_buffer_t *input, float scale_factor, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(resize_lanczos_uint16_up)
int resize_lanczos_uint16_down(struct halide_buffer_t *input, float scale_factor, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(resize_lanczos_uint16_down)

/* apps/gaussian_blur/gaussian_blur_generator.cpp:68-100, :104-349 — a Gaussian blur of a chosen sigma, truncated at `trunc` sigmas
 * (radius = (int)ceil(trunc * sigma)): f32 [x, y] in and out.  gaussian_blur_direct is the separable blur itself over the
 * edge-clamped input: any output region, any input min; a bounds query leaves both buffers as passed.  The 36 variants
 * gaussian_blur_<U>_<D>_<F> (upsample_order U in 2..4, downsample_order D in 1..3, factor F in 2, 4, 8, 16) reduce the input by F
 * with an order-D box-spline prefilter, blur at low resolution with a sigma corrected for the two splines, and expand by F with
 * an order-U box spline.  Particular to the variants (:344-347): output.min.0 == 0, output.min.1 == 0 and
 * output.stride.1 % 16 == 0 or -8; an output HOST pointer that is not 64-byte aligned -> -24 (unaligned_host_ptr; a null one
 * passes); a queried output gets mins 0; input mins are free.  Particular to all 37: !(sigma > 0 and finite) or trunc < 0
 * returns -9 naming the argument (the algorithm yields NaN or an empty sum there; the generator declares no range, so the
 * metadata has none).  A radius beyond the image is legal; one whose tables the scratch arena cannot hold returns -11. */
int gaussian_blur_direct(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_direct)
int gaussian_blur_2_1_2(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_2_1_2)
int gaussian_blur_2_1_4(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_2_1_4)
int gaussian_blur_2_1_8(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_2_1_8)
int gaussian_blur_2_1_16(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_2_1_16)
int gaussian_blur_2_2_2(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_2_2_2)
int gaussian_blur_2_2_4(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_2_2_4)
int gaussian_blur_2_2_8(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_2_2_8)
int gaussian_blur_2_2_16(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_2_2_16)
int gaussian_blur_2_3_2(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_2_3_2)
int gaussian_blur_2_3_4(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_2_3_4)
int gaussian_blur_2_3_8(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_2_3_8)
int gaussian_blur_2_3_16(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_2_3_16)
int gaussian_blur_3_1_2(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_3_1_2)
int gaussian_blur_3_1_4(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_3_1_4)
int gaussian_blur_3_1_8(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_3_1_8)
int gaussian_blur_3_1_16(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_3_1_16)
int gaussian_blur_3_2_2(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_3_2_2)
int gaussian_blur_3_2_4(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_3_2_4)
int gaussian_blur_3_2_8(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_3_2_8)
int gaussian_blur_3_2_16(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_3_2_16)
int gaussian_blur_3_3_2(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_3_3_2)
int gaussian_blur_3_3_4(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_3_3_4)
int gaussian_blur_3_3_8(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_3_3_8)
int gaussian_blur_3_3_16(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_3_3_16)
int gaussian_blur_4_1_2(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_4_1_2)
int gaussian_blur_4_1_4(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_4_1_4)
int gaussian_blur_4_1_8(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_4_1_8)
int gaussian_blur_4_1_16(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_4_1_16)
int gaussian_blur_4_2_2(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_4_2_2)
int gaussian_blur_4_2_4(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_4_2_4)
int gaussian_blur_4_2_8(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_4_2_8)
int gaussian_blur_4_2_16(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_4_2_16)
int gaussian_blur_4_3_2(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_4_3_2)
int gaussian_blur_4_3_4(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_4_3_4)
int gaussian_blur_4_3_8(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_4_3_8)
int gaussian_blur_4_3_16(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian_blur_4_3_16)

/* apps/linear_blur — the 3x3 box blur, plain and in linear light: f32 [x, y, c] in and out.
 * simple_blur (simple_blur_generator.cpp:5-22, built with input.type=float32 input.dim=3 output.dim=3): with in(x, y, c) =
 * input(max(min(x, width - 1), 0), max(min(y, height - 1), 0), c), blur_x = (in(x) + in(x + 1) + in(x + 2)) / 3 and output =
 * (blur_x(y) + blur_x(y + 1) + blur_x(y + 2)) / 3: the window is x .. x + 2, y .. y + 2, not centred; width and height are the
 * scalar arguments and need not be the buffer's extents (<= 0 reads column / row 0 everywhere).
 * linear_blur (linear_blur_generator.cpp:8-27): srgb_to_linear, that blur with width and height the input's EXTENTS (the clamp is
 * to [0, extent - 1] in absolute coordinates, whatever the input's mins), linear_to_srgb.
 * Any output region, channel range and mins, padded row and plane strides.  The input must cover columns cx(ox) .. cx(ox + ow + 1),
 * rows cy(oy) .. cy(oy + oh + 1) and the output's channels, or -4.  Bounds query: the output stays as passed; simple_blur's input
 * gets exactly that box, linear_blur's keeps x and y as passed and gets the output's channels.  Neither has an _auto_schedule
 * twin: the reference builds none. */
int linear_blur(struct halide_buffer_t *input, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(linear_blur)
int simple_blur(struct halide_buffer_t *input, int32_t width, int32_t height, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(simple_blur)

/* apps/wavelet — the one-level horizontal Haar and Daubechies-4 transforms and their inverses, all f32.  The forwards take in[x, y]
 * and give out[x, y, c]; the inverses take in[x, y, c] and give out[x, y]; x is scaled by two between the two sides.  `in` below is
 * repeat_edge of the input over the input buffer's own min and extent in EVERY dimension (for the inverses the channel too), and
 * D0 .. D3 are the four float literals of daubechies_constants.h:4-7, the D4 taps (1 +- sqrt 3) / (4 sqrt 2) and
 * (3 +- sqrt 3) / (4 sqrt 2), D3 < 0.
 * haar_x (haar_x_generator.cpp:15-21): c == 0: (in(2x, y) + in(2x + 1, y)) * 0.5f; any other c: (in(2x, y) - in(2x + 1, y)) * 0.5f
 * (mux: every index other than 0 selects the last value; / 2 is * 0.5f, src/Simplify_Div.cpp:204).
 * inverse_haar_x (inverse_haar_x_generator.cpp:15-20): x % 2 == 0: in(x/2, y, 0) + in(x/2, y, 1); otherwise in(x/2, y, 0) - in(x/2, y, 1).
 * daubechies_x (daubechies_x_generator.cpp:15-20), a .. d = in(2x - 1), in(2x), in(2x + 1), in(2x + 2): c == 0:
 * ((D0*a + D1*b) + D2*c) + D3*d; any other c: ((D3*a - D2*b) + D1*c) - D0*d.
 * inverse_daubechies_x (inverse_daubechies_x_generator.cpp:15-20), p, q, r, s = in(x/2, ., 0), in(x/2, ., 1), in(x/2 + 1, ., 0),
 * in(x/2 + 1, ., 1): even x: ((D2*p + D1*q) + D0*r) + D3*s; odd x: ((D3*p - D0*q) + D1*r) - D2*s.
 * x/2 and x%2 are Halide's (floor, Euclidean): output mins may be negative; 2x +- k and x/2 + 1 are formed in 64 bits before the clamp.
 * Float forms as in oracle/oracle_common.h: one rounding per operator in the order written, or, contracted, the sum of four
 * products mad(D3,d, mad(D2,c, mad2(D0,a, D1,b))) and the alternating one msub(mad(D1,c, mulsub(D3,a, D2*b)), D0, d) (the inverse
 * alike with its constants); Haar has no multiply that feeds an add.
 * Any output region, mins, channel range (extent 1, 3, min -1, ...) and padded strides; the reference's unroll(c, 2) / unroll(x, 2)
 * would refuse extents below 2, here the algorithm's value is computed for every extent.  Every read is clamped into the input's own
 * box, so the input only fails to cover where it has an empty dimension and the output is not empty (-4); nothing is read where
 * the output is empty.  Bounds query: both buffers stay as passed, return 0.  More workgroups than one launch holds: -6.  No
 * estimates and no _auto_schedule twins: the reference has none. */
int haar_x(struct halide_buffer_t *in, struct halide_buffer_t *out);
HLMI_DECLARE_AUX(haar_x)
int inverse_haar_x(struct halide_buffer_t *in, struct halide_buffer_t *out);
HLMI_DECLARE_AUX(inverse_haar_x)
int daubechies_x(struct halide_buffer_t *in, struct halide_buffer_t *out);
HLMI_DECLARE_AUX(daubechies_x)
int inverse_daubechies_x(struct halide_buffer_t *in, struct halide_buffer_t *out);
HLMI_DECLARE_AUX(inverse_daubechies_x)

/* apps/HelloWasm/generator/reaction_diffusion_generator.cpp — a three-channel reaction-diffusion simulation, one update per frame.
 * reaction_diffusion_init (:10-12): output f32 [x, y, c] = random_float(), any region.
 * reaction_diffusion_update (:34-105): state, new_state f32 [x, y, c], c pinned to [0, 3) on both (-8).  The pure stage: with in =
 * repeat_edge(state) over the state's own min and extent, blur = ((in(x-2) + in(x-1) + in(x) + in(x+1) + in(x+2)) + (the same in y))
 * * 0.1f per channel, each five-tap sum left to right; R, G, B = blur * (0.5f + (0.5f * blur) * (3 - 2 * blur)); dR = B * ((1 - R) - G),
 * dG = (1 - B) * (R - G), dB = (((1 - B) + (2 * G) * R) - R) - G; boost = 5 * max(0, 1.f - float(mx * mx + my * my) * 0.001f) + 1 with
 * mx = mouse_x - x, my = mouse_y - y in wrapping int32; R += (dR * 0.14f) * boost, G += (dG * 0.05f) * boost, B += (dB * 0.065f) * boost;
 * each clamped to [0, 1] as max(min(v, 1), 0).  Then, in this order: row state.min(1) and row state.max(1) = random_float(frame) * 0.2f
 * (hashed over c and x), column state.min(0) and column state.max(0) (hashed over c and y), each over the output's range in the other
 * dimension; then every pixel of the box x in [clamp(mouse_x - 10, 0, W - 1), clamp(mouse_x + 10, 0, W - 1)], y alike with H — W and
 * H the state's EXTENTS, the coordinates absolute whatever the mins — with float(dx * dx + dy * dy) < 100.0f becomes 0.25f * (n(x, y) +
 * n(x + 1, y) + n(x + 1, y + 1) + n(x, y + 1)), n = random_float(frame) hashed over c, y, x.  Float forms as in
 * oracle/oracle_common.h; the contracted one fuses (0.5f * blur) * (3 - 2 blur) + 0.5f, 3 - 2 * blur, (2 * G) * R + (1 - B),
 * 1 - d2 * 0.001f, 5 * max + 1 and the three rate products into their adds.  new_state must hold the two rows, the two columns and the
 * clobber box (-4); the pure stage is defined for any output region.  An empty state under an output that is not empty: -4.  Bounds
 * query: new_state grows to hold its own region and what the updates write, state keeps x and y as passed; both get channels [0, 3).
 * The frame counter is an int32 hashed as uint32.
 * reaction_diffusion_render (:150-174): state f32 [x, y, c] -> render u32 [x, y]; k = min(((s * (1.01f - s)) * 4)^4, 1) per channel,
 * R = min(k0, (k1 + k2) * 0.5f), G = clamp(((k1 + k0) + k2) * 0.5f, 0, 1), B = max(k0, max(k1, k2)), each cast<uint32_t>(ch * 255) &
 * 0xff, packed B | G << 8 | R << 16 | 255 << 24.  The state must cover render's x and y and channels [0, 3) (-4).  A NaN state has no
 * defined cast.  No estimates and no _auto_schedule twins: the reference has none.
 * The random hash (src/Random.cpp) is restated in halide_amd/csrc/hlmi_random.h; the call ids and definition tags it is fed are
 * derived by reading the reference and are NOT confirmed against a Halide build. */
int reaction_diffusion_init(struct halide_buffer_t *output);
HLMI_DECLARE_AUX(reaction_diffusion_init)
int reaction_diffusion_update(struct halide_buffer_t *state, int32_t mouse_x, int32_t mouse_y, int32_t frame, struct halide_buffer_t *new_state);
HLMI_DECLARE_AUX(reaction_diffusion_update)
int reaction_diffusion_render(struct halide_buffer_t *state, struct halide_buffer_t *render);
HLMI_DECLARE_AUX(reaction_diffusion_render)
/* Library extension (no argument table, _argv or _metadata): `steps` >= 1 updates with frames frame0 .. frame0 + steps - 1 (wrapping
 * int32) from state into new_state, then, render non-null, one render of the final state: bit for bit what that many calls of
 * reaction_diffusion_update and one of reaction_diffusion_render produce, in as few launches as the plan allows.  state and
 * new_state (and render) have the same box in x and y, state is not modified, state and new_state do not overlap; steps < 1, unequal
 * boxes or an overlap: -8.  Intermediate states live in new_state and in the stream's workspace.  The switch
 * HLMI_RD_STEPS_PER_LAUNCH (1, 2, 4) overrides the plan's steps per launch. */
int hlmi_reaction_diffusion_run(struct halide_buffer_t *state, int32_t mouse_x, int32_t mouse_y, int32_t frame0, int32_t steps,
                                struct halide_buffer_t *new_state, struct halide_buffer_t *render);

/* apps/compositing/compositing_generator.cpp:17-23,25-154 — Porter-Duff blending of six u8 RGBA layers [W,H,4] by five run-time
 * op codes (int32 [5]) into u8 [W,H,4]: a small interpreter.  THE CONTRACT IS THE GENERATOR'S INTEGER FORM (the branch a target
 * without a GPU feature takes, and what the reference's own test runs): the float form normalises by 255.0f / alpha, which at
 * alpha 0 is 0 * inf = NaN through a saturating_cast whose result for NaN is the target's business, and the driver reaches alpha 0
 * (`out` first, apps/compositing/process.cpp:35); it is not built.  No float operation: both library builds give the same bytes.
 * Per pixel, every type as written, additions wrapping in their type:
 *   state C[0..2] uint16, A uint8;  layer 0: C[i] = u16(v_i) * u16(a), A = a;  layers k = 1 .. 5 premultiplied alike into Bc[i], B3,
 *   then operator ops(k - 1), all four results formed from the OLD state (a tuple assignment).  ~e = 255 - e.
 *   scale16(a: u16, s: u8): c = u32(a) * u32(s); c += (c + 128) >> 8; c = (c + 128) >> 8; u16(c).   scale8(a: u8, s: u8): the same
 *   two steps on c = u16(a) * u16(s), u8(c).  The generator's comment "equivalent to c = (c + 127) / 255" (:64) holds for scale8
 *   only: for scale16 the two-shift form first departs at c = 65663 and is one lower on 4 096 162 of the 16 646 656 pairs
 *   a <= 65025, s <= 255.  The contract is the two-shift form.
 *     code  name   C[i]                                         A
 *     0     over   Bc[i] + scale16(C[i], ~B3)                   B3 + scale8(A, ~B3)
 *     1     atop   scale16(Bc[i], A) + scale16(C[i], ~B3)       A
 *     2     xor    scale16(Bc[i], ~A) + scale16(C[i], ~B3)      scale8(B3, ~A) + scale8(A, ~B3)
 *     3     in     scale16(C[i], B3)                            scale8(A, B3)
 *     4     out    scale16(C[i], ~B3)                           scale8(A, ~B3)
 *   Any other op code (negative, 5 or more) leaves the state unchanged: the RDom's where() matches no operator (:146-147).
 *   out[i] = sat_u8(A == 0 ? 0 : u16(C[i] + A / 2) / A), i < 3 (fast_integer_divide: the exact floor quotient, the numerator for a
 *   denominator of 1, 0 for a zero denominator, src/FastIntegerDivide.cpp:302-307); out[3] = A.  The saturation is real: after
 *   `over` a colour can exceed 255 * A by up to 127.
 * Entry contract: null (-12), type (-3), dimensionality (-43); the output's channels are min 0, extent 4 (-8: bound(c, 0, 4), all
 * four are produced together); then a bounds query answers every layer with the output's x, y box and channels [0, 4) and ops with
 * [0, 5), and leaves the output as passed; then sizes and coverage: nothing is clamped, each layer covers the output's x, y region
 * and channels [0, 4), ops covers [0, 5) (-4).  Every buffer has its own mins and strides; one buffer may be several layers.  ops
 * is read on the device.  Nothing is read or launched where the output's x or y extent is 0.  No _auto_schedule twin. */
int compositing(struct halide_buffer_t *layer_rgba_0, struct halide_buffer_t *layer_rgba_1, struct halide_buffer_t *layer_rgba_2,
                struct halide_buffer_t *layer_rgba_3, struct halide_buffer_t *layer_rgba_4, struct halide_buffer_t *layer_rgba_5,
                struct halide_buffer_t *ops, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(compositing)

/* apps/hexagon_benchmarks — six single-plane u8 stencils (conv3x3_generator.cpp with accumulator_type=int16 / int32,
 * dilate3x3_generator.cpp, median3x3_generator.cpp, gaussian5x5_generator.cpp, sobel_generator.cpp), signatures as the reference's
 * Makefile generates them.  input and output: uint8, 2-D; mask: int8, 2-D.  INTEGER ARITHMETIC ONLY: both library builds give the
 * same bytes.  in(x, y) is the input read at x clamped to [min0, min0 + extent0 - 1] and y clamped likewise: repeat_edge of the
 * INPUT's own box, not of the output's.
 *   dilate3x3    the maximum of the nine in(x + j, y + i), i, j in -1 .. 1.
 *   median3x3    the generator's network: max, min and mid of each column of three, mid(a, b, c) = max(min(max(a, b), c), min(a, b));
 *                the output is the mid of min(the three max_y), max(the three min_y) and mid(the three mid_y): the median of the nine.
 *   sobel        in uint16: ax(x, y) = in(x-1, y) + 2 in(x, y) + in(x+1, y), ay(x, y) = in(x, y-1) + 2 in(x, y) + in(x, y+1);
 *                out = min(|ax(x, y-1) - ax(x, y+1)| + |ay(x-1, y) - ay(x+1, y)|, 255).  Each term is at most 1020; no square root.
 *   gaussian5x5  weights (1, 4, 6, 4, 1) down the column, then along the row, in int16; out = u8(cols >> 8).  cols reaches 65280 and
 *                wraps in int16; the arithmetic shift and the narrowing cast undo the wrap: floor(true sum / 256) for every input.
 *                The shift truncates (no rounding), nothing is clamped; a constant image v gives v.
 *   conv3x3a32   S = sum over i, j in -1 .. 1 of in(x + j, y + i) * mask(j + 1, i + 1) in int32; out = u8(clamp(S >> 4, 0, 255)),
 *                an arithmetic shift.
 *   conv3x3a16   the same with S wrapped to int16 before the shift: two's complement modulo 2^16, neither saturated nor undefined
 *                (each product fits int16).  An all-255 image under an all-16 mask: S = 36720 wraps to -28816, >> 4 is -1801: 0,
 *                where conv3x3a32 writes 255.
 * Entry contract: null (-12), type (-3), dimensionality (-43); input.min.0 == 0 and input.min.1 == 0 on all six, output.min.0 == 0
 * and output.min.1 == 0 on all but sobel (-8), which takes an output region at any origin; then a bounds query answers mask with
 * [0, 3) x [0, 3) and leaves input and output as passed (the clamp's bound is the input's own box); then sizes (-8, -5, -6) and
 * coverage (-4): mask covers [0, 3) x [0, 3), its mins and strides otherwise free, and the input holds the clamped samples the
 * region reads, which only an empty input fails.  The output's extents are independent of the input's.  The mask's nine values are
 * read on the host at the call.  Nothing is launched for an empty output.  No _auto_schedule twins. */
int conv3x3a16(struct halide_buffer_t *input, struct halide_buffer_t *mask, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(conv3x3a16)
int conv3x3a32(struct halide_buffer_t *input, struct halide_buffer_t *mask, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(conv3x3a32)
int dilate3x3(struct halide_buffer_t *input, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(dilate3x3)
int median3x3(struct halide_buffer_t *input, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(median3x3)
int gaussian5x5(struct halide_buffer_t *input, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(gaussian5x5)
int sobel(struct halide_buffer_t *input, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(sobel)

/* apps/cuda_mat_mul/mat_mul_generator.cpp:15-32,74 — the square f32 matrix product, built with size = 1024 as the reference builds it:
 *   out(x, y) = acc_size,  acc_0 = +0.0f,  acc_{r+1} = fmaf(A(x, r), B(r, y), acc_r),  r = 0 .. size - 1
 * Dimension 0 is innermost, so in memory out[y][x] = sum_r B[y][r] * A[r][x]: with row-major arrays this is B @ A, not A @ B.  The
 * k-ordered fmaf chain is the contract in BOTH canonical float forms: both library builds give the same bits.  No step is padded (a
 * chain may end in -0.0f), subnormals are kept, NaN in gives NaN out, Inf and overflow follow fmaf.
 * A, B and out: float32, 2-D, min 0 and extent 1024 in both dimensions, stride 1 in dimension 0 (-8 otherwise); out may not alias an
 * input (-8).  A superset of the reference in two respects: the stride of dimension 1 may be any value >= 1024 (the reference pins
 * stride == size), and any element alignment is accepted (the reference asks for 16-byte host pointers).  A bounds query on any
 * buffer fills all three with [0, 1024) x [0, 1024), dense.  No _auto_schedule twin: the reference builds none. */
int mat_mul(struct halide_buffer_t *A, struct halide_buffer_t *B, struct halide_buffer_t *out);
HLMI_DECLARE_AUX(mat_mul)

/* apps/fft/fft_generator.cpp, the four objects of apps/fft/CMakeLists.txt:22-47 — the 2-D f32 Fourier transform of a 16 x 16 image:
 *   fft_forward_r2c   real [16, 16, 1] -> complex [16, 9, 2],  gain 1/256      fft_inverse_c2r   complex [16, >= 9, 2] -> real [16, 16, 1], gain 1
 *   fft_forward_c2c   complex [16, 16, 2] -> complex [16, 16, 2], gain 1/256   fft_inverse_c2c   the same, sign +1, gain 1
 * X(k0, k1) = gain * sum over n0, n1 of x(n0, n1) exp(sign 2 pi j (k0 n0 / N0 + k1 n1 / N1)), sign -1 forward and +1 inverse, evaluated
 * as the reference's Stockham passes (fft.cpp:295-421): radix_factor's radices (16 = {4, 4}), the codelets dft2 / dft4 / dft6 / dft8
 * with their literals, dimension 0 first with gain 1, then dimension 1; the gain is folded into the first twiddle table of the pass
 * that carries it.  Twiddles W(n) = (cosf(a), sinf(a)) * gain with a = ((float)(sign * 2) * (float)M_PI * (float)n) / (float)(R S),
 * a true f32 division, built on the host.  r2c and c2r pair real columns in groups of V = 8 (natural_vector_size of the reference's
 * x86-64 AVX2 build, vector_width = 0) and zip the DC and Nyquist rows as the reference writes them (fft.cpp:667-1061), so r2c equals
 * the first N1/2 + 1 rows of c2c within rounding, not bit for bit.  A complex product is (a.re b.re - a.im b.im, a.re b.im + a.im
 * b.re) with the first product of each fused in the default build (mulsub, mad2) and every operator rounded with HLMI_CANON_FMA=0;
 * `* j` swaps and negates once, `* sign` negates or does nothing, conj negates the imaginary part, 0.5f * is a rounded multiply.
 * Subnormals are kept; one NaN or Inf in the input reaches every output (each output of a 2-D transform depends on every input).
 * Buffers: float32, 3-D; dimension 2 is min 0, extent 1 (real) or 2 (complex: re, im), stride 1; dimension 0 has stride 1 (real) or 2
 * (complex); dimension 1 any stride >= the row (-8 otherwise).  The output is exactly [0, N0) x [0, rows); the input covers that box
 * of its own (-4) and may be larger: c2r reads rows 0 .. N1/2 only.  Input and output may not overlap (-8).  A bounds query fills the
 * query buffers with those boxes, interleaved and dense.  No _auto_schedule twin: the reference builds none. */
int fft_forward_r2c(struct halide_buffer_t *input, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(fft_forward_r2c)
int fft_inverse_c2r(struct halide_buffer_t *input, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(fft_inverse_c2r)
int fft_forward_c2c(struct halide_buffer_t *input, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(fft_forward_c2c)
int fft_inverse_c2c(struct halide_buffer_t *input, struct halide_buffer_t *output);
HLMI_DECLARE_AUX(fft_inverse_c2c)

/* apps/linear_algebra/src/blas_l{1,2,3}_generators.cpp, the twelve f32 objects of src/CMakeLists.txt — the pipelines behind
 * halide_blas.h (here: hlmi_blas.h, which adds the wrappers and the hblas_s* calls).  All buffers float32; dimension 0 is innermost
 * with stride 1 and min 0 (-8 otherwise); matrices are column-major, the stride of dimension 1 any value >= extent 0.  V = 8, the
 * natural_vector_size(float) of the reference's x86-64 AVX2 build.  mad(a, b, c) = a * b + c and mad2(a, b, c, d) = a * b + c * d are
 * fused (the first product) in the default build and round every operator with HLMI_CANON_FMA=0; `*` is a rounded multiply.
 *   halide_scopy_impl     result(i) = x(i); a and y unused, y may be null
 *   halide_sscal_impl     result(i) = a * x(i); y unused and may be null; result may be x itself
 *   halide_saxpy_impl     result(i) = mad(a, x(i), y(i)); result may be y itself
 *   halide_sdot           lane_i = +0, k upward over n / V: lane_i = mad(x(kV + i), y(kV + i), lane_i); s = +0, s = s + lane_i for
 *                         i = 0 .. V - 1; t = +0, upward over the tail: t = mad(x, y, t); result() = s + t (0-dimensional)
 *   halide_sasum          the same with lane_i + |x| and t + |x|
 *   halide_sgemv_notrans  A[M x N], x[N], y[M]: acc = b * y(i), k upward: acc = mad(a * A(i, k), x(k), acc); output(i) = acc
 *   halide_sgemv_trans    A[M x N], x[M], y[N]: per output i the V lane chains lane_j = mad(A(kV + j, i), x(kV + j), lane_j), s = +0,
 *                         s = s + lane_j, the tail upward s = mad(A(t, i), x(t), s); output(i) = mad2(b, y(i), a, s)
 *   halide_sger_impl      x[M], y[N]: result(i, j) = mad(a * y(j), x(i), result(i, j)), in place
 *   halide_sgemm_*        ab = +0, k upward: ab = mad(opA(i, k), opB(k, j), ab); result(i, j) = mad2(a, ab, b, C(i, j)); b * C is always
 *                         evaluated (b = 0 does not hide a NaN in C).  The sizes come from the stored matrices — M = A.extent.0,
 *                         K = A.extent.1 = B.extent.0, N = B.extent.1, C and result M x N — so notrans is fully rectangular, transA
 *                         (opA(i, k) = A(k, i)) needs A square, transB (opB(k, j) = B(j, k)) needs B square, transAB both (-8 otherwise)
 * The output may be exactly the y / C argument (the same buffer, or the same first element and layout): that is the call every wrapper
 * makes.  Any other overlap of the output with an input is refused (-8).  Vector lengths 0 .. 2^27, matrix extents 0 .. 8192 (-8
 * beyond); an empty output launches nothing, sdot and sasum of nothing write +0.  A bounds query fills the query buffers with the
 * shapes the given ones imply.  No _auto_schedule twins: the reference builds none. */
int halide_scopy_impl(float a, struct halide_buffer_t *x, struct halide_buffer_t *y, struct halide_buffer_t *result);
HLMI_DECLARE_AUX(halide_scopy_impl)
int halide_sscal_impl(float a, struct halide_buffer_t *x, struct halide_buffer_t *y, struct halide_buffer_t *result);
HLMI_DECLARE_AUX(halide_sscal_impl)
int halide_saxpy_impl(float a, struct halide_buffer_t *x, struct halide_buffer_t *y, struct halide_buffer_t *result);
HLMI_DECLARE_AUX(halide_saxpy_impl)
int halide_sdot(struct halide_buffer_t *x, struct halide_buffer_t *y, struct halide_buffer_t *result);
HLMI_DECLARE_AUX(halide_sdot)
int halide_sasum(struct halide_buffer_t *x, struct halide_buffer_t *result);
HLMI_DECLARE_AUX(halide_sasum)
int halide_sgemv_notrans(float a, struct halide_buffer_t *A, struct halide_buffer_t *x, float b, struct halide_buffer_t *y,
                         struct halide_buffer_t *output);
HLMI_DECLARE_AUX(halide_sgemv_notrans)
int halide_sgemv_trans(float a, struct halide_buffer_t *A, struct halide_buffer_t *x, float b, struct halide_buffer_t *y,
                       struct halide_buffer_t *output);
HLMI_DECLARE_AUX(halide_sgemv_trans)
int halide_sger_impl(float a, struct halide_buffer_t *x, struct halide_buffer_t *y, struct halide_buffer_t *result);
HLMI_DECLARE_AUX(halide_sger_impl)
int halide_sgemm_notrans(float a, struct halide_buffer_t *A, struct halide_buffer_t *B, float b, struct halide_buffer_t *C,
                         struct halide_buffer_t *result);
HLMI_DECLARE_AUX(halide_sgemm_notrans)
int halide_sgemm_transA(float a, struct halide_buffer_t *A, struct halide_buffer_t *B, float b, struct halide_buffer_t *C,
                        struct halide_buffer_t *result);
HLMI_DECLARE_AUX(halide_sgemm_transA)
int halide_sgemm_transB(float a, struct halide_buffer_t *A, struct halide_buffer_t *B, float b, struct halide_buffer_t *C,
                        struct halide_buffer_t *result);
HLMI_DECLARE_AUX(halide_sgemm_transB)
int halide_sgemm_transAB(float a, struct halide_buffer_t *A, struct halide_buffer_t *B, float b, struct halide_buffer_t *C,
                         struct halide_buffer_t *result);
HLMI_DECLARE_AUX(halide_sgemm_transAB)

/* The f64 half of apps/linear_algebra: the twelve `halide_d*` objects of src/CMakeLists.txt, the same generators at T = double (here:
 * hlmi_blas.h adds the wrappers and the hblas_d* calls).  The contract is the one above with three differences: every buffer is float64,
 * the scalars a and b are doubles, and V = 4, the natural_vector_size(double) of the reference's x86-64 AVX2 build — ddot, dasum and
 * dgemv_trans keep four lane chains.  mad and mad2 are the same two forms in binary64.  Shapes, aliasing, limits (vector lengths
 * 0 .. 2^27, matrix extents 0 .. 8192), empty outputs (ddot and dasum of nothing write the eight bytes of +0) and bounds queries are
 * as for the f32 half. */
int halide_dcopy_impl(double a, struct halide_buffer_t *x, struct halide_buffer_t *y, struct halide_buffer_t *result);
HLMI_DECLARE_AUX(halide_dcopy_impl)
int halide_dscal_impl(double a, struct halide_buffer_t *x, struct halide_buffer_t *y, struct halide_buffer_t *result);
HLMI_DECLARE_AUX(halide_dscal_impl)
int halide_daxpy_impl(double a, struct halide_buffer_t *x, struct halide_buffer_t *y, struct halide_buffer_t *result);
HLMI_DECLARE_AUX(halide_daxpy_impl)
int halide_ddot(struct halide_buffer_t *x, struct halide_buffer_t *y, struct halide_buffer_t *result);
HLMI_DECLARE_AUX(halide_ddot)
int halide_dasum(struct halide_buffer_t *x, struct halide_buffer_t *result);
HLMI_DECLARE_AUX(halide_dasum)
int halide_dgemv_notrans(double a, struct halide_buffer_t *A, struct halide_buffer_t *x, double b, struct halide_buffer_t *y,
                         struct halide_buffer_t *output);
HLMI_DECLARE_AUX(halide_dgemv_notrans)
int halide_dgemv_trans(double a, struct halide_buffer_t *A, struct halide_buffer_t *x, double b, struct halide_buffer_t *y,
                       struct halide_buffer_t *output);
HLMI_DECLARE_AUX(halide_dgemv_trans)
int halide_dger_impl(double a, struct halide_buffer_t *x, struct halide_buffer_t *y, struct halide_buffer_t *result);
HLMI_DECLARE_AUX(halide_dger_impl)
int halide_dgemm_notrans(double a, struct halide_buffer_t *A, struct halide_buffer_t *B, double b, struct halide_buffer_t *C,
                         struct halide_buffer_t *result);
HLMI_DECLARE_AUX(halide_dgemm_notrans)
int halide_dgemm_transA(double a, struct halide_buffer_t *A, struct halide_buffer_t *B, double b, struct halide_buffer_t *C,
                         struct halide_buffer_t *result);
HLMI_DECLARE_AUX(halide_dgemm_transA)
int halide_dgemm_transB(double a, struct halide_buffer_t *A, struct halide_buffer_t *B, double b, struct halide_buffer_t *C,
                         struct halide_buffer_t *result);
HLMI_DECLARE_AUX(halide_dgemm_transB)
int halide_dgemm_transAB(double a, struct halide_buffer_t *A, struct halide_buffer_t *B, double b, struct halide_buffer_t *C,
                         struct halide_buffer_t *result);
HLMI_DECLARE_AUX(halide_dgemm_transAB)

/* apps/resnet_50/Resnet50Generator.cpp:31-66,383 — the f32 ResNet-50 forward pass at its one fixed shape, 3 x 224 x 224 -> 1000 softmax
 * probabilities.  One generator, one entry point, 269 buffers in the generator's declaration order; an array member i is `<array>_<i>`:
 *   input [3, 224, 224];
 *   four groups `X` = gamma, beta, mu, sig of 53 vectors each: conv1_X [64], br1_X_0 .. 3, br2a_X_0 .. 15, br2b_X_0 .. 15, br2c_X_0 .. 15, each
 *   [CO] of its convolution;   the weights in the same order: conv1_weights, br1_conv_weights_0 .. 3, br2a_conv_weights_0 .. 15,
 *   br2b_conv_weights_0 .. 15, br2c_conv_weights_0 .. 15, each [CO, KW, KH, CI];   fc1000_weights [1000, 2048], fc1000_bias [1000];
 *   final_output [<= 1000].
 * Everything is float32, dimension 0 innermost with stride 1 (-8 otherwise), every min 0; activations are (c, x, y), convolution weights
 * (co, kx, ky, ci) — what the reference's load_weights.py writes and process.cpp:74-78 loads.
 * Shapes (:70-113): stem 7 x 7, stride 2, pad 3 -> 64 channels; max pool 3 x 3, stride 2, pad 1; four stages (mid channels, blocks, stride) =
 * (64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2) of bottleneck blocks br2a 1 x 1 -> mid, br2b 3 x 3 pad 1 -> mid, br2c 1 x 1 -> 4 mid; the
 * stage's stride sits on br2b and br1 of its first block; br1 (1 x 1 -> 4 mid, on the block's input) exists in blocks 0, 3, 7, 13.  Output
 * extents are compute_shape's (:245-251): (2 pad + in - k + 1 + stride - 1) / stride, truncating.
 * Arithmetic, with mad(a, b, c) = a * b + c fused in the default build and rounded twice with HLMI_CANON_FMA=0:
 *   conv       one chain per output from +0, k = (ky KW + kx) CI + ci strictly upward: acc = mad(w(co, kx, ky, ci), padded(ci, s i + kx - p,
 *              s j + ky - p), acc).  A tap outside the image is a step with the value +0 (constant_exterior), not a skipped step: w * 0 can
 *              be -0 or NaN.  No step is added to an odd K (conv1: K = 147).  br1 and every pad-0 layer read no exterior.
 *   norm+scale inlined into the consumer: t = (v - mu(c)) / sqrt(sig(c) + 1e-5f), correctly rounded sqrt and IEEE division, then
 *              mad(t, gamma(c), beta(c))
 *   relu       max(0.0f, v) as conv_layer's: v > 0 ? v : +0, so a NaN becomes +0
 *   residual   shortcut + scaled_2c, a plain add, then relu; the shortcut is the previous block's output or br1's scaled value (no relu)
 *   max pool   from -inf (the float type's minimum, as Halide's inline maximum), r.x fastest then r.y: acc = v > acc ? v : acc; the +0
 *              exterior takes part
 *   avg pool   from +0, acc = mad(n, v, acc) with n = 1.0f / 49.0f evaluated in float, r.x fastest
 *   fc         from bias(c): acc = mad(w(c, k), pool(k), acc), k = 0 .. 2047 upward
 *   softmax    e(c) = exp(fc(c)) with the reference's halide_exp; S = plain adds from +0 over c = 0 .. 999 upward; out(c) = e(c) / S.  No
 *              maximum is subtracted: a logit past exp's range gives inf / inf = NaN here as in the reference.
 * Protocol: final_output may be any box inside [0, 1000): only those classes are stored, the sum still runs over all 1000 and every input
 * is required in full.  A class outside [0, 1000) is a read of fc1000_bias / fc1000_weights outside theirs (-4, as in the reference).  Every
 * input must cover its box (-4) and may be larger or have padded strides.  A bounds query answers every input's fixed box and, for an
 * output without a shape, [0, 1000).  No _auto_schedule twin: the reference builds none.
 * HLMI_RN50_INPUTS(X) is the list of the 268 inputs in order, X(name) for each: callers with tables of their own may use it too. */
#define HLMI_RN50_R4(X, a) X(a##_0) X(a##_1) X(a##_2) X(a##_3)
#define HLMI_RN50_R16(X, a) HLMI_RN50_R4(X, a) X(a##_4) X(a##_5) X(a##_6) X(a##_7) X(a##_8) X(a##_9) X(a##_10) X(a##_11) X(a##_12) X(a##_13) X(a##_14) X(a##_15)
#define HLMI_RN50_GROUP(X, s) X(conv1_##s) HLMI_RN50_R4(X, br1_##s) HLMI_RN50_R16(X, br2a_##s) HLMI_RN50_R16(X, br2b_##s) HLMI_RN50_R16(X, br2c_##s)
#define HLMI_RN50_WEIGHTS(X) X(conv1_weights) HLMI_RN50_R4(X, br1_conv_weights) HLMI_RN50_R16(X, br2a_conv_weights) HLMI_RN50_R16(X, br2b_conv_weights) HLMI_RN50_R16(X, br2c_conv_weights)
#define HLMI_RN50_INPUTS(X) X(input) HLMI_RN50_GROUP(X, gamma) HLMI_RN50_GROUP(X, beta) HLMI_RN50_GROUP(X, mu) HLMI_RN50_GROUP(X, sig) HLMI_RN50_WEIGHTS(X) X(fc1000_weights) X(fc1000_bias)
#define HLMI_RN50_PARAM(name) struct halide_buffer_t *name,
int resnet50(HLMI_RN50_INPUTS(HLMI_RN50_PARAM) struct halide_buffer_t *final_output);
HLMI_DECLARE_AUX(resnet50)

/* resnet50_batch — a LIBRARY EXTENSION: the reference has no such generator (its resnet_50 has no batch dimension).  resnet50 over N images
 * per call; the same 269 buffers in the same order, two of them with one more dimension:
 *   input [3, 224, 224, N];   final_output [<= 1000, N];   the 267 parameter buffers exactly as resnet50 takes them.
 * Contract: column n of final_output holds, bit for bit and NaN for NaN, what resnet50 writes for image n of input, in both canonical
 * float forms.  Every chain, epilogue, pool, fc and softmax step of image n is resnet50's; no operation mixes two images.
 * Protocol: resnet50's, with one more range, the images [bmin, bmin + N): dimension 1 of final_output where that buffer is known (real,
 * or a query with a shape), else dimension 3 of input where that is known, else [0, 1).  input must cover that range in dimension 3 (-4)
 * and may be larger or padded in any dimension; the class box of final_output (dimension 0) keeps resnet50's rule.  A bounds query
 * answers every box, the image range included.  Checks and return codes are resnet50's, in its order.
 * Any N >= 1 runs as ceil(N / C) runs of the launch plan over at most C images each, in order on the call's stream; C is 64 unless
 * HLMI_RN50_BATCH_CHUNK (1 .. 64, read once per call; any other value is refused with -8) says otherwise.  The rule that every element
 * of a buffer lies within 2^31 - 1 elements of its first (-5) applies PER CHUNK to input and final_output — C images and C columns,
 * whatever N is — and to every other buffer as a whole. */
int resnet50_batch(HLMI_RN50_INPUTS(HLMI_RN50_PARAM) struct halide_buffer_t *final_output);
HLMI_DECLARE_AUX(resnet50_batch)

/* apps/camera_pipe/camera_pipe_generator.cpp:219-228,622 — raw u16 Bayer -> u8 [W,H,3]. */
int camera_pipe(struct halide_buffer_t *input, struct halide_buffer_t *matrix_3200,
                struct halide_buffer_t *matrix_7000, float color_temp, float gamma, float contrast,
                float sharpen_strength, int32_t blackLevel, int32_t whiteLevel,
                struct halide_buffer_t *processed);
HLMI_DECLARE_AUX(camera_pipe)

/* `<name>_auto_schedule` variants: the reference's drivers link both objects
 * (apps/local_laplacian/process.cpp:5-7,42-49); same algorithm, so they alias the entry above. */
int local_laplacian_auto_schedule(struct halide_buffer_t *input, int32_t levels, float alpha, float beta,
                                  struct halide_buffer_t *output);
int bilateral_grid_auto_schedule(struct halide_buffer_t *input, float r_sigma, struct halide_buffer_t *out);
int halide_blur_auto_schedule(struct halide_buffer_t *input, struct halide_buffer_t *blur_y);
int nl_means_auto_schedule(struct halide_buffer_t *input, int32_t patch_size, int32_t search_area, float sigma,
                           struct halide_buffer_t *non_local_means);
int stencil_chain_auto_schedule(struct halide_buffer_t *input, struct halide_buffer_t *output);
int conv_layer_auto_schedule(struct halide_buffer_t *input, struct halide_buffer_t *filter,
                             struct halide_buffer_t *bias, struct halide_buffer_t *relu);
int depthwise_separable_conv_auto_schedule(struct halide_buffer_t *input, struct halide_buffer_t *depthwise_filter,
                                           struct halide_buffer_t *pointwise_filter, struct halide_buffer_t *bias,
                                           struct halide_buffer_t *output);
int unsharp_auto_schedule(struct halide_buffer_t *input, struct halide_buffer_t *output);
int max_filter_auto_schedule(struct halide_buffer_t *input, struct halide_buffer_t *output);
int hist_auto_schedule(struct halide_buffer_t *input, struct halide_buffer_t *output);
int harris_auto_schedule(struct halide_buffer_t *input, struct halide_buffer_t *output);
int interpolate_auto_schedule(struct halide_buffer_t *input, struct halide_buffer_t *output);
int iir_blur_auto_schedule(struct halide_buffer_t *input, float alpha, struct halide_buffer_t *output);
int lens_blur_auto_schedule(struct halide_buffer_t *left_im, struct halide_buffer_t *right_im, int32_t slices,
                            int32_t focus_depth, float blur_radius_scale, int32_t aperture_samples,
                            struct halide_buffer_t *final);
int bgu_auto_schedule(float r_sigma, int32_t s_sigma, struct halide_buffer_t *splat_loc, struct halide_buffer_t *values,
                      struct halide_buffer_t *slice_loc, struct halide_buffer_t *output);
int gaussian_blur_direct_auto_schedule(struct halide_buffer_t *input, float sigma, int32_t trunc, struct halide_buffer_t *output);
int camera_pipe_auto_schedule(struct halide_buffer_t *input, struct halide_buffer_t *matrix_3200,
                              struct halide_buffer_t *matrix_7000, float color_temp, float gamma, float contrast,
                              float sharpen_strength, int32_t blackLevel, int32_t whiteLevel,
                              struct halide_buffer_t *processed);

#undef HLMI_DECLARE_AUX

#ifdef __cplusplus
}
#endif
#endif /* HLMI_PIPELINES_H */
