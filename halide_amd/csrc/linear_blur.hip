// linear_blur.hip — apps/linear_blur: the 3x3 box blur simple_blur, f32 [x, y, c], and linear_blur, the same blur in linear light
// (sRGB -> linear, blur, linear -> sRGB), the reference's demonstration of generator composition; 2 AOT entry points from one kernel
// template.  Reference semantics: apps/linear_blur/simple_blur_generator.cpp:5-22 (the blur over repeat_edge of [0, width) x
// [0, height)), srgb_to_linear_generator.cpp:14-16, linear_to_srgb_generator.cpp:14-16, linear_blur_generator.cpp:8-27 (the
// composition, width and height the input's EXTENTS); the contract the kernels share with the checker (tests/cpp/linear_blur_check.c)
// is restated in DESIGN.md §5.3.
//
//   lb_fused<LINEAR>   one launch, every shape.  A workgroup owns 64 x 32 outputs of one channel: it stages the 66 x 34 samples they
//                      read into LDS, each read with its clamp and converted to linear light ONCE on the way in (1.096 conversions per
//                      output, not 9); a wave then owns 8 rows, a lane one column, and slides a three-row register window of blur_x
//                      down them: 3 LDS reads per row of blur_x, 10 rows for 8 outputs; to_srgb, store.  LINEAR = false: no conversion
//   lb_to_linear, lb_blur_general, lb_to_srgb   the unfused composition hlmi_linear_blur_general runs: to_linear over the required
//                      region into the stream's scratch arena, one thread per output with its nine clamped taps from global memory,
//                      to_srgb over the output in place; simple_blur: the middle launch alone
// Every path forms blur_x = ((a + b) + c) * third and the output = ((blur_x0 + blur_x1) + blur_x2) * third from the same converted
// samples, so all of them agree bit for bit.
#include "hlmi_device_math.h"
#include "hlmi_internal.h"

using namespace hlmi;

namespace {

constexpr int TW = 64, TH = 32;            // outputs per workgroup
constexpr int SW = TW + 2, SH = TH + 2;    // staged samples: the window is x .. x + 2, y .. y + 2
constexpr int ROWS = TH / 4;               // rows per wave

struct LGeom {
    const float *src;     // sample (ix0, iy0) of the output's first channel
    long s_sy, s_sc;
    int ix0, iy0;         // coordinates of src[0]
    int w, h;             // the clamp: x to [0, w - 1], y to [0, h - 1]
    float *dst;           // the output's first element
    long d_sy, d_sc;
    int ox, oy, ow, oh;   // the output's region
};

// x / c -> x * fold(1 / c) (src/Simplify_Div.cpp:204); 1 + .055f is folded in f32 as the generators write it
constexpr float THIRD = 1.0f / 3.0f, A = 0.055f, ONE_A = 1.0f + 0.055f;

// srgb_to_linear_generator.cpp:14-16
__device__ __forceinline__ float to_linear(float s) {
    const float low = s * (1.0f / 12.92f);
    const float high = dev::halide_pow((s + A) * (1.0f / ONE_A), 2.4f);
    return s <= 0.04045f ? low : high;
}

// linear_to_srgb_generator.cpp:14-16; the last step is the one multiply that feeds a subtract
__device__ __forceinline__ float to_srgb(float l) {
    const float low = l * 12.92f;
    const float high = dev::mulsub(ONE_A, dev::halide_pow(l, 1.0f / 2.4f), A);
    return l <= 0.0031308f ? low : high;
}

// max(min(v, n - 1), 0): n <= 0 gives 0
__device__ __forceinline__ int clamp_to(long v, int n) { return (int)max(min(v, (long)n - 1), 0L); }

// in(X, Y) of the channel at p
__device__ __forceinline__ float sample(const LGeom &g, const float *p, long X, long Y) {
    return p[(long)(clamp_to(Y, g.h) - g.iy0) * g.s_sy + (clamp_to(X, g.w) - g.ix0)];
}

// ---------------------------------------------------------------------------------------------------------------- fused
template<bool LINEAR>
__global__ __launch_bounds__(256) void lb_fused(LGeom g) {
    __shared__ float s_in[SH * SW];
    const int tid = (int)threadIdx.x;
    const int tx0 = (int)blockIdx.x * TW, ty0 = (int)blockIdx.y * TH;
    const float *p = g.src + (long)blockIdx.z * g.s_sc;
    // samples past what the region's last output reads (column ow + 1, row oh + 1) are not read: the input need not hold them
    const int nx = min(SW, g.ow + 2 - tx0), ny = min(SH, g.oh + 2 - ty0);
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // columns 0 .. 63 by rows: wave w takes rows w, w + 4, ..., a lane one column, so the row's clamp and address are scalar and
    // the column's are formed once
    const long xoff = clamp_to((long)g.ox + tx0 + lane, g.w) - g.ix0;
    for (int sy = wave; sy < ny; sy += 4) {
        const float *row = p + (long)(clamp_to((long)g.oy + ty0 + sy, g.h) - g.iy0) * g.s_sy;
        if (lane < nx) {
            const float v = row[xoff];
            s_in[sy * SW + lane] = LINEAR ? to_linear(v) : v;
        }
    }
    // columns 64 and 65 by lanes on rows, one column each for waves 2 and 3, which had a row fewer above: 9 conversions a wave
    if (wave >= 2) {
        const int sx = TW - 2 + wave;
        if (sx < nx && lane < ny) {
            const float v = sample(g, p, (long)g.ox + tx0 + sx, (long)g.oy + ty0 + lane);
            s_in[lane * SW + sx] = LINEAR ? to_linear(v) : v;
        }
    }
    __syncthreads();
    const int r0 = wave * ROWS;
    const int x = tx0 + lane;
    auto blur_x = [&](int r) {
        const float *q = s_in + r * SW + lane;
        return ((q[0] + q[1]) + q[2]) * THIRD;
    };
    float b0 = blur_x(r0), b1 = blur_x(r0 + 1);   // a wave wholly below the region reads rows nobody staged here: stale LDS, never stored
    float *o = g.dst + (long)blockIdx.z * g.d_sc;
#pragma unroll
    for (int j = 0; j < ROWS; j++) {
        const int y = ty0 + r0 + j;
        if (y >= g.oh) break;   // scalar
        const float b2 = blur_x(r0 + j + 2);
        float v = ((b0 + b1) + b2) * THIRD;
        if (LINEAR) v = to_srgb(v);
        if (x < g.ow) o[(long)y * g.d_sy + x] = v;   // columns past the region: stale LDS, not stored
        b0 = b1, b1 = b2;
    }
}

// ---------------------------------------------------------------------------------------------------------------- general path
// mid[c][y][x] = to_linear(src(x, y, c)) over rw x rh samples of each channel
__global__ __launch_bounds__(256) void lb_to_linear(const float *__restrict__ src, long s_sy, long s_sc, float *__restrict__ mid, int rw, int rh) {
    const int x = (int)blockIdx.x * 256 + (int)threadIdx.x, y = (int)blockIdx.y, c = (int)blockIdx.z;
    if (x >= rw) return;
    mid[((size_t)c * rh + y) * rw + x] = to_linear(src[(long)c * s_sc + (long)y * s_sy + x]);
}

__global__ __launch_bounds__(256) void lb_blur_general(LGeom g) {
    const int x = (int)blockIdx.x * 256 + (int)threadIdx.x, y = (int)blockIdx.y;
    if (x >= g.ow) return;
    const float *p = g.src + (long)blockIdx.z * g.s_sc;
    const long X = (long)g.ox + x, Y = (long)g.oy + y;
    float b[3];
#pragma unroll
    for (int j = 0; j < 3; j++) b[j] = ((sample(g, p, X, Y + j) + sample(g, p, X + 1, Y + j)) + sample(g, p, X + 2, Y + j)) * THIRD;
    g.dst[(long)blockIdx.z * g.d_sc + (long)y * g.d_sy + x] = ((b[0] + b[1]) + b[2]) * THIRD;
}

__global__ __launch_bounds__(256) void lb_to_srgb(float *dst, long d_sy, long d_sc, int ow) {
    const int x = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (x >= ow) return;
    float *o = dst + (long)blockIdx.z * d_sc + (long)blockIdx.y * d_sy + x;
    *o = to_srgb(*o);
}

// ---------------------------------------------------------------------------------------------------------------- host
// the generator's estimates (linear_blur_generator.cpp:20-21); simple_blur is built without any (CMakeLists.txt:40-43)
const ArgTable lb_table("linear_blur", {in_buf("input", T_F32, 3, {0, 1536, 0, 2560, 0, 4}), out_buf("output", T_F32, 3, {0, 1536, 0, 2560, 0, 4})});
const ArgTable sb_table("simple_blur", {in_buf("input", T_F32, 3), scalar_i32("width"), scalar_i32("height"), out_buf("output", T_F32, 3)});

int host_clamp_to(long v, int n) { return (int)std::max<long>(std::min<long>(v, (long)n - 1), 0); }

int blocks_ok(void *uc, size_t gx, size_t gy, size_t gz) {
    if (gx <= 0x7fffffffu && gy <= 65535u && gz <= 65535u) return 0;
    return report(uc, halide_error_code_buffer_extents_too_large, "linear_blur: %zu x %zu x %zu workgroups exceed one launch", gx, gy, gz);
}

// linear: the clamp is to the input's extents in absolute coordinates (linear_blur_generator.cpp:16 passes input.width() and
// input.height()), whatever its mins are; width and height are not read
int entry(bool linear, halide_buffer_t *input, int32_t width, int32_t height, halide_buffer_t *output, bool general_only) {
    void *uc = nullptr;
    BufArg args[2];
    (linear ? lb_table : sb_table).bufs(args, {input, output});
    int r = check_not_null(uc, args, 2);
    if (r) return r;
    if ((r = check_type_and_dims(uc, args, 2))) return r;
    if (linear) width = input->dim[0].extent, height = input->dim[1].extent;
    const halide_dimension_t *id = input->dim, *od = output->dim;
    // what the output region reads: columns cx(ox) .. cx(ox + ow + 1), rows cy(oy) .. cy(oy + oh + 1), its own channels
    const int rx0 = host_clamp_to(od[0].min, width), rx1 = host_clamp_to((long)od[0].min + od[0].extent + 1, width);
    const int ry0 = host_clamp_to(od[1].min, height), ry1 = host_clamp_to((long)od[1].min + od[1].extent + 1, height);
    if (any_bounds_query(args, 2)) {
        // the output's region is the request and stays as passed.  simple_blur: the input gets the box above.  linear_blur: the box
        // depends on the input's own extents, so x and y stay as passed too (as for gaussian_blur_direct and resize) and the input
        // gets the output's channels
        int mins[3] = {rx0, ry0, od[2].min}, ext[3] = {rx1 - rx0 + 1, ry1 - ry0 + 1, od[2].extent};
        if (linear) mins[0] = id[0].min, mins[1] = id[1].min, ext[0] = id[0].extent, ext[1] = id[1].extent;
        answer_query(input, mins, ext);
        return 0;
    }
    if ((r = check_shapes(uc, args, 2))) return r;
    check_covers(uc, args[0], 0, rx0, rx1 - rx0 + 1);
    check_covers(uc, args[0], 1, ry0, ry1 - ry0 + 1);
    check_covers(uc, args[0], 2, od[2].min, od[2].extent);
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, 2))) return r;
    LGeom g;
    g.ox = od[0].min, g.oy = od[1].min, g.ow = od[0].extent, g.oh = od[1].extent;
    const int on = od[2].extent;
    if (g.ow > 0 && g.oh > 0 && on > 0) {
        g.src = dev_ptr<float>(input) + (long)(od[2].min - id[2].min) * id[2].stride;
        g.s_sy = id[1].stride, g.s_sc = id[2].stride, g.ix0 = id[0].min, g.iy0 = id[1].min;
        g.w = width, g.h = height;
        g.dst = dev_ptr<float>(output), g.d_sy = od[1].stride, g.d_sc = od[2].stride;
        hipStream_t st = ctx.stream;
        const double bytes = 8.0 * g.ow * g.oh * on;   // each value read once and written once
        const size_t gx = (g.ow + 255) / 256;
        if (!general_only) {
            const size_t tx = (g.ow + TW - 1) / TW, ty = (g.oh + TH - 1) / TH;
            if ((r = blocks_ok(uc, tx, ty, on))) return r;
            timing_note_bytes(bytes);
            if (linear) HLMI_LAUNCH(uc, "lb_fused", st, lb_fused<true>, dim3((unsigned)tx, (unsigned)ty, (unsigned)on), dim3(256), 0, g);
            else HLMI_LAUNCH(uc, "sb_fused", st, lb_fused<false>, dim3((unsigned)tx, (unsigned)ty, (unsigned)on), dim3(256), 0, g);
        } else {
            if ((r = blocks_ok(uc, gx, g.oh, on))) return r;
            if (linear) {
                // the required region in linear light, dense, in the scratch arena; the blur then reads it in the input's place
                const int rw = rx1 - rx0 + 1, rh = ry1 - ry0 + 1;
                if ((r = blocks_ok(uc, (rw + 255) / 256, rh, on))) return r;
                void *ws = nullptr;
                if ((r = get_workspace(uc, ctx, sizeof(float) * (size_t)rw * rh * on, &ws))) return r;
                const float *from = g.src + (long)(ry0 - g.iy0) * g.s_sy + (rx0 - g.ix0);
                HLMI_LAUNCH(uc, "lb_to_linear", st, lb_to_linear, dim3((unsigned)((rw + 255) / 256), (unsigned)rh, (unsigned)on), dim3(256), 0, from, g.s_sy,
                            g.s_sc, (float *)ws, rw, rh);
                g.src = (const float *)ws, g.s_sy = rw, g.s_sc = (long)rw * rh, g.ix0 = rx0, g.iy0 = ry0;
            }
            timing_note_bytes(bytes);
            HLMI_LAUNCH(uc, "lb_blur_general", st, lb_blur_general, dim3((unsigned)gx, (unsigned)g.oh, (unsigned)on), dim3(256), 0, g);
            if (linear) HLMI_LAUNCH(uc, "lb_to_srgb", st, lb_to_srgb, dim3((unsigned)gx, (unsigned)g.oh, (unsigned)on), dim3(256), 0, g.dst, g.d_sy, g.d_sc, g.ow);
        }
    }
    mark_output_written(output);
    return 0;
}

}  // namespace

extern "C" int linear_blur(halide_buffer_t *input, halide_buffer_t *output) { return entry(true, input, 0, 0, output, false); }
HLMI_ENTRY(linear_blur, lb_table.md)

extern "C" int simple_blur(halide_buffer_t *input, int32_t width, int32_t height, halide_buffer_t *output) {
    return entry(false, input, width, height, output, false);
}
HLMI_ENTRY(simple_blur, sb_table.md)

// Measurement and test hook (hlmi_internal.h): the named entry point as the unfused composition, whatever the sizes.
// Its grids take one output row per workgroup row, so it refuses an output of more than 65535 rows (-6) that the one-launch path, at 32
// rows per workgroup row, accepts.
extern "C" int hlmi_linear_blur_general(const char *name, halide_buffer_t *input, int32_t width, int32_t height, halide_buffer_t *output) {
    if (name && strcmp(name, "linear_blur") == 0) return entry(true, input, 0, 0, output, true);
    if (name && strcmp(name, "simple_blur") == 0) return entry(false, input, width, height, output, true);
    return report(nullptr, halide_error_code_constraint_violated, "hlmi_linear_blur_general: no entry point named %s", name ? name : "(null)");
}
