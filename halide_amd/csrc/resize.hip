// resize.hip — apps/resize: separable resampling of a planar [x, y, c] image to another size with a box, linear, cubic or lanczos
// kernel, for f32, u8 and u16 elements; 24 AOT variants (4 kernels x 3 types x up / down) from one templated host shim.
// Reference semantics: apps/resize/resize_generator.cpp:12-46 (the kernels), :85-147 (the arithmetic); the contract the kernels
// share with the checker (tests/cpp/resize_check.c) is restated in DESIGN.md §5.
//
// A gather with per-output-coordinate weight tables and a non-integer stride:
//   rs_tables   one thread per output x and per output y: begin (first input coordinate of the window) and the `taps` normalised
//               weights, laid out [k][coordinate]; recomputed at every call, into the stream's scratch arena
//   rs_fused    one launch, no intermediate in HBM: a workgroup owns an output tile and keeps the first pass's result in LDS
//               (_down: y-resampled rows of the tile's input columns, then the x gather; _up: x-resampled input rows, then y)
//   rs_pass_y / rs_pass_x   the general path for any factor: two launches with the f32 intermediate in the arena; the x pass
//               stages the contiguous input span of a workgroup's outputs in LDS, or gathers from global memory where the span
//               exceeds its array (very small factors)
// Every path sums s = mad(w_k, v_k, s) from 0 in ascending k, so all of them agree bit for bit.
#include "hlmi_device_math.h"
#include "hlmi_internal.h"

#include <algorithm>
#include <math.h>
#include <stdlib.h>
#include <type_traits>

using namespace hlmi;

namespace {

enum { K_BOX = 0, K_LINEAR = 1, K_CUBIC = 2, K_LANCZOS = 3 };
__host__ __device__ constexpr int taps_of(int kind) { return kind == K_BOX ? 1 : kind == K_LINEAR ? 2 : kind == K_CUBIC ? 4 : 6; }

struct RGeom {
    int ix0, iy0, W, H;             // the input's x / y region
    int ox0, oy0, ow, oh, oc;       // the output's region (absolute coordinates) and channel count
    long in_sy, in_sc, out_sy, out_sc;
    int taps;                       // _down: ceil(T / scale_factor); _up: T (the kernels use the constant)
    float scale, inv;
    int nxb, nyb, mid_stride;       // fused path: tiles per row / column; the footprint bound (_down: LDS row stride, _up: LDS rows)
    const int *bx, *by;             // begin per output x / y
    const float *wx, *wy;           // weights [k][x], [k][y]
};

// ---------------------------------------------------------------------------------------------------------------- tables
template<int KIND>
__device__ __forceinline__ float rs_kernel(float x) {
    const float xx = fabsf(x);
    if (KIND == K_BOX) return xx <= 0.5f ? 1.0f : 0.0f;
    if (KIND == K_LINEAR) return xx < 1.0f ? 1.0f - xx : 0.0f;
    if (KIND == K_CUBIC) {
        // a = -0.5: (a + 2) xx3 - (a + 3) xx2 + 1 and a xx3 - 5a xx2 + 8a xx - 4a (:26-28), constants folded by the C++ compiler
        const float xx2 = xx * xx, xx3 = xx2 * xx;
        const float inner = dev::mulsub(1.5f, xx3, 2.5f * xx2) + 1.0f;
        const float outer = dev::mad(-4.0f, xx, dev::mulsub(-0.5f, xx3, -2.5f * xx2)) - -2.0f;
        return xx < 1.0f ? inner : (xx < 2.0f ? outer : 0.0f);
    }
    const float a = x * 3.14159265359f, b = (x / 3.0f) * 3.14159265359f;
    float value = (dev::halide_sin(a) / a) * (dev::halide_sin(b) / b);
    if (x == 0.0f) value = 1.0f;
    if (x > 3.0f || x < -3.0f) value = 0.0f;
    return value;
}

template<int KIND, bool UP>
__global__ __launch_bounds__(256) void rs_tables(RGeom g, int *__restrict__ bx, float *__restrict__ wx, int *__restrict__ by,
                                                 float *__restrict__ wy) {
    int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const bool along_y = i >= g.ow;
    if (along_y) i -= g.ow;
    const int n = along_y ? g.oh : g.ow;
    if (i >= n) return;
    const int out_min = along_y ? g.oy0 : g.ox0, in_min = along_y ? g.iy0 : g.ix0, in_extent = along_y ? g.H : g.W;
    int *begin = along_y ? by : bx;
    float *w = along_y ? wy : wx;
    const int taps = UP ? taps_of(KIND) : g.taps;
    const float kernel_scaling = UP ? 1.0f : g.scale, inverse_kernel_scaling = UP ? 1.0f : g.inv;
    const float radius = (0.5f * (float)taps_of(KIND)) * inverse_kernel_scaling;
    const float xf = (float)(out_min + i) + 0.5f;
    // begin sits under strict_float (:112-113): every operation rounded on its own in both canonical forms
    int b = (int)ceilf((xf * g.inv - 0.5f) - radius);
    b = min(b, in_min + in_extent - taps);
    b = max(b, in_min);
    begin[i] = b;
    const float source = dev::mulsub(xf, g.inv, 0.5f);
    float sum = 0.0f;
    for (int k = 0; k < taps; k++) {
        const float u = rs_kernel<KIND>(((float)(k + b) - source) * kernel_scaling);
        w[(size_t)k * n + i] = u;
        sum = sum + u;
    }
    for (int k = 0; k < taps; k++) w[(size_t)k * n + i] = w[(size_t)k * n + i] / sum;
}

// ---------------------------------------------------------------------------------------------------------------- elements
__device__ __forceinline__ float ldf(const float *p) { return *p; }
__device__ __forceinline__ float ldf(const uint8_t *p) { return (float)*p; }
__device__ __forceinline__ float ldf(const uint16_t *p) { return (float)*p; }
// :141-145: float -> clamp(v, 0, 1); integers -> saturating_cast = clamp to the type's range, then truncate toward zero
__device__ __forceinline__ void st_out(float *p, float v) { *p = dev::clampf(v, 0.0f, 1.0f); }
__device__ __forceinline__ void st_out(uint8_t *p, float v) { *p = (uint8_t)(int)dev::clampf(v, 0.0f, 255.0f); }
__device__ __forceinline__ void st_out(uint16_t *p, float v) { *p = (uint16_t)(int)dev::clampf(v, 0.0f, 65535.0f); }
// the intermediate is f32 and unclamped
template<bool FINAL, typename D>
__device__ __forceinline__ void st(D *p, float v) {
    if constexpr (FINAL) st_out(p, v);
    else *p = v;
}

// ---------------------------------------------------------------------------------------------------------------- general path
// Along y: dst(x, y, c) = sum_k wy[k][y] * src(x, by[y] + k, c); consecutive lanes on consecutive x.  _down: input -> intermediate
// [oc][oh][W]; _up: intermediate [oc][H][ow] -> output.  Row 0 of src is input row iy0 in both.
template<typename T, int KIND, bool UP>
__global__ __launch_bounds__(256) void rs_pass_y(const std::conditional_t<UP, float, T> *__restrict__ src, long s_sy, long s_sc,
                                                 std::conditional_t<UP, T, float> *__restrict__ dst, long d_sy, long d_sc, int width, RGeom g) {
    const unsigned nxb = (unsigned)(width + 255) / 256u;
    const unsigned xb = blockIdx.x % nxb, row = blockIdx.x / nxb;
    const int y = (int)(row % (unsigned)g.oh), c = (int)(row / (unsigned)g.oh);
    const int x = (int)xb * 256 + (int)threadIdx.x;
    if (x >= width) return;
    const int taps = UP ? taps_of(KIND) : g.taps;
    const auto *p = src + c * s_sc + (long)(g.by[y] - g.iy0) * s_sy + x;
    float s = 0.0f;
    for (int k = 0; k < taps; k++) s = dev::mad(g.wy[(size_t)k * g.oh + y], ldf(p + k * s_sy), s);
    st<UP>(dst + c * d_sc + (long)y * d_sy + x, s);
}

// Along x, the gather: dst(x, y, c) = sum_k wx[k][x] * src(bx[x] + k, y, c).  A workgroup owns 256 consecutive outputs of PX_ROWS
// rows and stages the span begin(first) .. begin(last) + taps of each row in LDS; a span longer than the array is gathered from
// global memory instead.  _up: input (rows = H) -> intermediate; _down: intermediate (rows = oh) -> output.  Column 0 of src is
// input column ix0 in both.
constexpr int PX_ROWS = 4, PX_LDS = 8192;
template<typename T, int KIND, bool UP>
__global__ __launch_bounds__(256) void rs_pass_x(const std::conditional_t<UP, T, float> *__restrict__ src, long s_sy, long s_sc,
                                                 std::conditional_t<UP, float, T> *__restrict__ dst, long d_sy, long d_sc, int rows, RGeom g) {
    __shared__ float s_in[PX_LDS];
    const int tid = (int)threadIdx.x;
    const unsigned nxb = (unsigned)(g.ow + 255) / 256u, nrg = (unsigned)(rows + PX_ROWS - 1) / PX_ROWS;
    const unsigned xb = blockIdx.x % nxb, t = blockIdx.x / nxb;
    const int r0 = (int)(t % nrg) * PX_ROWS, c = (int)(t / nrg);
    const int nr = min(PX_ROWS, rows - r0);
    const int taps = UP ? taps_of(KIND) : g.taps;
    const int x0 = (int)xb * 256, xl = min(x0 + 255, g.ow - 1);
    const int b0 = g.bx[x0], span = g.bx[xl] + taps - b0;
    const bool staged = span >= taps && span <= PX_LDS / PX_ROWS;   // the same for the whole workgroup
    src += c * s_sc + (long)r0 * s_sy - g.ix0;
    if (staged) {
        for (int r = 0; r < nr; r++)
            for (int i = tid; i < span; i += 256) s_in[r * span + i] = ldf(src + r * s_sy + b0 + i);
        __syncthreads();
    }
    const int x = x0 + tid;
    if (x >= g.ow) return;
    const int b = g.bx[x], off = b - b0;
    // begin is non-decreasing in x for every factor the entry checks admit; a lane whose window is not inside the span (the
    // unspecified factors of the _up variants) reads global memory, where begin's clamp keeps it in bounds
    const bool mine = staged && off >= 0 && off + taps <= span;
    float acc[PX_ROWS];
#pragma unroll
    for (int r = 0; r < PX_ROWS; r++) acc[r] = 0.0f;
    for (int k = 0; k < taps; k++) {
        const float w = g.wx[(size_t)k * g.ow + x];
#pragma unroll
        for (int r = 0; r < PX_ROWS; r++) {
            if (r < nr) acc[r] = dev::mad(w, mine ? s_in[r * span + off + k] : ldf(src + r * s_sy + b + k), acc[r]);
        }
    }
    dst += c * d_sc + (long)r0 * d_sy + x;
#pragma unroll
    for (int r = 0; r < PX_ROWS; r++) {
        if (r < nr) st<!UP>(dst + r * d_sy, acc[r]);
    }
}

// ---------------------------------------------------------------------------------------------------------------- fused path
// One workgroup of 4 waves per output tile of FT_X columns x (_down: FD_Y, _up: FU_Y) rows of one channel; wave w takes rows
// w, w + 4, ... of either step, its lanes consecutive x.  The host takes this path only where the tile's footprint is bounded by
// FUSED_LDS floats (fused_fits below).
constexpr int FT_X = 64, FD_Y = 16, FU_Y = 32, FUSED_LDS = 12288;   // at most 48 KiB of the CU's 160 (three workgroups per CU); a launch asks for its footprint only

// One y-resampled row of a _down tile: lane `i` takes columns i, i + 64, ... (NJ of them) of the span, so that a tap issues NJ
// independent loads behind one wave-uniform weight.  Columns past the span re-read its last one (no branch in the tap loop) and
// are not stored.
template<int NJ, typename T>
__device__ __forceinline__ void down_row(const T *__restrict__ p, long in_sy, const float *__restrict__ w, int oh, int taps, int span, int i,
                                         float *__restrict__ dst) {
    unsigned col[NJ];
    float acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++) col[j] = (unsigned)min(i + 64 * j, span - 1), acc[j] = 0.0f;
#pragma unroll 2
    for (int k = 0; k < taps; k++) {
        const float wk = w[(size_t)k * oh];
        const T *row = p + k * in_sy;
#pragma unroll
        for (int j = 0; j < NJ; j++) acc[j] = dev::mad(wk, ldf(row + col[j]), acc[j]);
    }
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        if (i + 64 * j < span) dst[i + 64 * j] = acc[j];
    }
}

template<typename T, int KIND, bool UP>
__global__ __launch_bounds__(256) void rs_fused(const T *__restrict__ in, T *__restrict__ out, RGeom g) {
    extern __shared__ float s_mid[];   // _up: mid_stride rows of FT_X; _down: FD_Y rows of mid_stride (the host's bound on the footprint)
    constexpr int TY = UP ? FU_Y : FD_Y;
    const int tx = (int)threadIdx.x & 63, ty = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);   // ty: the wave, uniform
    const unsigned per_c = (unsigned)g.nxb * (unsigned)g.nyb;
    const int c = (int)(blockIdx.x / per_c);
    const unsigned tile = blockIdx.x % per_c;
    const int x0 = (int)(tile % (unsigned)g.nxb) * FT_X, y0 = (int)(tile / (unsigned)g.nxb) * TY;
    const int ny = min(TY, g.oh - y0);
    const int taps = UP ? taps_of(KIND) : g.taps;
    in += c * g.in_sc;
    out += c * g.out_sc;
    const int x = x0 + tx;
    if constexpr (UP) {
        // x-resampled rows by[y0] .. by[last] + taps of the input, FT_X columns each
        const int r0 = g.by[y0];
        const int nrows = min(g.by[y0 + ny - 1] + taps - r0, g.mid_stride);
        const int xc = min(x, g.ow - 1);
        float w[taps_of(KIND)];
#pragma unroll
        for (int k = 0; k < taps_of(KIND); k++) w[k] = g.wx[(size_t)k * g.ow + xc];
        const T *p = in + (long)(r0 - g.iy0) * g.in_sy + (g.bx[xc] - g.ix0);
        for (int r = ty; r < nrows; r += 4) {
            float s = 0.0f;
#pragma unroll
            for (int k = 0; k < taps_of(KIND); k++) s = dev::mad(w[k], ldf(p + r * g.in_sy + k), s);
            s_mid[r * FT_X + tx] = s;
        }
        __syncthreads();
        if (x >= g.ow) return;
        for (int yy = ty; yy < ny; yy += 4) {
            const int y = y0 + yy;
            const float *m = s_mid + (g.by[y] - r0) * FT_X + tx;
            float s = 0.0f;
#pragma unroll
            for (int k = 0; k < taps_of(KIND); k++) s = dev::mad(g.wy[(size_t)k * g.oh + y], m[k * FT_X], s);
            st_out(out + (long)y * g.out_sy + x, s);
        }
    } else {
        // y-resampled rows of the input columns bx[x0] .. bx[last] + taps, one LDS row per output row of the tile
        const int xl = min(x0 + FT_X - 1, g.ow - 1);
        const int c0 = g.bx[x0];
        const int span = min(g.bx[xl] + taps - c0, g.mid_stride);
        for (int yy = ty; yy < ny; yy += 4) {
            const int y = y0 + yy;
            const T *p = in + (long)(g.by[y] - g.iy0) * g.in_sy + (c0 - g.ix0);
            float *dst = s_mid + yy * g.mid_stride;
            for (int base = 0; base < span; base += 256) {   // up to four columns per lane and trip, as many as the span has left
                const int left = span - base;
                if (left > 192) down_row<4>(p, g.in_sy, g.wy + y, g.oh, taps, span, base + tx, dst);
                else if (left > 128) down_row<3>(p, g.in_sy, g.wy + y, g.oh, taps, span, base + tx, dst);
                else if (left > 64) down_row<2>(p, g.in_sy, g.wy + y, g.oh, taps, span, base + tx, dst);
                else down_row<1>(p, g.in_sy, g.wy + y, g.oh, taps, span, base + tx, dst);
            }
        }
        __syncthreads();
        if (x >= g.ow) return;
        const float *m = s_mid + ty * g.mid_stride + (g.bx[x] - c0);
        constexpr int NR = FD_Y / 4;
        float acc[NR];
#pragma unroll
        for (int j = 0; j < NR; j++) acc[j] = 0.0f;
#pragma unroll 4
        for (int k = 0; k < taps; k++) {
            const float w = g.wx[(size_t)k * g.ow + x];
#pragma unroll
            for (int j = 0; j < NR; j++) acc[j] = dev::mad(w, m[j * 4 * g.mid_stride + k], acc[j]);   // rows past ny: stale LDS, not stored
        }
#pragma unroll
        for (int j = 0; j < NR; j++) {
            const int y = y0 + ty + 4 * j;
            if (y < g.oh) st_out(out + (long)y * g.out_sy + x, acc[j]);
        }
    }
}

// The footprint of a fused tile along the gathered axis: n outputs whose source coordinates advance by `inv` start their windows
// within ceil(n * inv) of each other, the last window adds `taps`, and 3 more cover begin's ceil and the rounding of the source
// coordinates, which stays below 1 while the coordinates times `inv` stay below 2^21 (two f32 roundings of 2^-24 relative each).
// Outside that range, or where the footprint exceeds FUSED_LDS floats, the general path runs.
bool fused_fits(const RGeom &g, bool up, int *mid_stride) {
    const long reach_x = std::max(labs((long)g.ox0), labs((long)g.ox0 + g.ow)), reach_y = std::max(labs((long)g.oy0), labs((long)g.oy0 + g.oh));
    const float reach = (float)(std::max(reach_x, reach_y) + 1);
    if (!(g.inv > 0.0f && reach * g.inv < 2097152.0f)) return false;
    const long foot = (long)ceilf((float)(up ? FU_Y : FT_X) * g.inv) + g.taps + 3;   // _up: LDS rows of FT_X; _down: columns of each of FD_Y rows
    *mid_stride = (int)foot;
    return foot * (up ? FT_X : FD_Y) <= FUSED_LDS;
}

template<typename T> constexpr uint32_t abi_of();
template<> constexpr uint32_t abi_of<float>() { return T_F32; }
template<> constexpr uint32_t abi_of<uint8_t>() { return T_U8; }
template<> constexpr uint32_t abi_of<uint16_t>() { return T_U16; }

// one table per element type, shared by the eight variants of that type; no estimates: the generator sets none
template<typename T>
const ArgTable &rs_table() {
    static const ArgTable t("resize", {in_buf("input", abi_of<T>(), 3), scalar_f32("scale_factor"), out_buf("output", abi_of<T>(), 3)});
    return t;
}

template<typename T, int KIND, bool UP>
int resize_entry(halide_buffer_t *input, float scale_factor, halide_buffer_t *output, bool general_only) {
    void *uc = nullptr;
    BufArg args[2];
    rs_table<T>().bufs(args, {input, output});
    int r = check_not_null(uc, args, 2);
    if (r) return r;
    if ((r = check_type_and_dims(uc, args, 2))) return r;
    if (any_bounds_query(args, 2)) {
        // the output's region is the request and stays as passed; the windows are clamped to the input's own x / y extents
        // (:114-115), so those stay as passed too, and the input needs the output's channels
        int mins[3] = {input->dim[0].min, input->dim[1].min, output->dim[2].min};
        int ext[3] = {input->dim[0].extent, input->dim[1].extent, output->dim[2].extent};
        answer_query(input, mins, ext);
        return 0;
    }
    if ((r = check_shapes(uc, args, 2))) return r;
    RGeom g;
    g.ix0 = input->dim[0].min, g.iy0 = input->dim[1].min, g.W = input->dim[0].extent, g.H = input->dim[1].extent;
    g.ox0 = output->dim[0].min, g.oy0 = output->dim[1].min, g.ow = output->dim[0].extent, g.oh = output->dim[1].extent;
    g.oc = output->dim[2].extent;
    if ((r = check_covers(uc, args[0], 2, output->dim[2].min, g.oc))) return r;
    // one correctly rounded division (:92); the window of `taps` inputs must fit the input, or its clamp would leave it
    g.scale = scale_factor, g.inv = 1.0f / scale_factor;
    const float taps_f = ceilf((float)taps_of(KIND) * (UP ? 1.0f : g.inv));
    if (!(taps_f >= 1.0f && taps_f <= (float)g.W && taps_f <= (float)g.H)) {
        return report(uc, halide_error_code_access_out_of_bounds,
                      "Input buffer input: the %g-tap window of scale_factor %g does not fit its extents %d x %d", (double)taps_f,
                      (double)scale_factor, g.W, g.H);
    }
    g.taps = (int)taps_f;
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, 2))) return r;
    if (g.ow > 0 && g.oh > 0 && g.oc > 0) {
        g.in_sy = input->dim[1].stride, g.in_sc = input->dim[2].stride;
        g.out_sy = output->dim[1].stride, g.out_sc = output->dim[2].stride;
        g.nxb = g.nyb = g.mid_stride = 0;
        const bool fused = fused_fits(g, UP, &g.mid_stride) && !general_only;
        // arena: bx | by | wx | wy | the general path's intermediate (_up: [oc][H][ow], _down: [oc][oh][W])
        auto pad = [](size_t n) { return (n + 63) & ~(size_t)63; };
        const size_t n_bx = pad(g.ow), n_by = pad(g.oh), n_wx = pad((size_t)g.taps * g.ow), n_wy = pad((size_t)g.taps * g.oh);
        const size_t mid_w = UP ? g.ow : g.W, mid_h = UP ? g.H : g.oh;
        const size_t n_mid = fused ? 0 : (size_t)g.oc * mid_w * mid_h;
        void *ws = nullptr;
        if ((r = get_workspace(uc, ctx, 4 * (n_bx + n_by + n_wx + n_wy + n_mid), &ws))) return r;
        int *bx = (int *)ws, *by = bx + n_bx;
        float *wx = (float *)(by + n_by), *wy = wx + n_wx, *mid = wy + n_wy;
        g.bx = bx, g.by = by, g.wx = wx, g.wy = wy;
        hipStream_t st = ctx.stream;
        const T *din = dev_ptr<T>(input) + (long)(output->dim[2].min - input->dim[2].min) * g.in_sc;
        T *dout = dev_ptr<T>(output);
        HLMI_LAUNCH(uc, "rs_tables", st, (rs_tables<KIND, UP>), dim3((unsigned)(((long)g.ow + g.oh + 255) / 256)), dim3(256), 0, g, bx, wx, by, wy);
        const double bytes = sizeof(T) * ((double)g.W * g.H + (double)g.ow * g.oh) * g.oc;   // input read once + output written once
        auto blocks = [&](size_t n) -> int { return n <= 0x7fffffffu ? 0 : report(uc, halide_error_code_buffer_extents_too_large, "resize: %zu workgroups exceed one launch", n); };
        if (fused) {
            g.nxb = (g.ow + FT_X - 1) / FT_X, g.nyb = (g.oh + (UP ? FU_Y : FD_Y) - 1) / (UP ? FU_Y : FD_Y);
            const size_t nb = (size_t)g.nxb * g.nyb * g.oc;
            if ((r = blocks(nb))) return r;
            timing_note_bytes(bytes);
            HLMI_LAUNCH(uc, "rs_fused", st, (rs_fused<T, KIND, UP>), dim3((unsigned)nb), dim3(256), sizeof(float) * g.mid_stride * (UP ? FT_X : FD_Y), din, dout, g);
        } else if constexpr (UP) {
            const size_t nbx = (size_t)((g.ow + 255) / 256) * ((g.H + PX_ROWS - 1) / PX_ROWS) * g.oc;
            const size_t nby = (size_t)((g.ow + 255) / 256) * g.oh * g.oc;
            if ((r = blocks(nbx)) || (r = blocks(nby))) return r;
            timing_note_bytes(bytes);
            HLMI_LAUNCH(uc, "rs_pass_x", st, (rs_pass_x<T, KIND, UP>), dim3((unsigned)nbx), dim3(256), 0, din, g.in_sy, g.in_sc, mid, (long)mid_w,
                        (long)(mid_w * mid_h), g.H, g);
            HLMI_LAUNCH(uc, "rs_pass_y", st, (rs_pass_y<T, KIND, UP>), dim3((unsigned)nby), dim3(256), 0, mid, (long)mid_w, (long)(mid_w * mid_h), dout,
                        g.out_sy, g.out_sc, g.ow, g);
        } else {
            const size_t nby = (size_t)((g.W + 255) / 256) * g.oh * g.oc;
            const size_t nbx = (size_t)((g.ow + 255) / 256) * ((g.oh + PX_ROWS - 1) / PX_ROWS) * g.oc;
            if ((r = blocks(nbx)) || (r = blocks(nby))) return r;
            timing_note_bytes(bytes);
            HLMI_LAUNCH(uc, "rs_pass_y", st, (rs_pass_y<T, KIND, UP>), dim3((unsigned)nby), dim3(256), 0, din, g.in_sy, g.in_sc, mid, (long)mid_w,
                        (long)(mid_w * mid_h), g.W, g);
            HLMI_LAUNCH(uc, "rs_pass_x", st, (rs_pass_x<T, KIND, UP>), dim3((unsigned)nbx), dim3(256), 0, mid, (long)mid_w, (long)(mid_w * mid_h), dout,
                        g.out_sy, g.out_sc, g.oh, g);
        }
    }
    mark_output_written(output);
    return 0;
}

using float32 = float;
using uint8 = uint8_t;
using uint16 = uint16_t;

struct Variant {
    const char *name;
    int (*general)(halide_buffer_t *, float, halide_buffer_t *);
};

}  // namespace

#define RS_VARIANT(kname, KIND, tname, dname, UP)                                                                                     \
    namespace {                                                                                                                       \
    const halide_filter_metadata_t rs_md_##kname##_##tname##_##dname = rs_table<tname>().named("resize_" #kname "_" #tname "_" #dname); \
    int rs_general_##kname##_##tname##_##dname(halide_buffer_t *i, float s, halide_buffer_t *o) {                                     \
        return resize_entry<tname, KIND, UP>(i, s, o, true);                                                                          \
    }                                                                                                                                 \
    }                                                                                                                                 \
    extern "C" int resize_##kname##_##tname##_##dname(halide_buffer_t *input, float scale_factor, halide_buffer_t *output) {          \
        return resize_entry<tname, KIND, UP>(input, scale_factor, output, false);                                                     \
    }                                                                                                                                 \
    HLMI_ENTRY(resize_##kname##_##tname##_##dname, rs_md_##kname##_##tname##_##dname)
#define RS_TYPES(kname, KIND)                \
    RS_VARIANT(kname, KIND, float32, up, true)    \
    RS_VARIANT(kname, KIND, float32, down, false) \
    RS_VARIANT(kname, KIND, uint8, up, true)      \
    RS_VARIANT(kname, KIND, uint8, down, false)   \
    RS_VARIANT(kname, KIND, uint16, up, true)     \
    RS_VARIANT(kname, KIND, uint16, down, false)
RS_TYPES(box, K_BOX)
RS_TYPES(linear, K_LINEAR)
RS_TYPES(cubic, K_CUBIC)
RS_TYPES(lanczos, K_LANCZOS)

// Measurement and test hook (hlmi_internal.h): the named variant on the general two-launch path, whatever the sizes.
#define RS_ROW(kname, tname, dname) {"resize_" #kname "_" #tname "_" #dname, rs_general_##kname##_##tname##_##dname},
#define RS_ROWS(kname) \
    RS_ROW(kname, float32, up) RS_ROW(kname, float32, down) RS_ROW(kname, uint8, up) RS_ROW(kname, uint8, down) RS_ROW(kname, uint16, up) RS_ROW(kname, uint16, down)
extern "C" int hlmi_resize_general(const char *variant, halide_buffer_t *input, float scale_factor, halide_buffer_t *output) {
    static const Variant table[24] = {RS_ROWS(box) RS_ROWS(linear) RS_ROWS(cubic) RS_ROWS(lanczos)};
    for (const Variant &v : table)
        if (variant && strcmp(v.name, variant) == 0) return v.general(input, scale_factor, output);
    return report(nullptr, halide_error_code_constraint_violated, "hlmi_resize_general: no variant named %s", variant ? variant : "(null)");
}
