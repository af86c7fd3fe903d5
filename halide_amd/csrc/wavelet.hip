// wavelet.hip — apps/wavelet: the one-level horizontal Haar and Daubechies-4 transforms and their inverses, f32; 4 AOT entry points
// (haar_x, inverse_haar_x, daubechies_x, inverse_daubechies_x) from one forward and one inverse kernel template.  Reference semantics:
// apps/wavelet/haar_x_generator.cpp:15-21, inverse_haar_x_generator.cpp:15-20, daubechies_x_generator.cpp:15-20,
// inverse_daubechies_x_generator.cpp:15-20, daubechies_constants.h:4-7; the contract the kernels share with the checker
// (tests/cpp/wavelet_check.c) is restated in include/hlmi_pipelines.h and DESIGN.md §5.4.  The reference's unroll(c, 2) / unroll(x, 2)
// would make Halide refuse extents below 2; here the algorithm's value is computed for every extent.
//
//   wv_fwd<DAUB>   one launch, every shape.  The forward transforms: in[x, y] -> out[x, y, c], pair x reads samples 2x - 1 .. 2x + 2.
//                  A workgroup is 4 waves, a wave owns 128 pairs of one row, a lane two adjacent pairs: one 16-byte load of
//                  in(4j .. 4j + 3), an 8-byte store to each output plane.  Daubechies takes in(4j - 1) and in(4j + 4) from the
//                  neighbouring lanes by a wave shuffle; lanes 0 and 63 load theirs, clamped.
//   wv_inv<DAUB>   the inverses: in[x, y, c] -> out[x, y], outputs 2k and 2k + 1 read pairs k and k + 1 of planes 0 and 1.  A lane owns
//                  two pairs: an 8-byte load from each plane, one 16-byte store; Daubechies takes pair k + 2 from the next lane.
//                  Both take this wide path only where the whole wave may (a wave-uniform choice): every lane's own samples lie inside
//                  the input's box, every output inside the region, and the row's addresses are aligned for the vector accesses.  Any
//                  other wave — a row's partial last wave, a region reaching past the input, an odd row stride on alternate rows —
//                  forms the same values from per-tap clamped scalar loads.
//   wv_fwd_general<DAUB>, wv_inv_general<DAUB>   hlmi_wavelet_general: one thread per output, every tap a clamped scalar load.
// Every path forms an output through fwd_value / inv_value from the same samples, so all of them agree bit for bit.
#include "hlmi_device_math.h"
#include "hlmi_internal.h"

using namespace hlmi;

namespace {

constexpr int ROWS = 4;          // rows per workgroup: one per wave
constexpr int WAVE_PAIRS = 128;  // pairs per wave: two per lane

struct WGeom {
    const float *src;        // sample (ix0, iy0[, ic0]) of the input
    long s_sy, s_sc;         // s_sc: the inverses only
    int ix0, iy0, ic0;       // the input's box: the clamp of repeat_edge
    int iw, ih, ic;          // (ic0, ic: the inverses only)
    float *dst;              // the output's first element
    long d_sy, d_sc;         // d_sc: the forwards only
    int ox, oy, oc;          // the output's region (oc, on: the forwards only)
    int ow, oh, on;
};

// daubechies_constants.h:4-7
constexpr float D0 = 0.4829629131445341f, D1 = 0.83651630373780772f, D2 = 0.22414386804201339f, D3 = -0.12940952255126034f;

// clamp(v, lo, lo + n - 1) = max(min(v, lo + n - 1), lo), as an offset from lo; n >= 1
__device__ __forceinline__ long clamp_off(long v, int lo, int n) { return max(min(v, (long)lo + n - 1), (long)lo) - lo; }

// out(x, y, c) of a forward transform from a, b, c2, d = in(2x - 1), in(2x), in(2x + 1), in(2x + 2); low: c == 0.  Haar reads b and c2
template<bool DAUB>
__device__ __forceinline__ float fwd_value(float a, float b, float c2, float d, bool low) {
    if (!DAUB) return low ? (b + c2) * 0.5f : (b - c2) * 0.5f;   // / 2 -> * 0.5f (src/Simplify_Div.cpp:204)
    return low ? dev::mad(D3, d, dev::mad(D2, c2, dev::mad2(D0, a, D1, b))) : dev::msub(dev::mad(D1, c2, dev::mulsub(D3, a, D2 * b)), D0, d);
}

// out(x, y) of an inverse from p, q, r, s = in(k, y, 0), in(k, y, 1), in(k + 1, y, 0), in(k + 1, y, 1), k = x / 2; even: x % 2 == 0
template<bool DAUB>
__device__ __forceinline__ float inv_value(float p, float q, float r, float s, bool even) {
    if (!DAUB) return even ? p + q : p - q;
    return even ? dev::mad(D3, s, dev::mad(D0, r, dev::mad2(D2, p, D1, q))) : dev::msub(dev::mad(D1, r, dev::mulsub(D3, p, D0 * q)), D2, s);
}

// forward, pair X (absolute) of the row at `row` (= its sample ix0), from clamped scalar loads
template<bool DAUB>
__device__ __forceinline__ float fwd_scalar(const WGeom &g, const float *row, long X, bool low) {
    const float b = row[clamp_off(2 * X, g.ix0, g.iw)], c2 = row[clamp_off(2 * X + 1, g.ix0, g.iw)];
    float a = 0.0f, d = 0.0f;
    if (DAUB) a = row[clamp_off(2 * X - 1, g.ix0, g.iw)], d = row[clamp_off(2 * X + 2, g.ix0, g.iw)];
    return fwd_value<DAUB>(a, b, c2, d, low);
}

// inverse, output X (absolute) of the rows at p0 and p1 (planes clamp(0) and clamp(1), their pair ix0)
template<bool DAUB>
__device__ __forceinline__ float inv_scalar(const WGeom &g, const float *p0, const float *p1, long X) {
    const long K = X >> 1;   // floor
    const long k = clamp_off(K, g.ix0, g.iw);
    float r = 0.0f, s = 0.0f;
    if (DAUB) {
        const long k1 = clamp_off(K + 1, g.ix0, g.iw);
        r = p0[k1], s = p1[k1];
    }
    return inv_value<DAUB>(p0[k], p1[k], r, s, (X & 1) == 0);
}

__device__ __forceinline__ bool aligned(const void *p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }

// ---------------------------------------------------------------------------------------------------------------- forward
template<bool DAUB>
__global__ __launch_bounds__(256) void wv_fwd(WGeom g) {
    const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const long y = (long)blockIdx.y * ROWS + wave;
    if (y >= g.oh) return;   // scalar: no barrier follows
    const long j0 = (long)blockIdx.x * WAVE_PAIRS;   // the wave's first pair, from ox
    const float *row = g.src + clamp_off((long)g.oy + y, g.iy0, g.ih) * g.s_sy;
    float *orow = g.dst + y * g.d_sy + j0;
    const long S0 = 2 * ((long)g.ox + j0);   // the wave's own samples: S0 .. S0 + 255
    const long lo = g.ix0, hi = (long)g.ix0 + g.iw - 1;
    const bool wide = j0 + WAVE_PAIRS <= g.ow && S0 >= lo && S0 + 2 * WAVE_PAIRS - 1 <= hi && aligned(row + (S0 - lo), 16);
    if (wide) {
        const float4 v = *reinterpret_cast<const float4 *>(row + (S0 - lo) + 4 * lane);
        float m = 0.0f, n = 0.0f;
        if (DAUB) {
            m = __shfl_up(v.w, 1), n = __shfl_down(v.x, 1);
            if (lane == 0) m = row[clamp_off(S0 - 1, g.ix0, g.iw)];
            if (lane == 63) n = row[clamp_off(S0 + 2 * WAVE_PAIRS, g.ix0, g.iw)];
        }
        const float2 lo2 = make_float2(fwd_value<DAUB>(m, v.x, v.y, v.z, true), fwd_value<DAUB>(v.y, v.z, v.w, n, true));
        const float2 hi2 = make_float2(fwd_value<DAUB>(m, v.x, v.y, v.z, false), fwd_value<DAUB>(v.y, v.z, v.w, n, false));
        for (int c = 0; c < g.on; c++) {
            float *p = orow + (long)c * g.d_sc + 2 * lane;
            const float2 o = (long)g.oc + c == 0 ? lo2 : hi2;
            if (aligned(orow + (long)c * g.d_sc, 8)) *reinterpret_cast<float2 *>(p) = o;
            else p[0] = o.x, p[1] = o.y;
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const long j = j0 + 2 * lane + i;
        if (j >= g.ow) break;
        const float l = fwd_scalar<DAUB>(g, row, (long)g.ox + j, true), h = fwd_scalar<DAUB>(g, row, (long)g.ox + j, false);
        for (int c = 0; c < g.on; c++) orow[(long)c * g.d_sc + 2 * lane + i] = (long)g.oc + c == 0 ? l : h;
    }
}

// ---------------------------------------------------------------------------------------------------------------- inverse
// kb: the region's first pair, floor(ox / 2); the wave's pairs are kb + j0 .. kb + j0 + 127, its outputs twice as many
template<bool DAUB>
__global__ __launch_bounds__(256) void wv_inv(WGeom g, int kb) {
    const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const long y = (long)blockIdx.y * ROWS + wave;
    if (y >= g.oh) return;
    const long K0 = (long)kb + (long)blockIdx.x * WAVE_PAIRS;
    const float *row = g.src + clamp_off((long)g.oy + y, g.iy0, g.ih) * g.s_sy;
    const float *p0 = row + clamp_off(0, g.ic0, g.ic) * g.s_sc, *p1 = row + clamp_off(1, g.ic0, g.ic) * g.s_sc;
    const long lo = g.ix0, hi = (long)g.ix0 + g.iw - 1;
    const long x_end = (long)g.ox + g.ow;
    float *orow = g.dst + y * g.d_sy;
    const bool wide = 2 * K0 >= g.ox && 2 * (K0 + WAVE_PAIRS) <= x_end && K0 >= lo && K0 + WAVE_PAIRS - 1 <= hi && aligned(p0 + (K0 - lo), 8) &&
                      aligned(p1 + (K0 - lo), 8) && aligned(orow + (2 * K0 - g.ox), 16);
    if (wide) {
        const float2 L = *reinterpret_cast<const float2 *>(p0 + (K0 - lo) + 2 * lane), H = *reinterpret_cast<const float2 *>(p1 + (K0 - lo) + 2 * lane);
        float ln = 0.0f, hn = 0.0f;
        if (DAUB) {
            ln = __shfl_down(L.x, 1), hn = __shfl_down(H.x, 1);
            if (lane == 63) {
                const long k = clamp_off(K0 + WAVE_PAIRS, g.ix0, g.iw);
                ln = p0[k], hn = p1[k];
            }
        }
        float4 o;
        o.x = inv_value<DAUB>(L.x, H.x, L.y, H.y, true), o.y = inv_value<DAUB>(L.x, H.x, L.y, H.y, false);
        o.z = inv_value<DAUB>(L.y, H.y, ln, hn, true), o.w = inv_value<DAUB>(L.y, H.y, ln, hn, false);
        *reinterpret_cast<float4 *>(orow + (2 * K0 - g.ox) + 4 * lane) = o;
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const long X = 2 * K0 + 4 * lane + i;
        if (X >= g.ox && X < x_end) orow[X - g.ox] = inv_scalar<DAUB>(g, p0, p1, X);
    }
}

// ---------------------------------------------------------------------------------------------------------------- general path
template<bool DAUB>
__global__ __launch_bounds__(256) void wv_fwd_general(WGeom g) {
    const long x = (long)blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, c = blockIdx.z;
    if (x >= g.ow) return;
    const float *row = g.src + clamp_off((long)g.oy + y, g.iy0, g.ih) * g.s_sy;
    g.dst[c * g.d_sc + y * g.d_sy + x] = fwd_scalar<DAUB>(g, row, (long)g.ox + x, (long)g.oc + c == 0);
}

template<bool DAUB>
__global__ __launch_bounds__(256) void wv_inv_general(WGeom g) {
    const long x = (long)blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= g.ow) return;
    const float *row = g.src + clamp_off((long)g.oy + y, g.iy0, g.ih) * g.s_sy;
    const float *p0 = row + clamp_off(0, g.ic0, g.ic) * g.s_sc, *p1 = row + clamp_off(1, g.ic0, g.ic) * g.s_sc;
    g.dst[y * g.d_sy + x] = inv_scalar<DAUB>(g, p0, p1, (long)g.ox + x);
}

// ---------------------------------------------------------------------------------------------------------------- host
// no estimates: the generators declare none
const ArgTable haar_table("haar_x", {in_buf("in", T_F32, 2), out_buf("out", T_F32, 3)});
const ArgTable daub_table("daubechies_x", {in_buf("in", T_F32, 2), out_buf("out", T_F32, 3)});
const ArgTable ihaar_table("inverse_haar_x", {in_buf("in", T_F32, 3), out_buf("out", T_F32, 2)});
const ArgTable idaub_table("inverse_daubechies_x", {in_buf("in", T_F32, 3), out_buf("out", T_F32, 2)});

int blocks_ok(void *uc, size_t gx, size_t gy, size_t gz) {
    if (gx <= 0x7fffffffu && gy <= 65535u && gz <= 65535u) return 0;
    return report(uc, halide_error_code_buffer_extents_too_large, "wavelet: %zu x %zu x %zu workgroups exceed one launch", gx, gy, gz);
}

int entry(bool inverse, bool daub, halide_buffer_t *in, halide_buffer_t *out, bool general_only) {
    void *uc = nullptr;
    BufArg args[2];
    (inverse ? (daub ? idaub_table : ihaar_table) : (daub ? daub_table : haar_table)).bufs(args, {in, out});
    int r = check_not_null(uc, args, 2);
    if (r) return r;
    if ((r = check_type_and_dims(uc, args, 2))) return r;
    // every read clamps into the input's own box, whatever the output's region: a bounds query leaves both buffers as passed
    if (any_bounds_query(args, 2)) return 0;
    if ((r = check_shapes(uc, args, 2))) return r;
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, 2))) return r;
    const halide_dimension_t *id = in->dim, *od = out->dim;
    WGeom g = {};
    g.ox = od[0].min, g.oy = od[1].min, g.ow = od[0].extent, g.oh = od[1].extent;
    g.oc = inverse ? 0 : od[2].min, g.on = inverse ? 1 : od[2].extent;
    if (g.ow > 0 && g.oh > 0 && g.on > 0) {   // nothing is read where the output is empty
        g.ix0 = id[0].min, g.iy0 = id[1].min, g.iw = id[0].extent, g.ih = id[1].extent;
        g.ic0 = inverse ? id[2].min : 0, g.ic = inverse ? id[2].extent : 1;
        if (g.iw <= 0 || g.ih <= 0 || g.ic <= 0) return report(uc, halide_error_code_access_out_of_bounds, "Input buffer in is empty: there is no edge to repeat");
        g.src = dev_ptr<float>(in), g.s_sy = id[1].stride, g.s_sc = inverse ? id[2].stride : 0;
        g.dst = dev_ptr<float>(out), g.d_sy = od[1].stride, g.d_sc = inverse ? 0 : od[2].stride;
        hipStream_t st = ctx.stream;
        const double bytes = 8.0 * g.ow * g.oh * g.on;   // each output value written once, as many input values read once
        if (!general_only) {
            // the inverse's waves start at the pair that holds the region's first output
            const int kb = floor_div(g.ox, 2);
            const size_t pairs = inverse ? ((size_t)g.ow + (g.ox & 1) + 1) / 2 : (size_t)g.ow;
            const size_t gx = (pairs + WAVE_PAIRS - 1) / WAVE_PAIRS, gy = ((size_t)g.oh + ROWS - 1) / ROWS;
            if ((r = blocks_ok(uc, gx, gy, 1))) return r;
            const dim3 grid((unsigned)gx, (unsigned)gy);
            timing_note_bytes(bytes);
            if (!inverse && !daub) HLMI_LAUNCH(uc, "wv_fwd", st, wv_fwd<false>, grid, dim3(256), 0, g);
            else if (!inverse) HLMI_LAUNCH(uc, "wv_fwd", st, wv_fwd<true>, grid, dim3(256), 0, g);
            else if (!daub) HLMI_LAUNCH(uc, "wv_inv", st, wv_inv<false>, grid, dim3(256), 0, g, kb);
            else HLMI_LAUNCH(uc, "wv_inv", st, wv_inv<true>, grid, dim3(256), 0, g, kb);
        } else {
            const size_t gx = ((size_t)g.ow + 255) / 256;
            if ((r = blocks_ok(uc, gx, g.oh, g.on))) return r;
            const dim3 grid((unsigned)gx, (unsigned)g.oh, (unsigned)g.on);
            timing_note_bytes(bytes);
            if (!inverse && !daub) HLMI_LAUNCH(uc, "wv_fwd_general", st, wv_fwd_general<false>, grid, dim3(256), 0, g);
            else if (!inverse) HLMI_LAUNCH(uc, "wv_fwd_general", st, wv_fwd_general<true>, grid, dim3(256), 0, g);
            else if (!daub) HLMI_LAUNCH(uc, "wv_inv_general", st, wv_inv_general<false>, grid, dim3(256), 0, g);
            else HLMI_LAUNCH(uc, "wv_inv_general", st, wv_inv_general<true>, grid, dim3(256), 0, g);
        }
    }
    mark_output_written(out);
    return 0;
}

}  // namespace

extern "C" int haar_x(halide_buffer_t *in, halide_buffer_t *out) { return entry(false, false, in, out, false); }
HLMI_ENTRY(haar_x, haar_table.md)

extern "C" int inverse_haar_x(halide_buffer_t *in, halide_buffer_t *out) { return entry(true, false, in, out, false); }
HLMI_ENTRY(inverse_haar_x, ihaar_table.md)

extern "C" int daubechies_x(halide_buffer_t *in, halide_buffer_t *out) { return entry(false, true, in, out, false); }
HLMI_ENTRY(daubechies_x, daub_table.md)

extern "C" int inverse_daubechies_x(halide_buffer_t *in, halide_buffer_t *out) { return entry(true, true, in, out, false); }
HLMI_ENTRY(inverse_daubechies_x, idaub_table.md)

// Measurement and test hook (hlmi_internal.h): the named entry point with one thread per output, whatever the sizes.  Its grids take
// one output row per workgroup row, so it refuses an output of more than 65535 rows (-6) that the default path, at 4 rows per
// workgroup row, accepts.
extern "C" int hlmi_wavelet_general(const char *name, halide_buffer_t *in, halide_buffer_t *out) {
    if (name && strcmp(name, "haar_x") == 0) return entry(false, false, in, out, true);
    if (name && strcmp(name, "inverse_haar_x") == 0) return entry(true, false, in, out, true);
    if (name && strcmp(name, "daubechies_x") == 0) return entry(false, true, in, out, true);
    if (name && strcmp(name, "inverse_daubechies_x") == 0) return entry(true, true, in, out, true);
    return report(nullptr, halide_error_code_constraint_violated, "hlmi_wavelet_general: no entry point named %s", name ? name : "(null)");
}
