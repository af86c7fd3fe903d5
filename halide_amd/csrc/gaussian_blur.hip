// gaussian_blur.hip — apps/gaussian_blur: a Gaussian blur of a chosen sigma truncated at `trunc` sigmas, f32 [x, y]:
// gaussian_blur_direct, the separable blur itself, and the 36 variants gaussian_blur_<U>_<D>_<F> that reduce by F with an order-D
// box spline, blur at low resolution with a corrected sigma and expand by F with an order-U box spline; 37 AOT entry points, the
// 36 from one templated host shim.  Reference semantics: apps/gaussian_blur/gaussian_blur_generator.cpp:18-63 (the blur), :117-150
// (the splines), :160-214 (the resampled pipeline), :344-347 (its constraints); the contract the kernels share with the checker
// (tests/cpp/gaussian_blur_check.c) is restated in DESIGN.md §5.2.
//
//   gb_tables     one workgroup: kernel(x) = halide_exp(-(x x) / (2 sigma sigma)) on [-R, R], its sum by ONE lane in ascending x, the
//                 normalised table kn[] into the stream's scratch arena; at every call
//   gb_blur_y     blur_y on the source's columns x the output's rows (f32, arena): lanes on consecutive x, a thread owns 16 (or 4)
//                 consecutive output rows in registers and walks the source rows once, ascending, a batch of loads ahead
//   gb_blur_x     a wave stages row spans of 256 + 2 R columns in LDS; a lane owns 4 consecutive outputs of 4 rows (or 1) and slides
//                 over the spans with one 16-byte LDS read per row and 4 taps (16 fused operations per read)
//   gb_blur_y_general / gb_blur_x_general   one thread per output, every tap from global memory with its clamp: any radius; what
//                 hlmi_gaussian_blur_general forces, what the x pass takes when its spans exceed 64 KiB of LDS, and what a blur of
//                 too few pixels to fill the device with tiles takes
//   gb_down       down_y (in phases) for 256 full-resolution columns x 4 low-resolution rows into LDS, then the down_x gather
//   gb_up         a thread owns an output column and 16 rows, keeps the U rows of up_x it needs in registers
// Every sum runs s = mad(w_r, v_r, s) from 0 in ascending r on every path, so all of them agree bit for bit.
#include "hlmi_device_math.h"
#include "hlmi_internal.h"

#include <math.h>
#include <stdlib.h>

using namespace hlmi;

namespace {

// One separable blur: the source's rows and columns clamp to [0, sh) x [0, sw); the output region is in the source's coordinates.
struct BGeom {
    const float *src;
    long s_sy;
    int sw, sh;
    float *mid;        // blur_y: [oh][sw]
    float *dst;
    long d_sy;
    int x0, y0, ow, oh;
    int radius;
    const float *kn;   // 2 radius + 1 normalised weights
};

// ---------------------------------------------------------------------------------------------------------------- tables
constexpr int TB_CHUNK = 2048;
__global__ __launch_bounds__(256) void gb_tables(float sigma, int radius, float *__restrict__ kn) {
    __shared__ float s_k[TB_CHUNK];
    __shared__ float s_sum;
    const int tid = (int)threadIdx.x, n = 2 * radius + 1;
    const float denom = (2.0f * sigma) * sigma;
    float sum = 0.0f;   // lane 0's
    for (int base = 0; base < n; base += TB_CHUNK) {
        const int m = min(TB_CHUNK, n - base);
        for (int i = tid; i < m; i += 256) {
            const int x = base + i - radius;
            const float k = dev::halide_exp((float)(int)(0u - (unsigned)x * (unsigned)x) / denom);   // -(x * x) in wrapping int32
            s_k[i] = k;
            kn[base + i] = k;
        }
        __syncthreads();
        if (tid == 0)
            for (int i = 0; i < m; i++) sum = sum + s_k[i];
        __syncthreads();
    }
    if (tid == 0) s_sum = sum;
    __syncthreads();
    const float total = s_sum;
    for (int i = tid; i < n; i += 256) kn[i] = kn[i] / total;   // each thread divides what it wrote itself
}

// ---------------------------------------------------------------------------------------------------------------- general path
__global__ __launch_bounds__(256) void gb_blur_y_general(BGeom g) {
    const int x = (int)blockIdx.x * 256 + (int)threadIdx.x, y = (int)blockIdx.y;
    if (x >= g.sw) return;
    const float *p = g.src + x;
    float s = 0.0f;
    for (int r = -g.radius; r <= g.radius; r++) s = dev::mad(g.kn[r + g.radius], p[(long)dev::clampi(g.y0 + y + r, 0, g.sh - 1) * g.s_sy], s);
    g.mid[(size_t)y * g.sw + x] = s;
}

__global__ __launch_bounds__(256) void gb_blur_x_general(BGeom g) {
    const int x = (int)blockIdx.x * 256 + (int)threadIdx.x, y = (int)blockIdx.y;
    if (x >= g.ow) return;
    const float *p = g.mid + (size_t)y * g.sw;
    float s = 0.0f;
    for (int r = -g.radius; r <= g.radius; r++) s = dev::mad(g.kn[r + g.radius], p[dev::clampi(g.x0 + x + r, 0, g.sw - 1)], s);
    g.dst[(long)y * g.d_sy + x] = s;
}

// ---------------------------------------------------------------------------------------------------------------- tiled path
// A value v at position t of a walk (source row or span column) belongs to tap k = t - j of output j; with N outputs per thread
// the walk has N + 2 R positions.  Positions N - 1 .. 2 R feed every output (`whole`); at the others the tap is computed with a
// clamped weight and kept only where k is a tap: a select, not a branch — a branch per tap would wait for its own weight load.
// t, j and k are wave-uniform, so the weights are scalar loads.
template<int N, bool WHOLE>
__device__ __forceinline__ void taps(float (&acc)[N], const float *__restrict__ kn, int t, int last, float v) {
#pragma unroll
    for (int j = 0; j < N; j++) {
        const int k = t - j;
        if (WHOLE) {
            acc[j] = dev::mad(kn[k], v, acc[j]);
        } else {
            const float s = dev::mad(kn[dev::clampi(k, 0, last)], v, acc[j]);
            acc[j] = (k >= 0 && k <= last) ? s : acc[j];
        }
    }
}

// RY output rows per thread (16, or 4 where 16 would leave the device short of workgroups).  The walk goes in batches of BY_BATCH
// source rows: the next batch's loads are issued before the current batch's taps, so that a load's latency hides behind them.
constexpr int BY_BATCH = 8;
template<int RY>
__global__ __launch_bounds__(256) void gb_blur_y(BGeom g) {
    const int x = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const int yb = (int)blockIdx.y * RY;
    const float *p = g.src + min(x, g.sw - 1);   // lanes past the source re-read its last column and store nothing
    const int last = 2 * g.radius, T = RY + last;
    const int top = g.y0 + yb - g.radius;        // source row of walk position 0
    float acc[RY];
#pragma unroll
    for (int j = 0; j < RY; j++) acc[j] = 0.0f;
    auto load = [&](float (&v)[BY_BATCH], int t0) {   // positions past the walk read clamped rows and feed no tap
#pragma unroll
        for (int i = 0; i < BY_BATCH; i++) v[i] = p[(long)dev::clampi(top + t0 + i, 0, g.sh - 1) * g.s_sy];
    };
    float cur[BY_BATCH], nxt[BY_BATCH];
    load(cur, 0);
    for (int t0 = 0; t0 < T; t0 += BY_BATCH) {
        load(nxt, t0 + BY_BATCH);
        if (t0 >= RY - 1 && t0 + BY_BATCH - 1 <= last) {
#pragma unroll
            for (int i = 0; i < BY_BATCH; i++) taps<RY, true>(acc, g.kn, t0 + i, last, cur[i]);
        } else {
#pragma unroll
            for (int i = 0; i < BY_BATCH; i++) taps<RY, false>(acc, g.kn, t0 + i, last, cur[i]);
        }
#pragma unroll
        for (int i = 0; i < BY_BATCH; i++) cur[i] = nxt[i];
    }
    if (x >= g.sw) return;
#pragma unroll
    for (int j = 0; j < RY; j++) {
        if (yb + j < g.oh) g.mid[(size_t)(yb + j) * g.sw + x] = acc[j];
    }
}

// RW rows per wave (4, or 1 where 4 would leave the device short of workgroups or the spans would not fit), 256 outputs per row:
// span position i of a row holds blur_y at source column clamp(x0 + xb 256 - R + i); lane l owns outputs 4 l .. 4 l + 3 of each of
// its wave's rows and reads positions 4 l + 4 m .. + 3 as one float4, the weights of a step shared by the RW rows.  The results go
// back through the (then free) spans so that the stores are lane-consecutive.
constexpr int BX_LDS_FLOATS = 16384;   // 64 KiB
__device__ __host__ constexpr int bx_span(int radius) { return (256 + 2 * radius + 7) & ~3; }   // >= 256 + 2 R + 4, a multiple of 4 floats
template<int RW>
__global__ __launch_bounds__(256) void gb_blur_x(BGeom g) {
    extern __shared__ float4 s_span4[];
    const int lane = (int)threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int span = bx_span(g.radius);
    float *s_rows = reinterpret_cast<float *>(s_span4) + w * RW * span;
    const int xb = (int)blockIdx.x * 256, yw = ((int)blockIdx.y * 4 + w) * RW;
    const int left = g.x0 + xb - g.radius;
#pragma unroll
    for (int r = 0; r < RW; r++) {
        const float *p = g.mid + (size_t)min(yw + r, g.oh - 1) * g.sw;   // a row past the last repeats it and is not stored
        for (int i = lane; i < span; i += 64) s_rows[r * span + i] = p[dev::clampi(left + i, 0, g.sw - 1)];
    }
    __syncthreads();
    const int last = 2 * g.radius, M = (last + 4 + 3) / 4;   // float4 steps that hold a tap of this lane's outputs
    float acc[RW][4];
#pragma unroll
    for (int r = 0; r < RW; r++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[r][j] = 0.0f;
    auto step = [&](int m, auto whole) {
        float4 v[RW];
#pragma unroll
        for (int r = 0; r < RW; r++) v[r] = reinterpret_cast<const float4 *>(s_rows + r * span)[lane + m];
#pragma unroll
        for (int r = 0; r < RW; r++) {
            taps<4, decltype(whole)::value>(acc[r], g.kn, 4 * m, last, v[r].x);
            taps<4, decltype(whole)::value>(acc[r], g.kn, 4 * m + 1, last, v[r].y);
            taps<4, decltype(whole)::value>(acc[r], g.kn, 4 * m + 2, last, v[r].z);
            taps<4, decltype(whole)::value>(acc[r], g.kn, 4 * m + 3, last, v[r].w);
        }
    };
    // step m is whole when 4 m - 3 >= 0 and 4 m + 3 <= 2 R
    const int m_whole_end = (last - 3 >= 0) ? (last - 3) / 4 : -1;
    int m = 0;
    for (; m < min(1, M); m++) step(m, std::false_type{});
#pragma unroll 2
    for (; m <= m_whole_end; m++) step(m, std::true_type{});
    for (; m < M; m++) step(m, std::false_type{});
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RW; r++) reinterpret_cast<float4 *>(s_rows + r * span)[lane] = make_float4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RW; r++) {
        if (yw + r >= g.oh) break;
        float *o = g.dst + (long)(yw + r) * g.d_sy + xb;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (xb + 64 * j + lane < g.ow) o[64 * j + lane] = s_rows[r * span + 64 * j + lane];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- resampling
// make_resampling_kernel (:117-150) in f32, as the generator evaluates it: every value is a dyadic rational with a numerator
// below 2^12, so every operation is exact.  k[0 .. order * F).
constexpr int RK_DOM = 256, RK_OFF = 96;
void resampling_kernel(int order, int F, float *k) {
    float box[RK_DOM], cur[RK_DOM], next[RK_DOM];
    for (int i = 0; i < RK_DOM; i++) box[i] = (i - RK_OFF >= 0 && i - RK_OFF < F) ? 1.0f / (float)F : 0.0f;
    memcpy(cur, box, sizeof cur);
    for (int i = 1; i < order; i++) {
        for (int x = 0; x < RK_DOM; x++) {
            float s = 0.0f;
            for (int r = 0; r < F; r++) s = s + (x - r >= 0 ? cur[x - r] : 0.0f) * box[r + RK_OFF];
            next[x] = s;
        }
        for (int x = 0; x < RK_DOM; x++) cur[x] = (next[x] + (x >= 1 ? next[x - 1] : 0.0f)) * 0.5f;
    }
    for (int x = 0; x < order * F; x++) k[x] = cur[x + RK_OFF];
}
float resampling_variance(int order, int F) {
    float variance = (float)order * ((float)F * (float)F - 1.0f) / 12.0f;
    variance += (float)(order - 1) / 4.0f;
    return variance;
}

struct DownTab { float k[48]; };   // dk[rf + p F]
struct UpTab { float c[64]; };     // c(i, p) = uk[i F + p] * F at [i F + p]

struct RGeom {
    const float *in;
    long in_sy;
    int ix0, iy0, W, H;       // the input's region, absolute
    int shift;
    float *lo;                // down_x on columns [lx0, lx0 + lw) x rows [ly0, ly0 + lh), dense
    int lx0, ly0, lw, lh;
    const float *bl;          // blurred on columns [bx0, bx0 + bw) x rows [by0, ...), dense
    int bx0, by0, bw;
    float *out;
    long out_sy;
    int ow, oh;
};

// A workgroup owns DN_COLS(F, D) low-resolution columns x DN_ROWS rows.  Thread i takes position i of the 256 full-resolution
// columns F xl0 + shift + i the tile's gathers read (clamped to the input's columns when loading), walks the DN_ROWS + D - 1 groups
// of F input rows once, ascending, and adds group g's phase p to row g - p: for a row that is p = 0, 1, ... in ascending order.
// Position i sits at LDS index i + i / 32, which keeps the gather's stride-F reads on distinct banks for every F.
constexpr int DN_ROWS = 4, DN_LDS = 256 + 8;
__host__ __device__ constexpr int dn_cols(int F, int D) { return 256 / F - (D - 1); }
template<int F, int D>
__global__ __launch_bounds__(256) void gb_down(RGeom g, DownTab tab) {
    __shared__ float s_dy[DN_ROWS][DN_LDS];
    const int tid = (int)threadIdx.x;
    const int xl0 = g.lx0 + (int)blockIdx.x * dn_cols(F, D), yl0 = g.ly0 + (int)blockIdx.y * DN_ROWS;
    const float *p = g.in + (dev::clampi(F * xl0 + g.shift + tid, g.ix0, g.ix0 + g.W - 1) - g.ix0);
    float acc[DN_ROWS];
#pragma unroll
    for (int j = 0; j < DN_ROWS; j++) acc[j] = 0.0f;
#pragma unroll
    for (int grp = 0; grp < DN_ROWS + D - 1; grp++) {
        float ph[D];
#pragma unroll
        for (int q = 0; q < D; q++) ph[q] = 0.0f;
#pragma unroll
        for (int rf = 0; rf < F; rf++) {
            const int y = dev::clampi(F * (yl0 + grp) + rf + g.shift, g.iy0, g.iy0 + g.H - 1);
            const float v = p[(long)(y - g.iy0) * g.in_sy];
#pragma unroll
            for (int q = 0; q < D; q++) ph[q] = dev::mad(v, tab.k[rf + q * F], ph[q]);
        }
#pragma unroll
        for (int q = 0; q < D; q++) {
            if (grp - q >= 0 && grp - q < DN_ROWS) acc[grp - q] = acc[grp - q] + ph[q];
        }
    }
#pragma unroll
    for (int j = 0; j < DN_ROWS; j++) s_dy[j][tid + (tid >> 5)] = acc[j];
    __syncthreads();
    constexpr int NC = dn_cols(F, D);
    for (int o = tid; o < NC * DN_ROWS; o += 256) {
        const int c = o % NC, j = o / NC;
        const int xl = xl0 + c, yl = yl0 + j;
        if (xl >= g.lx0 + g.lw || yl >= g.ly0 + g.lh) continue;
        float s = 0.0f;
#pragma unroll
        for (int rx = 0; rx < F * D; rx++) {
            const int i = F * c + rx;
            s = dev::mad(s_dy[j][i + (i >> 5)], tab.k[rx], s);
        }
        g.lo[(size_t)(yl - g.ly0) * g.lw + (xl - g.lx0)] = s;
    }
}

// e = t_0 + t_1 + ... with the leading 0.f folded away (the checker's header): the first add contracts its first product
template<int U>
__device__ __forceinline__ float expand(const float (&v)[U], const float (&c)[U]) {
    float e = dev::mad2(v[0], c[0], v[1], c[1]);
#pragma unroll
    for (int i = 2; i < U; i++) e = dev::mad(v[i], c[i], e);
    return e;
}

constexpr int UP_ROWS = 16;   // a multiple of every F
template<int F, int U>
__global__ __launch_bounds__(256) void gb_up(RGeom g, UpTab tab) {
    const int x = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (x >= g.ow) return;
    const int xl = x / F, px = x % F;   // x >= 0
    float cx[U];
#pragma unroll
    for (int i = 0; i < U; i++) cx[i] = tab.c[i * F + px];
    const int y0 = (int)blockIdx.y * UP_ROWS, yl0 = y0 / F;
    const float *b = g.bl + (xl - g.bx0);
    auto up_x = [&](int yl) {
        const float *row = b + (size_t)(yl - g.by0) * g.bw;
        float v[U];
#pragma unroll
        for (int i = 0; i < U; i++) v[i] = row[-i];
        return expand<U>(v, cx);
    };
    float win[U];   // win[i] = up_x(x, yl - i)
#pragma unroll
    for (int i = 1; i < U; i++) win[i] = up_x(yl0 - i);
    float *o = g.out + x;
#pragma unroll
    for (int k = 0; k < UP_ROWS / F; k++) {
        if (y0 + k * F >= g.oh) break;   // scalar
        win[0] = up_x(yl0 + k);
#pragma unroll
        for (int py = 0; py < F; py++) {
            const int y = y0 + k * F + py;
            float cy[U];
#pragma unroll
            for (int i = 0; i < U; i++) cy[i] = tab.c[i * F + py];
            if (y < g.oh) o[(long)y * g.out_sy] = expand<U>(win, cy);
        }
#pragma unroll
        for (int i = U - 1; i >= 1; i--) win[i] = win[i - 1];
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
constexpr int MAX_RADIUS = (1 << 30) - 1;   // 2 R + 1 stays an int; the arena decides long before

// no estimates and no ranges: the generator declares none
const ArgTable gb_table("gaussian_blur_direct", {in_buf("input", T_F32, 2), scalar_f32("sigma"), scalar_i32("trunc"), out_buf("output", T_F32, 2)});

int check_scalars(void *uc, float sigma, int32_t trunc) {
    // the algorithm has no answer there: a NaN table, or an empty sum divided by itself
    if (!(sigma > 0.0f && sigma <= 3.402823466e38f)) return report(uc, halide_error_code_param_too_small, "Parameter sigma is %g but must be finite and greater than 0", (double)sigma);
    if (trunc < 0) return report(uc, halide_error_code_param_too_small, "Parameter trunc is %d but must be at least 0", (int)trunc);
    return 0;
}

size_t pad(size_t n) { return (n + 63) & ~(size_t)63; }

// radius = (int)ceil((float)trunc * sigma), or -11 where no table of that size can exist
int radius_of(void *uc, float sigma, int32_t trunc, int *radius) {
    const float rf = ceilf((float)trunc * sigma);
    if (!(rf <= (float)MAX_RADIUS)) return report(uc, halide_error_code_out_of_memory, "gaussian_blur: a radius of %g taps exceeds any table", (double)rf);
    *radius = (int)rf;
    return 0;
}

int workspace(void *uc, const DeviceCtx &ctx, size_t floats, void **ws) {
    const size_t bytes = 4 * floats;
    if (bytes > ((size_t)1 << 30)) {   // rare: ask the device before the arena tries
        size_t free_b = 0, total_b = 0;
        HLMI_HIP(uc, hipMemGetInfo(&free_b, &total_b));
        if (bytes > free_b) return report(uc, halide_error_code_out_of_memory, "gaussian_blur: %zu bytes of tables and intermediates exceed the device's %zu free", bytes, free_b);
    }
    return get_workspace(uc, ctx, bytes, ws);
}

int blocks_ok(void *uc, size_t gx, size_t gy) {
    if (gx <= 0x7fffffffu && gy <= 65535u) return 0;
    return report(uc, halide_error_code_buffer_extents_too_large, "gaussian_blur: %zu x %zu workgroups exceed one launch", gx, gy);
}

// tables + the two passes of one blur; g.kn and g.mid are set.  Which kernels run is a matter of speed only.  By size: a pass takes its
// larger tile where that still makes TILE_BLOCKS_BIG workgroups, its smaller one where that makes TILE_BLOCKS_SMALL, and the
// general kernel otherwise (the low-resolution blur of a large factor is a few hundred pixels a side).  HLMI_GB_TILE overrides it for
// the tests: 16 / 4 = the larger / smaller tile whatever the size (the x pass still needs its spans to fit), 0 = general.
constexpr size_t TILE_BLOCKS_BIG = 768, TILE_BLOCKS_SMALL = 256;
int run_blur(void *uc, hipStream_t st, const BGeom &g, float sigma, bool general_only) {
    int r;
    HLMI_LAUNCH(uc, "gb_tables", st, gb_tables, dim3(1), dim3(256), 0, sigma, g.radius, const_cast<float *>(g.kn));
    const int forced = general_only ? 0 : env_int("HLMI_GB_TILE").value_or(-1);
    const size_t gx_mid = (g.sw + 255) / 256, gx_out = (g.ow + 255) / 256, span = bx_span(g.radius);
    auto rows = [&](int per) { return (size_t)(g.oh + per - 1) / per; };
    // the grid's y is a row or a group of rows: more than 65535 of them are not supported (-6)
    const int ry = forced >= 0 ? forced : gx_mid * rows(16) >= TILE_BLOCKS_BIG ? 16 : gx_mid * rows(4) >= TILE_BLOCKS_SMALL ? 4 : 0;
    int rw = forced >= 0 ? forced / 4 : gx_out * rows(16) >= TILE_BLOCKS_BIG ? 4 : gx_out * rows(4) >= TILE_BLOCKS_SMALL ? 1 : 0;
    if (rw == 4 && 16 * span > BX_LDS_FLOATS) rw = 1;
    if (rw == 1 && 4 * span > BX_LDS_FLOATS) rw = 0;
    if ((r = blocks_ok(uc, gx_mid, rows(ry ? ry : 1))) || (r = blocks_ok(uc, gx_out, rows(rw ? 4 * rw : 1)))) return r;
    if (ry == 16) HLMI_LAUNCH(uc, "gb_blur_y", st, gb_blur_y<16>, dim3(gx_mid, rows(16)), dim3(256), 0, g);
    else if (ry == 4) HLMI_LAUNCH(uc, "gb_blur_y", st, gb_blur_y<4>, dim3(gx_mid, rows(4)), dim3(256), 0, g);
    else HLMI_LAUNCH(uc, "gb_blur_y_general", st, gb_blur_y_general, dim3(gx_mid, g.oh), dim3(256), 0, g);
    if (rw == 4) HLMI_LAUNCH(uc, "gb_blur_x", st, gb_blur_x<4>, dim3(gx_out, rows(16)), dim3(256), sizeof(float) * 16 * span, g);
    else if (rw == 1) HLMI_LAUNCH(uc, "gb_blur_x", st, gb_blur_x<1>, dim3(gx_out, rows(4)), dim3(256), sizeof(float) * 4 * span, g);
    else HLMI_LAUNCH(uc, "gb_blur_x_general", st, gb_blur_x_general, dim3(gx_out, g.oh), dim3(256), 0, g);
    return 0;
}

int direct_entry(halide_buffer_t *input, float sigma, int32_t trunc, halide_buffer_t *output, bool general_only) {
    void *uc = nullptr;
    BufArg args[2];
    gb_table.bufs(args, {input, output});
    int r = check_not_null(uc, args, 2);
    if (r) return r;
    if ((r = check_scalars(uc, sigma, trunc))) return r;
    if ((r = check_type_and_dims(uc, args, 2))) return r;
    if (any_bounds_query(args, 2)) return 0;   // repeat_edge needs nothing beyond the input's own region: both stay as passed
    if ((r = check_shapes(uc, args, 2))) return r;
    int radius = 0;
    if ((r = radius_of(uc, sigma, trunc, &radius))) return r;
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, 2))) return r;
    BGeom g;
    g.sw = input->dim[0].extent, g.sh = input->dim[1].extent;
    g.ow = output->dim[0].extent, g.oh = output->dim[1].extent;
    if (g.ow > 0 && g.oh > 0) {
        if (g.sw <= 0 || g.sh <= 0) return report(uc, halide_error_code_access_out_of_bounds, "Input buffer input is empty: there is no edge to repeat");
        g.src = dev_ptr<float>(input), g.s_sy = input->dim[1].stride;
        g.dst = dev_ptr<float>(output), g.d_sy = output->dim[1].stride;
        g.x0 = output->dim[0].min - input->dim[0].min, g.y0 = output->dim[1].min - input->dim[1].min;
        g.radius = radius;
        const size_t n_kn = pad(2 * (size_t)radius + 1);
        void *ws = nullptr;
        if ((r = workspace(uc, ctx, n_kn + (size_t)g.sw * g.oh, &ws))) return r;
        g.kn = (float *)ws, g.mid = (float *)ws + n_kn;
        timing_note_bytes(4.0 * ((double)g.sw * g.sh + (double)g.ow * g.oh));
        if ((r = run_blur(uc, ctx.stream, g, sigma, general_only))) return r;
    }
    mark_output_written(output);
    return 0;
}

template<int U, int D, int F>
int resampled_entry(halide_buffer_t *input, float sigma, int32_t trunc, halide_buffer_t *output, bool general_only) {
    void *uc = nullptr;
    BufArg args[2];
    gb_table.bufs(args, {input, output});
    int r = check_not_null(uc, args, 2);
    if (r) return r;
    if ((r = check_scalars(uc, sigma, trunc))) return r;
    if ((r = check_type_and_dims(uc, args, 2))) return r;
    if (any_bounds_query(args, 2)) {
        // every read of the input clamps to its own region: it stays as passed; the output's mins are pinned to 0 (:345-347)
        int mins[2] = {0, 0}, ext[2] = {output->dim[0].extent, output->dim[1].extent};
        answer_query(output, mins, ext);
        return 0;
    }
    if ((r = check_shapes(uc, args, 2))) return r;
    check_equal(uc, "output.min.0", output->dim[0].min, "0", 0);
    check_equal(uc, "output.min.1", output->dim[1].min, "0", 0);
    check_equal(uc, "output.stride.1", output->dim[1].stride, "(output.stride.1 / 16) * 16", output->dim[1].stride & ~15);
    check_host_aligned(uc, args[1], 64);
    static const float up_variance = resampling_variance(U, F), down_variance = resampling_variance(D, F);
    const float t = (dev::CANON_FMA ? fmaf(sigma, sigma, -up_variance) : sigma * sigma - up_variance) - down_variance;
    const float sigma_lo = sqrtf(fmaxf(t, 1e-4f)) / (float)F;
    int radius = 0;
    if ((r = radius_of(uc, sigma_lo, trunc, &radius))) return r;
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, 2))) return r;
    RGeom g;
    g.W = input->dim[0].extent, g.H = input->dim[1].extent;
    g.ow = output->dim[0].extent, g.oh = output->dim[1].extent;
    if (g.ow > 0 && g.oh > 0) {
        if (g.W <= 0 || g.H <= 0) return report(uc, halide_error_code_access_out_of_bounds, "Input buffer input is empty: there is no edge to repeat");
        static const DownTab dtab = [] { DownTab t{}; resampling_kernel(D, F, t.k); return t; }();
        static const UpTab utab = [] { float k[64]; UpTab t{}; resampling_kernel(U, F, k); for (int i = 0; i < U * F; i++) t.c[i] = k[i] * (float)F; return t; }();
        g.in = dev_ptr<float>(input), g.in_sy = input->dim[1].stride, g.ix0 = input->dim[0].min, g.iy0 = input->dim[1].min;
        g.out = dev_ptr<float>(output), g.out_sy = output->dim[1].stride;
        g.shift = floor_div((U - D) * F, 2);
        // blurred on [bx0, bx1] x [by0, by1] is what the expansions read; the small blur reads down_x on those columns widened by
        // the radius and on those rows widened by it and clamped to [-U, div_up(H, F)] (:191) — both ends of the row range are
        // images of that clamp, so clamping to the range is that clamp
        const int bx1 = (g.ow - 1) / F, by1 = (g.oh - 1) / F, top = (g.H + F - 1) / F;   // H > 0
        g.bx0 = -(U - 1), g.by0 = -(U - 1), g.bw = bx1 - g.bx0 + 1;
        const int bh = by1 - g.by0 + 1;
        const long lx1 = (long)bx1 + radius, ly1 = std::min<long>((long)by1 + radius, top);
        const long lx0 = (long)g.bx0 - radius, ly0 = std::max<long>(std::min<long>((long)g.by0 - radius, top), -U);
        if (lx1 - lx0 + 1 > 0x7fffffffL / F) return report(uc, halide_error_code_out_of_memory, "gaussian_blur: a radius of %d low-resolution taps exceeds any intermediate", radius);
        g.lx0 = (int)lx0, g.ly0 = (int)ly0, g.lw = (int)(lx1 - lx0 + 1), g.lh = (int)(std::max(ly1, ly0) - ly0 + 1);
        const size_t n_kn = pad(2 * (size_t)radius + 1), n_lo = pad((size_t)g.lw * g.lh), n_mid = pad((size_t)g.lw * bh), n_bl = pad((size_t)g.bw * bh);
        void *ws = nullptr;
        if ((r = workspace(uc, ctx, n_kn + n_lo + n_mid + n_bl, &ws))) return r;
        float *kn = (float *)ws, *lo = kn + n_kn, *mid = lo + n_lo, *bl = mid + n_mid;
        g.lo = lo, g.bl = bl;
        hipStream_t st = ctx.stream;
        const size_t dgx = (g.lw + dn_cols(F, D) - 1) / dn_cols(F, D), dgy = (g.lh + DN_ROWS - 1) / DN_ROWS;
        const size_t ugx = (g.ow + 255) / 256, ugy = (g.oh + UP_ROWS - 1) / UP_ROWS;
        if ((r = blocks_ok(uc, dgx, dgy)) || (r = blocks_ok(uc, ugx, ugy))) return r;
        timing_note_bytes(4.0 * ((double)g.W * g.H + (double)g.ow * g.oh));
        HLMI_LAUNCH(uc, "gb_down", st, (gb_down<F, D>), dim3((unsigned)dgx, (unsigned)dgy), dim3(256), 0, g, dtab);
        BGeom b;
        b.src = lo, b.s_sy = g.lw, b.sw = g.lw, b.sh = g.lh;
        b.mid = mid, b.dst = bl, b.d_sy = g.bw;
        b.x0 = g.bx0 - g.lx0, b.y0 = g.by0 - g.ly0, b.ow = g.bw, b.oh = bh;
        b.radius = radius, b.kn = kn;
        if ((r = run_blur(uc, st, b, sigma_lo, general_only))) return r;
        HLMI_LAUNCH(uc, "gb_up", st, (gb_up<F, U>), dim3((unsigned)ugx, (unsigned)ugy), dim3(256), 0, g, utab);
    }
    mark_output_written(output);
    return 0;
}

struct Variant {
    const char *name;
    int (*general)(halide_buffer_t *, float, int32_t, halide_buffer_t *);
};

int direct_general(halide_buffer_t *i, float s, int32_t t, halide_buffer_t *o) { return direct_entry(i, s, t, o, true); }

}  // namespace

extern "C" int gaussian_blur_direct(halide_buffer_t *input, float sigma, int32_t trunc, halide_buffer_t *output) {
    return direct_entry(input, sigma, trunc, output, false);
}
HLMI_ENTRY_AUTO(gaussian_blur_direct, gb_table.md)

#define GB_VARIANT(U, D, F)                                                                                                        \
    namespace {                                                                                                                    \
    const halide_filter_metadata_t gb_md_##U##_##D##_##F = gb_table.named("gaussian_blur_" #U "_" #D "_" #F);                      \
    int gb_general_##U##_##D##_##F(halide_buffer_t *i, float s, int32_t t, halide_buffer_t *o) {                                   \
        return resampled_entry<U, D, F>(i, s, t, o, true);                                                                         \
    }                                                                                                                              \
    }                                                                                                                              \
    extern "C" int gaussian_blur_##U##_##D##_##F(halide_buffer_t *input, float sigma, int32_t trunc, halide_buffer_t *output) {   \
        return resampled_entry<U, D, F>(input, sigma, trunc, output, false);                                                       \
    }                                                                                                                              \
    HLMI_ENTRY(gaussian_blur_##U##_##D##_##F, gb_md_##U##_##D##_##F)
#define GB_FACTORS(M, U, D) M(U, D, 2) M(U, D, 4) M(U, D, 8) M(U, D, 16)
#define GB_ORDERS(M, U) GB_FACTORS(M, U, 1) GB_FACTORS(M, U, 2) GB_FACTORS(M, U, 3)
#define GB_ALL(M) GB_ORDERS(M, 2) GB_ORDERS(M, 3) GB_ORDERS(M, 4)
GB_ALL(GB_VARIANT)

// Measurement and test hook (hlmi_internal.h): the named blur with its blur passes on the general path, whatever the sizes.  The
// reduction and the expansion of the variants have no size conditions: they are the same launches on both paths.
#define GB_ROW(U, D, F) {"gaussian_blur_" #U "_" #D "_" #F, gb_general_##U##_##D##_##F},
extern "C" int hlmi_gaussian_blur_general(const char *variant, halide_buffer_t *input, float sigma, int32_t trunc, halide_buffer_t *output) {
    static const Variant table[37] = {{"gaussian_blur_direct", direct_general}, GB_ALL(GB_ROW)};
    for (const Variant &v : table)
        if (variant && strcmp(v.name, variant) == 0) return v.general(input, sigma, trunc, output);
    return report(nullptr, halide_error_code_constraint_violated, "hlmi_gaussian_blur_general: no variant named %s", variant ? variant : "(null)");
}
