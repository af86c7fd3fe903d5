// hannk_nn.hip — the pooling, reduction, elementwise and normalisation ops of apps/hannk's op library (apps/hannk/halide/
// pool_generator.cpp, reductions_generator.cpp, elementwise_generator.cpp, normalizations_generator.cpp), C++-mangled in namespace hannk
// as the reference builds them:
//   hannk::average_pool_uint8, hannk::max_pool_uint8, hannk::mean_uint8, hannk::add_uint8_uint8, hannk::mul_uint8_uint8_uint8,
//   hannk::softmax_uint8, hannk::l2_normalization_uint8, each with _argv and _metadata (include/aot/halide/<name>.h).
//
// The contract is integer throughout (the element rules are in hannk_math.h) and the same in both builds of the library.
//   avg pool  sum(c, x, y, b) = u16 sum of in(c, x*sx + rx, y*sy + ry, b) over the taps inside the input; n = (x_end - x_start)(y_end - y_start);
//             out = clamp(u8_sat(rounding_mul_shift_right(sum, u16_sat((2^17 + n) / (2 n)), 16)), lo, hi)
//   max pool  out = min(max(lo, taps inside the input ...), hi)
//   mean      out = u8((u32 sum over the 4-D region + extent / 2) / extent), in i32
//   add, mul  hannk_math.h: add_u8, mul_u8;  softmax: softmax_exp / softmax_inv_sum / softmax_out;  l2: l2norm_inv_sqrt / l2norm_out
// Every reduction here is an integer sum modulo 2^n or a maximum: it may be split and combined in any order without changing a byte.
//
// Kernels (each op: a default plan and the general kernel, one thread per output with the loops as written, behind hlmi_hannk_general):
//   hannk_pool4        outputs that fill the device: a lane owns 4 adjacent channels of one output pixel: one dword load per tap where the
//                      input is dword-aligned (pointer and the x, y, b strides), bytes for a last partial quad; sums in 32-bit registers,
//                      masked to 16 bits once; inv_filter_count once per thread, the host's constant for windows wholly inside
//   hannk_pool_split   few output pixels under a large window (the global pool): a workgroup owns one pixel and 64 channels, its 16
//                      slices of 16 lanes take every 16th tap, partial sums (maxima) meet in LDS
//   hannk_mean_wg      lanes along c, the (x, y, b) region split over the 4 waves of a workgroup and combined in LDS
//   hannk_mean_lanes   c itself reduced: one wave per output, lanes over the flattened region (c innermost), combined by shuffles
//   hannk_ew           add and mul: 16 bytes per lane (one 16-byte load per operand, one store) where the chunk is whole and the three
//                      addresses are 16-byte aligned; a stride-0 operand is one byte per row; any other chunk goes byte by byte
//   hannk_rows         softmax and l2_normalization with both dimension-0 strides 1: one wave per row, dword loads where the row is
//                      aligned, row maximum / i32 sum by wave shuffles, the reciprocal once per row, and where the row fits 64 x 16
//                      elements the loaded bytes and exp2_diff stay in registers between the passes (otherwise they are recomputed)
//
// Host path: every entry point reads top to bottom: check arguments -> bounds query (the three ops that answer one) -> device and
// buffers -> empty output -> plan -> launch -> mark_output_written.
#include "hlmi_internal.h"
#include "hannk_entry.h"
#include "hannk_math.h"

using namespace hlmi;

namespace {

using namespace hlmi::hannk_math;
using namespace hlmi::hannk_entry;

// four bytes c .. c + 3 of one pixel: one dword where all four exist and the address allows it
__device__ __forceinline__ void store4_u8(uint8_t *p, int n, const uint32_t (&v)[4]) {
    if (n >= 4 && ((uintptr_t)p & 3) == 0) {
        *reinterpret_cast<uint32_t *>(p) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
    } else {
#pragma unroll
        for (int r = 0; r < 4; r++)
            if (r < n) p[r] = (uint8_t)v[r];
    }
}

// ---------------------------------------------------------------------------------------------------------------- pools
struct PoolGeom {
    const uint8_t *in;     // input element (c_min, x_min, y_min, b_min)
    uint8_t *out;          // output element (c_min, x_min, y_min, b_min)
    int C, OW, OH, OB;
    int ox0, oy0;          // the output's x and y min
    int ix0, iy0, IW, IH;  // the input's x and y min and extent
    long in_sx, in_sy, in_sb, o_sx, o_sy, o_sb;
    int sx, sy, FW, FH;
    int lo, hi;
    uint32_t inv_full;     // inv_filter_count of a window wholly inside the input
};
struct PoolWindow {
    int rx0, rx1, ry0, ry1;   // the taps inside the input: [rx0, rx1) x [ry0, ry1), possibly empty
    long ax, ay;              // input offsets (elements from x_min, y_min) of tap (0, 0)
    uint32_t inv;
};
__device__ __forceinline__ PoolWindow pool_window(const PoolGeom &g, int x, int y, bool avg) {
    PoolWindow w;
    const long x0 = (long)(x + g.ox0) * g.sx, y0 = (long)(y + g.oy0) * g.sy;
    const long xs = max(x0, (long)g.ix0), xe = min(x0 + g.FW, (long)g.ix0 + g.IW), ys = max(y0, (long)g.iy0), ye = min(y0 + g.FH, (long)g.iy0 + g.IH);
    w.ax = x0 - g.ix0, w.ay = y0 - g.iy0;
    w.rx0 = (int)(xs - x0), w.rx1 = (int)max(xe - x0, xs - x0), w.ry0 = (int)(ys - y0), w.ry1 = (int)max(ye - y0, ys - y0);
    if (xs >= xe || ys >= ye) w.rx1 = w.rx0, w.ry1 = w.ry0;
    w.inv = 0;
    if (avg) {
        const bool full = xe - xs == g.FW && ye - ys == g.FH;
        w.inv = full ? g.inv_full : pool_inv_count(wrap<32>((xe - xs) * (ye - ys)));   // (as written: two negative factors give a positive count)
    }
    return w;
}

template<bool AVG>
__global__ __launch_bounds__(256) void hannk_pool_general(PoolGeom g) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)g.C * g.OW * g.OH * g.OB) return;
    const int c = (int)(i % g.C);
    const long p = i / g.C;
    const int x = (int)(p % g.OW), y = (int)((p / g.OW) % g.OH), b = (int)(p / ((long)g.OW * g.OH));
    const PoolWindow w = pool_window(g, x, y, AVG);
    const uint8_t *in = g.in + b * g.in_sb + c;
    uint32_t acc = AVG ? 0u : (uint32_t)g.lo;
    for (int ry = w.ry0; ry < w.ry1; ry++)
        for (int rx = w.rx0; rx < w.rx1; rx++) {
            const uint32_t v = in[(w.ay + ry) * g.in_sy + (w.ax + rx) * g.in_sx];
            acc = AVG ? acc + v : max(acc, v);
        }
    const int r = AVG ? pool_average(acc & 0xffffu, w.inv, g.lo, g.hi) : min((int)acc, g.hi);
    g.out[b * g.o_sb + y * g.o_sy + x * g.o_sx + c] = (uint8_t)r;
}

// one tap of a channel quad: a dword where the quad is whole (the caller has checked the alignment), its n bytes otherwise
template<bool AVG>
__device__ __forceinline__ void pool_tap(const uint8_t *at, int n, uint32_t (&acc)[4]) {
    uint32_t d;
    if (n >= 4) {
        d = *reinterpret_cast<const uint32_t *>(at);
    } else {
        d = at[0];
        if (n > 1) d |= (uint32_t)at[1] << 8;
        if (n > 2) d |= (uint32_t)at[2] << 16;
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint32_t v = (d >> (8 * r)) & 0xffu;
        acc[r] = AVG ? acc[r] + v : max(acc[r], v);
    }
}
template<bool AVG>
__device__ __forceinline__ void pool_finish(const PoolGeom &g, const PoolWindow &w, uint8_t *out, int n, const uint32_t (&acc)[4]) {
    uint32_t v[4];
#pragma unroll
    for (int r = 0; r < 4; r++) v[r] = (uint32_t)(AVG ? pool_average(acc[r] & 0xffffu, w.inv, g.lo, g.hi) : min((int)max(acc[r], (uint32_t)g.lo), g.hi));
    store4_u8(out, n, v);
}

template<bool AVG>
__global__ __launch_bounds__(256) void hannk_pool4(PoolGeom g) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int nq = (g.C + 3) / 4;
    if (i >= (long)nq * g.OW * g.OH * g.OB) return;
    const int c0 = (int)(i % nq) * 4;
    const long p = i / nq;
    const int x = (int)(p % g.OW), y = (int)((p / g.OW) % g.OH), b = (int)(p / ((long)g.OW * g.OH));
    const PoolWindow w = pool_window(g, x, y, AVG);
    const uint8_t *in = g.in + b * g.in_sb + c0;
    const int n = min(g.C - c0, 4);
    uint32_t acc[4] = {0, 0, 0, 0};
    for (int ry = w.ry0; ry < w.ry1; ry++)
        for (int rx = w.rx0; rx < w.rx1; rx++) pool_tap<AVG>(in + (w.ay + ry) * g.in_sy + (w.ax + rx) * g.in_sx, n, acc);
    pool_finish<AVG>(g, w, g.out + b * g.o_sb + y * g.o_sy + x * g.o_sx + c0, n, acc);
}

// a workgroup: one output pixel, 16 channel quads; thread = (quad q = tid & 15, slice = tid >> 4), slice s takes taps s, s + 16, ...
constexpr int PS_QUADS = 16, PS_SLICES = 16;
template<bool AVG>
__global__ __launch_bounds__(256) void hannk_pool_split(PoolGeom g) {
    __shared__ uint32_t part[PS_SLICES][PS_QUADS][4];
    const int q = threadIdx.x & (PS_QUADS - 1), slice = threadIdx.x >> 4;
    const int nqg = ((g.C + 3) / 4 + PS_QUADS - 1) / PS_QUADS;
    const int qg = (int)(blockIdx.x % nqg);
    const long p = blockIdx.x / nqg;
    const int x = (int)(p % g.OW), y = (int)((p / g.OW) % g.OH), b = (int)(p / ((long)g.OW * g.OH));
    const PoolWindow w = pool_window(g, x, y, AVG);
    const int c0 = (qg * PS_QUADS + q) * 4, n = min(g.C - c0, 4);
    uint32_t acc[4] = {0, 0, 0, 0};
    if (n > 0) {
        const uint8_t *in = g.in + b * g.in_sb + c0;
        const int tw = w.rx1 - w.rx0, nt = tw * (w.ry1 - w.ry0);
        for (int t = slice; t < nt; t += PS_SLICES) {
            const int ry = w.ry0 + t / tw, rx = w.rx0 + t % tw;
            pool_tap<AVG>(in + (w.ay + ry) * g.in_sy + (w.ax + rx) * g.in_sx, n, acc);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) part[slice][q][r] = acc[r];
    __syncthreads();
    if (slice != 0 || n <= 0) return;
    for (int s = 1; s < PS_SLICES; s++)
#pragma unroll
        for (int r = 0; r < 4; r++) acc[r] = AVG ? acc[r] + part[s][q][r] : max(acc[r], part[s][q][r]);
    pool_finish<AVG>(g, w, g.out + b * g.o_sb + y * g.o_sy + x * g.o_sx + c0, n, acc);
}

// ---------------------------------------------------------------------------------------------------------------- mean
struct MeanGeom {
    const uint8_t *in;   // the input element the output's first element reads at the region's first tap
    uint8_t *out;
    int oext[4];
    long ostr[4], istr[4];
    int rext[4];         // the region's extents, none negative
    int extent;          // c_extent * x_extent * y_extent * b_extent as the i32 product of the arguments
};
__device__ __forceinline__ void mean_coords(const MeanGeom &g, long i, int (&o)[4], long &ooff, long &ioff) {
    ooff = 0, ioff = 0;
#pragma unroll
    for (int d = 0; d < 4; d++) {
        o[d] = (int)(i % g.oext[d]);
        i /= g.oext[d];
        ooff += o[d] * g.ostr[d], ioff += o[d] * g.istr[d];
    }
}
__global__ __launch_bounds__(256) void hannk_mean_general(MeanGeom g) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)g.oext[0] * g.oext[1] * g.oext[2] * g.oext[3]) return;
    int o[4];
    long ooff, ioff;
    mean_coords(g, i, o, ooff, ioff);
    uint32_t sum = 0;
    for (int rb = 0; rb < g.rext[3]; rb++)
        for (int ry = 0; ry < g.rext[2]; ry++)
            for (int rx = 0; rx < g.rext[1]; rx++)
                for (int rc = 0; rc < g.rext[0]; rc++) sum += g.in[ioff + rc * g.istr[0] + rx * g.istr[1] + ry * g.istr[2] + rb * g.istr[3]];
    g.out[ooff] = (uint8_t)mean_out(sum, g.extent);
}
// a workgroup: 64 output channels of one (x, y, b); wave w takes (x, y, b) taps w, w + 4, ... and the whole c range of each
__global__ __launch_bounds__(256) void hannk_mean_wg(MeanGeom g) {
    __shared__ uint32_t part[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ncg = (g.oext[0] + 63) / 64;
    const int c = (int)(blockIdx.x % ncg) * 64 + lane;
    const long p = blockIdx.x / ncg;
    uint32_t sum = 0;
    long ooff = 0;
    if (c < g.oext[0]) {
        int o[4];
        long ioff;
        mean_coords(g, p * g.oext[0] + c, o, ooff, ioff);
        const int nt = g.rext[1] * g.rext[2] * g.rext[3];   // (the plan keeps the product inside an int)
        for (int t = wave; t < nt; t += 4) {
            const int rx = t % g.rext[1], ry = (t / g.rext[1]) % g.rext[2], rb = t / (g.rext[1] * g.rext[2]);
            const uint8_t *at = g.in + ioff + rx * g.istr[1] + ry * g.istr[2] + rb * g.istr[3];
            for (int rc = 0; rc < g.rext[0]; rc++) sum += at[rc * g.istr[0]];
        }
    }
    part[wave][lane] = sum;
    __syncthreads();
    if (wave != 0 || c >= g.oext[0]) return;
    sum += part[1][lane] + part[2][lane] + part[3][lane];
    g.out[ooff] = (uint8_t)mean_out(sum, g.extent);
}
// one wave per output: lanes over the flattened region, c innermost
__global__ __launch_bounds__(64) void hannk_mean_lanes(MeanGeom g) {
    int o[4];
    long ooff, ioff;
    mean_coords(g, blockIdx.x, o, ooff, ioff);
    const int nt = g.rext[0] * g.rext[1] * g.rext[2] * g.rext[3];   // (inside an int: the plan)
    uint32_t sum = 0;
    for (int t = threadIdx.x; t < nt; t += 64) {
        int r = t;
        const int rc = r % g.rext[0];
        r /= g.rext[0];
        const int rx = r % g.rext[1];
        r /= g.rext[1];
        const int ry = r % g.rext[2], rb = r / g.rext[2];
        sum += g.in[ioff + rc * g.istr[0] + rx * g.istr[1] + ry * g.istr[2] + rb * g.istr[3]];
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sum += (uint32_t)__shfl_xor((int)sum, m);
    if (threadIdx.x == 0) g.out[ooff] = (uint8_t)mean_out(sum, g.extent);
}

// ---------------------------------------------------------------------------------------------------------------- add, mul
struct EwGeom {
    const uint8_t *a, *b;   // the inputs' elements at the output's (x_min, y_min); a stride-0 operand: at (its own x_min, y_min)
    uint8_t *out;
    int W, H;
    long a_s0, a_s1, b_s0, b_s1, o_s1;   // a_s0, b_s0: 0 or 1
};
__device__ __forceinline__ int32_t ew_op(int32_t a, int32_t b, const AddParams &p) { return add_u8(a, b, p); }
__device__ __forceinline__ int32_t ew_op(int32_t a, int32_t b, const MulParams &p) { return mul_u8(a, b, p); }

template<typename P>
__global__ __launch_bounds__(256) void hannk_ew_general(EwGeom g, P p) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)g.W * g.H) return;
    const int x = (int)(i % g.W);
    const long y = i / g.W;
    g.out[y * g.o_s1 + x] = (uint8_t)ew_op(g.a[y * g.a_s1 + x * g.a_s0], g.b[y * g.b_s1 + x * g.b_s0], p);
}
template<typename P>
__global__ __launch_bounds__(256) void hannk_ew(EwGeom g, P p) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int nch = (g.W + 15) / 16;
    if (i >= (long)nch * g.H) return;
    const int x0 = (int)(i % nch) * 16;
    const long y = i / nch;
    const uint8_t *pa = g.a + y * g.a_s1 + x0 * g.a_s0, *pb = g.b + y * g.b_s1 + x0 * g.b_s0;
    uint8_t *po = g.out + y * g.o_s1 + x0;
    const bool wide = x0 + 16 <= g.W && ((uintptr_t)po & 15) == 0 && (g.a_s0 == 0 || ((uintptr_t)pa & 15) == 0) && (g.b_s0 == 0 || ((uintptr_t)pb & 15) == 0);
    if (wide) {
        uint32_t va[4], vb[4], vo[4];
        if (g.a_s0) {
            const uint4 t = *reinterpret_cast<const uint4 *>(pa);
            va[0] = t.x, va[1] = t.y, va[2] = t.z, va[3] = t.w;
        } else {
            va[0] = va[1] = va[2] = va[3] = (uint32_t)pa[0] * 0x01010101u;
        }
        if (g.b_s0) {
            const uint4 t = *reinterpret_cast<const uint4 *>(pb);
            vb[0] = t.x, vb[1] = t.y, vb[2] = t.z, vb[3] = t.w;
        } else {
            vb[0] = vb[1] = vb[2] = vb[3] = (uint32_t)pb[0] * 0x01010101u;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            vo[k] = 0;
#pragma unroll
            for (int r = 0; r < 4; r++) vo[k] |= (uint32_t)ew_op((va[k] >> (8 * r)) & 0xffu, (vb[k] >> (8 * r)) & 0xffu, p) << (8 * r);
        }
        *reinterpret_cast<uint4 *>(po) = make_uint4(vo[0], vo[1], vo[2], vo[3]);
    } else {
        const int n = min(16, g.W - x0);
        for (int k = 0; k < n; k++) po[k] = (uint8_t)ew_op(pa[k * g.a_s0], pb[k * g.b_s0], p);
    }
}

// ---------------------------------------------------------------------------------------------------------------- softmax, l2_normalization
struct RowGeom {
    const uint8_t *in;   // input element (its own x_min, the output's y_min): the start of the first reduced row
    uint8_t *out;        // the output's first element
    int N;               // the input's extent 0: the reduction runs over the input's own dimension 0
    int W, H;            // the output's extents
    int xoff;            // output.min(0) - input.min(0)
    long i_s0, i_s1, o_s0, o_s1;
    int zero;            // l2_normalization's input_zero
};
template<bool L2>
__global__ __launch_bounds__(256) void hannk_rows_general(RowGeom g, SoftmaxParams p) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)g.W * g.H) return;
    const int x = (int)(i % g.W);
    const long y = i / g.W;
    const uint8_t *row = g.in + y * g.i_s1;
    const int32_t v = row[(x + g.xoff) * g.i_s0];
    int32_t r;
    if (L2) {
        uint32_t sum = 0;
        for (int k = 0; k < g.N; k++) {
            const int32_t d = (int32_t)row[k * g.i_s0] - g.zero;
            sum += (uint32_t)(d * d);
        }
        r = l2norm_out(v - g.zero, l2norm_inv_sqrt((int32_t)sum));
    } else {
        int32_t mx = 0;
        for (int k = 0; k < g.N; k++) mx = max(mx, (int32_t)row[k * g.i_s0]);
        uint32_t sum = 0;
        for (int k = 0; k < g.N; k++) sum += (uint32_t)softmax_exp(row[k * g.i_s0], mx, p);
        r = softmax_out(softmax_exp(v, mx, p), softmax_inv_sum((int32_t)sum), p);
    }
    g.out[y * g.o_s1 + x * g.o_s0] = (uint8_t)r;
}

constexpr int ROW_KEEP_CHUNKS = 4, ROW_KEEP_MAX = 64 * 4 * ROW_KEEP_CHUNKS;   // 64 lanes x 16 elements
// the row's elements e0 .. e0 + 3 as one dword (absent ones 0)
__device__ __forceinline__ uint32_t row_load4(const uint8_t *row, bool aligned, int e0, int N) {
    if (e0 + 3 < N && aligned) return *reinterpret_cast<const uint32_t *>(row + e0);
    uint32_t d = 0;
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (e0 + j < N) d |= (uint32_t)row[e0 + j] << (8 * j);
    return d;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m);
    return v;
}
__device__ __forceinline__ int32_t wave_max(int32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m));
    return v;
}
// both strides of dimension 0 are 1.  KEEP: N <= ROW_KEEP_MAX, chunk k of lane l is elements 4 (64 k + l) .. + 3
template<bool L2, bool KEEP>
__global__ __launch_bounds__(256) void hannk_rows(RowGeom g, SoftmaxParams p) {
    const int lane = threadIdx.x & 63;
    const long y = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (y >= g.H) return;   // (no barrier in this kernel)
    const uint8_t *row = g.in + y * g.i_s1;
    uint8_t *out = g.out + y * g.o_s1;
    const bool aligned = ((uintptr_t)row & 3) == 0;
    const int nchunk = KEEP ? ROW_KEEP_CHUNKS : (g.N + 255) / 256;
    uint32_t raw[KEEP ? ROW_KEEP_CHUNKS : 1];
    int32_t ex[KEEP ? ROW_KEEP_CHUNKS * 4 : 1];
    // ---- pass 1: the row maximum (softmax) or the sum of squares (l2)
    uint32_t red = 0;
#pragma unroll KEEP ? ROW_KEEP_CHUNKS : 1
    for (int k = 0; k < nchunk; k++) {
        const int e0 = (k * 64 + lane) * 4;
        const uint32_t d = row_load4(row, aligned, e0, g.N);
        if (KEEP) raw[KEEP ? k : 0] = d;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int32_t v = (int32_t)((d >> (8 * j)) & 0xffu);
            if (L2) {
                const int32_t z = v - g.zero;
                if (e0 + j < g.N) red += (uint32_t)(z * z);
            } else {
                red = max(red, (uint32_t)v);   // an absent element is 0, the maximum's start
            }
        }
    }
    int32_t scale;   // inv_sqrt (l2) or inv_sum_exp_row (softmax): once per row, the same in every lane
    int32_t mx = 0;
    if (L2) {
        scale = l2norm_inv_sqrt((int32_t)wave_sum(red));
    } else {
        mx = wave_max((int32_t)red);
        // ---- pass 2: exp2_diff and its i32 sum
        uint32_t sum = 0;
#pragma unroll KEEP ? ROW_KEEP_CHUNKS : 1
        for (int k = 0; k < nchunk; k++) {
            const int e0 = (k * 64 + lane) * 4;
            const uint32_t d = KEEP ? raw[KEEP ? k : 0] : row_load4(row, aligned, e0, g.N);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int32_t e = softmax_exp((int32_t)((d >> (8 * j)) & 0xffu), mx, p);
                if (KEEP) ex[KEEP ? 4 * k + j : 0] = e;
                if (e0 + j < g.N) sum += (uint32_t)e;
            }
        }
        scale = softmax_inv_sum((int32_t)wave_sum(sum));
    }
    // ---- pass 3: the output's elements [xoff, xoff + W) of the row
#pragma unroll KEEP ? ROW_KEEP_CHUNKS : 1
    for (int k = 0; k < nchunk; k++) {
        const int e0 = (k * 64 + lane) * 4;
        if (e0 >= g.xoff + g.W || e0 + 3 < g.xoff) continue;
        const uint32_t d = KEEP ? raw[KEEP ? k : 0] : row_load4(row, aligned, e0, g.N);
        uint32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int32_t in = (int32_t)((d >> (8 * j)) & 0xffu);
            if (L2) v[j] = (uint32_t)l2norm_out(in - g.zero, scale);
            else v[j] = (uint32_t)softmax_out(KEEP ? ex[KEEP ? 4 * k + j : 0] : softmax_exp(in, mx, p), scale, p);
        }
        const int xo = e0 - g.xoff;   // the output element of v[0]
        if (xo >= 0 && xo + 3 < g.W && (((uintptr_t)(out + xo)) & 3) == 0) {
            *reinterpret_cast<uint32_t *>(out + xo) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (xo + j >= 0 && xo + j < g.W) out[xo + j] = (uint8_t)v[j];
        }
    }
}

// the debug hook's kernel: fn as hlmi_debug_hannk_approx
__global__ __launch_bounds__(256) void dbg_hannk_approx(int fn, int q, const int32_t *__restrict__ x, size_t n, int q_x, int bits, int32_t *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t v = x[i];
    int32_t r;
    if (bits == 16) {
        r = fn == 0 ? approx_log2<16>(q, v, q_x) : fn == 1 ? approx_exp2<32, 16>(q, v, (uint32_t)q_x) : fn == 2 ? approx_reciprocal<16>(q, v) : approx_reciprocal_sqrt<16>(q, v);
    } else {
        r = fn == 0 ? approx_log2<32>(q, v, q_x) : fn == 1 ? approx_exp2<32, 32>(q, v, (uint32_t)q_x) : fn == 2 ? approx_reciprocal<32>(q, v) : approx_reciprocal_sqrt<32>(q, v);
    }
    out[i] = r;
}

// ---------------------------------------------------------------------------------------------------------------- host: tables
const ArgTable avg_table("average_pool_uint8", {L(in_buf("input", T_U8, 4)), L(scalar_i32("stride_x")), L(scalar_i32("stride_y")), L(scalar_i32("filter_width")),
                                                L(scalar_i32("filter_height")), L(scalar_u8("output_min")), L(scalar_u8("output_max")), L(out_buf("output", T_U8, 4))});
const ArgTable max_table("max_pool_uint8", {L(in_buf("input", T_U8, 4)), L(scalar_i32("stride_x")), L(scalar_i32("stride_y")), L(scalar_i32("filter_width")),
                                            L(scalar_i32("filter_height")), L(scalar_u8("output_min")), L(scalar_u8("output_max")), L(out_buf("output", T_U8, 4))});
const ArgTable mean_table("mean_uint8", {L(in_buf("input", T_U8, 4)), L(scalar_i32("c_min")), L(scalar_i32("c_extent")), L(scalar_i32("x_min")), L(scalar_i32("x_extent")),
                                         L(scalar_i32("y_min")), L(scalar_i32("y_extent")), L(scalar_i32("b_min")), L(scalar_i32("b_extent")), L(out_buf("output", T_U8, 4))});
const ArgTable add_table("add_uint8_uint8", {L(in_buf("input1", T_U8, 2)), L(scalar_u8("input1_zero")), L(scalar_i16("input1_multiplier")), L(in_buf("input2", T_U8, 2)),
                                             L(scalar_u8("input2_zero")), L(scalar_i16("input2_multiplier")), L(scalar_u8("output_zero")), L(scalar_u8("output_min")),
                                             L(scalar_u8("output_max")), L(out_buf("output", T_U8, 2))});
const ArgTable mul_table("mul_uint8_uint8_uint8", {L(in_buf("input1", T_U8, 2)), L(scalar_u8("input1_zero")), L(in_buf("input2", T_U8, 2)), L(scalar_u8("input2_zero")),
                                                   L(scalar_u8("output_zero")), L(scalar_i32("output_multiplier")), L(scalar_u32("output_shift")),
                                                   L(scalar_u8("output_min")), L(scalar_u8("output_max")), L(out_buf("output", T_U8, 2))});
const ArgTable softmax_table("softmax_uint8", {L(in_buf("input", T_U8, 2)), L(scalar_i16("beta_multiplier")), L(scalar_u16("beta_shift")), L(scalar_u8("output_zero")),
                                               L(scalar_i16("output_multiplier")), L(scalar_u16("output_shift")), L(out_buf("output", T_U8, 2))});
const ArgTable l2_table("l2_normalization_uint8", {L(in_buf("input", T_U8, 2)), L(scalar_u8("input_zero")), L(out_buf("output", T_U8, 2))});

// ---------------------------------------------------------------------------------------------------------------- host: pools
// ---- the plan of a pool call.  Where the input allows dword taps (pointer and x, y, b strides multiples of 4) and the output has a
// workgroup of quads for every compute unit (POOL_MIN_QUADS, as depthwise_conv_uint8's DW_MIN_THREADS), hannk_pool4.  Below that the one-thread-per-output kernel
// has four times the threads and measured no slower (max 3 x 3 stride 2 over 112^2 x 64 at batch 1: 6.6 against 7.1 us; at batch 32
// hannk_pool4 takes 20 against 54 us), unless the window has at least POOL_SPLIT_MIN_TAPS taps for the 16 slices of hannk_pool_split to
// share (the global 7 x 7 pool over 1024 channels: 8.2 against 10.0 us at batch 1, 7.4 against 10.1 us at batch 32).
// Switches, read once per call (tests/test_hannk_nn.py):
//   HLMI_HANNK_POOL_VECTOR  0: the general kernel; 1: hannk_pool4 wherever the alignment allows and the window is not split
//   HLMI_HANNK_POOL_SPLIT   0: never the split kernel; 1: wherever the alignment allows
constexpr int POOL_SPLIT_MIN_TAPS = 16;
constexpr long POOL_MIN_QUADS = 256L * 256;
enum class PoolKernel { general, quad, split };
PoolKernel pool_plan(long quads_px, int taps, bool aligned, std::optional<int> vector, std::optional<int> split) {
    if (!aligned || (vector && *vector == 0)) return PoolKernel::general;
    const bool small = quads_px < POOL_MIN_QUADS;
    if (split ? *split != 0 : (small && taps >= POOL_SPLIT_MIN_TAPS)) return PoolKernel::split;
    if (vector) return PoolKernel::quad;
    return small ? PoolKernel::general : PoolKernel::quad;
}

template<bool AVG, bool GENERAL>
int pool_entry(halide_buffer_t *input, int32_t stride_x, int32_t stride_y, int32_t filter_width, int32_t filter_height, uint8_t output_min,
               uint8_t output_max, halide_buffer_t *output) {
    void *uc = nullptr;
    const ArgTable &table = AVG ? avg_table : max_table;
    BufArg args[2];
    table.bufs(args, {input, output});
    own_lanes(args);
    int r = check_not_null(uc, args, 2);
    if (r || (r = check_type_and_dims(uc, args, 2))) return r;
    halide_dimension_t *id = input->dim, *od = output->dim;
    if (any_bounds_query(args, 2)) {
        // The x and y coordinates are clamped into the input, so any extent of either side is sufficient: the side that is asked about
        // gets the other's dimensions 0 and 3 (require_same_min_extent) and keeps the x and y the caller gave it.
        const int imin[4] = {od[0].min, id[1].min, id[2].min, od[3].min}, iext[4] = {od[0].extent, id[1].extent, id[2].extent, od[3].extent};
        const int omin[4] = {id[0].min, od[1].min, od[2].min, id[3].min}, oext[4] = {id[0].extent, od[1].extent, od[2].extent, id[3].extent};
        answer_query(input, imin, iext);
        answer_query(output, omin, oext);
        return 0;
    }
    // ---- constraints (pool_generator.cpp:76-77, :140-141)
    check_dim(uc, "output", output, 0, &id[0].min, &id[0].extent, nullptr);
    check_dim(uc, "output", output, 3, &id[3].min, &id[3].extent, nullptr);
    if ((r = check_shapes(uc, args, 2))) return r;
    const std::optional<int> sw_vector = env_int("HLMI_HANNK_POOL_VECTOR"), sw_split = env_int("HLMI_HANNK_POOL_SPLIT");
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, 2))) return r;
    PoolGeom g = {};
    g.C = od[0].extent, g.OW = od[1].extent, g.OH = od[2].extent, g.OB = od[3].extent;
    if (g.C <= 0 || g.OW <= 0 || g.OH <= 0 || g.OB <= 0) {
        mark_output_written(output);
        return 0;
    }
    g.in = dev_ptr<uint8_t>(input), g.out = dev_ptr<uint8_t>(output);
    g.ox0 = od[1].min, g.oy0 = od[2].min;
    g.ix0 = id[1].min, g.iy0 = id[2].min, g.IW = id[1].extent, g.IH = id[2].extent;
    g.in_sx = id[1].stride, g.in_sy = id[2].stride, g.in_sb = id[3].stride;
    g.o_sx = od[1].stride, g.o_sy = od[2].stride, g.o_sb = od[3].stride;
    g.sx = stride_x, g.sy = stride_y, g.FW = std::max(filter_width, 0), g.FH = std::max(filter_height, 0);
    g.lo = output_min, g.hi = output_max;
    g.inv_full = pool_inv_count(wrap<32>((int64_t)g.FW * g.FH));
    const long npix = (long)g.OW * g.OH * g.OB, nq = (g.C + 3) / 4;
    const bool aligned = (uintptr_t)g.in % 4 == 0 && g.in_sx % 4 == 0 && g.in_sy % 4 == 0 && g.in_sb % 4 == 0;
    const long taps = (long)std::min(g.FW, g.IW) * std::min(g.FH, g.IH);
    const PoolKernel k = GENERAL ? PoolKernel::general
                                 : pool_plan(nq * npix, (int)std::min(taps, 1L << 30), aligned, sw_vector, sw_split);
    timing_note_bytes((double)npix * g.C + (double)g.IW * g.IH * g.OB * g.C);
    unsigned blocks;
    if (k == PoolKernel::general) {
        if ((r = blocks_ok(uc, table.md.name, npix * g.C, &blocks))) return r;
        HLMI_LAUNCH(uc, "hannk_pool_general", ctx.stream, hannk_pool_general<AVG>, dim3(blocks), dim3(256), 0, g);
    } else if (k == PoolKernel::quad) {
        if ((r = blocks_ok(uc, table.md.name, npix * nq, &blocks))) return r;
        HLMI_LAUNCH(uc, "hannk_pool4", ctx.stream, hannk_pool4<AVG>, dim3(blocks), dim3(256), 0, g);
    } else {
        const long nb = npix * ((nq + PS_QUADS - 1) / PS_QUADS);
        if ((r = blocks_ok(uc, table.md.name, nb * 256, &blocks))) return r;
        HLMI_LAUNCH(uc, "hannk_pool_split", ctx.stream, hannk_pool_split<AVG>, dim3(blocks), dim3(256), 0, g);
    }
    mark_output_written(output);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- host: mean
// ---- the plan: below MEAN_SPLIT_MIN_TAPS taps a thread per output walks them alone; above, the region is shared: across the lanes of
// a wave where c itself is reduced, across the waves of a workgroup otherwise.  HLMI_HANNK_MEAN_SPLIT (0 / 1) forces the choice.
constexpr int MEAN_SPLIT_MIN_TAPS = 16;
template<bool GENERAL>
int mean_entry(halide_buffer_t *input, int32_t c_min, int32_t c_extent, int32_t x_min, int32_t x_extent, int32_t y_min, int32_t y_extent, int32_t b_min,
               int32_t b_extent, halide_buffer_t *output) {
    void *uc = nullptr;
    BufArg args[2];
    mean_table.bufs(args, {input, output});
    own_lanes(args);
    int r = check_not_null(uc, args, 2);
    if (r || (r = check_type_and_dims(uc, args, 2))) return r;
    halide_dimension_t *id = input->dim, *od = output->dim;
    const int rmin[4] = {c_min, x_min, y_min, b_min}, rext[4] = {c_extent, x_extent, y_extent, b_extent};
    if (any_bounds_query(args, 2)) {
        // the input: [out.min(d) + d_min, out.max(d) + d_min + d_extent - 1]; a query output keeps the shape the caller gave it
        int mins[4], ext[4], omin[4], oext[4];
        for (int d = 0; d < 4; d++) {
            mins[d] = od[d].min + rmin[d], ext[d] = std::max(od[d].extent, 1) + std::max(rext[d], 1) - 1;
            omin[d] = od[d].min, oext[d] = od[d].extent;
        }
        answer_query(input, mins, ext);
        answer_query(output, omin, oext);
        return 0;
    }
    if ((r = check_shapes(uc, args, 2))) return r;
    bool empty = false, no_taps = false;
    for (int d = 0; d < 4; d++) empty = empty || od[d].extent <= 0, no_taps = no_taps || rext[d] <= 0;
    if (!empty && !no_taps)
        for (int d = 0; d < 4; d++) check_covers(uc, args[0], d, od[d].min + rmin[d], od[d].extent + rext[d] - 1);
    const std::optional<int> sw_split = env_int("HLMI_HANNK_MEAN_SPLIT");
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, 2))) return r;
    if (empty) {
        mark_output_written(output);
        return 0;
    }
    MeanGeom g = {};
    g.in = dev_ptr<uint8_t>(input), g.out = dev_ptr<uint8_t>(output);
    long outputs = 1, taps = 1;
    for (int d = 0; d < 4; d++) {
        g.oext[d] = od[d].extent, g.ostr[d] = od[d].stride, g.istr[d] = id[d].stride;
        g.rext[d] = no_taps ? 0 : rext[d];
        if (!no_taps) g.in += elem_offset(input, d, (long)od[d].min + rmin[d]);
        outputs *= od[d].extent, taps *= g.rext[d];
    }
    g.extent = wrap<32>((int64_t)wrap<32>((int64_t)wrap<32>((int64_t)c_extent * x_extent) * y_extent) * b_extent);
    const bool split = !GENERAL && taps < (1L << 30) && (sw_split ? *sw_split != 0 : taps >= MEAN_SPLIT_MIN_TAPS);
    timing_note_bytes((double)outputs + (double)(od[0].extent + std::max(rext[0], 1) - 1) * (od[1].extent + std::max(rext[1], 1) - 1) *
                                            (od[2].extent + std::max(rext[2], 1) - 1) * (od[3].extent + std::max(rext[3], 1) - 1));
    unsigned blocks;
    if (!split) {
        if ((r = blocks_ok(uc, "mean_uint8", outputs, &blocks))) return r;
        HLMI_LAUNCH(uc, "hannk_mean_general", ctx.stream, hannk_mean_general, dim3(blocks), dim3(256), 0, g);
    } else if (g.rext[0] > 1) {
        if ((r = blocks_ok(uc, "mean_uint8", outputs * 256, &blocks))) return r;
        HLMI_LAUNCH(uc, "hannk_mean_lanes", ctx.stream, hannk_mean_lanes, dim3(blocks), dim3(64), 0, g);
    } else {
        const long nb = (outputs / od[0].extent) * ((od[0].extent + 63) / 64);
        if ((r = blocks_ok(uc, "mean_uint8", nb * 256, &blocks))) return r;
        HLMI_LAUNCH(uc, "hannk_mean_wg", ctx.stream, hannk_mean_wg, dim3(blocks), dim3(256), 0, g);
    }
    mark_output_written(output);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- host: add, mul
// ---- the plan: rows of at least one whole 16-byte chunk go to hannk_ew (which decides per chunk whether its addresses allow the wide
// access); shorter rows have nothing to gain from it.  HLMI_HANNK_EW_VECTOR (0 / 1) forces the choice.
template<bool GENERAL, typename P>
int ew_entry(const ArgTable &table, halide_buffer_t *input1, halide_buffer_t *input2, halide_buffer_t *output, const P &p) {
    void *uc = nullptr;
    BufArg args[3];
    table.bufs(args, {input1, input2, output});
    own_lanes(args);
    int r = check_not_null(uc, args, 3);
    // built with no_bounds_query (apps/hannk/halide/CMakeLists.txt): an unallocated buffer is no query; every check below runs on it
    // and the host pointer check ends the call (src/AddImageChecks.cpp:713 leaves the early return out, :689 keeps asserts_host_non_null)
    if (r || (r = check_unallocated_types(uc, args, 3)) || (r = check_type_and_dims(uc, args, 3))) return r;
    halide_dimension_t *d1 = input1->dim, *d2 = input2->dim, *od = output->dim;
    check_shape_any_stride0(uc, args[0]);
    check_shape_any_stride0(uc, args[1]);
    check_shape(uc, args[2]);
    const bool empty = od[0].extent <= 0 || od[1].extent <= 0;
    if (!empty)
        for (int d = 0; d < 2; d++) {
            check_covers(uc, args[0], d, od[d].min, od[d].extent);
            check_covers(uc, args[1], d, od[d].min, od[d].extent);
        }
    const std::optional<int> sw_vector = env_int("HLMI_HANNK_EW_VECTOR");
    if ((r = check_unallocated_host(uc, args, 3))) return r;
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, 3))) return r;
    // the specialisations (elementwise_generator.cpp:51-58, :99-106): (1, 1), (1, 0), (0, 1); anything else is specialize_fail
    const int s1 = d1[0].stride, s2 = d2[0].stride;
    if (!((s1 == 1 && s2 == 1) || (s1 == 1 && s2 == 0) || (s1 == 0 && s2 == 1)))
        return report(uc, halide_error_code_specialize_fail, "A schedule specialized with specialize_fail() was chosen: input dimension 0 must have a stride of 0 or 1.");
    if (empty) {
        mark_output_written(output);
        return 0;
    }
    EwGeom g = {};
    g.W = od[0].extent, g.H = od[1].extent;
    g.a = dev_ptr<uint8_t>(input1) + elem_offset(input1, 0, od[0].min) + elem_offset(input1, 1, od[1].min);
    g.b = dev_ptr<uint8_t>(input2) + elem_offset(input2, 0, od[0].min) + elem_offset(input2, 1, od[1].min);
    g.out = dev_ptr<uint8_t>(output);
    g.a_s0 = s1, g.a_s1 = d1[1].stride, g.b_s0 = s2, g.b_s1 = d2[1].stride, g.o_s1 = od[1].stride;
    // rows that follow each other without a gap in all three buffers are one long row (MobileNet-v2's residual add: rows of 24 bytes)
    if (s1 == 1 && s2 == 1 && g.a_s1 == g.W && g.b_s1 == g.W && g.o_s1 == g.W && (long)g.W * g.H < (1L << 31)) g.W *= g.H, g.H = 1;
    const bool vector = !GENERAL && (sw_vector ? *sw_vector != 0 : g.W >= 16);
    timing_note_bytes((double)g.H * (g.W * (1.0 + s1 + s2) + (s1 ? 0 : 1) + (s2 ? 0 : 1)));
    unsigned blocks;
    if (vector) {
        if ((r = blocks_ok(uc, table.md.name, (long)((g.W + 15) / 16) * g.H, &blocks))) return r;
        HLMI_LAUNCH(uc, "hannk_ew", ctx.stream, hannk_ew<P>, dim3(blocks), dim3(256), 0, g, p);
    } else {
        if ((r = blocks_ok(uc, table.md.name, (long)g.W * g.H, &blocks))) return r;
        HLMI_LAUNCH(uc, "hannk_ew_general", ctx.stream, hannk_ew_general<P>, dim3(blocks), dim3(256), 0, g, p);
    }
    mark_output_written(output);
    return 0;
}
template<bool GENERAL>
int add_entry(halide_buffer_t *input1, uint8_t input1_zero, int16_t input1_multiplier, halide_buffer_t *input2, uint8_t input2_zero, int16_t input2_multiplier,
              uint8_t output_zero, uint8_t output_min, uint8_t output_max, halide_buffer_t *output) {
    const AddParams p = {input1_zero, input1_multiplier, input2_zero, input2_multiplier, output_zero, output_min, output_max};
    return ew_entry<GENERAL>(add_table, input1, input2, output, p);
}
template<bool GENERAL>
int mul_entry(halide_buffer_t *input1, uint8_t input1_zero, halide_buffer_t *input2, uint8_t input2_zero, uint8_t output_zero, int32_t output_multiplier,
              uint32_t output_shift, uint8_t output_min, uint8_t output_max, halide_buffer_t *output) {
    const MulParams p = {input1_zero, input2_zero, output_zero, output_multiplier, output_shift, output_min, output_max};
    return ew_entry<GENERAL>(mul_table, input1, input2, output, p);
}

// ---------------------------------------------------------------------------------------------------------------- host: softmax, l2_normalization
// ---- the plan: hannk_rows wherever both strides of dimension 0 are 1 (the general kernel walks the whole row once per output), keeping a
// row of at most ROW_KEEP_MAX elements in registers.  Switches: HLMI_HANNK_ROWS_WAVE (0: the general kernel), HLMI_HANNK_ROWS_KEEP (0:
// recompute in every pass).
template<bool L2, bool GENERAL>
int rows_entry(const ArgTable &table, halide_buffer_t *input, halide_buffer_t *output, const SoftmaxParams &p, int zero) {
    void *uc = nullptr;
    BufArg args[2];
    table.bufs(args, {input, output});
    own_lanes(args);
    int r = check_not_null(uc, args, 2);
    // no_bounds_query, as add and mul
    if (r || (r = check_unallocated_types(uc, args, 2)) || (r = check_type_and_dims(uc, args, 2))) return r;
    halide_dimension_t *id = input->dim, *od = output->dim;
    check_shape_any_stride0(uc, args[0]);   // normalizations_generator.cpp:56-57, :139-140
    check_shape_any_stride0(uc, args[1]);
    const bool empty = od[0].extent <= 0 || od[1].extent <= 0;
    if (!empty)
        for (int d = 0; d < 2; d++) check_covers(uc, args[0], d, od[d].min, od[d].extent);
    const std::optional<int> sw_wave = env_int("HLMI_HANNK_ROWS_WAVE"), sw_keep = env_int("HLMI_HANNK_ROWS_KEEP");
    if ((r = check_unallocated_host(uc, args, 2))) return r;
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, 2))) return r;
    if (empty) {
        mark_output_written(output);
        return 0;
    }
    RowGeom g = {};
    g.in = dev_ptr<uint8_t>(input) + elem_offset(input, 1, od[1].min);
    g.out = dev_ptr<uint8_t>(output);
    g.N = id[0].extent, g.W = od[0].extent, g.H = od[1].extent, g.xoff = od[0].min - id[0].min;
    g.i_s0 = id[0].stride, g.i_s1 = id[1].stride, g.o_s0 = od[0].stride, g.o_s1 = od[1].stride;
    g.zero = zero;
    const bool wave = !GENERAL && g.i_s0 == 1 && g.o_s0 == 1 && sw_wave.value_or(1) != 0;
    const bool keep = g.N <= ROW_KEEP_MAX && sw_keep.value_or(1) != 0;
    timing_note_bytes((double)g.H * ((double)g.N + g.W));
    unsigned blocks;
    if (!wave) {
        if ((r = blocks_ok(uc, table.md.name, (long)g.W * g.H, &blocks))) return r;
        HLMI_LAUNCH(uc, "hannk_rows_general", ctx.stream, hannk_rows_general<L2>, dim3(blocks), dim3(256), 0, g, p);
    } else {
        if ((r = blocks_ok(uc, table.md.name, (long)g.H * 64, &blocks))) return r;
        if (keep) HLMI_LAUNCH(uc, "hannk_rows", ctx.stream, (hannk_rows<L2, true>), dim3(blocks), dim3(256), 0, g, p);
        else HLMI_LAUNCH(uc, "hannk_rows", ctx.stream, (hannk_rows<L2, false>), dim3(blocks), dim3(256), 0, g, p);
    }
    mark_output_written(output);
    return 0;
}
template<bool GENERAL>
int softmax_entry(halide_buffer_t *input, int16_t beta_multiplier, uint16_t beta_shift, uint8_t output_zero, int16_t output_multiplier, uint16_t output_shift,
                  halide_buffer_t *output) {
    const SoftmaxParams p = {beta_multiplier, beta_shift, output_zero, output_multiplier, output_shift};
    return rows_entry<false, GENERAL>(softmax_table, input, output, p, 0);
}
template<bool GENERAL>
int l2_entry(halide_buffer_t *input, uint8_t input_zero, halide_buffer_t *output) {
    return rows_entry<true, GENERAL>(l2_table, input, output, SoftmaxParams{}, input_zero);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------- the entry points
#define HLMI_HANNK_ENTRY(name, table)                                             \
    int name##_argv(void **a) { return ::hlmi::argv_call(name, a); }              \
    const halide_filter_metadata_t *name##_metadata() { return &(table).md; }
namespace hannk {

int average_pool_uint8(halide_buffer_t *input, int32_t stride_x, int32_t stride_y, int32_t filter_width, int32_t filter_height, uint8_t output_min,
                       uint8_t output_max, halide_buffer_t *output) {
    return pool_entry<true, false>(input, stride_x, stride_y, filter_width, filter_height, output_min, output_max, output);
}
int max_pool_uint8(halide_buffer_t *input, int32_t stride_x, int32_t stride_y, int32_t filter_width, int32_t filter_height, uint8_t output_min,
                   uint8_t output_max, halide_buffer_t *output) {
    return pool_entry<false, false>(input, stride_x, stride_y, filter_width, filter_height, output_min, output_max, output);
}
int mean_uint8(halide_buffer_t *input, int32_t c_min, int32_t c_extent, int32_t x_min, int32_t x_extent, int32_t y_min, int32_t y_extent, int32_t b_min,
               int32_t b_extent, halide_buffer_t *output) {
    return mean_entry<false>(input, c_min, c_extent, x_min, x_extent, y_min, y_extent, b_min, b_extent, output);
}
int add_uint8_uint8(halide_buffer_t *input1, uint8_t input1_zero, int16_t input1_multiplier, halide_buffer_t *input2, uint8_t input2_zero,
                    int16_t input2_multiplier, uint8_t output_zero, uint8_t output_min, uint8_t output_max, halide_buffer_t *output) {
    return add_entry<false>(input1, input1_zero, input1_multiplier, input2, input2_zero, input2_multiplier, output_zero, output_min, output_max, output);
}
int mul_uint8_uint8_uint8(halide_buffer_t *input1, uint8_t input1_zero, halide_buffer_t *input2, uint8_t input2_zero, uint8_t output_zero,
                          int32_t output_multiplier, uint32_t output_shift, uint8_t output_min, uint8_t output_max, halide_buffer_t *output) {
    return mul_entry<false>(input1, input1_zero, input2, input2_zero, output_zero, output_multiplier, output_shift, output_min, output_max, output);
}
int softmax_uint8(halide_buffer_t *input, int16_t beta_multiplier, uint16_t beta_shift, uint8_t output_zero, int16_t output_multiplier,
                  uint16_t output_shift, halide_buffer_t *output) {
    return softmax_entry<false>(input, beta_multiplier, beta_shift, output_zero, output_multiplier, output_shift, output);
}
int l2_normalization_uint8(halide_buffer_t *input, uint8_t input_zero, halide_buffer_t *output) { return l2_entry<false>(input, input_zero, output); }
HLMI_HANNK_ENTRY(average_pool_uint8, avg_table)
HLMI_HANNK_ENTRY(max_pool_uint8, max_table)
HLMI_HANNK_ENTRY(mean_uint8, mean_table)
HLMI_HANNK_ENTRY(add_uint8_uint8, add_table)
HLMI_HANNK_ENTRY(mul_uint8_uint8_uint8, mul_table)
HLMI_HANNK_ENTRY(softmax_uint8, softmax_table)
HLMI_HANNK_ENTRY(l2_normalization_uint8, l2_table)

}  // namespace hannk
#undef HLMI_HANNK_ENTRY

int hlmi::hannk_nn_general(const char *name, void **argv) {
    if (!strcmp(name, "average_pool_uint8")) return argv_call(pool_entry<true, true>, argv);
    if (!strcmp(name, "max_pool_uint8")) return argv_call(pool_entry<false, true>, argv);
    if (!strcmp(name, "mean_uint8")) return argv_call(mean_entry<true>, argv);
    if (!strcmp(name, "add_uint8_uint8")) return argv_call(add_entry<true>, argv);
    if (!strcmp(name, "mul_uint8_uint8_uint8")) return argv_call(mul_entry<true>, argv);
    if (!strcmp(name, "softmax_uint8")) return argv_call(softmax_entry<true>, argv);
    if (!strcmp(name, "l2_normalization_uint8")) return argv_call(l2_entry<true>, argv);
    return hannk_program_general(name, argv);   // the elementwise programs, copy, fill and upsample_channels
}

// x, out: host pointers to n elements.  One launch.
extern "C" int hlmi_debug_hannk_approx(int fn, int32_t q, const int32_t *x, size_t n, int32_t q_x, int32_t bits, int32_t *out) {
    if (fn < 0 || fn > 3 || !x || !out || n == 0 || (n + 255) / 256 > 0x7fffffffu || (bits != 16 && bits != 32) || q < 0 || q > 30 || q_x < 0) return -1;
    void *d[2] = {nullptr, nullptr};
    int rc = 0;
    for (int i = 0; i < 2 && !rc; i++)
        if (hipMalloc(&d[i], 4 * n) != hipSuccess) rc = -2;
    if (!rc && hipMemcpy(d[0], x, 4 * n, hipMemcpyHostToDevice) != hipSuccess) rc = -3;
    if (!rc) {
        hipLaunchKernelGGL(dbg_hannk_approx, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, fn, (int)q, (const int32_t *)d[0], n, (int)q_x, (int)bits, (int32_t *)d[1]);
        if (hipGetLastError() != hipSuccess || hipMemcpy(out, d[1], 4 * n, hipMemcpyDeviceToHost) != hipSuccess) rc = -4;
    }
    for (int i = 0; i < 2; i++)
        if (d[i]) (void)hipFree(d[i]);
    return rc;
}
