// hannk_conv.hip — the quantised convolution ops of apps/hannk's op library (apps/hannk/halide/conv_generator.cpp,
// depthwise_conv_generator.cpp, common_halide.cpp), C++-mangled in namespace hannk as the reference builds them:
//   hannk::tile_conv_filter_uint8, hannk::conv_u8_u8_u8, hannk::conv_u8_u8_i16, hannk::depthwise_conv_uint8,
//   hannk::depthwise_conv_broadcast_uint8, hannk::depthwise_conv_shallow_uint8, each with _argv and _metadata (include/aot/halide/<name>.h).
//
// The contract is integer throughout and is the same in both builds of the library: no float is touched.
//   tile    output(ci, bi, co, bo, x, y) = u8(i16(in(co*4 + ci, x, y, bo*16 + bi)) - i16(input_zero) + output_zero), in = input_zero
//           outside the input
//   conv    acc(c, x, y, b) = bias(c) + sum over ry, rx, rz of (in(rz, x*sx + rx*dx, y*sy + ry*dy, b) - input_zero)
//                                                              * (filter(rz % 4, c % 16, rz / 4, c / 16, rx, ry) - filter_zero), mod 2^32
//   depthw. acc(c, x, y, b) = bias(c) + sum over ry, rx of (filter(c, rx, ry) - filter_zero) * (in(c * inv, x*sx + rx*dx, y*sy + ry*dy, b) - input_zero)
//   shallow the depthwise sum with c the fused c-x index of an output whose x is 0: filter and bias at (c % 16) % D, the input at
//           (c + rx*dx*input_stride_x, 0, y*sy + ry*dy, b): a template flag on the two depthwise kernels
//   out     quantize_i16 = i16_sat(rounding_shift_right(multiply_2x_high(acc, multiplier), shift)); quantize_and_relu_u8 =
//           max(min(u8_sat(sat_add_i16(quantize_i16, zero)), hi), lo)
// The layout constants (4, 16, 16) are in include/aot/halide/hannk_target.h.
//
// Kernels:
//   hannk_tile_filter   one thread per output byte (the only implementation: default and general)
//   hannk_conv_mfma     the default conv path: an implicit GEMM on v_mfma_i32_16x16x64_i8, D[co][pixel] = sum_k F[co][k] I[k][pixel] with
//                       k = (ry, rx, rz).  The tiled filter holds 4 k-bytes of one co in a dword and consecutive co in consecutive
//                       dwords, so a wave's filter fragment is four coalesced dword loads per k-block and needs no re-ordering; the
//                       input fragment is four dwords (16 contiguous bytes where ci % 16 == 0) of a pixel's channel run.  Nothing is
//                       staged in LDS: a wave owns 32 co x 32 pixels (2 x 2 MFMA tiles), neighbouring waves share their pixels through
//                       L1.  The instruction is signed and the operands are u8: both are re-centred by ^ 0x80 (x' = x - 128) in
//                       registers, and with az' = input_zero - 128, fz' = filter_zero - 128 the exact identity
//                           sum (a - az)(f - fz) = sum a'f' - fz' sum a' - az' sum f' + K az' fz'
//                       gives the contract's sum; sum a' per pixel and sum f' per co come from the fragments themselves (v_sad_u8 on
//                       the bytes as loaded: one VALU op per dword, no pre-pass and nothing to cache).  k past the end is padded with
//                       0x80 bytes (a' = f' = 0) on both sides.  Everything is u32 arithmetic: it wraps like the contract's i32.
//                       The lane's four accumulators are four consecutive co of one pixel (C/D map: col = lane & 15 the pixel,
//                       row = 4 (lane >> 4) + r the co): the epilogue quantizes them in registers and stores one dword (u8) or 8 bytes (i16).
//   split-K             where the plan finds too few wave tiles for the device: blockIdx.y owns a range of k-blocks, writes its partial
//                       (corrections included: they are linear in the k range) as i32 into the scratch arena, and hannk_conv_finish adds the
//                       partials in split order, the bias, and runs the epilogue.  i32 addition wraps associatively: the bytes cannot
//                       depend on the number of splits or on their order, and no atomic is used.
//   hannk_dw            the default depthwise path where the output fills the device (dw_vector): a lane owns 4 adjacent channels of
//                       4 output rows of one pixel column, one dword load per tap, the filter taps of its channels in registers (3 x 3
//                       unrolled; any other size loops and re-reads them through L1); the input_zero term is folded into the bias
//                       (offset_c of the generator)
//   hannk_*_general     one thread per output, byte loads, the loops as written above: hlmi_hannk_general, the default path where the
//                       device pointers are not dword-aligned, and small depthwise outputs (dw_vector)
//
// Host path: every entry point reads top to bottom: check arguments -> bounds query -> device and buffers -> empty output -> plan ->
// stages -> mark_output_written.  hannk_conv_plan() chooses kernel, tiling and splits without a HIP call.
#include "hlmi_internal.h"
#include "hannk_entry.h"
#include "hannk_math.h"

#include "aot/halide/hannk_target.h"

using namespace hlmi;

namespace {

constexpr int VR = HLMI_HANNK_VECTOR_REDUCTION, VT = HLMI_HANNK_ACCUM_VECTOR_SIZE, DV = HLMI_HANNK_DEPTHWISE_VECTOR;
constexpr int FTILE = VR * VT;    // bytes of one (ci / 4, co / 16) filter tile: filter.dim(2).stride and the filter's host alignment
constexpr int KB_QUADS = 16;      // channel quads (dwords) per MFMA k-block of 64
constexpr int WAVE_PX = 32;      // a wave's tile: 32 pixels x 32 co, 2 x 2 MFMA tiles of 16 x 16
constexpr int DW_ROWS = 4;        // output rows per thread of hannk_dw

typedef int v4i __attribute__((ext_vector_type(4)));

// n / d for 0 <= n < 2^31 by a multiply and a shift (conv_layer_bf16.hip has the derivation)
struct FastDiv {
    uint32_t m, sh, d;
};
FastDiv make_fastdiv(uint32_t d) {
    FastDiv f;
    uint32_t s = 0;
    while ((1ull << s) < d) s++;
    f.m = (uint32_t)((((unsigned long long)1 << (31 + s)) + d - 1) / d);
    f.sh = 31 + s, f.d = d;
    return f;
}
__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FastDiv &f) { return (uint32_t)(((unsigned long long)n * f.m) >> f.sh); }

// ---------------------------------------------------------------------------------------------------------------- the epilogue
// Quant, multiply_2x_high, rounding_shift_right, quantize_i16 and quantize_and_relu_u8 are in hannk_math.h, shared with hannk_nn.hip
using namespace hlmi::hannk_math;
using namespace hlmi::hannk_entry;

// four consecutive channels c .. c + 3 of one pixel: one packed store where all four exist and the address allows it
template<bool I16>
__device__ __forceinline__ void store4(void *out, long off, int c, int C, const uint32_t (&acc)[4], const Quant &q) {
    if (I16) {
        int16_t *p = (int16_t *)out + off;
        int32_t v[4];
#pragma unroll
        for (int r = 0; r < 4; r++) v[r] = quantize_i16((int32_t)acc[r], q);
        if (c + 3 < C && ((uintptr_t)p & 7) == 0) {
            *reinterpret_cast<uint2 *>(p) = make_uint2(((uint32_t)v[0] & 0xffffu) | ((uint32_t)v[1] << 16), ((uint32_t)v[2] & 0xffffu) | ((uint32_t)v[3] << 16));
        } else {
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (c + r < C) p[r] = (int16_t)v[r];
        }
    } else {
        uint8_t *p = (uint8_t *)out + off;
        uint32_t v[4];
#pragma unroll
        for (int r = 0; r < 4; r++) v[r] = (uint32_t)quantize_and_relu_u8((int32_t)acc[r], q);
        if (c + 3 < C && ((uintptr_t)p & 3) == 0) {
            *reinterpret_cast<uint32_t *>(p) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        } else {
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (c + r < C) p[r] = (uint8_t)v[r];
        }
    }
}

__global__ __launch_bounds__(256) void dbg_hannk_quantize(int fn, const int32_t *__restrict__ acc, size_t n, Quant q, void *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (fn == 0) ((int16_t *)out)[i] = (int16_t)quantize_i16(acc[i], q);
    else ((uint8_t *)out)[i] = (uint8_t)quantize_and_relu_u8(acc[i], q);
}

// ---------------------------------------------------------------------------------------------------------------- tile_conv_filter
struct TileGeom {
    const uint8_t *in;        // element (min0, min1, min2, min3) of the input
    uint8_t *out;
    int imin[4], iext[4];
    long istr[4];
    int omin[6], oext[6];
    long ostr[6];
    int input_zero, output_zero;
    long total;
};
__global__ __launch_bounds__(256) void hannk_tile_filter(TileGeom g) {
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.total) return;
    int p[6];
    long o = 0;
#pragma unroll
    for (int d = 0; d < 6; d++) {
        const int e = g.oext[d];
        const int v = (int)(i % e);
        i /= e;
        o += v * g.ostr[d];
        p[d] = v + g.omin[d];
    }
    const int at[4] = {p[2] * VR + p[0], p[4], p[5], p[3] * VT + p[1]};   // (c, x, y, b) of the input
    bool inside = true;
    long s = 0;
#pragma unroll
    for (int d = 0; d < 4; d++) {
        const int r = at[d] - g.imin[d];
        inside = inside && r >= 0 && r < g.iext[d];
        s += r * g.istr[d];
    }
    const int v = inside ? g.in[s] : g.input_zero;
    g.out[o] = (uint8_t)(v - g.input_zero + g.output_zero);   // i16 arithmetic never wraps here; the cast to u8 does
}

// ---------------------------------------------------------------------------------------------------------------- conv
struct ConvGeom {
    const uint8_t *in;        // the input element the output's first pixel reads at tap (0, 0), channel 0
    const uint8_t *filt;
    const int32_t *bias;
    void *out;                // element (0, xmin, ymin, bmin) of the output
    int C, OW, OH, OB;        // output extents
    long npix;
    long in_sx, in_sy, in_sb; // input strides of x, y, b
    long o_sx, o_sy, o_sb;
    long f_s3, f_s4, f_s5;    // filter strides of co / 16, fx, fy
    int sx, sy, dx, dy, FW, FH, CQ;   // CQ = filter.dim(2).extent: channel quads
    int az, fz;               // the zero points
    Quant q;
};

template<bool I16>
__global__ __launch_bounds__(256) void hannk_conv_general(ConvGeom g) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.npix * g.C) return;
    const int c = (int)(i % g.C);
    const long p = i / g.C;
    const int x = (int)(p % g.OW), y = (int)((p / g.OW) % g.OH), b = (int)(p / ((long)g.OW * g.OH));
    const uint8_t *in = g.in + b * g.in_sb + (long)y * g.sy * g.in_sy + (long)x * g.sx * g.in_sx;
    const uint8_t *f = g.filt + (c / VT) * g.f_s3 + (c % VT) * VR;
    uint32_t acc = (uint32_t)g.bias[c];
    for (int ry = 0; ry < g.FH; ry++)
        for (int rx = 0; rx < g.FW; rx++)
            for (int rz = 0; rz < VR * g.CQ; rz++) {
                const int a = in[(long)ry * g.dy * g.in_sy + (long)rx * g.dx * g.in_sx + rz];
                const int w = f[ry * g.f_s5 + rx * g.f_s4 + (long)(rz / VR) * FTILE + rz % VR];
                acc += (uint32_t)((a - g.az) * (w - g.fz));
            }
    const long o = b * g.o_sb + y * g.o_sy + x * g.o_sx + c;
    if (I16) ((int16_t *)g.out)[o] = (int16_t)quantize_i16((int32_t)acc, g.q);
    else ((uint8_t *)g.out)[o] = (uint8_t)quantize_and_relu_u8((int32_t)acc, g.q);
}

struct ConvTiling {
    int nkb, kb_per_split, splits;   // k-blocks of 64 in all, per split, splits
    int total_quads;                 // FH * FW * CQ
    int ncp, co16;                   // wave tiles along co; filter tiles of 16 co the output needs
    long wave_tiles;
    long ws_row;                     // i32 per pixel of a split-K partial: 16 co16
    FastDiv d_cq, d_fw;
};

// VEC: CQ % 4 == 0, so a lane's four quads of a k-block belong to one tap and are 16 contiguous input bytes
// SPLIT: partials to the arena (part), no bias, no epilogue
template<bool VEC, bool SPLIT, bool I16>
__global__ __launch_bounds__(256) void hannk_conv_mfma(ConvGeom g, ConvTiling t, int32_t *__restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long wt = (long)blockIdx.x * 4 + wave;
    if (wt >= t.wave_tiles) return;   // (no barrier in this kernel)
    const int cp = (int)(wt % t.ncp);
    const long pt = wt / t.ncp;
    const int split = blockIdx.y;
    const int kb0 = split * t.kb_per_split, kb1 = min(kb0 + t.kb_per_split, t.nkb);
    const int r16 = lane & 15, grp = lane >> 4;

    long in_off[2], f_off[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const long p = min(pt * WAVE_PX + 16 * j + r16, g.npix - 1);   // a tail pixel is computed from the last one and never stored
        const int x = (int)(p % g.OW), y = (int)((p / g.OW) % g.OH), b = (int)(p / ((long)g.OW * g.OH));
        in_off[j] = b * g.in_sb + (long)y * g.sy * g.in_sy + (long)x * g.sx * g.in_sx;
    }
#pragma unroll
    for (int i = 0; i < 2; i++) f_off[i] = (long)min(cp * 2 + i, t.co16 - 1) * g.f_s3 + 4 * r16;   // (the filter covers co16 tiles: checked)

    v4i acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[i][j] = v4i{0, 0, 0, 0};
    uint32_t sa[2] = {0, 0}, sf[2] = {0, 0};   // byte sums of the fragments as loaded (u8), this lane's share of k

    for (int kb = kb0; kb < kb1; kb++) {
        uint32_t fa[2][4], fb[2][4];
        const int kq0 = kb * KB_QUADS + 4 * grp;
        if (VEC) {
            const bool valid = kq0 < t.total_quads;   // with CQ % 4 == 0 the four quads are valid together
            const uint32_t kqc = valid ? kq0 : 0;
            const uint32_t tap = fdiv(kqc, t.d_cq), q = kqc - tap * g.CQ, ry = fdiv(tap, t.d_fw), rx = tap - ry * g.FW;
            const long ao = (long)ry * g.dy * g.in_sy + (long)rx * g.dx * g.in_sx + 4 * q, fo = ry * g.f_s5 + rx * g.f_s4 + (long)q * FTILE;
#pragma unroll
            for (int e = 0; e < 4; e++) {
#pragma unroll
                for (int j = 0; j < 2; j++) fb[j][e] = valid ? *reinterpret_cast<const uint32_t *>(g.in + in_off[j] + ao + 4 * e) : 0x80808080u;
#pragma unroll
                for (int i = 0; i < 2; i++) fa[i][e] = valid ? *reinterpret_cast<const uint32_t *>(g.filt + f_off[i] + fo + e * FTILE) : 0x80808080u;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const bool valid = kq0 + e < t.total_quads;
                const uint32_t kqc = valid ? kq0 + e : 0;
                const uint32_t tap = fdiv(kqc, t.d_cq), q = kqc - tap * g.CQ, ry = fdiv(tap, t.d_fw), rx = tap - ry * g.FW;
                const long ao = (long)ry * g.dy * g.in_sy + (long)rx * g.dx * g.in_sx + 4 * q, fo = ry * g.f_s5 + rx * g.f_s4 + (long)q * FTILE;
#pragma unroll
                for (int j = 0; j < 2; j++) fb[j][e] = valid ? *reinterpret_cast<const uint32_t *>(g.in + in_off[j] + ao) : 0x80808080u;
#pragma unroll
                for (int i = 0; i < 2; i++) fa[i][e] = valid ? *reinterpret_cast<const uint32_t *>(g.filt + f_off[i] + fo) : 0x80808080u;
            }
        }
        v4i va[2], vb[2];
#pragma unroll
        for (int e = 0; e < 4; e++) {
#pragma unroll
            for (int j = 0; j < 2; j++) {
                sa[j] = __builtin_amdgcn_sad_u8(fb[j][e], 0u, sa[j]);
                vb[j][e] = (int)(fb[j][e] ^ 0x80808080u);
            }
#pragma unroll
            for (int i = 0; i < 2; i++) {
                sf[i] = __builtin_amdgcn_sad_u8(fa[i][e], 0u, sf[i]);
                va[i][e] = (int)(fa[i][e] ^ 0x80808080u);
            }
        }
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(va[i], vb[j], acc[i][j], 0, 0, 0);
    }

    // the four lane groups hold four shares of k: their sum is the fragment row's (column's) byte sum
#pragma unroll
    for (int j = 0; j < 2; j++) {
        sa[j] += __shfl_xor(sa[j], 16);
        sa[j] += __shfl_xor(sa[j], 32);
        sf[j] += __shfl_xor(sf[j], 16);
        sf[j] += __shfl_xor(sf[j], 32);
    }
    const uint32_t kpad = (uint32_t)(kb1 - kb0) * 64u;                                                       // bytes summed, padding included
    const uint32_t kreal = (uint32_t)max(min(kb1 * KB_QUADS, t.total_quads) - kb0 * KB_QUADS, 0) * 4u;       // k of the contract in this range
    const uint32_t azp = (uint32_t)(g.az - 128), fzp = (uint32_t)(g.fz - 128);
    const uint32_t konst = kreal * azp * fzp;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int ct = cp * 2 + i;
        if (ct >= t.co16) continue;   // (wave-uniform)
        const int c0 = ct * VT + 4 * grp;
        uint32_t sfr[4], bias[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            sfr[r] = (uint32_t)__shfl((int)sf[i], 4 * grp + r) - 128u * kpad;   // lane 4 grp + r holds the sum of fragment row 4 grp + r
            bias[r] = (!SPLIT && c0 + r < g.C) ? (uint32_t)g.bias[c0 + r] : 0u;
        }
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const long p = pt * WAVE_PX + 16 * j + r16;
            const uint32_t sap = sa[j] - 128u * kpad;
            uint32_t v[4];
#pragma unroll
            for (int r = 0; r < 4; r++) v[r] = (uint32_t)acc[i][j][r] - fzp * sap - azp * sfr[r] + konst + bias[r];
            if (p >= g.npix) continue;
            if (SPLIT) {
                *reinterpret_cast<v4i *>(part + ((long)split * g.npix + p) * t.ws_row + c0) = v4i{(int)v[0], (int)v[1], (int)v[2], (int)v[3]};
            } else if (c0 < g.C) {
                const int x = (int)(p % g.OW), y = (int)((p / g.OW) % g.OH), b = (int)(p / ((long)g.OW * g.OH));
                store4<I16>(g.out, b * g.o_sb + y * g.o_sy + x * g.o_sx + c0, c0, g.C, v, g.q);
            }
        }
    }
}

// the second launch of a split-K call: partials in split order + bias, the epilogue, the packed store
template<bool I16>
__global__ __launch_bounds__(256) void hannk_conv_finish(ConvGeom g, ConvTiling t, const int32_t *__restrict__ part) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int nq = (g.C + 3) / 4;
    if (i >= g.npix * nq) return;
    const int c0 = (int)(i % nq) * 4;
    const long p = i / nq;
    uint32_t v[4];
#pragma unroll
    for (int r = 0; r < 4; r++) v[r] = c0 + r < g.C ? (uint32_t)g.bias[c0 + r] : 0u;
    for (int s = 0; s < t.splits; s++) {
        const v4i w = *reinterpret_cast<const v4i *>(part + ((long)s * g.npix + p) * t.ws_row + c0);
#pragma unroll
        for (int r = 0; r < 4; r++) v[r] += (uint32_t)w[r];
    }
    const int x = (int)(p % g.OW), y = (int)((p / g.OW) % g.OH), b = (int)(p / ((long)g.OW * g.OH));
    store4<I16>(g.out, b * g.o_sb + y * g.o_sy + x * g.o_sx + c0, c0, g.C, v, g.q);
}

// ---------------------------------------------------------------------------------------------------------------- depthwise
struct DwGeom {
    const uint8_t *in;        // as ConvGeom::in
    const uint8_t *filt;      // element (0, 0, 0)
    const int32_t *bias;
    uint8_t *out;
    int C, OW, OH, OB;
    long in_sx, in_sy, in_sb;
    long o_sx, o_sy, o_sb;
    long f_sx, f_sy;
    int sx, sy, dx, dy, FW, FH;
    int az, fz;
    int D;                    // the shallow variant: the filter's extent 0
    Quant q;
};
// The shallow variant (depthwise_conv_generator.cpp:75-83, :124-125): c is the fused c-x index of an output whose dimension 1 is {0, 1};
// filter and bias repeat at multiples of the channel vector, then of the filter's depth.  The host passes input_stride_x as in_sx, so
// with x = 0 the tap address rx * dx * in_sx is the generator's c + rx * dilation_x * input_stride_x.
template<bool SHALLOW>
__device__ __forceinline__ int dw_filter_c(const DwGeom &g, int c) { return SHALLOW ? (c % DV) % g.D : c; }

template<bool BCAST, bool SHALLOW = false>
__global__ __launch_bounds__(256) void hannk_dw_general(DwGeom g) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)g.C * g.OW * g.OH * g.OB) return;
    const int c = (int)(i % g.C);
    const long p = i / g.C;
    const int x = (int)(p % g.OW), y = (int)((p / g.OW) % g.OH), b = (int)(p / ((long)g.OW * g.OH));
    const uint8_t *in = g.in + b * g.in_sb + (long)y * g.sy * g.in_sy + (long)x * g.sx * g.in_sx + (BCAST ? 0 : c);
    const int fc = dw_filter_c<SHALLOW>(g, c);
    uint32_t acc = (uint32_t)g.bias[fc];
    for (int ry = 0; ry < g.FH; ry++)
        for (int rx = 0; rx < g.FW; rx++) {
            const int a = in[(long)ry * g.dy * g.in_sy + (long)rx * g.dx * g.in_sx];
            const int w = g.filt[fc + rx * g.f_sx + ry * g.f_sy];
            acc += (uint32_t)((w - g.fz) * (a - g.az));
        }
    g.out[b * g.o_sb + y * g.o_sy + x * g.o_sx + c] = (uint8_t)quantize_and_relu_u8((int32_t)acc, g.q);
}

// K3: the 3 x 3 specialisation (taps in registers, loops unrolled).  A thread: channels 4 cq .. 4 cq + 3 of DW_ROWS output rows of
// one (x, b).  The input covers round_up(C, 16) channels (checked), so the dword at channel 4 cq is inside it whenever 4 cq < C; filter
// and bias are read at [0, C) only.  SHALLOW: the plan has checked that C is a multiple of 4 and every tap offset too, so each dword
// lies inside the fused row.
template<bool K3, bool BCAST, bool SHALLOW = false>
__global__ __launch_bounds__(256) void hannk_dw(DwGeom g) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int nq = (g.C + 3) / 4, nyb = (g.OH + DW_ROWS - 1) / DW_ROWS;
    if (i >= (long)nq * g.OW * nyb * g.OB) return;
    const int c0 = (int)(i % nq) * 4;
    long p = i / nq;
    const int x = (int)(p % g.OW);
    p /= g.OW;
    const int y0 = (int)(p % nyb) * DW_ROWS, b = (int)(p / nyb);
    const int FW = K3 ? 3 : g.FW, FH = K3 ? 3 : g.FH;
    constexpr int UNR = K3 ? 3 : 1;
    auto tap = [&](int c, int rx, int ry) { return c < g.C ? (int)g.filt[dw_filter_c<SHALLOW>(g, c) + rx * g.f_sx + ry * g.f_sy] - g.fz : 0; };
    // offset_c = bias - input_zero * sum of the zeroed taps
    uint32_t off[4];
    int w[K3 ? 9 : 1][4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        int s = 0;
        for (int ry = 0; ry < FH; ry++)
            for (int rx = 0; rx < FW; rx++) {
                const int v = tap(c0 + r, rx, ry);
                if (K3) w[ry * 3 + rx][r] = v;
                s += v;
            }
        off[r] = (c0 + r < g.C ? (uint32_t)g.bias[dw_filter_c<SHALLOW>(g, c0 + r)] : 0u) - (uint32_t)g.az * (uint32_t)s;
    }
    const uint8_t *in = g.in + b * g.in_sb + (long)x * g.sx * g.in_sx + (BCAST ? 0 : c0);
    for (int y = y0; y < min(y0 + DW_ROWS, g.OH); y++) {
        uint32_t acc[4] = {off[0], off[1], off[2], off[3]};
        const uint8_t *row = in + (long)y * g.sy * g.in_sy;
#pragma unroll UNR
        for (int ry = 0; ry < FH; ry++)
#pragma unroll UNR
            for (int rx = 0; rx < FW; rx++) {
                const uint8_t *at = row + (long)ry * g.dy * g.in_sy + (long)rx * g.dx * g.in_sx;
                const uint32_t d = BCAST ? (uint32_t)at[0] * 0x01010101u : *reinterpret_cast<const uint32_t *>(at);
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int wt = K3 ? w[K3 ? ry * 3 + rx : 0][r] : tap(c0 + r, rx, ry);
                    acc[r] += (uint32_t)(wt * (int)((d >> (8 * r)) & 0xffu));
                }
            }
        store4<false>(g.out, b * g.o_sb + y * g.o_sy + x * g.o_sx + c0, c0, g.C, acc, g.q);
    }
}

// ---------------------------------------------------------------------------------------------------------------- host: tables
// (L, own_lanes, blocks_ok, check_stride_multiple and check_dim are in hannk_entry.h, shared with hannk_nn.hip)
#define HLMI_HANNK_CONV_HEAD(FD)                                                                                                            \
    L(in_buf("input", T_U8, 4)), L(scalar_u8("input_zero")), L(in_buf("filter", T_U8, FD)), L(scalar_u8("filter_zero")), L(in_buf("bias", T_I32, 1)), \
        L(scalar_i32("stride_x")), L(scalar_i32("stride_y")), L(scalar_i32("dilation_x")), L(scalar_i32("dilation_y"))
#define HLMI_HANNK_CONV_TAIL(OT)                                                                                                        \
    L(scalar_i32("output_multiplier")), L(scalar_i32("output_shift")), L(scalar_u8("output_zero")), L(scalar_u8("output_min")), L(scalar_u8("output_max")), \
        L(out_buf("output", OT, 4))
const ArgTable tile_table("tile_conv_filter_uint8",
                          {L(in_buf("input", T_U8, 4)), L(scalar_u8("input_zero")), L(scalar_u8("output_zero")), L(out_buf("output", T_U8, 6))});
const ArgTable conv_u8_table("conv_u8_u8_u8", {HLMI_HANNK_CONV_HEAD(6), HLMI_HANNK_CONV_TAIL(T_U8)});
const ArgTable conv_i16_table("conv_u8_u8_i16", {HLMI_HANNK_CONV_HEAD(6), HLMI_HANNK_CONV_TAIL(T_I16)});
const ArgTable dw_table("depthwise_conv_uint8", {HLMI_HANNK_CONV_HEAD(3), L(scalar_i32("input_stride_x")), HLMI_HANNK_CONV_TAIL(T_U8)});
const ArgTable dwb_table("depthwise_conv_broadcast_uint8", {HLMI_HANNK_CONV_HEAD(3), L(scalar_i32("input_stride_x")), HLMI_HANNK_CONV_TAIL(T_U8)});
const ArgTable dws_table("depthwise_conv_shallow_uint8", {HLMI_HANNK_CONV_HEAD(3), L(scalar_i32("input_stride_x")), HLMI_HANNK_CONV_TAIL(T_U8)});
#undef HLMI_HANNK_CONV_HEAD
#undef HLMI_HANNK_CONV_TAIL

const int k0 = 0, k1 = 1, k4 = VR, k16 = VT, k64 = FTILE;

// the input region of an output span [omin, omin + oext) under stride s and taps 0 .. (f - 1) * d
void in_span(int omin, int oext, int s, int f, int d, int *imin, int *iext) {
    const long a0 = (long)omin * s, a1 = (long)(omin + oext - 1) * s, t = (long)(f - 1) * d;
    const long lo = std::min(a0, a1) + std::min(0L, t), hi = std::max(a0, a1) + std::max(0L, t);
    *imin = (int)lo, *iext = (int)(hi - lo + 1);
}

// ---------------------------------------------------------------------------------------------------------------- host: tile
int tile_entry(halide_buffer_t *input, uint8_t input_zero, uint8_t output_zero, halide_buffer_t *output) {
    void *uc = nullptr;
    BufArg args[2];
    tile_table.bufs(args, {input, output});
    own_lanes(args);
    int r = check_not_null(uc, args, 2);
    if (r || (r = check_type_and_dims(uc, args, 2))) return r;
    halide_dimension_t *od = output->dim;
    if (any_bounds_query(args, 2)) {
        // the output: the tiling's two fixed dimensions and its tile stride; the input: every element the output's box names
        // (constant_exterior keeps a real input's own box: nothing is asked of it)
        if (!buffer_is_real(output)) {
            int mins[6], ext[6];
            for (int d = 0; d < 6; d++) mins[d] = d < 3 ? 0 : od[d].min, ext[d] = d == 0 ? VR : d == 1 ? VT : std::max(od[d].extent, 1);
            answer_query(output, mins, ext);
        }
        const int mins[4] = {0, od[4].min, od[5].min, od[3].min * VT}, ext[4] = {od[2].extent * VR, od[4].extent, od[5].extent, od[3].extent * VT};
        answer_query(input, mins, ext);
        return 0;
    }
    // conv_generator.cpp:353-355
    check_dim(uc, "output", output, 0, &k0, &k4, nullptr);
    check_dim(uc, "output", output, 1, &k0, &k16, &k4);
    check_dim(uc, "output", output, 2, &k0, nullptr, &k64);
    if ((r = check_shapes(uc, args, 2))) return r;
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, 2))) return r;
    TileGeom g = {};
    g.total = 1;
    for (int d = 0; d < 6; d++) g.omin[d] = od[d].min, g.oext[d] = od[d].extent, g.ostr[d] = od[d].stride, g.total *= od[d].extent;
    for (int d = 0; d < 4; d++) g.imin[d] = input->dim[d].min, g.iext[d] = input->dim[d].extent, g.istr[d] = input->dim[d].stride;
    g.in = dev_ptr<uint8_t>(input), g.out = dev_ptr<uint8_t>(output);
    g.input_zero = input_zero, g.output_zero = output_zero;
    if (g.total > 0) {
        unsigned blocks;
        if ((r = blocks_ok(uc, "tile_conv_filter_uint8", g.total, &blocks))) return r;
        timing_note_bytes(2.0 * g.total);
        HLMI_LAUNCH(uc, "hannk_tile_filter", ctx.stream, hannk_tile_filter, dim3(blocks), dim3(256), 0, g);
    }
    mark_output_written(output);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- host: conv
// ---- run-time switch, read once per call (env_int, hlmi_internal.h):
//   HLMI_HANNK_SPLIT_K   unset: the plan's choice; n >= 1: n splits of k (1 = none) wherever the k-blocks allow   (tests/test_hannk_conv.py)
struct ConvSwitches {
    std::optional<int> split_k;
};

// ---- the plan of one conv call: kernel, tiling and splits, made before anything is enqueued; no pointer, no HIP call.
struct ConvPlan {
    bool mfma;          // operands dword-aligned and the sizes inside the kernel's 32-bit k arithmetic; otherwise hannk_conv_general
    bool vec;           // CQ % 4 == 0
    ConvTiling t;
    size_t ws_bytes;    // split-K partials
    unsigned blocks;    // of 4 waves
};
// Split-K threshold: a wave tile is 32 co x 32 pixels and a compute unit wants at least one wave per SIMD, so below 4 * cus wave
// tiles the k range is cut until there are that many, as long as every split keeps MIN_KB k-blocks and at most MAX_SPLITS partials
// are written.  (Every batch-1 layer of a MobileNet is below the threshold.)
constexpr int MIN_KB = 2, MAX_SPLITS = 16;
void hannk_conv_plan(ConvPlan &pl, long npix, int C, int total_quads, int CQ, int FW, int cus, bool aligned, const ConvSwitches &sw) {
    ConvTiling &t = pl.t;
    t.d_cq = make_fastdiv((uint32_t)CQ), t.d_fw = make_fastdiv((uint32_t)FW);
    t.total_quads = total_quads;
    t.nkb = (total_quads + KB_QUADS - 1) / KB_QUADS;
    t.co16 = (C + VT - 1) / VT;
    t.ncp = (t.co16 + 1) / 2;
    t.wave_tiles = ((npix + WAVE_PX - 1) / WAVE_PX) * t.ncp;
    t.ws_row = (long)t.co16 * VT;
    pl.mfma = aligned && (long)t.nkb * KB_QUADS < (1L << 24) && t.wave_tiles < (1L << 32);
    pl.vec = CQ % 4 == 0;
    int want = 1;
    if (sw.split_k) want = *sw.split_k;
    else if (t.wave_tiles < 4L * cus) want = (int)std::min<long>((4L * cus + t.wave_tiles - 1) / t.wave_tiles, MAX_SPLITS);
    const int splits = std::max(1, std::min(want, sw.split_k ? t.nkb : t.nkb / MIN_KB));
    t.kb_per_split = (t.nkb + splits - 1) / splits;
    t.splits = (t.nkb + t.kb_per_split - 1) / std::max(t.kb_per_split, 1);   // no empty split
    if (t.splits < 1) t.splits = 1;
    pl.ws_bytes = t.splits > 1 ? (size_t)t.splits * npix * t.ws_row * sizeof(int32_t) : 0;
    pl.blocks = (unsigned)((t.wave_tiles + 3) / 4);
}

template<bool I16>
int conv_stage_main(void *uc, const DeviceCtx &ctx, const ConvPlan &pl, const ConvGeom &g, bool general) {
    const double bytes = (double)g.npix * g.CQ * VR + (double)pl.t.co16 * FTILE * pl.t.total_quads + (double)g.npix * g.C * (I16 ? 2 : 1);
    if (general || !pl.mfma) {
        unsigned blocks;
        if (int r = blocks_ok(uc, "conv", g.npix * g.C, &blocks)) return r;
        timing_note_bytes(bytes);
        HLMI_LAUNCH(uc, "hannk_conv_general", ctx.stream, hannk_conv_general<I16>, dim3(blocks), dim3(256), 0, g);
        return 0;
    }
    const ConvTiling &t = pl.t;
    int32_t *part = nullptr;
    if (t.splits > 1) {
        void *ws;
        if (int r = get_workspace(uc, ctx, pl.ws_bytes, &ws)) return r;
        part = (int32_t *)ws;
    }
    timing_note_bytes(bytes);
    int r = with_flags([&](auto vec, auto split) -> int {
        HLMI_LAUNCH(uc, "hannk_conv_mfma", ctx.stream, (hannk_conv_mfma<decltype(vec)::value, decltype(split)::value, I16>), dim3(pl.blocks, t.splits), dim3(256), 0, g, t, part);
        return 0;
    }, pl.vec, t.splits > 1);
    if (r) return r;
    if (t.splits > 1) {
        unsigned blocks;
        if ((r = blocks_ok(uc, "conv", g.npix * ((g.C + 3) / 4), &blocks))) return r;
        HLMI_LAUNCH(uc, "hannk_conv_finish", ctx.stream, hannk_conv_finish<I16>, dim3(blocks), dim3(256), 0, g, t, (const int32_t *)part);
    }
    return 0;
}

template<bool I16, bool GENERAL>
int conv_entry(halide_buffer_t *input, uint8_t input_zero, halide_buffer_t *filter, uint8_t filter_zero, halide_buffer_t *bias, int32_t stride_x,
               int32_t stride_y, int32_t dilation_x, int32_t dilation_y, int32_t output_multiplier, int32_t output_shift, uint8_t output_zero,
               uint8_t output_min, uint8_t output_max, halide_buffer_t *output) {
    void *uc = nullptr;
    const ArgTable &table = I16 ? conv_i16_table : conv_u8_table;
    BufArg args[4];
    table.bufs(args, {input, filter, bias, output});
    own_lanes(args);
    int r = check_not_null(uc, args, 4);
    if (r || (r = check_type_and_dims(uc, args, 4))) return r;
    halide_dimension_t *id = input->dim, *fd = filter->dim, *bd = bias->dim, *od = output->dim;
    if (any_bounds_query(args, 4)) {
        // What ConvOp::prepare asks with every extent 1: the filter's tiling.  A query filter gets the two fixed dimensions, the
        // tile stride and the co tiles the output needs; then the input and the bias get the regions the (shaped) output reads.
        const int co16 = std::max((od[0].extent + VT - 1) / VT, 1);
        if (!buffer_is_real(filter)) {
            const int mins[6] = {0, 0, 0, 0, 0, 0};
            const int ext[6] = {VR, VT, std::max(fd[2].extent, 1), std::max(fd[3].extent, co16), std::max(fd[4].extent, 1), std::max(fd[5].extent, 1)};
            answer_query(filter, mins, ext);
        }
        int mins[4] = {0, 0, 0, od[3].min}, ext[4] = {VR * fd[2].extent, 0, 0, od[3].extent};
        in_span(od[1].min, std::max(od[1].extent, 1), stride_x, fd[4].extent, dilation_x, &mins[1], &ext[1]);
        in_span(od[2].min, std::max(od[2].extent, 1), stride_y, fd[5].extent, dilation_y, &mins[2], &ext[2]);
        answer_query(input, mins, ext);
        const int bmin[1] = {0}, bext[1] = {od[0].extent};
        answer_query(bias, bmin, bext);
        return 0;
    }
    // ---- constraints (conv_generator.cpp:162-182), recorded and reported in the reference's order
    const int depth = VR * fd[2].extent;
    check_dim(uc, "input", input, 0, &k0, &depth, nullptr);
    for (int d = 1; d < 4; d++) check_stride_multiple(uc, "input", input, d, VR);
    check_dim(uc, "filter", filter, 0, &k0, &k4, &k1);
    check_dim(uc, "filter", filter, 1, &k0, &k16, &k4);
    check_dim(uc, "filter", filter, 2, &k0, nullptr, &k64);
    for (int d = 3; d < 6; d++) {
        check_dim(uc, "filter", filter, d, &k0, nullptr, nullptr);
        check_stride_multiple(uc, "filter", filter, d, FTILE);
    }
    check_dim(uc, "bias", bias, 0, &k0, nullptr, &k1);
    check_dim(uc, "output", output, 0, &bd[0].min, &bd[0].extent, &k1);   // require_same_min_extent(0, bias_, output_)
    check_dim(uc, "output", output, 3, &id[3].min, &id[3].extent, nullptr);
    if ((r = check_shapes(uc, args, 4))) return r;
    const int C = od[0].extent, OW = od[1].extent, OH = od[2].extent, OB = od[3].extent, FW = fd[4].extent, FH = fd[5].extent, CQ = fd[2].extent;
    const bool empty = C <= 0 || OW <= 0 || OH <= 0 || OB <= 0;
    if (!empty) {
        int mn, ex;
        check_covers(uc, args[1], 3, 0, (C + VT - 1) / VT);
        if (FW > 0 && FH > 0 && CQ > 0) {
            in_span(od[1].min, OW, stride_x, FW, dilation_x, &mn, &ex);
            check_covers(uc, args[0], 1, mn, ex);
            in_span(od[2].min, OH, stride_y, FH, dilation_y, &mn, &ex);
            check_covers(uc, args[0], 2, mn, ex);
        }
    }
    check_host_aligned(uc, args[1], FTILE);
    check_host_aligned(uc, args[0], VR);
    const ConvSwitches sw = {env_int("HLMI_HANNK_SPLIT_K")};
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, 4))) return r;
    if (empty) {
        mark_output_written(output);
        return 0;
    }
    ConvGeom g = {};
    g.C = C, g.OW = OW, g.OH = OH, g.OB = OB, g.npix = (long)OW * OH * OB;
    g.in_sx = id[1].stride, g.in_sy = id[2].stride, g.in_sb = id[3].stride;
    g.o_sx = od[1].stride, g.o_sy = od[2].stride, g.o_sb = od[3].stride;
    g.f_s3 = fd[3].stride, g.f_s4 = fd[4].stride, g.f_s5 = fd[5].stride;
    g.sx = stride_x, g.sy = stride_y, g.dx = dilation_x, g.dy = dilation_y, g.FW = FW, g.FH = FH, g.CQ = CQ;
    g.az = input_zero, g.fz = filter_zero;
    g.q = {output_multiplier, output_shift, output_zero, output_min, output_max};
    g.in = dev_ptr<uint8_t>(input) + ((long)od[1].min * stride_x - id[1].min) * g.in_sx + ((long)od[2].min * stride_y - id[2].min) * g.in_sy;
    g.filt = dev_ptr<uint8_t>(filter), g.bias = dev_ptr<int32_t>(bias) - bd[0].min;
    g.out = dev_ptr<uint8_t>(output);

    ConvPlan pl = {};
    const bool aligned = ((uintptr_t)g.in % 4 == 0) && ((uintptr_t)g.filt % 4 == 0) && (long)FW * FH * CQ < (1L << 30);
    hannk_conv_plan(pl, g.npix, C, (int)std::min<long>((long)FW * FH * CQ, 1L << 30), CQ, FW, stream_cu_count(ctx.device, ctx.stream), aligned, sw);
    if ((r = conv_stage_main<I16>(uc, ctx, pl, g, GENERAL))) return r;
    mark_output_written(output);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- host: depthwise
// ---- the plan of a depthwise call: hannk_dw (4 channels x DW_ROWS output rows per thread, taps in registers) where the input is
// dword-aligned (the broadcast variant reads bytes) and the output gives every compute unit a workgroup of it (DW_MIN_THREADS threads);
// below that the one-thread-per-output kernel has 16 times the threads and measured faster (MobileNet's 512 x 14 x 14 at batch 1:
// 7.4 against 9.1 us; at batch 32 hannk_dw takes 17.3 against 26.5 us).  The switch HLMI_HANNK_DW_VECTOR (1 / 0) forces the kernel
// wherever the alignment allows it   (tests/test_hannk_conv.py).
constexpr long DW_MIN_THREADS = 256L * 256;
bool dw_vector(long threads, bool aligned, std::optional<int> forced) {
    if (!aligned) return false;
    return forced ? *forced != 0 : threads >= DW_MIN_THREADS;
}

// SHALLOW (depthwise_conv_shallow_uint8): the output's dimension 1 is {0, 1} and dimension 0 the fused c-x index; the
// input is read at (c + rx * dilation_x * input_stride_x, 0, y * stride_y + ry * dilation_y, b); filter and bias at (c % 16) % D of their
// own [0, D); no alignment is required and neither filter nor bias follows the output's extent.  Its dword kernel needs what the
// plain variant's constraints give for free: every tap offset, the row strides and the fused extent multiples of 4.
template<bool BCAST, bool GENERAL, bool SHALLOW = false>
int dw_entry(halide_buffer_t *input, uint8_t input_zero, halide_buffer_t *filter, uint8_t filter_zero, halide_buffer_t *bias, int32_t stride_x,
             int32_t stride_y, int32_t dilation_x, int32_t dilation_y, int32_t input_stride_x, int32_t output_multiplier, int32_t output_shift,
             uint8_t output_zero, uint8_t output_min, uint8_t output_max, halide_buffer_t *output) {
    void *uc = nullptr;
    const ArgTable &table = SHALLOW ? dws_table : BCAST ? dwb_table : dw_table;
    BufArg args[4];
    table.bufs(args, {input, filter, bias, output});
    own_lanes(args);
    int r = check_not_null(uc, args, 4);
    if (r || (r = check_type_and_dims(uc, args, 4))) return r;
    halide_dimension_t *id = input->dim, *fd = filter->dim, *bd = bias->dim, *od = output->dim;
    const int C = od[0].extent, CIN = BCAST ? 1 : (std::max(C, 1) + DV - 1) / DV * DV;
    if constexpr (SHALLOW) {
        const int D = std::max(fd[0].extent, 1);
        // the fused row: channels [0, C) shifted by the taps 0 .. (FW - 1) * dilation_x * input_stride_x
        const long t = (long)(std::max(fd[1].extent, 1) - 1) * dilation_x * input_stride_x;
        const long lo = std::min(0L, t), hi = (long)std::max(C, 1) - 1 + std::max(0L, t);
        if (lo < -(1L << 30) || hi > (1L << 30))
            return report(uc, halide_error_code_buffer_extents_too_large, "depthwise_conv_shallow_uint8: the taps span %ld elements", hi - lo + 1);
        int ymin, yext;
        in_span(od[2].min, std::max(od[2].extent, 1), stride_y, std::max(fd[2].extent, 1), dilation_y, &ymin, &yext);
        if (any_bounds_query(args, 4)) {
            const int mins[4] = {(int)lo, 0, ymin, od[3].min}, ext[4] = {(int)(hi - lo + 1), 1, yext, od[3].extent};
            answer_query(input, mins, ext);
            const int fmin[3] = {0, 0, 0}, fext[3] = {D, std::max(fd[1].extent, 1), std::max(fd[2].extent, 1)}, bext[1] = {D};
            answer_query(filter, fmin, fext);
            answer_query(bias, fmin, bext);
            return 0;
        }
        // ---- constraints (depthwise_conv_generator.cpp:93-94, :138-146)
        check_dim(uc, "input", input, 0, &k0, nullptr, nullptr);
        check_dim(uc, "filter", filter, 0, &k0, nullptr, &k1);
        check_dim(uc, "filter", filter, 1, &k0, nullptr, nullptr);
        check_dim(uc, "filter", filter, 2, &k0, nullptr, nullptr);
        check_dim(uc, "bias", bias, 0, &k0, nullptr, &k1);
        check_dim(uc, "output", output, 0, &k0, nullptr, &k1);
        check_dim(uc, "output", output, 1, &k0, &k1, nullptr);
        check_dim(uc, "output", output, 3, &id[3].min, &id[3].extent, nullptr);
        if ((r = check_shapes(uc, args, 4))) return r;
        if (C > 0 && od[2].extent > 0 && od[3].extent > 0) {
            check_covers(uc, args[1], 0, 0, D);   // filter(c % D, ...) and bias(c % D): [0, D)
            check_covers(uc, args[2], 0, 0, D);
            if (fd[1].extent > 0 && fd[2].extent > 0) {
                check_covers(uc, args[0], 0, (int)lo, (int)(hi - lo + 1));
                check_covers(uc, args[0], 1, 0, 1);
                check_covers(uc, args[0], 2, ymin, yext);
            }
        }
    }
    if (!SHALLOW && any_bounds_query(args, 4)) {
        // DepthwiseConv2DOp::prepare reads the channel alignment from the input's extent 0
        int mins[4] = {0, 0, 0, od[3].min}, ext[4] = {CIN, 0, 0, od[3].extent};
        in_span(od[1].min, std::max(od[1].extent, 1), stride_x, std::max(fd[1].extent, 1), dilation_x, &mins[1], &ext[1]);
        in_span(od[2].min, std::max(od[2].extent, 1), stride_y, std::max(fd[2].extent, 1), dilation_y, &mins[2], &ext[2]);
        answer_query(input, mins, ext);
        const int fmin[3] = {0, 0, 0}, fext[3] = {C, std::max(fd[1].extent, 1), std::max(fd[2].extent, 1)}, bext[1] = {C};
        answer_query(filter, fmin, fext);
        answer_query(bias, fmin, bext);
        return 0;
    }
    if constexpr (!SHALLOW) {
    // ---- constraints (depthwise_conv_generator.cpp:93-94, :138-168)
    check_dim(uc, "input", input, 0, &k0, BCAST ? &k1 : nullptr, nullptr);
    if (!BCAST)
        for (int d = 1; d < 4; d++) check_stride_multiple(uc, "input", input, d, DV);
    check_dim(uc, "filter", filter, 0, &od[0].min, &od[0].extent, &k1);
    check_dim(uc, "filter", filter, 1, &k0, nullptr, nullptr);
    check_dim(uc, "filter", filter, 2, &k0, nullptr, nullptr);
    check_dim(uc, "bias", bias, 0, &od[0].min, &od[0].extent, &k1);
    check_dim(uc, "output", output, 0, &k0, nullptr, &k1);
    check_dim(uc, "output", output, 3, &id[3].min, &id[3].extent, nullptr);
    if ((r = check_shapes(uc, args, 4))) return r;
    }
    const int OW = od[1].extent, OH = od[2].extent, OB = od[3].extent, FW = fd[1].extent, FH = fd[2].extent;
    const bool empty = C <= 0 || OW <= 0 || OH <= 0 || OB <= 0;
    if (!SHALLOW && !empty) {
        int mn, ex;
        check_covers(uc, args[0], 0, 0, CIN);
        if (FW > 0 && FH > 0) {
            in_span(od[1].min, OW, stride_x, FW, dilation_x, &mn, &ex);
            check_covers(uc, args[0], 1, mn, ex);
            in_span(od[2].min, OH, stride_y, FH, dilation_y, &mn, &ex);
            check_covers(uc, args[0], 2, mn, ex);
        }
    }
    if (!BCAST && !SHALLOW) check_host_aligned(uc, args[0], DV);
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, 4))) return r;
    if (empty) {
        mark_output_written(output);
        return 0;
    }
    DwGeom g = {};
    g.C = C, g.OW = OW, g.OH = OH, g.OB = OB;
    g.in_sx = SHALLOW ? input_stride_x : id[1].stride, g.in_sy = id[2].stride, g.in_sb = id[3].stride;
    g.D = SHALLOW ? std::max(fd[0].extent, 1) : 0;
    g.o_sx = od[1].stride, g.o_sy = od[2].stride, g.o_sb = od[3].stride;
    g.f_sx = fd[1].stride, g.f_sy = fd[2].stride;
    g.sx = stride_x, g.sy = stride_y, g.dx = dilation_x, g.dy = dilation_y, g.FW = FW, g.FH = FH;
    g.az = input_zero, g.fz = filter_zero;
    g.q = {output_multiplier, output_shift, output_zero, output_min, output_max};
    g.in = dev_ptr<uint8_t>(input) + ((long)od[2].min * stride_y - id[2].min) * g.in_sy;
    if (SHALLOW) g.in += (0L - id[1].min) * id[1].stride;   // x = 0 of the input; dimension 0 starts at 0 on both sides
    else g.in += ((long)od[1].min * stride_x - id[1].min) * g.in_sx;
    g.filt = dev_ptr<uint8_t>(filter), g.bias = dev_ptr<int32_t>(bias) - bd[0].min, g.out = dev_ptr<uint8_t>(output);
    const double bytes = (double)OW * OH * OB * C * 2 + (double)C * (FW * FH + 4);
    unsigned blocks;
    const long threads = (long)((C + 3) / 4) * OW * ((OH + DW_ROWS - 1) / DW_ROWS) * OB;
    bool aligned = BCAST || (uintptr_t)g.in % 4 == 0;
    if (SHALLOW) aligned = aligned && C % 4 == 0 && ((long)dilation_x * input_stride_x) % 4 == 0 && g.in_sy % 4 == 0 && g.in_sb % 4 == 0;
    if (GENERAL || !dw_vector(threads, aligned, env_int("HLMI_HANNK_DW_VECTOR"))) {
        if ((r = blocks_ok(uc, table.md.name, (long)C * OW * OH * OB, &blocks))) return r;
        timing_note_bytes(bytes);
        HLMI_LAUNCH(uc, "hannk_dw_general", ctx.stream, (hannk_dw_general<BCAST, SHALLOW>), dim3(blocks), dim3(256), 0, g);
    } else {
        if ((r = blocks_ok(uc, table.md.name, threads, &blocks))) return r;
        timing_note_bytes(bytes);
        if (FW == 3 && FH == 3) HLMI_LAUNCH(uc, "hannk_dw", ctx.stream, (hannk_dw<true, BCAST, SHALLOW>), dim3(blocks), dim3(256), 0, g);
        else HLMI_LAUNCH(uc, "hannk_dw", ctx.stream, (hannk_dw<false, BCAST, SHALLOW>), dim3(blocks), dim3(256), 0, g);
    }
    mark_output_written(output);
    return 0;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------- the entry points
#define HLMI_HANNK_ENTRY(name, table)                                             \
    int name##_argv(void **a) { return ::hlmi::argv_call(name, a); }              \
    const halide_filter_metadata_t *name##_metadata() { return &(table).md; }
namespace hannk {

int tile_conv_filter_uint8(halide_buffer_t *input, uint8_t input_zero, uint8_t output_zero, halide_buffer_t *output) {
    return tile_entry(input, input_zero, output_zero, output);
}
int conv_u8_u8_u8(halide_buffer_t *input, uint8_t input_zero, halide_buffer_t *filter, uint8_t filter_zero, halide_buffer_t *bias, int32_t stride_x,
                  int32_t stride_y, int32_t dilation_x, int32_t dilation_y, int32_t output_multiplier, int32_t output_shift, uint8_t output_zero,
                  uint8_t output_min, uint8_t output_max, halide_buffer_t *output) {
    return conv_entry<false, false>(input, input_zero, filter, filter_zero, bias, stride_x, stride_y, dilation_x, dilation_y, output_multiplier, output_shift,
                                    output_zero, output_min, output_max, output);
}
int conv_u8_u8_i16(halide_buffer_t *input, uint8_t input_zero, halide_buffer_t *filter, uint8_t filter_zero, halide_buffer_t *bias, int32_t stride_x,
                   int32_t stride_y, int32_t dilation_x, int32_t dilation_y, int32_t output_multiplier, int32_t output_shift, uint8_t output_zero,
                   uint8_t output_min, uint8_t output_max, halide_buffer_t *output) {
    return conv_entry<true, false>(input, input_zero, filter, filter_zero, bias, stride_x, stride_y, dilation_x, dilation_y, output_multiplier, output_shift,
                                   output_zero, output_min, output_max, output);
}
int depthwise_conv_uint8(halide_buffer_t *input, uint8_t input_zero, halide_buffer_t *filter, uint8_t filter_zero, halide_buffer_t *bias, int32_t stride_x,
                         int32_t stride_y, int32_t dilation_x, int32_t dilation_y, int32_t input_stride_x, int32_t output_multiplier, int32_t output_shift,
                         uint8_t output_zero, uint8_t output_min, uint8_t output_max, halide_buffer_t *output) {
    return dw_entry<false, false>(input, input_zero, filter, filter_zero, bias, stride_x, stride_y, dilation_x, dilation_y, input_stride_x, output_multiplier,
                                  output_shift, output_zero, output_min, output_max, output);
}
int depthwise_conv_broadcast_uint8(halide_buffer_t *input, uint8_t input_zero, halide_buffer_t *filter, uint8_t filter_zero, halide_buffer_t *bias,
                                   int32_t stride_x, int32_t stride_y, int32_t dilation_x, int32_t dilation_y, int32_t input_stride_x,
                                   int32_t output_multiplier, int32_t output_shift, uint8_t output_zero, uint8_t output_min, uint8_t output_max,
                                   halide_buffer_t *output) {
    return dw_entry<true, false>(input, input_zero, filter, filter_zero, bias, stride_x, stride_y, dilation_x, dilation_y, input_stride_x, output_multiplier,
                                 output_shift, output_zero, output_min, output_max, output);
}
int depthwise_conv_shallow_uint8(halide_buffer_t *input, uint8_t input_zero, halide_buffer_t *filter, uint8_t filter_zero, halide_buffer_t *bias,
                                 int32_t stride_x, int32_t stride_y, int32_t dilation_x, int32_t dilation_y, int32_t input_stride_x,
                                 int32_t output_multiplier, int32_t output_shift, uint8_t output_zero, uint8_t output_min, uint8_t output_max,
                                 halide_buffer_t *output) {
    return dw_entry<false, false, true>(input, input_zero, filter, filter_zero, bias, stride_x, stride_y, dilation_x, dilation_y, input_stride_x,
                                        output_multiplier, output_shift, output_zero, output_min, output_max, output);
}
HLMI_HANNK_ENTRY(depthwise_conv_shallow_uint8, dws_table)
HLMI_HANNK_ENTRY(tile_conv_filter_uint8, tile_table)
HLMI_HANNK_ENTRY(conv_u8_u8_u8, conv_u8_table)
HLMI_HANNK_ENTRY(conv_u8_u8_i16, conv_i16_table)
HLMI_HANNK_ENTRY(depthwise_conv_uint8, dw_table)
HLMI_HANNK_ENTRY(depthwise_conv_broadcast_uint8, dwb_table)

}  // namespace hannk
#undef HLMI_HANNK_ENTRY

// Measurement and test hook (hlmi_internal.h): the named entry point, in argv form, with one thread per output.
extern "C" int hlmi_hannk_general(const char *name, void **argv) {
    if (!name || !argv) return -1;
    if (!strcmp(name, "tile_conv_filter_uint8")) return hannk::tile_conv_filter_uint8_argv(argv);   // its one kernel is the general one
    if (!strcmp(name, "conv_u8_u8_u8")) return argv_call(conv_entry<false, true>, argv);
    if (!strcmp(name, "conv_u8_u8_i16")) return argv_call(conv_entry<true, true>, argv);
    if (!strcmp(name, "depthwise_conv_uint8")) return argv_call(dw_entry<false, true>, argv);
    if (!strcmp(name, "depthwise_conv_broadcast_uint8")) return argv_call(dw_entry<true, true>, argv);
    if (!strcmp(name, "depthwise_conv_shallow_uint8")) return argv_call(dw_entry<false, true, true>, argv);
    return hannk_nn_general(name, argv);   // the pooling, reduction, elementwise and normalisation ops
}

extern "C" int hlmi_debug_hannk_conv_plan(int64_t npix, int32_t channels, int32_t quads, int32_t cus, int32_t *out) {
    if (npix < 1 || channels < 1 || quads < 1 || cus < 1 || !out) return -1;
    ConvPlan pl = {};
    hannk_conv_plan(pl, npix, channels, quads, quads, 1, cus, true, ConvSwitches{env_int("HLMI_HANNK_SPLIT_K")});
    out[0] = pl.mfma, out[1] = pl.t.splits, out[2] = (int32_t)std::min<long>(pl.t.wave_tiles, 0x7fffffffL);
    return 0;
}

// acc, out: host pointers to n elements.  One launch.
extern "C" int hlmi_debug_hannk_quantize(int fn, const int32_t *acc, size_t n, int32_t multiplier, int32_t shift, uint8_t zero, uint8_t lo, uint8_t hi,
                                         void *out) {
    if (fn < 0 || fn > 1 || !acc || !out || n == 0 || (n + 255) / 256 > 0x7fffffffu) return -1;
    void *d[2] = {nullptr, nullptr};
    const size_t bytes[2] = {4 * n, fn == 0 ? 2 * n : n};
    int rc = 0;
    for (int i = 0; i < 2 && !rc; i++)
        if (hipMalloc(&d[i], bytes[i]) != hipSuccess) rc = -2;
    if (!rc && hipMemcpy(d[0], acc, bytes[0], hipMemcpyHostToDevice) != hipSuccess) rc = -3;
    if (!rc) {
        const Quant q = {multiplier, shift, zero, lo, hi};
        hipLaunchKernelGGL(dbg_hannk_quantize, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, fn, (const int32_t *)d[0], n, q, d[1]);
        if (hipGetLastError() != hipSuccess || hipMemcpy(out, d[1], bytes[1], hipMemcpyDeviceToHost) != hipSuccess) rc = -4;
    }
    for (int i = 0; i < 2; i++)
        if (d[i]) (void)hipFree(d[i]);
    return rc;
}
