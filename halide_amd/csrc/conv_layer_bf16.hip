// conv_layer_bf16.hip — bf16 matrix-core variant of the conv_layer pipeline (BASELINE.json configs[4]:
// N=16, CI=CO=128, H=W=56, k=3, "bf16 MFMA im2col-GEMM").
//
// Same algorithm, boundary and layouts as conv_layer.hip (reference: /root/reference/apps/conv_layer/
// conv_layer_generator.cpp:21-27, :35-50): f32 halide buffers input [CI, W+2, H+2, N], filter [CO, 3, 3, CI],
// bias [CO], relu [CO, W, H, N].  Only the arithmetic differs: input and filter are rounded to bfloat16
// (round-to-nearest-even, v_cvt_pk_bf16_f32), products are exact in f32 and are accumulated in f32 by
// `v_mfma_f32_32x32x16_bf16`, starting from the f32 bias.  Parity is therefore by tolerance against
// oracle_conv_layer_bf16 (same rounding of the operands, double accumulation), not bit-exact; the exact f32
// entry point is `conv_layer`.
//
// Implicit GEMM  D[pixel][co] = bias[co] + sum_k A[pixel][k] B[k][co],  k = (ky, kx, ci):
//   conv_filter_bf16   filter f32 [ci][ky][kx][co] -> bf16, either rows of k (im2col kernel) or pre-ordered into 1 KB
//                      MFMA B fragments (input-linear kernel)
//   conv3x3_bf16_lin   the kernel that runs for W <= 125: tiles of 128 consecutive INPUT-LINEAR pixels, the window of
//                      a 32-ci chunk staged once in LDS (double-buffered), nine taps = nine row offsets, B fragments
//                      streamed L2 -> registers three taps ahead (see the comment at the kernel)
//   conv3x3_bf16_mfma  fallback for wider images: workgroup = 4 waves = 128 pixels x 128 output channels; per (ky, kx)
//                      and 64-ci chunk A and B are staged in LDS (rows padded to 144 B), three chunks in flight
//   Algorithmic bytes: input + output once (f32) + the bf16 filter: 27.6 + 25.7 + 0.3 MB at configs[4];
//   flops 2 N H W CI CO 9 = 14.8 G.
//
// Host path: conv_layer_bf16() reads top to bottom: check arguments -> switch -> device and buffers -> empty output -> plan -> stages
// -> done with the filter image -> mark_output_written.  conv_bf16_plan() fills a ConvBf16Plan (CGeom, the filter layout and with it
// the main kernel, the window size class, AR / ARp, LDS sizes, grids) without a HIP call; ConvBf16Buffers holds the pointers;
// conv_stage_filter (the cached producer: derived_acquire, conv_filter_bf16, filled) and conv_stage_main (hipFuncSetAttribute and the
// launch, once, in a lambda called with the kernel and its LDS size) launch from both.
#include "hlmi_internal.h"

#include <string.h>
#include <type_traits>

using namespace hlmi;

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));  // native vector: stays in registers (HIP's uint4 class does not always)

constexpr int TP = 128;       // pixels per workgroup
constexpr int TC = 128;       // output channels per workgroup
constexpr int KC = 64;        // ci per staged chunk
constexpr int PA = KC + 8;    // LDS row pitch in bf16 elements (144 B: ds_read_b128 rows fall on distinct banks)

struct CGeom {
    int CI, CO, W, H, N;
    long npix;
};

// n / d for 0 <= n < 2^31 by a multiply and a shift (d is uniform and known on the host): with s = ceil(log2 d) and
// m = ceil(2^(31+s) / d) the error term m d - 2^(31+s) is < d <= 2^s, so floor(n m / 2^(31+s)) == floor(n / d).
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

__device__ __forceinline__ uint32_t pk_bf16(float lo, float hi) {  // {bf16(lo), bf16(hi)}, round to nearest even
    uint32_t r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}

// filter f32 [ci][ky][kx][co] (co fastest) -> bf16
//   FRAG = false: wB[kk][co][ci]                                  (rows of k, staged through LDS by conv3x3_bf16_mfma)
//   FRAG = true : wB[kk][ci / 32][(ci % 32) / 16][co / 32][lane][8], lane = co % 32 + 32 ((ci % 16) / 8): every
//                 32x16 MFMA B fragment is 1 KB contiguous in lane order (one coalesced 16-byte load per lane)
//   FRAG = 2    : wB[ci / 32][kk][(ci % 32) / 16][co / 32][lane][8]: the same 1 KB fragments in the order conv3x3_bf16_p
//                 consumes them — tap (ci chunk, kk) is one contiguous 2 x (CO / 32) KB block, a workgroup's four
//                 co-fragments of a k-step are 4 KB contiguous: one coalesced 16-byte load per thread and k-step
template<int FRAG>
__global__ void conv_filter_bf16(const float *__restrict__ filt, uint16_t *__restrict__ wb, int CI, int CO) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;  // one thread per (kk, co, ci pair)
    const int half = CI / 2, total = 9 * CO * half;
    if (e >= total) return;
    const int cp = e % half, co = (e / half) % CO, kk = e / (half * CO);
    const float a = filt[((size_t)(2 * cp) * 9 + kk) * CO + co], b = filt[((size_t)(2 * cp + 1) * 9 + kk) * CO + co];
    size_t o;                                             // in bf16 pairs
    if (FRAG == 1) {
        const int ci = 2 * cp, cc = ci / 32, ks = (ci % 32) / 16, kh = (ci % 16) / 8, j = ci % 8;   // 32-ci chunks (KL)
        o = ((((((size_t)kk * (CI / 32) + cc) * 2 + ks) * (CO / 32) + co / 32) * 64 + (co % 32) + 32 * kh) * 8 + j) / 2;
    } else if (FRAG == 2) {
        const int ci = 2 * cp, cc = ci / 32, ks = (ci % 32) / 16, kh = (ci % 16) / 8, j = ci % 8;
        o = ((((((size_t)cc * 9 + kk) * 2 + ks) * (CO / 32) + co / 32) * 64 + (co % 32) + 32 * kh) * 8 + j) / 2;
    } else {
        o = ((size_t)kk * CO + co) * half + cp;
    }
    reinterpret_cast<uint32_t *>(wb)[o] = pk_bf16(a, b);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv3x3_bf16_mfma(const float *__restrict__ in, const uint16_t *__restrict__ wb,
                                                           const float *__restrict__ bias, float *__restrict__ out, CGeom g) {
    extern __shared__ uint16_t smem[];                       // [2][A: TP x PA | B: TC x PA] bf16
    constexpr int BUF = (TP + TC) * PA;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const long p0 = (long)blockIdx.x * TP;
    const int co0 = blockIdx.y * TC;

    // loader roles.  A: float4 index aq of the 64-ci chunk, pixels ap + 16 i.  B: 16-byte piece bq, rows bp + 32 i.
    const int aq = tid & 15, ap = tid >> 4;
    const int bq = tid & 7, bp = tid >> 3;
    uint32_t a_base[8];                                      // element offsets (buffers hold < 2^31 elements)
#pragma unroll
    for (int i = 0; i < 8; i++) {
        long pl = p0 + ap + 16 * i;
        if (pl >= g.npix) pl = g.npix - 1;                   // padded rows are computed but never stored
        const int p = (int)pl;                               // npix < 2^31 (check_shape)
        const int x = p % g.W, t = p / g.W;
        const int y = t % g.H, n = t / g.H;
        a_base[i] = (uint32_t)((((long)n * (g.H + 2) + y) * (g.W + 2) + x) * g.CI + 4 * aq);
    }
    const uint32_t in_row = (uint32_t)(g.W + 2) * g.CI;
    const int cpk = g.CI / KC, nchunk = 9 * cpk;             // chunks per (ky, kx); total

    // A (HBM / MALL latency) travels two chunks ahead through two register sets (chunk j in set j & 1) and one
    // chunk ahead through the second LDS buffer; B (the 295 KB bf16 filter, L2-resident) one chunk ahead.
    float4 ra[2][8];
    u32x4 rb[4];
    auto chunk_off = [&](int c, uint32_t &a_off, uint32_t &b_off) {
        const int kk = c / cpk, ci0 = (c - kk * cpk) * KC;
        const int ky = kk / 3, kx = kk - 3 * ky;
        a_off = (uint32_t)ky * in_row + (uint32_t)kx * g.CI + ci0;
        b_off = ((uint32_t)kk * g.CO + co0 + bp) * g.CI + ci0 + 8 * bq;
    };
    auto gload_a = [&](int c, float4 (&xa)[8]) {
        uint32_t a_off, b_off;
        chunk_off(c, a_off, b_off);
#pragma unroll
        for (int i = 0; i < 8; i++) xa[i] = *reinterpret_cast<const float4 *>(in + (a_base[i] + a_off));
    };
    auto gload_b = [&](int c) {
        uint32_t a_off, b_off;
        chunk_off(c, a_off, b_off);
#pragma unroll
        for (int i = 0; i < 4; i++) rb[i] = *reinterpret_cast<const u32x4 *>(wb + (b_off + (uint32_t)(32 * i) * g.CI));
    };
    auto lstore = [&](int buf, const float4 (&xa)[8]) {
        uint16_t *sA = smem + buf * BUF, *sB = sA + TP * PA;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            uint2 v;
            v.x = pk_bf16(xa[i].x, xa[i].y), v.y = pk_bf16(xa[i].z, xa[i].w);
            *reinterpret_cast<uint2 *>(sA + (ap + 16 * i) * PA + 4 * aq) = v;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) *reinterpret_cast<u32x4 *>(sB + (bp + 32 * i) * PA + 8 * bq) = rb[i];
    };

    floatx16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) {
            const float bv = bias[co0 + 64 * wn + 32 * b + (lane & 31)];  // C init = bias broadcast down the rows
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][b][r] = bv;
        }
    auto compute = [&](int buf) {
        const uint16_t *sA = smem + buf * BUF, *sB = sA + TP * PA;
        const uint16_t *pa = sA + (64 * wm + (lane & 31)) * PA + 8 * (lane >> 5);
        const uint16_t *pb = sB + (64 * wn + (lane & 31)) * PA + 8 * (lane >> 5);
#pragma unroll
        for (int ks = 0; ks < KC / 16; ks++) {
            const bf16x8 a0 = *reinterpret_cast<const bf16x8 *>(pa + 16 * ks);
            const bf16x8 a1 = *reinterpret_cast<const bf16x8 *>(pa + 32 * PA + 16 * ks);
            const bf16x8 b0 = *reinterpret_cast<const bf16x8 *>(pb + 16 * ks);
            const bf16x8 b1 = *reinterpret_cast<const bf16x8 *>(pb + 32 * PA + 16 * ks);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1][1], 0, 0, 0);
        }
    };
    // one chunk: B(c+1) loads, MFMAs on LDS buffer c & 1, chunk c+1 registers -> the other LDS buffer, A(c+3) loads
    // into the register set just freed; one barrier
    auto chunk = [&](int c, float4 (&xa)[8]) {
        if (c + 1 < nchunk) gload_b(c + 1);
        compute(c & 1);
        if (c + 1 < nchunk) lstore((c + 1) & 1, xa);
        if (c + 3 < nchunk) gload_a(c + 3, xa);
        __syncthreads();
    };

    gload_a(0, ra[0]);
    gload_b(0);
    lstore(0, ra[0]);
    if (1 < nchunk) gload_a(1, ra[1]);
    if (2 < nchunk) gload_a(2, ra[0]);
    __syncthreads();
#pragma unroll 1
    for (int c = 0; c < nchunk; c += 2) {
        chunk(c, ra[1]);                              // chunk c+1 lives in set 1 (c even)
        if (c + 1 < nchunk) chunk(c + 1, ra[0]);
    }
    // ---- epilogue: relu = max(0, conv), store (co fastest); C/D map: row = (r&3) + 8 (r>>2) + 4 (lane>>5), col = lane&31
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            const long p = p0 + 64 * wm + 32 * a + row;
            if (p < g.npix) {
#pragma unroll
                for (int b = 0; b < 2; b++) {
                    const float v = acc[a][b][r];
                    out[p * g.CO + co0 + 64 * wn + 32 * b + (lane & 31)] = v > 0.0f ? v : 0.0f;
                }
            }
        }
}

// ---- conv3x3_bf16_lin: the same GEMM tiled in INPUT-LINEAR pixel space.
// With q = (n (H+2) + y) (W+2) + x the tap (ky, kx) of output pixel q reads input pixel q + ky (W+2) + kx: for a tile
// of 128 consecutive q all nine taps read rows of ONE window of 128 + 2 (W+2) + 2 input pixels.  The window of a
// 64-ci chunk is staged in LDS once (f32 -> bf16) and the nine taps are nine row offsets into it — 9x less A traffic
// through L1 / LDS than re-staging an im2col slice per tap; B streams from L2 into registers.
// Positions q with x >= W or y >= H are not outputs (7 % of a 56x56 image): computed, never stored.
// Measured with compile-time ablations in round 2 (profiles/r02_conv_bf16_pmc.txt; the switches are gone): 29.4 us as built at
// configs[4]; without output stores 28.5, without the main loop 9.8, with only the first A window loaded 27.2, with only the first
// three taps' B fragments 24.0 — the main loop is 19-20 us whatever the A loads and the stores do, 14 us of it without any B
// traffic, against 7.7 us of MFMA time per SIMD.
constexpr int KL = 32;        // ci per window chunk of conv3x3_bf16_lin
constexpr int PL = KL + 8;    // its LDS row pitch in bf16 elements (80 B)
// NP: staging passes of 32 window rows per thread (window rows AR <= 32 NP)
template<int NP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void conv3x3_bf16_lin(const float *__restrict__ in, const uint16_t *__restrict__ wb, const float *__restrict__ bias,
                      float *__restrict__ out, CGeom g, int AR, FastDiv d_img, FastDiv d_row) {
    extern __shared__ uint16_t smem[];                       // two A windows: 2 x AR x PL bf16
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int Wp = g.W + 2, Hp = g.H + 2;
    const long NQ = (long)g.N * Hp * Wp;
    const long Q0 = (long)blockIdx.x * TP;
    const int co0 = blockIdx.y * TC;
    const int aq = tid & 7, ap = tid >> 3;                   // A loader: float4 aq of the 32-ci chunk, window rows ap + 32 i
    const int cpk = g.CI / KL, ntap = 9 * cpk;

    floatx16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) {
            const float bv = bias[co0 + 64 * wn + 32 * b + (lane & 31)];
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][b][r] = bv;
        }
    // B operands come straight from the fragment-ordered bf16 filter in L2 (one coalesced 16-byte load per lane and
    // 32x16 fragment), three taps ahead through three register stages; tap t uses stage t % 3 (9 taps per chunk, so the
    // stage is kk % 3).  No LDS and no barrier on the B side.
    bf16x8 bfr[3][2][2];
    const uint32_t cot0 = (uint32_t)(co0 + 64 * wn) / 32, ncot = (uint32_t)g.CO / 32;
    auto load_b = [&](int t, bf16x8 (&dst)[2][2]) {          // tap t = cc * 9 + kk; layout of conv_filter_bf16<true>
        const int cc = t / 9, kk = t - 9 * cc;
        const uint32_t f0 = ((uint32_t)kk * cpk + cc) * 2;
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int ks = 0; ks < 2; ks++)
                dst[b][ks] = *reinterpret_cast<const bf16x8 *>(wb + ((((f0 + ks) * ncot + cot0 + b) * 64 + lane) * 8));
    };
    // A: the input-linear window of a 32-ci chunk, f32 -> bf16 on the way into LDS.  The window of chunk cc+1 is
    // requested when chunk cc starts, converted and written to the OTHER LDS window when chunk cc's taps are done:
    // only the first window's memory latency is exposed.
    float4 va[NP];
    auto load_a = [&](int cc) {
#pragma unroll
        for (int i = 0; i < NP; i++) {
            const uint32_t q = min((uint32_t)Q0 + ap + 32 * i, (uint32_t)NQ - 1);   // NQ CI < 2^31 elements
            va[i] = *reinterpret_cast<const float4 *>(in + (q * g.CI + cc * KL + 4 * aq));
        }
    };
    auto store_a = [&](int buf) {
        uint16_t *sA = smem + (size_t)buf * AR * PL;
#pragma unroll
        for (int i = 0; i < NP; i++) {
            if (ap + 32 * i < AR) {
                uint2 w;
                w.x = pk_bf16(va[i].x, va[i].y), w.y = pk_bf16(va[i].z, va[i].w);
                *reinterpret_cast<uint2 *>(sA + (ap + 32 * i) * PL + 4 * aq) = w;
            }
        }
    };
    auto tap = [&](int t, int kk, const uint16_t *sA, bf16x8 (&bs)[2][2]) {
        const int ky = kk / 3, kx = kk - 3 * ky;
        const uint16_t *pa = sA + (64 * wm + (lane & 31) + ky * Wp + kx) * PL + 8 * (lane >> 5);
#pragma unroll
        for (int ks = 0; ks < KL / 16; ks++) {
            bf16x8 a0, a1;
            a0 = *reinterpret_cast<const bf16x8 *>(pa + 16 * ks);
            a1 = *reinterpret_cast<const bf16x8 *>(pa + 32 * PL + 16 * ks);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, bs[0][ks], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, bs[1][ks], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, bs[0][ks], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, bs[1][ks], acc[1][1], 0, 0, 0);
        }
        if (t + 3 < ntap) load_b(t + 3, bs);   // refill the stage just consumed
    };
    load_a(0);
    load_b(0, bfr[0]);
    load_b(1, bfr[1]);
    load_b(2, bfr[2]);
    store_a(0);
    __syncthreads();
#pragma unroll 1
    for (int cc = 0; cc < cpk; cc++) {
        if (cc + 1 < cpk) load_a(cc + 1);
        const uint16_t *sA = smem + (size_t)(cc & 1) * AR * PL;
#pragma unroll 1
        for (int k3 = 0; k3 < 9; k3 += 3) {
            tap(cc * 9 + k3, k3, sA, bfr[0]);
            tap(cc * 9 + k3 + 1, k3 + 1, sA, bfr[1]);
            tap(cc * 9 + k3 + 2, k3 + 2, sA, bfr[2]);
        }
        if (cc + 1 < cpk) store_a((cc + 1) & 1);             // that window was last read before the previous barrier
        __syncthreads();
    }
    // ---- epilogue
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            const long q = Q0 + 64 * wm + 32 * a + row;
            if (q < NQ) {
                const uint32_t qi = (uint32_t)q;
                const uint32_t n = fdiv(qi, d_img), rem = qi - n * d_img.d, y = fdiv(rem, d_row), x = rem - y * d_row.d;
                if ((int)y < g.H && (int)x < g.W) {
                    const long p = ((long)n * g.H + y) * g.W + x;
#pragma unroll
                    for (int b = 0; b < 2; b++) {
                        const float v = acc[a][b][r];
                        out[p * g.CO + co0 + 64 * wn + 32 * b + (lane & 31)] = v > 0.0f ? v : 0.0f;
                    }
                }
            }
        }
}


// ---- conv3x3_bf16_p: the same input-linear GEMM, ONE workgroup per compute unit with everything it streams staged once.
// What conv3x3_bf16_lin left on the table at configs[4] (29.4 us): every wave pulled its own copy of the B
// fragments through L1 (590 KB per workgroup at 64 B/clk: 5.5 us), 421 workgroups on 256 CUs ran load / MFMA / store in
// lock-step, and a barrier per chunk drained the prefetch.  Here:
//   * a workgroup of EIGHT waves owns TQ = 256 consecutive input-linear positions x 128 output channels (211 workgroups at
//     configs[4]: one round, one per CU, XCD-contiguous so that neighbouring tiles find their shared halo rows in the XCD's
//     L2); a wave owns 64 positions x 64 channels (acc[2][2]).  Two waves per SIMD are essential: an MFMA blocks the wave
//     that issued it, so with one wave per SIMD every ds_read, address add and wait between two MFMAs is time the matrix
//     pipe idles (the four-wave version of this kernel, 64 x 128 per wave, measured 26.5 us: half the pipe's time);
//   * B: the fragment-ordered bf16 filter comes through LDS ONCE per workgroup — per tap 8 KB (2 k-steps x 4 fragments), one
//     16-byte load per thread, BD = 6 taps ahead through a register ring (a wave's vmcnt is in order: loads that far ahead
//     never make a wait drain the A window requested behind them), two LDS slots;
//   * A: the window of a 32-ci chunk (TQ + 2 (W+2) + 2 rows) is requested when the previous chunk starts and converted into
//     the other LDS buffer under that chunk's last tap;
//   * ONE barrier per tap, placed after the first half of the tap's first k-step: the fragments of the second k-step were
//     requested before it, the next tap's B slot is written just before the barrier and its first fragments are requested
//     right after it.
// Only plain loads are in flight at a barrier (no stores before the epilogue), so __syncthreads() costs lgkmcnt(0) + s_barrier.
// All requests are unconditional (indices clamped at the end of the K loop): a load behind a branch makes the compiler's
// vmcnt bookkeeping assume nothing younger may be in flight, and every wait for a ring slot became vmcnt(0).
constexpr int TQ = 256;        // input-linear positions per workgroup
constexpr int PT = 512;        // threads per workgroup
constexpr int BD = 6;          // B taps in flight
constexpr int BSLOT = 4096;    // bf16 elements of one tap's B slot in LDS: [2 k-steps][4 co-fragments][64 lanes][8]
// What round 3's ablation masks and the two-workgroups-per-CU variant measured is in profiles/r03_conv_bf16_ablation.txt (the
// switches are gone): prologue (first A window + the B ring) ~6 us and epilogue (131 KB of stores) 2.4 us exposed, 8.3 of 24.7 us
// with the matrix pipe idle; 128-position tiles with four waves and two workgroups per CU: 26.5 us.
template<int NP>  // A staging passes of PT / 8 window rows (AR <= PT / 8 * NP)
__global__ __launch_bounds__(512) void conv3x3_bf16_p(const float *__restrict__ in, const uint16_t *__restrict__ wb,
                                                    const float *__restrict__ bias, float *__restrict__ out, CGeom g, int AR,
                                                    FastDiv d_img, FastDiv d_row) {
    extern __shared__ uint16_t smem[];                       // [A window 0][A window 1][B slot 0][B slot 1]
    constexpr int RPP = PT / 8, NBP = 512 / PT;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wq = wave >> 1, wc = wave & 1;                 // the wave's 64 positions / 64 channels of the tile
    const int Wp = g.W + 2, Hp = g.H + 2;
    const uint32_t NQ = (uint32_t)g.N * Hp * Wp;
    // XCD-contiguous tiles (blocks are dealt round-robin to the 8 XCDs; bijective for any grid size)
    const int nwg = gridDim.x, q8 = nwg >> 3, r8 = nwg & 7, xcd = blockIdx.x & 7, slot_in_xcd = blockIdx.x >> 3;
    const int tile = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot_in_xcd;
    const uint32_t Q0 = (uint32_t)tile * TQ;
    const int co0 = blockIdx.y * TC;
    const uint32_t ncot = (uint32_t)g.CO / 32, cot0 = (uint32_t)co0 / 32;
    const int cpk = g.CI / KL, ntap = 9 * cpk;
    uint16_t *const sA0 = smem, *const sA1 = smem + (size_t)AR * PL, *const sB = smem + (size_t)2 * AR * PL;

    floatx16 acc[2][2];
#pragma unroll
    for (int b = 0; b < 2; b++) {
        const float bv = bias[co0 + 64 * wc + 32 * b + (lane & 31)];   // C init = bias broadcast down the rows
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][b][r] = bv;
    }
    // ---- staging roles
    const int aq = tid & 7, ap = tid >> 3;                   // A: float4 aq of the 32-ci chunk, window rows ap + RPP i
    float4 va[NP];
    auto load_a = [&](int cc) {
#pragma unroll
        for (int i = 0; i < NP; i++) {
            const uint32_t q = min(Q0 + (uint32_t)(ap + RPP * i), NQ - 1);   // NQ CI < 2^31 elements
            va[i] = *reinterpret_cast<const float4 *>(in + (q * (uint32_t)g.CI + (uint32_t)(cc * KL + 4 * aq)));
        }
    };
    auto store_a = [&](uint16_t *sA) {
#pragma unroll
        for (int i = 0; i < NP; i++) {
            if (ap + RPP * i < AR) {
                uint2 w;
                w.x = pk_bf16(va[i].x, va[i].y), w.y = pk_bf16(va[i].z, va[i].w);
                *reinterpret_cast<uint2 *>(sA + (ap + RPP * i) * PL + 4 * aq) = w;
            }
        }
    };
    struct BReg {
        u32x4 v[NBP];
    };
    BReg rb[BD];                                             // B taps in flight: 512 16-byte pieces per tap, NBP per thread
    uint32_t b_lane[NBP];
#pragma unroll
    for (int j = 0; j < NBP; j++) {
        const uint32_t pc = (uint32_t)tid + (uint32_t)PT * j;   // piece: k-step pc >> 8
        b_lane[j] = ((pc >> 8) * ncot + cot0) * 512 + (pc & 255) * 8;
    }
    auto load_b = [&](int T, BReg &dst) {                    // T = chunk * 9 + kk; layout of conv_filter_bf16<2>
#pragma unroll
        for (int j = 0; j < NBP; j++) dst.v[j] = *reinterpret_cast<const u32x4 *>(wb + ((uint32_t)T * 2 * ncot * 512 + b_lane[j]));
    };
    auto store_b = [&](int slot, const BReg &src) {
#pragma unroll
        for (int j = 0; j < NBP; j++) reinterpret_cast<u32x4 *>(sB + slot * BSLOT)[tid + PT * j] = src.v[j];
    };
    // ---- fragments: two register sets, one per k-step of a tap
    bf16x8 fa[2][2], fb[2][2];
    const int a_lane = (64 * wq + (lane & 31)) * PL + 8 * (lane >> 5);
    const int b_frag = 2 * wc * 512 + lane * 8;
    auto read_frags = [&](int fs, const uint16_t *sA, int tapoff, int ks, int slot) {
        const uint16_t *pa = sA + a_lane + tapoff + 16 * ks;
        fa[fs][0] = *reinterpret_cast<const bf16x8 *>(pa);
        fa[fs][1] = *reinterpret_cast<const bf16x8 *>(pa + 32 * PL);
        const uint16_t *pb = sB + slot * BSLOT + ks * 2048 + b_frag;
        fb[fs][0] = *reinterpret_cast<const bf16x8 *>(pb);
        fb[fs][1] = *reinterpret_cast<const bf16x8 *>(pb + 512);
    };
    auto mfma2 = [&](int fs, int a) {
#pragma unroll
        for (int b = 0; b < 2; b++) {
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[fs][a], fb[fs][b], acc[a][b], 0, 0, 0);
        }
    };
    const int WpPL = Wp * PL;
    // One tap, one barrier, placed after the first half of the tap's first k-step: the fragments of the second k-step were
    // requested before it, the next tap's B slot is written just before the barrier and its first fragments are requested
    // right after it.  Measured alternatives (all correct, profiles/r03_conv_bf16_ablation.txt): four waves of 64 x 128 per
    // workgroup 26.5 us; this schedule 24.7 us; all eight fragments of a tap requested a whole tap ahead (three B slots) 26.5 us;
    // request phase / MFMA phase with two barriers per tap and the two waves of a SIMD one barrier apart 29-32 us.  In every
    // variant the K loop costs the SUM of its MFMA time (9.3 us for 288 MFMAs per wave, two waves per SIMD) and of the staging
    // (global requests + LDS writes, 5-6 us), fragment reads and barriers (3.6 us): the matrix pipe does not run under them.
    // Hazards: B slot (t + 1) & 1 is written before the barrier of tap t; its previous contents (tap t - 1) were last read
    // before the barrier of tap t - 1 (second k-step) — every wave has passed that barrier.  The A window of chunk c + 1 is
    // written before the barrier of chunk c's last tap into the buffer chunk c - 1 used.
    auto tap = [&](auto tt, int Tb) {
        constexpr int t = decltype(tt)::value, kk = t % 9, half = t / 9, ky = kk / 3, kx = kk % 3;
        constexpr int kn = (kk + 1) % 9, kyn = kn / 3, kxn = kn % 3;
        const int T = Tb + t, cc = Tb / 9 + half;
        uint16_t *const sAc = half ? sA1 : sA0, *const sAo = half ? sA0 : sA1;
        // requests: B of tap T + BD into the ring slot tap T's data left when it went to LDS; next chunk's A window
        load_b(min(T + BD, ntap - 1), rb[t % BD]);
        if (kk == 0) load_a(min(cc + 1, cpk - 1));
        __builtin_amdgcn_sched_barrier(0);
        read_frags(1, sAc, ky * WpPL + kx * PL, 1, t & 1);   // second k-step of this tap
        mfma2(0, 0);
        __builtin_amdgcn_sched_barrier(0);
        store_b((t + 1) & 1, rb[(t + 1) % BD]);
        if (kk == 8) store_a(sAo);
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
        mfma2(0, 1);
        __builtin_amdgcn_sched_barrier(0);
        read_frags(0, kk == 8 ? sAo : sAc, kyn * WpPL + kxn * PL, 0, (t + 1) & 1);   // first k-step of the next tap
        mfma2(1, 0), mfma2(1, 1);
        __builtin_amdgcn_sched_barrier(0);
    };
    // ---- prologue
    load_a(0);
#pragma unroll
    for (int j = 0; j < BD; j++) load_b(min(j, ntap - 1), rb[j]);
    store_a(sA0);
    store_b(0, rb[0]);
    __syncthreads();
    read_frags(0, sA0, 0, 0, 0);
#pragma unroll 1
    for (int Tb = 0; Tb < ntap; Tb += 18) {
        tap(std::integral_constant<int, 0>{}, Tb);
        tap(std::integral_constant<int, 1>{}, Tb);
        tap(std::integral_constant<int, 2>{}, Tb);
        tap(std::integral_constant<int, 3>{}, Tb);
        tap(std::integral_constant<int, 4>{}, Tb);
        tap(std::integral_constant<int, 5>{}, Tb);
        tap(std::integral_constant<int, 6>{}, Tb);
        tap(std::integral_constant<int, 7>{}, Tb);
        tap(std::integral_constant<int, 8>{}, Tb);
        tap(std::integral_constant<int, 9>{}, Tb);
        tap(std::integral_constant<int, 10>{}, Tb);
        tap(std::integral_constant<int, 11>{}, Tb);
        tap(std::integral_constant<int, 12>{}, Tb);
        tap(std::integral_constant<int, 13>{}, Tb);
        tap(std::integral_constant<int, 14>{}, Tb);
        tap(std::integral_constant<int, 15>{}, Tb);
        tap(std::integral_constant<int, 16>{}, Tb);
        tap(std::integral_constant<int, 17>{}, Tb);
    }
    // ---- epilogue: relu, store (co fastest); C/D map: row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5), col = lane & 31
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            const uint32_t q = Q0 + (uint32_t)(64 * wq + 32 * a + row);
            if (q < NQ) {
                const uint32_t n = fdiv(q, d_img), rem = q - n * d_img.d, y = fdiv(rem, d_row), x = rem - y * d_row.d;
                if ((int)y < g.H && (int)x < g.W) {
                    float *o = out + ((((size_t)n * g.H + y) * g.W + x) * g.CO + co0 + 64 * wc + (lane & 31));
#pragma unroll
                    for (int b = 0; b < 2; b++) {
                        const float v = acc[a][b][r];
                        o[32 * b] = v > 0.0f ? v : 0.0f;
                    }
                }
            }
        }
}

// Measured and not kept (round 5, profiles/r05_conv_bf16_rows.txt): `conv3x3_bf16_g`, this kernel with ONE barrier per filter row —
// the B slot holds a row's three taps (24 KB, two slots), the waves meet 12 times instead of 36 and run 24 MFMAs each in between,
// the fragments of k-step s + 1 requested under the MFMAs of k-step s.  Bit-identical, 0.0262 against 0.0257 ms per call: the
// barriers are not what the K loop waits for.  What the counters say: 486 144 MFMAs x 32 cycles = 18.4 k cycles per SIMD of a busy
// CU, and SQ_BUSY_CU_CYCLES / 211 busy CUs = 47 k cycles in 25.8 us — the shader clock under this kernel is ~1.8 GHz, not the
// 2.4 GHz the 2.5 PFLOP/s peak is quoted at; at that clock the matrix pipe is busy 10.1 us, 58 % of the K loop.

// Also measured and not kept (round 5, profiles/NOTES.md): `conv3x3_bf16_w`, the verdict's loader-wave split — twelve waves, eight that
// run only fragment reads, MFMAs and the tap's barrier and four loaders (one per SIMD) that request, convert and write A and B.
// Bit-identical (15 tests), 0.0275-0.0279 against 0.0261-0.0262 ms per call: taking the staging out of the MFMA waves' instruction
// streams does not put the matrix pipe under it either.

const ArgTable conv_table = conv_arg_table("conv_layer_bf16", 56, 56, 16);   // estimates: BASELINE.json configs[4] (N=16, 56x56 output)

// ---- cache of re-ordered filters: one entry per (device, filter allocation, version, layout) in the runtime's cache of
// derived device data (hlmi_internal.h), read by the main kernel of every call that hits it.  Filters in memory the runtime
// does not own (version 0: wrapped pointers, e.g. every torch tensor) are never cached: their image lives in the calling
// stream's own scratch arena, where stream order alone protects it.
struct FilterKey {
    int device, layout;
    uint64_t handle, version;
};
static_assert(sizeof(FilterKey) <= DERIVED_KEY_BYTES, "key does not fit an entry");
DerivedCache g_filters(8);

// ---- run-time switch: an environment variable, read into a ConvSwitches by conv_layer_bf16() once per call — on every call, since
// the tests flip it inside one process (env_flag, hlmi_internal.h).
//   HLMI_CONV_NO_FILTER_CACHE  default 0; 1: conv_filter_bf16 runs in every call   (tests/test_conv_layer.py: test_hip_bf16_filter_is_reordered_once_…)
struct ConvSwitches {
    bool no_filter_cache;
};

// ---- the plan of one call: which main kernel runs, on which filter layout, and how it is launched, made by conv_bf16_plan() before
// anything is enqueued.  It holds no pointer (ConvBf16Buffers does); it lives on conv_layer_bf16()'s stack and the stages read it by reference.
struct ConvBf16Plan {
    CGeom g;
    long NQ;            // input-linear positions: N (H + 2) (W + 2)
    // layout  of the bf16 filter image (conv_filter_bf16<layout>) and with it the main kernel:
    //   2  conv3x3_bf16_p: 256-position tiles, B through LDS; the window ARp takes 6 or 8 staging passes (`wide`: 8)
    //   1  conv3x3_bf16_lin: 128-position tiles, for what conv3x3_bf16_p does not take; the window AR takes 8 or 12 passes (`wide`: 12)
    //   0  conv3x3_bf16_mfma: the fallback for W > 125, im2col tiles of 128 pixels
    int layout;
    bool wide;
    int AR, ARp;        // input-linear window of a 128- / 256-position tile
    size_t sh_lin, sh_p, sh_mfma, wb_bytes;   // dynamic LDS of the three kernels; the filter image
    bool cache;         // the image of a filter in memory the runtime owns is kept (!HLMI_CONV_NO_FILTER_CACHE)
    FastDiv d_img, d_row;
    dim3 filter_grid, main_grid;
};

// the resolved pointers of one call
struct ConvBf16Buffers {
    const float *in, *filt, *bias;
    float *out;
    uint16_t *wb;       // the filter image: the cache's entry, or (not cacheable, every slot pinned) the stream's arena
};

// No HIP call, no lock, no allocation: a function of the checked extents and the switch.
void conv_bf16_plan(ConvBf16Plan &pl, const ConvSwitches &sw) {
    const CGeom &g = pl.g;
    pl.wb_bytes = (size_t)9 * g.CO * g.CI * sizeof(uint16_t);
    pl.cache = !sw.no_filter_cache;
    pl.AR = TP + 2 * (g.W + 2) + 2, pl.ARp = TQ + 2 * (g.W + 2) + 2;
    pl.sh_lin = (size_t)2 * pl.AR * PL * sizeof(uint16_t);                  // two windows of 32-ci chunks, 80-byte rows
    pl.sh_p = ((size_t)2 * pl.ARp * PL + 2 * BSLOT) * sizeof(uint16_t);     // two A windows, two B slots
    pl.sh_mfma = (size_t)2 * (TP + TC) * PA * sizeof(uint16_t);             // 73.7 KB: above the 64 KB default window
    const long NQ = pl.NQ = (long)g.N * (g.H + 2) * (g.W + 2);
    const bool lin = pl.AR <= 32 * 12 && NQ < (1L << 31) && NQ * g.CI < (1L << 31);   // W <= 125
    const bool pers = lin && pl.ARp <= 64 * 8 && pl.sh_p <= 160 * 1024 && g.CO % TC == 0 && g.CI % (2 * KL) == 0;
    pl.layout = pers ? 2 : (lin ? 1 : 0);
    pl.wide = pers ? pl.ARp > 64 * 6 : pl.AR > 32 * 8;
    pl.d_img = make_fastdiv((uint32_t)((g.H + 2) * (g.W + 2))), pl.d_row = make_fastdiv((uint32_t)(g.W + 2));
    pl.filter_grid = dim3((9 * g.CO * (g.CI / 2) + 255) / 256);
    pl.main_grid = dim3((unsigned)(pers ? (NQ + TQ - 1) / TQ : lin ? (NQ + TP - 1) / TP : (g.npix + TP - 1) / TP), g.CO / TC);
}

// ---- the two stages of the chain, in launch order.  Each takes the plan, the resolved pointers and the stream; a non-zero return
// is the error code of the call.

// stage 1, the filter: its bf16 MFMA-B image is a function of the filter's contents only.  It is kept per (filter allocation, version,
// layout) and the pre-pass re-runs only when the filter changed (uploaded again because the caller set host_dirty, written by another
// pipeline, re-allocated).  Weights that stay resident — the inference case — pay the re-ordering once.
int conv_stage_filter(void *uc, const DeviceCtx &ctx, const ConvBf16Plan &pl, ConvBf16Buffers &b, DerivedUse &use, const halide_buffer_t *filter) {
    FilterKey key;
    memset(&key, 0, sizeof key);
    key.device = ctx.device, key.layout = pl.layout, key.handle = filter->device, key.version = buffer_version(filter);
    int r = derived_acquire(uc, ctx, g_filters, &key, sizeof key, pl.wb_bytes, key.version != 0 && pl.cache, &use);
    if (r) return r;
    void *wb_mem = use.ptr;   // not cached: the image goes into the stream's arena
    if (!wb_mem && (r = get_workspace(uc, ctx, pl.wb_bytes, &wb_mem))) return r;
    b.wb = (uint16_t *)wb_mem;
    if (use.fill) {
        timing_note_bytes(6.0 * 9 * pl.g.CO * pl.g.CI);
        auto pre = [&](auto *kernel) -> int {
            HLMI_LAUNCH(uc, "conv_filter_bf16", ctx.stream, kernel, pl.filter_grid, dim3(256), 0, b.filt, b.wb, pl.g.CI, pl.g.CO);
            return 0;
        };
        if ((r = pl.layout == 2 ? pre(conv_filter_bf16<2>) : pl.layout == 1 ? pre(conv_filter_bf16<1>) : pre(conv_filter_bf16<0>))) return r;
        use.filled(ctx.stream);
    }
    return 0;
}

// stage 2, the main launch: every kernel asks for more LDS than the default window, which is raised first
int conv_stage_main(void *uc, const ConvBf16Plan &pl, const ConvBf16Buffers &b, hipStream_t st) {
    const CGeom &g = pl.g;
    timing_note_bytes(4.0 * ((double)pl.NQ * g.CI + (double)g.npix * g.CO) + (double)pl.wb_bytes);
    auto run = [&](auto *kernel, unsigned threads, size_t lds, auto... window) -> int {
        HLMI_HIP(uc, hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        HLMI_LAUNCH(uc, "conv3x3_bf16_mfma", st, kernel, pl.main_grid, dim3(threads), lds, b.in, b.wb, b.bias, b.out, g, window...);
        return 0;
    };
    if (pl.layout == 2) return pl.wide ? run(conv3x3_bf16_p<8>, PT, pl.sh_p, pl.ARp, pl.d_img, pl.d_row) : run(conv3x3_bf16_p<6>, PT, pl.sh_p, pl.ARp, pl.d_img, pl.d_row);
    if (pl.layout == 1) return pl.wide ? run(conv3x3_bf16_lin<12>, 256, pl.sh_lin, pl.AR, pl.d_img, pl.d_row) : run(conv3x3_bf16_lin<8>, 256, pl.sh_lin, pl.AR, pl.d_img, pl.d_row);
    return run(conv3x3_bf16_mfma, 256, pl.sh_mfma);
}

}  // namespace

extern "C" int conv_layer_bf16(halide_buffer_t *input, halide_buffer_t *filter, halide_buffer_t *bias, halide_buffer_t *relu) {
    void *uc = nullptr;
    BufArg args[4];
    conv_table.bufs(args, {input, filter, bias, relu});
    ConvBf16Plan pl = {};
    CGeom &g = pl.g;
    bool query;
    int r = conv_check_args(uc, args, &g.CI, &g.CO, &g.W, &g.H, &g.N, &query);
    if (r || query) return r;
    if (g.CI % KC != 0) {
        return report(uc, halide_error_code_constraint_violated,
                      "Constraint violated: conv_layer_bf16 needs input channels (%d) to be a multiple of %d", g.CI, KC);
    }
    const ConvSwitches sw = {env_flag("HLMI_CONV_NO_FILTER_CACHE")};
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, 4))) return r;
    g.npix = (long)g.W * g.H * g.N;
    if (g.npix == 0) {
        mark_output_written(relu);
        return 0;
    }

    conv_bf16_plan(pl, sw);

    ConvBf16Buffers b = {dev_ptr<float>(input), dev_ptr<float>(filter), dev_ptr<float>(bias), dev_ptr<float>(relu), nullptr};
    DerivedUse use;
    if ((r = conv_stage_filter(uc, ctx, pl, b, use, filter)) || (r = conv_stage_main(uc, pl, b, ctx.stream))) return r;
    use.done(ctx.stream);
    mark_output_written(relu);
    return 0;
}

HLMI_ENTRY(conv_layer_bf16, conv_table.md)
