// linear_algebra.hip — gfx950 implementation of the twelve f32 AOT pipelines of apps/linear_algebra (the `halide_s*` objects behind
// halide_blas.h) and of the CBLAS-shaped hblas_s* calls over them (include/hlmi_blas.h).
//
// Algorithms: apps/linear_algebra/src/blas_l1_generators.cpp (AXPY :27-70, Dot :90-124, AbsSum :144-176), blas_l2_generators.cpp
// (GEMV :27-196, GER :217-242), blas_l3_generators.cpp (GEMM :25-172); which generator parameters make which entry point:
// src/CMakeLists.txt.  The contract the kernels share with the checker (tests/cpp/linear_algebra_check.c) is restated in
// include/hlmi_pipelines.h and DESIGN.md section 5.8.  In short: dimension 0 is innermost with stride 1 and min 0, matrices are
// column-major, every reduction runs its index strictly upward, a vectorised reduction keeps the V = 8 lane sums of the reference's
// x86-64 AVX2 build, and the float forms are dev::mad / dev::mad2 of hlmi_device_math.h (fused in the default build, one rounding
// per operator with HLMI_CANON_FMA=0).
//
// Every pipeline has two implementations.  The second one — one thread per output running the chain as written — is reached only
// through hlmi_linear_algebra_general(); `<family>_plan()` is the one place that chooses a launch:
//   scopy / sscal / saxpy / sger   la_elem<MODE, VEC>: 16-byte accesses where every address (and the matrix's column stride) allows,
//                                  one element per thread otherwise
//   sdot / sasum                   la_reduce: ONE wave.  The contract is eight chains of n / 8 dependent steps, so the only job is
//                                  that loads never stall the chains: the wave loads 256 elements of each operand with coalesced
//                                  256-byte loads, one block ahead, hands them through LDS to the eight chain lanes (each reads
//                                  its 32 steps as eight 16-byte LDS loads), and lanes 0 .. 7 step the chains
//   sgemv_notrans                  la_gemv_n: one sequential chain per output, lanes along i (coalesced), 64-thread workgroups so
//                                  that a small M still spreads over CUs, k unrolled by GEMV_U with the next GEMV_U loads in
//                                  flight under the fmas; x(k) is wave-uniform
//   sgemv_trans                    la_gemv_t: a wave owns 8 outputs x 8 chains; the lanes of a chain group read 32 contiguous
//                                  bytes of their column per step, GEMV_U steps ahead
//   sgemm (four variants)          sgemm_mfma<W, FAST, TA, TB>: mat_mul.hip's tile loop for M != N != K.  The variants are the
//                                  2 x 2 of "opA is i-contiguous or k-contiguous" x "opB is k-contiguous or j-contiguous": an
//                                  operand contiguous along its tile dimension is copied straight into LDS, one contiguous along
//                                  k is turned k-major on the way in.  transAB needs no swap of roles here: the product commutes,
//                                  and k still runs upward.  k strictly upward, no zero-padded step (an odd K ends in a VALU fmaf
//                                  on the accumulator registers through the C/D map), global loads two chunks ahead, LDS
//                                  double-buffered, the mad2 epilogue on the accumulator registers with C read in the 128-byte
//                                  half-wave rows the store uses.  v_mfma_f32_32x32x2_f32 is a chain of fused steps, so these
//                                  kernels exist in the default build only: with HLMI_CANON_FMA=0 (each product rounded before
//                                  the add) the plan always answers the one-thread-per-output kernel.
#include "hlmi_blas.h"
#include "hlmi_device_math.h"
#include "hlmi_internal.h"
#include "linear_algebra_host.h"

#include <math.h>

using namespace hlmi;
using namespace hlmi::la_host;

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int V = 8;                     // natural_vector_size(float) of the reference's x86-64 AVX2 target: a choice
constexpr int MAX_VECTOR = 134217728;    // vector lengths 0 .. 2^27
constexpr int MAX_EXTENT = 8192;         // matrix extents 0 .. 8192
constexpr int RED_BLOCK = 256;           // elements of each operand la_reduce stages per step of its pipeline: 32 chain steps
constexpr int RED_PITCH = 36;            // floats between the chain lanes' rows in LDS: 32 steps + 4, rows stay 16-byte aligned
constexpr int GEMV_WG = 64;              // threads of a gemv workgroup: one wave
constexpr int GEMV_U = 8;                // k steps per unrolled group of the two gemv kernels
constexpr int SMALL_TILE = 64;           // sgemm workgroup tile with one accumulator per wave
constexpr int LARGE_TILE = 128;          // sgemm workgroup tile with 2 x 2 accumulators per wave
constexpr int LARGE_FROM_WGS = 256;      // the large tile where it still leaves this many workgroups (x 4 waves = 256 CUs x 4 SIMDs)
constexpr int KC = 32;                   // k steps per staged chunk of the small tile; the large tile stages KC / 2

// ---------------------------------------------------------------------------------------------------------------- elementwise
enum ElemMode { E_COPY, E_SCAL, E_AXPY, E_GER };

struct EGeom {
    const float *x;   // [n]
    const float *y;   // AXPY: [n], read at i; GER: [rows], read at j
    float *r;         // [n] or [n x rows]; GER reads it too
    long n, ldr;
    int rows;
    float a;
};

template<int MODE>
__device__ __forceinline__ float elem_value(float a, float x, float y, float r) {
    if (MODE == E_COPY) return x;
    if (MODE == E_SCAL) return a * x;
    if (MODE == E_AXPY) return dev::mad(a, x, y);
    return dev::mad(a * y, x, r);   // GER: (a * y(j)) * x(i) + result(i, j)
}

template<int MODE, bool VEC>
__global__ __launch_bounds__(256) void la_elem(EGeom g) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    float *row = g.r + j * g.ldr;
    const float yj = MODE == E_GER ? g.y[j] : 0.0f;
    if (VEC) {
        const long i = 4 * idx;
        if (i >= g.n) return;
        if (i + 4 <= g.n) {
            const float4 xv = *reinterpret_cast<const float4 *>(g.x + i);
            float4 yv = make_float4(yj, yj, yj, yj), rv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (MODE == E_AXPY) yv = *reinterpret_cast<const float4 *>(g.y + i);
            if (MODE == E_GER) rv = *reinterpret_cast<const float4 *>(row + i);
            *reinterpret_cast<float4 *>(row + i) = make_float4(elem_value<MODE>(g.a, xv.x, yv.x, rv.x), elem_value<MODE>(g.a, xv.y, yv.y, rv.y),
                                                               elem_value<MODE>(g.a, xv.z, yv.z, rv.z), elem_value<MODE>(g.a, xv.w, yv.w, rv.w));
            return;
        }
        for (long e = i; e < g.n; e++)   // the last, partial group of four
            row[e] = elem_value<MODE>(g.a, g.x[e], MODE == E_AXPY ? g.y[e] : yj, MODE == E_GER ? row[e] : 0.0f);
    } else {
        if (idx >= g.n) return;
        row[idx] = elem_value<MODE>(g.a, g.x[idx], MODE == E_AXPY ? g.y[idx] : yj, MODE == E_GER ? row[idx] : 0.0f);
    }
}

// ---------------------------------------------------------------------------------------------------------------- sdot, sasum
template<bool ASUM>
__device__ __forceinline__ float red_step(float x, float y, float acc) { return ASUM ? acc + fabsf(x) : dev::mad(x, y, acc); }

// one wave; y is not read by sasum
template<bool ASUM>
__global__ __launch_bounds__(64) void la_reduce(const float *x, const float *y, float *result, long n) {
    __shared__ __attribute__((aligned(16))) float sx[2][V * RED_PITCH];
    __shared__ __attribute__((aligned(16))) float sy[2][V * RED_PITCH];
    const int lane = threadIdx.x;
    const long nblk = n / RED_BLOCK;
    float px[4], py[4];   // the block in flight: element 64 c + lane of it
    auto load = [&](long blk) {
#pragma unroll
        for (int c = 0; c < 4; c++) {
            px[c] = x[blk * RED_BLOCK + 64 * c + lane];
            if (!ASUM) py[c] = y[blk * RED_BLOCK + 64 * c + lane];
        }
    };
    // element e of a block belongs to chain e % 8, step e / 8: chain lane i finds its 32 steps in row i
    auto stage = [&](int buf) {
#pragma unroll
        for (int c = 0; c < 4; c++) {
            sx[buf][(lane & 7) * RED_PITCH + 8 * c + (lane >> 3)] = px[c];
            if (!ASUM) sy[buf][(lane & 7) * RED_PITCH + 8 * c + (lane >> 3)] = py[c];
        }
    };
    float acc = 0.0f;   // lanes 0 .. 7: the chains
    if (nblk > 0) {
        load(0);
        stage(0);
        if (nblk > 1) load(1);
        __syncthreads();
    }
#pragma unroll 1
    for (long blk = 0; blk < nblk; blk++) {
        const int buf = (int)(blk & 1);
        if (blk + 1 < nblk) stage(buf ^ 1);   // last read in iteration blk - 1, behind its barrier
        if (blk + 2 < nblk) load(blk + 2);    // in flight under this block's chain steps
        if (lane < V) {
            const float4 *rx = reinterpret_cast<const float4 *>(&sx[buf][lane * RED_PITCH]);
            const float4 *ry = reinterpret_cast<const float4 *>(&sy[buf][lane * RED_PITCH]);
            float4 vx[RED_BLOCK / V / 4], vy[RED_BLOCK / V / 4];
#pragma unroll
            for (int q = 0; q < RED_BLOCK / V / 4; q++) {
                vx[q] = rx[q];
                vy[q] = ASUM ? vx[q] : ry[q];
            }
#pragma unroll
            for (int q = 0; q < RED_BLOCK / V / 4; q++) {
                acc = red_step<ASUM>(vx[q].x, vy[q].x, acc);
                acc = red_step<ASUM>(vx[q].y, vy[q].y, acc);
                acc = red_step<ASUM>(vx[q].z, vy[q].z, acc);
                acc = red_step<ASUM>(vx[q].w, vy[q].w, acc);
            }
        }
        __syncthreads();
    }
    // the whole steps past the last block, straight from global memory
    const long nvec = n / V;
    if (lane < V)
        for (long k = nblk * (RED_BLOCK / V); k < nvec; k++) acc = red_step<ASUM>(x[k * V + lane], ASUM ? 0.0f : y[k * V + lane], acc);
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < V; i++) s = s + __shfl(acc, i);
    float t = 0.0f;
    for (long e = nvec * V; e < n; e++) t = red_step<ASUM>(x[e], ASUM ? 0.0f : y[e], t);
    if (lane == 0) *result = s + t;
}

template<bool ASUM>
__global__ __launch_bounds__(64) void la_reduce_general(const float *x, const float *y, float *result, long n) {
    if (threadIdx.x != 0) return;
    float lanes[V];
#pragma unroll
    for (int i = 0; i < V; i++) lanes[i] = 0.0f;
    const long nvec = n / V;
    for (long k = 0; k < nvec; k++)
#pragma unroll
        for (int i = 0; i < V; i++) lanes[i] = red_step<ASUM>(x[k * V + i], ASUM ? 0.0f : y[k * V + i], lanes[i]);
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < V; i++) s = s + lanes[i];
    float t = 0.0f;
    for (long e = nvec * V; e < n; e++) t = red_step<ASUM>(x[e], ASUM ? 0.0f : y[e], t);
    *result = s + t;
}

// ---------------------------------------------------------------------------------------------------------------- sgemv
struct VGeom {
    const float *A, *x, *y;
    float *out;
    int w, h;   // A's extents: dimension 0 (contiguous) and dimension 1
    long lda;
    float a, b;
};

// notrans: output(i) = the chain over k of mad(a * A(i, k), x(k), .) from b * y(i); i < w, k < h
__global__ __launch_bounds__(GEMV_WG) void la_gemv_n(VGeom g) {
    const int i = blockIdx.x * GEMV_WG + threadIdx.x;
    if (i >= g.w) return;
    float acc = g.b * g.y[i];
    const float *col = g.A + i;
    int k = 0;
    if (g.h >= GEMV_U) {
        float cur[GEMV_U], nxt[GEMV_U];
#pragma unroll
        for (int u = 0; u < GEMV_U; u++) cur[u] = col[(long)u * g.lda];
        for (; k + 2 * GEMV_U <= g.h; k += GEMV_U) {
#pragma unroll
            for (int u = 0; u < GEMV_U; u++) nxt[u] = col[(long)(k + GEMV_U + u) * g.lda];
#pragma unroll
            for (int u = 0; u < GEMV_U; u++) acc = dev::mad(g.a * cur[u], g.x[k + u], acc);
#pragma unroll
            for (int u = 0; u < GEMV_U; u++) cur[u] = nxt[u];
        }
#pragma unroll
        for (int u = 0; u < GEMV_U; u++) acc = dev::mad(g.a * cur[u], g.x[k + u], acc);
        k += GEMV_U;
    }
    for (; k < g.h; k++) acc = dev::mad(g.a * col[(long)k * g.lda], g.x[k], acc);
    g.out[i] = acc;
}

__global__ __launch_bounds__(256) void la_gemv_n_general(VGeom g) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.w) return;
    float acc = g.b * g.y[i];
    for (int k = 0; k < g.h; k++) acc = dev::mad(g.a * g.A[(long)k * g.lda + i], g.x[k], acc);
    g.out[i] = acc;
}

// trans: output(i), i < h, from column i of A: V lane chains over k of mad(A(kV + j, i), x(kV + j), .), their sum from +0 in lane
// order, the tail on top of the sum, then mad2(b, y(i), a, s).  Lane l: output 8 * block + l / 8, chain l % 8.
__global__ __launch_bounds__(GEMV_WG) void la_gemv_t(VGeom g) {
    const int lane = threadIdx.x, j = lane & (V - 1);
    const int o = blockIdx.x * (GEMV_WG / V) + lane / V;
    const float *col = g.A + (long)min(o, g.h - 1) * g.lda;   // the lanes past the last output repeat it and store nothing
    const int nvec = g.w / V;
    float acc = 0.0f;
    int k = 0;
    if (nvec >= GEMV_U) {
        float ca[GEMV_U], cx[GEMV_U], na[GEMV_U], nx[GEMV_U];
#pragma unroll
        for (int u = 0; u < GEMV_U; u++) ca[u] = col[u * V + j], cx[u] = g.x[u * V + j];
        for (; k + 2 * GEMV_U <= nvec; k += GEMV_U) {
#pragma unroll
            for (int u = 0; u < GEMV_U; u++) na[u] = col[(k + GEMV_U + u) * V + j], nx[u] = g.x[(k + GEMV_U + u) * V + j];
#pragma unroll
            for (int u = 0; u < GEMV_U; u++) acc = dev::mad(ca[u], cx[u], acc);
#pragma unroll
            for (int u = 0; u < GEMV_U; u++) ca[u] = na[u], cx[u] = nx[u];
        }
#pragma unroll
        for (int u = 0; u < GEMV_U; u++) acc = dev::mad(ca[u], cx[u], acc);
        k += GEMV_U;
    }
    for (; k < nvec; k++) acc = dev::mad(col[k * V + j], g.x[k * V + j], acc);
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < V; i++) s = s + __shfl(acc, i, V);
    for (int t = nvec * V; t < g.w; t++) s = dev::mad(col[t], g.x[t], s);
    if (j == 0 && o < g.h) g.out[o] = dev::mad2(g.b, g.y[o], g.a, s);
}

__global__ __launch_bounds__(256) void la_gemv_t_general(VGeom g) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= g.h) return;
    const float *col = g.A + (long)o * g.lda;
    float lanes[V];
#pragma unroll
    for (int i = 0; i < V; i++) lanes[i] = 0.0f;
    const int nvec = g.w / V;
    for (int k = 0; k < nvec; k++)
#pragma unroll
        for (int i = 0; i < V; i++) lanes[i] = dev::mad(col[k * V + i], g.x[k * V + i], lanes[i]);
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < V; i++) s = s + lanes[i];
    for (int t = nvec * V; t < g.w; t++) s = dev::mad(col[t], g.x[t], s);
    g.out[o] = dev::mad2(g.b, g.y[o], g.a, s);
}

// ---------------------------------------------------------------------------------------------------------------- sgemm
struct GGeom {
    const float *A, *B, *C;
    float *out;
    int M, N, K;             // result is M x N (i < M contiguous), the sum runs over K
    long sa, sb, sc, so;     // column strides in elements
    float a, b;
};

#if HLMI_CANON_FMA
// mat_mul.hip's mm_mfma for M != N != K with either operand stored either way.  x = i (the MFMA's column, contiguous in C and the
// result), y = j.  Operand X[k][x] = opA(x, k): A[k * sa + x] (straight) or, TA, A[x * sa + k] (turned).  Operand Y[k][y] = opB(k, y):
// B[y * sb + k] (turned) or, TB, B[k * sb + y] (straight).
template<int W, bool FAST, bool TA, bool TB>
__global__ __launch_bounds__(256) void sgemm_mfma(GGeom g) {
    constexpr int T = 64 * W;          // tile edge
    constexpr int KCH = KC / W;        // k per chunk
    constexpr bool XTURN = TA, YTURN = !TB;
    constexpr int XP = XTURN ? T + 1 : T, YP = YTURN ? T + 1 : T;   // LDS pitches: conflict-light scalar stores / float4 stores
    constexpr int TQ = T / 4;          // float4 per LDS row of a straight operand
    constexpr int KQ = KCH / 4;        // float4 per tile row of a turned operand
    static_assert(KCH * T / 4 == 512, "two float4 per thread and operand");
    __shared__ __attribute__((aligned(16))) float sX[2][KCH * XP];  // [k][x]
    __shared__ __attribute__((aligned(16))) float sY[2][KCH * YP];  // [k][y]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wy = (wave >> 1) * 32 * W, wx = (wave & 1) * 32 * W;   // wave tile origin inside the workgroup tile
    const int x0 = blockIdx.x * T, y0 = blockIdx.y * T;
    const int K = g.K;

    // float4 number f of a chunk of one operand: `t0` the tile's origin in the operand's tile dimension, `tn` that dimension's extent
    auto load_op = [&](auto turned, const float *base, long stride, int t0, int tn, int k0, int f, float4 &p) {
        if constexpr (decltype(turned)::value) {
            const int tt = f / KQ, kk = 4 * (f % KQ);   // tile row tt, first k
            if constexpr (FAST) {
                p = *reinterpret_cast<const float4 *>(base + (long)(t0 + tt) * stride + k0 + kk);
            } else {   // clamped: what lies past the matrix is loaded from its last row / column and never reaches a stored result
                const float *r = base + (long)min(t0 + tt, tn - 1) * stride;
                p = make_float4(r[min(k0 + kk, K - 1)], r[min(k0 + kk + 1, K - 1)], r[min(k0 + kk + 2, K - 1)], r[min(k0 + kk + 3, K - 1)]);
            }
        } else {
            const int kk = f / TQ, tc = 4 * (f % TQ);   // row k, first tile column
            if constexpr (FAST) {
                p = *reinterpret_cast<const float4 *>(base + (long)(k0 + kk) * stride + t0 + tc);
            } else {
                const float *r = base + (long)min(k0 + kk, K - 1) * stride;
                p = make_float4(r[min(t0 + tc, tn - 1)], r[min(t0 + tc + 1, tn - 1)], r[min(t0 + tc + 2, tn - 1)], r[min(t0 + tc + 3, tn - 1)]);
            }
        }
    };
    auto stage_op = [&](auto turned, float *buf, int pitch, int f, const float4 &p) {
        if constexpr (decltype(turned)::value) {
            const int tt = f / KQ, kk = 4 * (f % KQ);
            buf[(kk + 0) * pitch + tt] = p.x;
            buf[(kk + 1) * pitch + tt] = p.y;
            buf[(kk + 2) * pitch + tt] = p.z;
            buf[(kk + 3) * pitch + tt] = p.w;
        } else {
            const int kk = f / TQ, tc = 4 * (f % TQ);
            *reinterpret_cast<float4 *>(&buf[kk * pitch + tc]) = p;
        }
    };
    constexpr std::integral_constant<bool, XTURN> xturn{};
    constexpr std::integral_constant<bool, YTURN> yturn{};

    // Two chunks in flight: two float4 of each operand per thread and chunk, float4 number f = tid and tid + 256 of the chunk
    float4 ax0, ax1, ay0, ay1, bx0, bx1, by0, by1;   // set a: even chunks, set b: odd chunks (named registers, as in mat_mul.hip)
    auto load = [&](int k0, float4 &rx0, float4 &rx1, float4 &ry0, float4 &ry1) {
        load_op(xturn, g.A, g.sa, x0, g.M, k0, tid, rx0);
        load_op(yturn, g.B, g.sb, y0, g.N, k0, tid, ry0);
        load_op(xturn, g.A, g.sa, x0, g.M, k0, tid + 256, rx1);
        load_op(yturn, g.B, g.sb, y0, g.N, k0, tid + 256, ry1);
    };
    auto stage = [&](int buf, const float4 &rx0, const float4 &rx1, const float4 &ry0, const float4 &ry1) {
        stage_op(xturn, sX[buf], XP, tid, rx0);
        stage_op(yturn, sY[buf], YP, tid, ry0);
        stage_op(xturn, sX[buf], XP, tid + 256, rx1);
        stage_op(yturn, sY[buf], YP, tid + 256, ry1);
    };

    floatx16 acc[W][W];
#pragma unroll
    for (int a = 0; a < W; a++)
#pragma unroll
        for (int b = 0; b < W; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][b][r] = 0.0f;

    // one MFMA step: k = 2 * s (lanes 0 .. 31) and 2 * s + 1 (lanes 32 .. 63), in that order inside the instruction
    auto step = [&](const float *pa, const float *pb, int s) {
        float av[W], bv[W];
#pragma unroll
        for (int a = 0; a < W; a++) av[a] = pa[2 * s * YP + 32 * a];
#pragma unroll
        for (int b = 0; b < W; b++) bv[b] = pb[2 * s * XP + 32 * b];
#pragma unroll
        for (int a = 0; a < W; a++)
#pragma unroll
            for (int b = 0; b < W; b++) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[b], acc[a][b], 0, 0, 0);
    };

    // Chunk c is computed from LDS buffer c & 1 while the loads of chunk c + 2 are issued and, after the MFMAs, chunk c + 1 (loaded one
    // whole chunk earlier) goes to the other buffer, last read in iteration c - 1 behind that iteration's barrier.
    const int nchunk = (K + KCH - 1) / KCH;
    auto chunk = [&](int c, float4 &nx0, float4 &nx1, float4 &ny0, float4 &ny1, const float4 &sx0, const float4 &sx1, const float4 &sy0, const float4 &sy1) {
        const int buf = c & 1;
        load(min(c + 2, nchunk - 1) * KCH, nx0, nx1, ny0, ny1);   // unconditional (past the end: the last chunk again, never staged into a buffer that is read)
        const float *pa = sY[buf] + (lane >> 5) * YP + wy + (lane & 31);
        const float *pb = sX[buf] + (lane >> 5) * XP + wx + (lane & 31);
        const int kc = FAST ? KCH : min(KCH, K - c * KCH);   // k steps this chunk holds
        if (FAST || kc == KCH) {
            // a whole chunk: every operand read from LDS first, so that the reads of later steps are in flight under the MFMAs of earlier ones
            float av[KCH / 2][W], bv[KCH / 2][W];
#pragma unroll
            for (int s = 0; s < KCH / 2; s++) {
#pragma unroll
                for (int a = 0; a < W; a++) av[s][a] = pa[2 * s * YP + 32 * a];
#pragma unroll
                for (int b = 0; b < W; b++) bv[s][b] = pb[2 * s * XP + 32 * b];
            }
            __builtin_amdgcn_sched_barrier(0);   // or the scheduler sinks each read to its MFMA again, to save registers
#pragma unroll
            for (int s = 0; s < KCH / 2; s++)
#pragma unroll
                for (int a = 0; a < W; a++)
#pragma unroll
                    for (int b = 0; b < W; b++) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s][a], bv[s][b], acc[a][b], 0, 0, 0);
        } else {
#pragma unroll 1
            for (int s = 0; s < kc / 2; s++) step(pa, pb, s);
            if (kc & 1) {
                // The last step of an odd K has no partner: a zero-padded one would turn a chain that ends in -0 into +0.  It is a
                // VALU fmaf on each accumulator register instead, operands picked through the C/D map.
                const float *ky = sY[buf] + (kc - 1) * YP + wy + 4 * (lane >> 5);
                const float *kx = sX[buf] + (kc - 1) * XP + wx + (lane & 31);
#pragma unroll
                for (int a = 0; a < W; a++)
#pragma unroll
                    for (int b = 0; b < W; b++) {
                        const float xv = kx[32 * b];
#pragma unroll
                        for (int r = 0; r < 16; r++) {
                            const int row = (r & 3) + 8 * (r >> 2);
                            acc[a][b][r] = __builtin_fmaf(xv, ky[32 * a + row], acc[a][b][r]);
                        }
                    }
            }
        }
        stage(buf ^ 1, sx0, sx1, sy0, sy1);
        __syncthreads();
    };
    load(0, ax0, ax1, ay0, ay1);
    stage(0, ax0, ax1, ay0, ay1);
    load(min(1, nchunk - 1) * KCH, bx0, bx1, by0, by1);
    __syncthreads();
#pragma unroll 1
    for (int c = 0; c < nchunk; c += 2) {
        chunk(c, ax0, ax1, ay0, ay1, bx0, bx1, by0, by1);
        if (c + 1 < nchunk) chunk(c + 1, bx0, bx1, by0, by1, ax0, ax1, ay0, ay1);
    }

    // ---- epilogue: result(x, y) = mad2(a, ab, b, C(x, y)), x = lane & 31 contiguous; C is read where the result is written
#pragma unroll
    for (int a = 0; a < W; a++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int y = y0 + wy + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
#pragma unroll
            for (int b = 0; b < W; b++) {
                const int x = x0 + wx + 32 * b + (lane & 31);
                if (FAST || (y < g.N && x < g.M)) g.out[(long)y * g.so + x] = dev::mad2(g.a, acc[a][b][r], g.b, g.C[(long)y * g.sc + x]);
            }
        }
}
#endif   // HLMI_CANON_FMA

// The second implementation: one thread per output, the chain as written.
template<bool TA, bool TB>
__global__ __launch_bounds__(256) void sgemm_general(GGeom g) {
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= g.M) return;
    const float *pa = TA ? g.A + (long)i * g.sa : g.A + i;
    const float *pb = TB ? g.B + j : g.B + (long)j * g.sb;
    const long da = TA ? 1 : g.sa, db = TB ? g.sb : 1;
    float ab = 0.0f;
    for (int k = 0; k < g.K; k++) ab = dev::mad(pa[k * da], pb[k * db], ab);
    g.out[(long)j * g.so + i] = dev::mad2(g.a, ab, g.b, g.C[(long)j * g.sc + i]);
}

// ---------------------------------------------------------------------------------------------------------------- host: tables
// no estimates: the generators declare none
const ArgTable scopy_table("halide_scopy_impl", {scalar_f32("a"), in_buf("x", T_F32, 1), in_buf("y", T_F32, 1), out_buf("result", T_F32, 1)});
const ArgTable sscal_table("halide_sscal_impl", {scalar_f32("a"), in_buf("x", T_F32, 1), in_buf("y", T_F32, 1), out_buf("result", T_F32, 1)});
const ArgTable saxpy_table("halide_saxpy_impl", {scalar_f32("a"), in_buf("x", T_F32, 1), in_buf("y", T_F32, 1), out_buf("result", T_F32, 1)});
const ArgTable sdot_table("halide_sdot", {in_buf("x", T_F32, 1), in_buf("y", T_F32, 1), out_buf("result", T_F32, 0)});
const ArgTable sasum_table("halide_sasum", {in_buf("x", T_F32, 1), out_buf("result", T_F32, 0)});
const ArgTable sgemv_n_table("halide_sgemv_notrans", {scalar_f32("a"), in_buf("A", T_F32, 2), in_buf("x", T_F32, 1), scalar_f32("b"),
                                                      in_buf("y", T_F32, 1), out_buf("output", T_F32, 1)});
const ArgTable sgemv_t_table("halide_sgemv_trans", {scalar_f32("a"), in_buf("A", T_F32, 2), in_buf("x", T_F32, 1), scalar_f32("b"),
                                                    in_buf("y", T_F32, 1), out_buf("output", T_F32, 1)});
const ArgTable sger_table("halide_sger_impl", {scalar_f32("a"), in_buf("x", T_F32, 1), in_buf("y", T_F32, 1), out_buf("result", T_F32, 2)});
#define HLMI_SGEMM_ARGS {scalar_f32("a_"), in_buf("A_", T_F32, 2), in_buf("B_", T_F32, 2), scalar_f32("b_"), in_buf("C_", T_F32, 2), out_buf("result", T_F32, 2)}
const ArgTable sgemm_tables[4] = {{"halide_sgemm_notrans", HLMI_SGEMM_ARGS}, {"halide_sgemm_transA", HLMI_SGEMM_ARGS},
                                  {"halide_sgemm_transB", HLMI_SGEMM_ARGS}, {"halide_sgemm_transAB", HLMI_SGEMM_ARGS}};   // index: tA + 2 * tB

// the host-side checks (alignment, overlap, pins, derived extents, limits, query answers): linear_algebra_host.h, shared with the f64 half

// ---------------------------------------------------------------------------------------------------------------- host: scopy, sscal, saxpy, sger
enum ElemLaunch { EL_VEC4, EL_SCALAR, EL_GENERAL };
const char *const elem_names[4][3] = {{"scopy_vec4", "scopy_scalar", "scopy_general"},
                                      {"sscal_vec4", "sscal_scalar", "sscal_general"},
                                      {"saxpy_vec4", "saxpy_scalar", "saxpy_general"},
                                      {"sger_vec4", "sger_scalar", "sger_general"}};

// THE predicate of the four elementwise pipelines: 16-byte accesses where every address a lane forms is a multiple of 16 bytes — x, the
// result, saxpy's y and, for sger, the result's column stride — and one element per thread otherwise.
ElemLaunch elem_plan(int mode, const EGeom &g, bool general_only) {
    if (general_only) return EL_GENERAL;
    const bool vec = aligned16(g.x) && aligned16(g.r) && (mode != E_AXPY || aligned16(g.y)) && (mode != E_GER || g.ldr % 4 == 0);
    return vec ? EL_VEC4 : EL_SCALAR;
}

template<int MODE>
int elem_launch_mode(void *uc, hipStream_t st, const EGeom &g, ElemLaunch l) {
    const char *name = elem_names[MODE][l];
    const double elems = (double)g.n * g.rows;
    timing_note_bytes(MODE == E_COPY || MODE == E_SCAL ? 8.0 * elems : MODE == E_AXPY ? 12.0 * elems : 8.0 * elems + 4.0 * (g.n + g.rows));
    const long per_thread = l == EL_VEC4 ? 4 : 1;
    const dim3 grid((unsigned)((g.n + 256 * per_thread - 1) / (256 * per_thread)), (unsigned)g.rows);
    if (l == EL_VEC4) HLMI_LAUNCH(uc, name, st, (la_elem<MODE, true>), grid, dim3(256), 0, g);
    else HLMI_LAUNCH(uc, name, st, (la_elem<MODE, false>), grid, dim3(256), 0, g);
    return 0;
}

int elem_launch(void *uc, hipStream_t st, int mode, const EGeom &g, ElemLaunch l) {
    if (g.n <= 0 || g.rows <= 0) return 0;   // a zero extent launches nothing
    switch (mode) {
    case E_COPY: return elem_launch_mode<E_COPY>(uc, st, g, l);
    case E_SCAL: return elem_launch_mode<E_SCAL>(uc, st, g, l);
    case E_AXPY: return elem_launch_mode<E_AXPY>(uc, st, g, l);
    default: return elem_launch_mode<E_GER>(uc, st, g, l);
    }
}

// scopy / sscal / saxpy.  y is looked at by saxpy only: the reference's wrappers pass a null pointer for it to the other two.
int vec_entry(int mode, float a, halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result, bool general_only) {
    void *uc = nullptr;
    const ArgTable &table = mode == E_COPY ? scopy_table : mode == E_SCAL ? sscal_table : saxpy_table;
    BufArg all[3];
    table.bufs(all, {x, y, result});
    BufArg args[3];
    int n = 0;
    args[n++] = all[0];
    if (mode == E_AXPY) args[n++] = all[1];
    args[n++] = all[2];
    int r = prologue(uc, args, n);
    if (r < 0) return r;
    const int size = derive({{x, 0}, {result, 0}, {mode == E_AXPY ? y : nullptr, 0}});
    if (r == 1) {
        for (int i = 0; i < n; i++) answer1(args[i].buf, size);
        return 0;
    }
    if ((r = limit(uc, table.md.name, "x.extent.0", size, MAX_VECTOR))) return r;
    check_shapes(uc, args, n);
    for (int i = 0; i < n; i++) pin(uc, args[i], 0, size, "x.extent.0");
    if ((r = checks_done(uc))) return r;
    // the wrappers' calls: sscal's result is x, saxpy's result is y
    if (overlap(result, x, mode == E_SCAL)) return report(uc, halide_error_code_constraint_violated, "Constraint violated: result may not overlap x");
    if (mode == E_AXPY && overlap(result, y, true))
        return report(uc, halide_error_code_constraint_violated, "Constraint violated: result may overlap y only where it is y");
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, n))) return r;
    const EGeom g = {dev_ptr<float>(x), mode == E_AXPY ? dev_ptr<float>(y) : nullptr, dev_ptr<float>(result), size, 0, 1, a};
    if ((r = elem_launch(uc, ctx.stream, mode, g, elem_plan(mode, g, general_only)))) return r;
    mark_output_written(result);
    return 0;
}

// sger: the result is read and written in place
int ger_entry(float a, halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result, bool general_only) {
    void *uc = nullptr;
    BufArg args[3];
    sger_table.bufs(args, {x, y, result});
    int r = prologue(uc, args, 3);
    if (r < 0) return r;
    const int m = derive({{x, 0}, {result, 0}}), n = derive({{y, 0}, {result, 1}});
    if (r == 1) {
        answer1(x, m), answer1(y, n), answer2(result, m, n);
        return 0;
    }
    if ((r = limit(uc, "halide_sger_impl", "x.extent.0", m, MAX_EXTENT)) || (r = limit(uc, "halide_sger_impl", "y.extent.0", n, MAX_EXTENT))) return r;
    check_shapes(uc, args, 3);
    pin(uc, args[0], 0, m, "x.extent.0");
    pin(uc, args[1], 0, n, "y.extent.0");
    pin(uc, args[2], 0, m, "x.extent.0");
    pin(uc, args[2], 1, n, "y.extent.0");
    if ((r = checks_done(uc))) return r;
    if (overlap(result, x, false) || overlap(result, y, false))
        return report(uc, halide_error_code_constraint_violated, "Constraint violated: result may not overlap %s", overlap(result, x, false) ? "x" : "y");
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, 3))) return r;
    // the matrix is an input as well: bring a host-dirty one to the device before it is marked as the output
    if (result->flags & halide_buffer_flag_host_dirty) {
        if (result->host == nullptr) return report(uc, halide_error_code_host_is_null, "Output buffer result host pointer is null");
        if ((r = input_to_device(uc, ctx, args[2]))) return r;
    }
    const EGeom g = {dev_ptr<float>(x), dev_ptr<float>(y), dev_ptr<float>(result), m, result->dim[1].stride, n, a};
    if ((r = elem_launch(uc, ctx.stream, E_GER, g, elem_plan(E_GER, g, general_only)))) return r;
    mark_output_written(result);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- host: sdot, sasum
int red_entry(bool asum, halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result, bool general_only) {
    void *uc = nullptr;
    BufArg args[3];
    int n = 0;
    if (asum) {
        BufArg two[2];
        sasum_table.bufs(two, {x, result});
        args[0] = two[0], args[1] = two[1], n = 2;
    } else {
        sdot_table.bufs(args, {x, y, result});
        n = 3;
    }
    const char *entry = asum ? "halide_sasum" : "halide_sdot";
    int r = prologue(uc, args, n);
    if (r < 0) return r;
    const int size = derive({{x, 0}, {asum ? nullptr : y, 0}});
    if (r == 1) {
        answer1(x, size);
        if (!asum) answer1(y, size);
        return 0;   // the 0-dimensional result has nothing to answer
    }
    if ((r = limit(uc, entry, "x.extent.0", size, MAX_VECTOR))) return r;
    check_shapes(uc, args, n);
    for (int i = 0; i < n - 1; i++) pin(uc, args[i], 0, size, "x.extent.0");
    if ((r = checks_done(uc))) return r;
    if (overlap(result, x, false) || (!asum && overlap(result, y, false)))
        return report(uc, halide_error_code_constraint_violated, "Constraint violated: result may not overlap %s", overlap(result, x, false) ? "x" : "y");
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, n))) return r;
    float *out = dev_ptr<float>(result);
    if (size == 0) {
        HLMI_HIP(uc, hipMemsetAsync(out, 0, 4, ctx.stream));   // a zero extent launches nothing: +0
    } else {
        const float *px = dev_ptr<float>(x), *py = asum ? nullptr : dev_ptr<float>(y);
        timing_note_bytes((asum ? 4.0 : 8.0) * size + 4.0);
        // THE predicate: the staged wave everywhere; one thread only where the caller asks for it by name
        const char *name = asum ? (general_only ? "sasum_general" : "sasum_wave") : (general_only ? "sdot_general" : "sdot_wave");
        const long ln = size;
        if (asum && general_only) HLMI_LAUNCH(uc, name, ctx.stream, la_reduce_general<true>, dim3(1), dim3(64), 0, px, py, out, ln);
        else if (asum) HLMI_LAUNCH(uc, name, ctx.stream, la_reduce<true>, dim3(1), dim3(64), 0, px, py, out, ln);
        else if (general_only) HLMI_LAUNCH(uc, name, ctx.stream, la_reduce_general<false>, dim3(1), dim3(64), 0, px, py, out, ln);
        else HLMI_LAUNCH(uc, name, ctx.stream, la_reduce<false>, dim3(1), dim3(64), 0, px, py, out, ln);
    }
    mark_output_written(result);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- host: sgemv
// A is w x h as stored.  notrans: x[h], y[w], output[w].  trans: x[w], y[h], output[h].
int gemv_entry(bool trans, float a, halide_buffer_t *A, halide_buffer_t *x, float b, halide_buffer_t *y, halide_buffer_t *output, bool general_only) {
    void *uc = nullptr;
    BufArg args[4];
    (trans ? sgemv_t_table : sgemv_n_table).bufs(args, {A, x, y, output});
    const char *entry = trans ? "halide_sgemv_trans" : "halide_sgemv_notrans";
    int r = prologue(uc, args, 4);
    if (r < 0) return r;
    const int w = trans ? derive({{A, 0}, {x, 0}}) : derive({{A, 0}, {y, 0}, {output, 0}});
    const int h = trans ? derive({{A, 1}, {y, 0}, {output, 0}}) : derive({{A, 1}, {x, 0}});
    const int nx = trans ? w : h, ny = trans ? h : w;
    if (r == 1) {
        answer2(A, w, h), answer1(x, nx), answer1(y, ny), answer1(output, ny);
        return 0;
    }
    if ((r = limit(uc, entry, "A.extent.0", w, MAX_EXTENT)) || (r = limit(uc, entry, "A.extent.1", h, MAX_EXTENT))) return r;
    check_shapes(uc, args, 4);
    pin(uc, args[0], 0, w, "A.extent.0");
    pin(uc, args[0], 1, h, "A.extent.1");
    pin(uc, args[1], 0, nx, trans ? "A.extent.0" : "A.extent.1");
    pin(uc, args[2], 0, ny, trans ? "A.extent.1" : "A.extent.0");
    pin(uc, args[3], 0, ny, trans ? "A.extent.1" : "A.extent.0");
    if ((r = checks_done(uc))) return r;
    if (overlap(output, A, false) || overlap(output, x, false))
        return report(uc, halide_error_code_constraint_violated, "Constraint violated: output may not overlap %s", overlap(output, A, false) ? "A" : "x");
    if (overlap(output, y, true)) return report(uc, halide_error_code_constraint_violated, "Constraint violated: output may overlap y only where it is y");
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, 4))) return r;
    if (ny > 0) {   // an empty sum still leaves b * y
        const VGeom g = {dev_ptr<float>(A), dev_ptr<float>(x), dev_ptr<float>(y), dev_ptr<float>(output), w, h, A->dim[1].stride, a, b};
        timing_note_bytes(4.0 * ((double)w * h + nx + 2.0 * ny));
        // THE predicate: the wave kernels everywhere; one thread per output only where the caller asks for it by name
        hipStream_t st = ctx.stream;
        if (!trans && !general_only) HLMI_LAUNCH(uc, "sgemv_notrans_wave", st, la_gemv_n, dim3((unsigned)((w + GEMV_WG - 1) / GEMV_WG)), dim3(GEMV_WG), 0, g);
        else if (!trans) HLMI_LAUNCH(uc, "sgemv_notrans_general", st, la_gemv_n_general, dim3((unsigned)((w + 255) / 256)), dim3(256), 0, g);
        else if (!general_only) HLMI_LAUNCH(uc, "sgemv_trans_wave", st, la_gemv_t, dim3((unsigned)((h + GEMV_WG / V - 1) / (GEMV_WG / V))), dim3(GEMV_WG), 0, g);
        else HLMI_LAUNCH(uc, "sgemv_trans_general", st, la_gemv_t_general, dim3((unsigned)((h + 255) / 256)), dim3(256), 0, g);
    }
    mark_output_written(output);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- host: sgemm
enum GemmLaunch { GM_MFMA, GM_MFMA_EDGE, GM_GENERAL };
const char *const gemm_names[3] = {"sgemm_mfma", "sgemm_mfma_edge", "sgemm_general"};

struct GemmPlan {
    GemmLaunch launch;
    int tile;   // workgroup tile edge of the two MFMA launches
};

// the large tile (LDS reuse 2 x) only where it still leaves a wave for every SIMD
constexpr int gemm_tile(int M, int N) {
    return ((M + LARGE_TILE - 1) / LARGE_TILE) * ((N + LARGE_TILE - 1) / LARGE_TILE) >= LARGE_FROM_WGS ? LARGE_TILE : SMALL_TILE;
}

// THE predicate.  The MFMA is a chain of fused steps: it is the contract's chain in the default build only, and needs one step at least.
// There the aligned kernel takes a call whose M and N are multiples of its tile and whose K is one of KC, with all four buffers on 16
// bytes and column strides a multiple of 16 bytes; the edge variant takes every other call; the general kernel runs where the caller
// asks for it by name, for K == 0, and for every call of the build with one rounding per operator.
GemmPlan gemm_plan(const GGeom &g, bool general_only) {
    const int tile = gemm_tile(g.M, g.N);
    if (general_only || !dev::CANON_FMA || g.K == 0) return {GM_GENERAL, tile};
    const bool fast = g.M % tile == 0 && g.N % tile == 0 && g.K % KC == 0 && aligned16(g.A, g.sa, 4) && aligned16(g.B, g.sb, 4) && aligned16(g.C, g.sc, 4) &&
                      aligned16(g.out, g.so, 4);
    return {fast ? GM_MFMA : GM_MFMA_EDGE, tile};
}

int gemm_launch(void *uc, hipStream_t st, bool tA, bool tB, const GGeom &g, const GemmPlan &p) {
    timing_note_bytes(4.0 * ((double)g.M * g.K + (double)g.K * g.N + 2.0 * g.M * g.N));   // each matrix read or written once
    const char *name = gemm_names[p.launch];
    if (p.launch == GM_GENERAL) {
        const dim3 grid((unsigned)((g.M + 255) / 256), (unsigned)g.N);
        return with_flags([&](auto ta, auto tb) {
            HLMI_LAUNCH(uc, name, st, (sgemm_general<ta.value, tb.value>), grid, dim3(256), 0, g);
            return 0;
        }, tA, tB);
    }
#if HLMI_CANON_FMA
    const dim3 grid((unsigned)((g.M + p.tile - 1) / p.tile), (unsigned)((g.N + p.tile - 1) / p.tile));
    return with_flags([&](auto large, auto fast, auto ta, auto tb) {
        HLMI_LAUNCH(uc, name, st, (sgemm_mfma<large.value ? 2 : 1, fast.value, ta.value, tb.value>), grid, dim3(256), 0, g);
        return 0;
    }, p.tile == LARGE_TILE, p.launch == GM_MFMA, tA, tB);
#else
    return report(uc, halide_error_code_internal_error, "sgemm: no MFMA kernel in this build");
#endif
}

// The shapes (blas_l3_generators.cpp:37-53, :167-171): num_rows = A_.width(), num_cols = B_.height() and sum_size = A_.height() are
// taken from the STORED A and B whatever the flags, B_.extent.0 is pinned to sum_size, C_ and result to num_rows x num_cols.  transA
// reads A_(k, i) for i < A_.width() and k < A_.height(): inside A_ only where A_ is square (elsewhere constant_exterior's zeros or
// nothing).  transB reads B_(j, k) for j < B_.height(), k < sum_size == B_.width(): square B_.  transAB swaps the two inputs and
// reads B_(i, k) and A_(k, j) over i < A_.width(), j < B_.height(), k < A_.height(): all three extents equal.
int gemm_entry(bool tA, bool tB, float a, halide_buffer_t *A, halide_buffer_t *B, float b, halide_buffer_t *C, halide_buffer_t *result, bool general_only) {
    void *uc = nullptr;
    const ArgTable &table = sgemm_tables[(tA ? 1 : 0) + (tB ? 2 : 0)];
    const char *entry = table.md.name;
    BufArg args[4];
    table.bufs(args, {A, B, C, result});
    int r = prologue(uc, args, 4);
    if (r < 0) return r;
    const int M = derive({{A, 0}, {C, 0}, {result, 0}}), K = derive({{A, 1}, {B, 0}}), N = derive({{B, 1}, {C, 1}, {result, 1}});
    if (r == 1) {
        answer2(A, M, K), answer2(B, K, N), answer2(C, M, N), answer2(result, M, N);
        return 0;
    }
    if ((r = limit(uc, entry, "A_.extent.0", M, MAX_EXTENT)) || (r = limit(uc, entry, "A_.extent.1", K, MAX_EXTENT)) ||
        (r = limit(uc, entry, "B_.extent.1", N, MAX_EXTENT)))
        return r;
    check_shapes(uc, args, 4);
    pin(uc, args[0], 0, M, "A_.extent.0");
    pin(uc, args[0], 1, K, "A_.extent.1");
    pin(uc, args[1], 0, K, "A_.extent.1");
    pin(uc, args[1], 1, N, "B_.extent.1");
    for (int i = 2; i < 4; i++) {
        pin(uc, args[i], 0, M, "A_.extent.0");
        pin(uc, args[i], 1, N, "B_.extent.1");
    }
    if (tA) check_equal(uc, "A_.extent.1", K, "A_.extent.0", M);   // a transposed operand is square
    if (tB) check_equal(uc, "B_.extent.1", N, "B_.extent.0", K);
    if ((r = checks_done(uc))) return r;
    if (overlap(result, A, false) || overlap(result, B, false))
        return report(uc, halide_error_code_constraint_violated, "Constraint violated: result may not overlap %s", overlap(result, A, false) ? "A_" : "B_");
    if (overlap(result, C, true)) return report(uc, halide_error_code_constraint_violated, "Constraint violated: result may overlap C_ only where it is C_");
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, 4))) return r;
    if (M > 0 && N > 0) {   // an empty sum still leaves mad2(a, +0, b, C)
        const GGeom g = {dev_ptr<float>(A), dev_ptr<float>(B), dev_ptr<float>(C), dev_ptr<float>(result), M, N, K,
                         A->dim[1].stride, B->dim[1].stride, C->dim[1].stride, result->dim[1].stride, a, b};
        if ((r = gemm_launch(uc, ctx.stream, tA, tB, g, gemm_plan(g, general_only)))) return r;
    }
    mark_output_written(result);
    return 0;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------- entry points
extern "C" int halide_scopy_impl(float a, halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result) { return vec_entry(E_COPY, a, x, y, result, false); }
HLMI_ENTRY(halide_scopy_impl, scopy_table.md)
extern "C" int halide_sscal_impl(float a, halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result) { return vec_entry(E_SCAL, a, x, y, result, false); }
HLMI_ENTRY(halide_sscal_impl, sscal_table.md)
extern "C" int halide_saxpy_impl(float a, halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result) { return vec_entry(E_AXPY, a, x, y, result, false); }
HLMI_ENTRY(halide_saxpy_impl, saxpy_table.md)
extern "C" int halide_sdot(halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result) { return red_entry(false, x, y, result, false); }
HLMI_ENTRY(halide_sdot, sdot_table.md)
extern "C" int halide_sasum(halide_buffer_t *x, halide_buffer_t *result) { return red_entry(true, x, nullptr, result, false); }
HLMI_ENTRY(halide_sasum, sasum_table.md)
extern "C" int halide_sgemv_notrans(float a, halide_buffer_t *A, halide_buffer_t *x, float b, halide_buffer_t *y, halide_buffer_t *output) {
    return gemv_entry(false, a, A, x, b, y, output, false);
}
HLMI_ENTRY(halide_sgemv_notrans, sgemv_n_table.md)
extern "C" int halide_sgemv_trans(float a, halide_buffer_t *A, halide_buffer_t *x, float b, halide_buffer_t *y, halide_buffer_t *output) {
    return gemv_entry(true, a, A, x, b, y, output, false);
}
HLMI_ENTRY(halide_sgemv_trans, sgemv_t_table.md)
extern "C" int halide_sger_impl(float a, halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result) { return ger_entry(a, x, y, result, false); }
HLMI_ENTRY(halide_sger_impl, sger_table.md)
extern "C" int halide_sgemm_notrans(float a, halide_buffer_t *A, halide_buffer_t *B, float b, halide_buffer_t *C, halide_buffer_t *result) {
    return gemm_entry(false, false, a, A, B, b, C, result, false);
}
HLMI_ENTRY(halide_sgemm_notrans, sgemm_tables[0].md)
extern "C" int halide_sgemm_transA(float a, halide_buffer_t *A, halide_buffer_t *B, float b, halide_buffer_t *C, halide_buffer_t *result) {
    return gemm_entry(true, false, a, A, B, b, C, result, false);
}
HLMI_ENTRY(halide_sgemm_transA, sgemm_tables[1].md)
extern "C" int halide_sgemm_transB(float a, halide_buffer_t *A, halide_buffer_t *B, float b, halide_buffer_t *C, halide_buffer_t *result) {
    return gemm_entry(false, true, a, A, B, b, C, result, false);
}
HLMI_ENTRY(halide_sgemm_transB, sgemm_tables[2].md)
extern "C" int halide_sgemm_transAB(float a, halide_buffer_t *A, halide_buffer_t *B, float b, halide_buffer_t *C, halide_buffer_t *result) {
    return gemm_entry(true, true, a, A, B, b, C, result, false);
}
HLMI_ENTRY(halide_sgemm_transAB, sgemm_tables[3].md)

// Measurement and test hook (hlmi_internal.h): the named entry point with one thread per output.  p0 .. p3 are the entry point's
// buffers in its own order (the unused trailing ones null); a and b are read where the entry point has them.
extern "C" int hlmi_linear_algebra_general(const char *name, float a, float b, halide_buffer_t *p0, halide_buffer_t *p1, halide_buffer_t *p2,
                                           halide_buffer_t *p3) {
    const char *n = name ? name : "(null)";
    if (!strcmp(n, "halide_scopy_impl")) return vec_entry(E_COPY, a, p0, p1, p2, true);
    if (!strcmp(n, "halide_sscal_impl")) return vec_entry(E_SCAL, a, p0, p1, p2, true);
    if (!strcmp(n, "halide_saxpy_impl")) return vec_entry(E_AXPY, a, p0, p1, p2, true);
    if (!strcmp(n, "halide_sdot")) return red_entry(false, p0, p1, p2, true);
    if (!strcmp(n, "halide_sasum")) return red_entry(true, p0, nullptr, p1, true);
    if (!strcmp(n, "halide_sgemv_notrans")) return gemv_entry(false, a, p0, p1, b, p2, p3, true);
    if (!strcmp(n, "halide_sgemv_trans")) return gemv_entry(true, a, p0, p1, b, p2, p3, true);
    if (!strcmp(n, "halide_sger_impl")) return ger_entry(a, p0, p1, p2, true);
    if (!strcmp(n, "halide_sgemm_notrans")) return gemm_entry(false, false, a, p0, p1, b, p2, p3, true);
    if (!strcmp(n, "halide_sgemm_transA")) return gemm_entry(true, false, a, p0, p1, b, p2, p3, true);
    if (!strcmp(n, "halide_sgemm_transB")) return gemm_entry(false, true, a, p0, p1, b, p2, p3, true);
    if (!strcmp(n, "halide_sgemm_transAB")) return gemm_entry(true, true, a, p0, p1, b, p2, p3, true);
    return report(nullptr, halide_error_code_constraint_violated, "hlmi_linear_algebra_general: no entry point named %s", n);
}

// ---------------------------------------------------------------------------------------------------------------- hblas_s*
// include/hlmi_blas.h states the interface and where it departs from the reference's.  Each call wraps the caller's host arrays in
// buffers, runs the entry point, brings the result home and lets go of the device side.
namespace {

struct HostVec {
    halide_dimension_t dim[2];
    halide_buffer_t buf;
    HostVec(const float *p, int w, int h = -1, int ld = 0) {
        dim[0] = {0, w, 1, 0};
        dim[1] = {0, h, ld, 0};
        memset(&buf, 0, sizeof buf);
        buf.host = (uint8_t *)const_cast<float *>(p);
        buf.flags = halide_buffer_flag_host_dirty;
        buf.type.code = halide_type_float, buf.type.bits = 32;
        buf.dimensions = h < 0 ? 1 : 2;
        buf.dim = dim;
    }
    ~HostVec() { halide_device_free(nullptr, &buf); }
    HostVec(const HostVec &) = delete;
};

bool hblas_refuse(const char *fn, const char *why) {
    fprintf(stderr, "%s: %s: nothing computed\n", fn, why);
    return true;
}
bool bad_inc(const char *fn, int incx, int incy = 1) { return (incx != 1 || incy != 1) && hblas_refuse(fn, "only increments of 1 are supported"); }
bool bad_order(const char *fn, enum HBLAS_ORDER order) { return order != HblasColMajor && hblas_refuse(fn, "only HblasColMajor is supported"); }

// the entry point's code; the result comes home whatever it was
int finish(const char *fn, int code, halide_buffer_t *out) {
    if (code == 0) code = halide_copy_to_host(nullptr, out);
    if (code != 0) fprintf(stderr, "%s: the pipeline returned %d\n", fn, code);
    return code;
}

}  // namespace

extern "C" void hblas_scopy(const int N, const float *X, const int incX, float *Y, const int incY) {
    if (bad_inc("hblas_scopy", incX, incY)) return;
    HostVec x(X, N), y(Y, N);
    finish("hblas_scopy", halide_scopy(&x.buf, &y.buf), &y.buf);
}

extern "C" void hblas_sscal(const int N, const float alpha, float *X, const int incX) {
    if (bad_inc("hblas_sscal", incX)) return;
    HostVec x(X, N);
    finish("hblas_sscal", halide_sscal(alpha, &x.buf), &x.buf);
}

extern "C" void hblas_saxpy(const int N, const float alpha, const float *X, const int incX, float *Y, const int incY) {
    if (bad_inc("hblas_saxpy", incX, incY)) return;
    HostVec x(X, N), y(Y, N);
    finish("hblas_saxpy", halide_saxpy(alpha, &x.buf, &y.buf), &y.buf);
}

extern "C" float hblas_sdot(const int N, const float *X, const int incX, const float *Y, const int incY) {
    if (bad_inc("hblas_sdot", incX, incY)) return NAN;
    float result = NAN;
    HostVec x(X, N), y(Y, N), r(&result, 0);
    r.buf.dimensions = 0;
    return finish("hblas_sdot", halide_sdot(&x.buf, &y.buf, &r.buf), &r.buf) == 0 ? result : NAN;
}

extern "C" float hblas_snrm2(const int N, const float *X, const int incX) {
    if (bad_inc("hblas_snrm2", incX)) return NAN;
    float result = NAN;
    HostVec x(X, N), r(&result, 0);
    r.buf.dimensions = 0;
    return finish("hblas_snrm2", halide_sdot(&x.buf, &x.buf, &r.buf), &r.buf) == 0 ? sqrtf(result) : NAN;
}

extern "C" float hblas_sasum(const int N, const float *X, const int incX) {
    if (bad_inc("hblas_sasum", incX)) return NAN;
    float result = NAN;
    HostVec x(X, N), r(&result, 0);
    r.buf.dimensions = 0;
    return finish("hblas_sasum", halide_sasum(&x.buf, &r.buf), &r.buf) == 0 ? result : NAN;
}

extern "C" void hblas_sgemv(const enum HBLAS_ORDER order, const enum HBLAS_TRANSPOSE TransA, const int M, const int N, const float alpha, const float *A,
                            const int lda, const float *X, const int incX, const float beta, float *Y, const int incY) {
    if (bad_order("hblas_sgemv", order) || bad_inc("hblas_sgemv", incX, incY)) return;
    const bool t = TransA != HblasNoTrans;
    HostVec a(A, M, N, lda), x(X, t ? M : N), y(Y, t ? N : M);
    finish("hblas_sgemv", halide_sgemv(t, alpha, &a.buf, &x.buf, beta, &y.buf), &y.buf);
}

extern "C" void hblas_sger(const enum HBLAS_ORDER order, const int M, const int N, const float alpha, const float *X, const int incX, const float *Y,
                           const int incY, float *A, const int lda) {
    if (bad_order("hblas_sger", order) || bad_inc("hblas_sger", incX, incY)) return;
    HostVec x(X, M), y(Y, N), a(A, M, N, lda);
    finish("hblas_sger", halide_sger(alpha, &x.buf, &y.buf, &a.buf), &a.buf);
}

extern "C" void hblas_sgemm(const enum HBLAS_ORDER Order, const enum HBLAS_TRANSPOSE TransA, const enum HBLAS_TRANSPOSE TransB, const int M, const int N,
                            const int K, const float alpha, const float *A, const int lda, const float *B, const int ldb, const float beta, float *C,
                            const int ldc) {
    if (bad_order("hblas_sgemm", Order)) return;
    const bool tA = TransA != HblasNoTrans, tB = TransB != HblasNoTrans;
    // the generator's shapes (hlmi_pipelines.h): a transposed operand is square
    if (((tA && M != K) || (tB && N != K)) && hblas_refuse("hblas_sgemm", "a transposed operand must be square (M == K for TransA, N == K for TransB)")) return;
    HostVec a(A, tA ? K : M, tA ? M : K, lda), b(B, tB ? N : K, tB ? K : N, ldb), c(C, M, N, ldc);
    finish("hblas_sgemm", halide_sgemm(tA, tB, alpha, &a.buf, &b.buf, beta, &c.buf), &c.buf);
}
