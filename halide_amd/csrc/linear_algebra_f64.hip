// linear_algebra_f64.hip — gfx950 implementation of the twelve f64 AOT pipelines of apps/linear_algebra (the `halide_d*` objects behind
// halide_blas.h) and of the CBLAS-shaped hblas_d* calls over them (include/hlmi_blas.h).  The sibling of linear_algebra.hip: the
// generators are templates on T, and this file is their instantiation at T = double.
//
// Algorithms: apps/linear_algebra/src/blas_l1_generators.cpp, blas_l2_generators.cpp, blas_l3_generators.cpp; the contract the kernels
// share with the checker (tests/cpp/linear_algebra_f64_check.c) is restated in include/hlmi_pipelines.h and DESIGN.md section 5.10.
// What differs from the f32 half: elements are 8 bytes, the scalars a and b are doubles, and a vectorised reduction keeps V = 4 lane
// sums — natural_vector_size(double) of the reference's x86-64 AVX2 build.  The float forms are the double overloads of dev::mad /
// dev::mad2 (fused in the default build, one rounding per operator with HLMI_CANON_FMA=0).
//
// Every pipeline has two implementations.  The second one — one thread per output running the chain as written — is reached only
// through hlmi_linear_algebra_general_f64(); `<family>_plan()` is the one place that chooses a launch:
//   dcopy / dscal / daxpy / dger   ld_elem<MODE, VEC>: two 16-byte accesses (2 x 2 doubles) per lane where every address (and the
//                                  matrix's column stride) allows, one element per thread otherwise
//   ddot / dasum                   ld_reduce: ONE wave, four chain lanes.  The wave loads 128 elements of each operand with coalesced
//                                  512-byte loads, one block ahead, hands them through LDS to the four chain lanes (each reads its 32
//                                  steps as sixteen 16-byte LDS loads), and lanes 0 .. 3 step the chains
//   dgemv_notrans                  ld_gemv_n: one sequential chain per output, lanes along i, k unrolled by GEMV_U with the next
//                                  GEMV_U loads in flight under the fmas
//   dgemv_trans                    ld_gemv_t: a wave owns 16 outputs x 4 chains; the lane sum is __shfl with width 4
//   dgemm (four variants)          dgemm_tile<TM, FAST, TA, TB>: 256 threads as 16 x 16, each with a TM x 4 register block of outputs
//                                  stepped by v_fma_f64 (or v_mul_f64 + v_add_f64) strictly upward in k: the contract's chain by
//                                  construction, in BOTH canonical forms.  Both operands are staged k-major in LDS — an operand
//                                  contiguous along its tile dimension is copied straight in with 16-byte stores, one contiguous
//                                  along k is turned on the way in (pitch + 2) — double-buffered, the next chunk's global loads in
//                                  flight under this chunk's fmas.  One 16-byte LDS read per two A values and per two B values.  No
//                                  zero-padded k step: the K edge is a loop bound.  The C loads of the mad2 epilogue are issued
//                                  under the last chunk.  The f64 MFMA is not used (an open question).
#include "hlmi_blas.h"
#include "hlmi_device_math.h"
#include "hlmi_internal.h"
#include "linear_algebra_host.h"

#include <math.h>

using namespace hlmi;
using namespace hlmi::la_host;

namespace {

constexpr int V = 4;                     // natural_vector_size(double) of the reference's x86-64 AVX2 target
constexpr int MAX_VECTOR = 134217728;    // vector lengths 0 .. 2^27
constexpr int MAX_EXTENT = 8192;         // matrix extents 0 .. 8192
constexpr int ELEM_BLOCK = 1024;         // elements a 256-thread workgroup of ld_elem<., true> moves: two double2 per lane
constexpr int RED_BLOCK = 128;           // elements of each operand ld_reduce stages per step of its pipeline: 32 chain steps
constexpr int RED_PITCH = 40;            // doubles between the chain lanes' rows in LDS: rows 16-byte aligned, 16 banks apart
constexpr int GEMV_WG = 64;              // threads of a gemv workgroup: one wave
constexpr int GEMV_U = 8;                // k steps per unrolled group of the two gemv kernels
constexpr int TILE_N = 64;               // dgemm workgroup tile along j: 16 threads x 4 outputs
constexpr int SMALL_TILE = 64;           // dgemm workgroup tile along i with 4 x 4 outputs per thread
constexpr int LARGE_TILE = 128;          // dgemm workgroup tile along i with 8 x 4 outputs per thread
constexpr int LARGE_FROM_WGS = 256;      // the large tile where it still leaves a workgroup for every CU
constexpr int KC = 16;                   // k steps per staged chunk

// ---------------------------------------------------------------------------------------------------------------- elementwise
enum ElemMode { E_COPY, E_SCAL, E_AXPY, E_GER };

struct EGeom {
    const double *x;   // [n]
    const double *y;   // AXPY: [n], read at i; GER: [rows], read at j
    double *r;         // [n] or [n x rows]; GER reads it too
    long n, ldr;
    int rows;
    double a;
};

template<int MODE>
__device__ __forceinline__ double elem_value(double a, double x, double y, double r) {
    if (MODE == E_COPY) return x;
    if (MODE == E_SCAL) return a * x;
    if (MODE == E_AXPY) return dev::mad(a, x, y);
    return dev::mad(a * y, x, r);   // GER: (a * y(j)) * x(i) + result(i, j)
}

template<int MODE, bool VEC>
__global__ __launch_bounds__(256) void ld_elem(EGeom g) {
    const long j = blockIdx.y;
    double *row = g.r + j * g.ldr;
    const double yj = MODE == E_GER ? g.y[j] : 0.0;
    if (VEC) {
        // pair p of the workgroup's 512: elements 2 p and 2 p + 1; a lane moves pairs tid and tid + 256, so each access of a wave is 1 KiB
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const long i = (long)blockIdx.x * ELEM_BLOCK + 2 * (threadIdx.x + 256 * h);
            if (i + 2 <= g.n) {
                const double2 xv = *reinterpret_cast<const double2 *>(g.x + i);
                double2 yv = make_double2(yj, yj), rv = make_double2(0.0, 0.0);
                if (MODE == E_AXPY) yv = *reinterpret_cast<const double2 *>(g.y + i);
                if (MODE == E_GER) rv = *reinterpret_cast<const double2 *>(row + i);
                *reinterpret_cast<double2 *>(row + i) = make_double2(elem_value<MODE>(g.a, xv.x, yv.x, rv.x), elem_value<MODE>(g.a, xv.y, yv.y, rv.y));
            } else if (i < g.n) {   // the last element of an odd n
                row[i] = elem_value<MODE>(g.a, g.x[i], MODE == E_AXPY ? g.y[i] : yj, MODE == E_GER ? row[i] : 0.0);
            }
        }
    } else {
        const long idx = (long)blockIdx.x * 256 + threadIdx.x;
        if (idx >= g.n) return;
        row[idx] = elem_value<MODE>(g.a, g.x[idx], MODE == E_AXPY ? g.y[idx] : yj, MODE == E_GER ? row[idx] : 0.0);
    }
}

// ---------------------------------------------------------------------------------------------------------------- ddot, dasum
template<bool ASUM>
__device__ __forceinline__ double red_step(double x, double y, double acc) { return ASUM ? acc + fabs(x) : dev::mad(x, y, acc); }

// one wave; y is not read by dasum
template<bool ASUM>
__global__ __launch_bounds__(64) void ld_reduce(const double *x, const double *y, double *result, long n) {
    __shared__ __attribute__((aligned(16))) double sx[2][V * RED_PITCH];
    __shared__ __attribute__((aligned(16))) double sy[2][V * RED_PITCH];
    constexpr int PER_LANE = RED_BLOCK / 64;     // loads per lane, operand and block
    constexpr int STEPS = RED_BLOCK / V;         // chain steps per block
    const int lane = threadIdx.x;
    const long nblk = n / RED_BLOCK;
    double px[PER_LANE], py[PER_LANE];   // the block in flight: element 64 c + lane of it
    auto load = [&](long blk) {
#pragma unroll
        for (int c = 0; c < PER_LANE; c++) {
            px[c] = x[blk * RED_BLOCK + 64 * c + lane];
            if (!ASUM) py[c] = y[blk * RED_BLOCK + 64 * c + lane];
        }
    };
    // element e of a block belongs to chain e % 4, step e / 4: chain lane i finds its 32 steps in row i
    auto stage = [&](int buf) {
#pragma unroll
        for (int c = 0; c < PER_LANE; c++) {
            sx[buf][(lane & (V - 1)) * RED_PITCH + (64 / V) * c + lane / V] = px[c];
            if (!ASUM) sy[buf][(lane & (V - 1)) * RED_PITCH + (64 / V) * c + lane / V] = py[c];
        }
    };
    double acc = 0.0;   // lanes 0 .. 3: the chains
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
            const double2 *rx = reinterpret_cast<const double2 *>(&sx[buf][lane * RED_PITCH]);
            const double2 *ry = reinterpret_cast<const double2 *>(&sy[buf][lane * RED_PITCH]);
            double2 vx[STEPS / 2], vy[STEPS / 2];
#pragma unroll
            for (int q = 0; q < STEPS / 2; q++) {
                vx[q] = rx[q];
                vy[q] = ASUM ? vx[q] : ry[q];
            }
#pragma unroll
            for (int q = 0; q < STEPS / 2; q++) {
                acc = red_step<ASUM>(vx[q].x, vy[q].x, acc);
                acc = red_step<ASUM>(vx[q].y, vy[q].y, acc);
            }
        }
        __syncthreads();
    }
    // the whole steps past the last block, straight from global memory
    const long nvec = n / V;
    if (lane < V)
        for (long k = nblk * STEPS; k < nvec; k++) acc = red_step<ASUM>(x[k * V + lane], ASUM ? 0.0 : y[k * V + lane], acc);
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < V; i++) s = s + __shfl(acc, i);
    double t = 0.0;
    for (long e = nvec * V; e < n; e++) t = red_step<ASUM>(x[e], ASUM ? 0.0 : y[e], t);
    if (lane == 0) *result = s + t;
}

template<bool ASUM>
__global__ __launch_bounds__(64) void ld_reduce_general(const double *x, const double *y, double *result, long n) {
    if (threadIdx.x != 0) return;
    double lanes[V];
#pragma unroll
    for (int i = 0; i < V; i++) lanes[i] = 0.0;
    const long nvec = n / V;
    for (long k = 0; k < nvec; k++)
#pragma unroll
        for (int i = 0; i < V; i++) lanes[i] = red_step<ASUM>(x[k * V + i], ASUM ? 0.0 : y[k * V + i], lanes[i]);
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < V; i++) s = s + lanes[i];
    double t = 0.0;
    for (long e = nvec * V; e < n; e++) t = red_step<ASUM>(x[e], ASUM ? 0.0 : y[e], t);
    *result = s + t;
}

// ---------------------------------------------------------------------------------------------------------------- dgemv
struct VGeom {
    const double *A, *x, *y;
    double *out;
    int w, h;   // A's extents: dimension 0 (contiguous) and dimension 1
    long lda;
    double a, b;
};

// notrans: output(i) = the chain over k of mad(a * A(i, k), x(k), .) from b * y(i); i < w, k < h
__global__ __launch_bounds__(GEMV_WG) void ld_gemv_n(VGeom g) {
    const int i = blockIdx.x * GEMV_WG + threadIdx.x;
    if (i >= g.w) return;
    double acc = g.b * g.y[i];
    const double *col = g.A + i;
    int k = 0;
    if (g.h >= GEMV_U) {
        double cur[GEMV_U], nxt[GEMV_U];
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

__global__ __launch_bounds__(256) void ld_gemv_n_general(VGeom g) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.w) return;
    double acc = g.b * g.y[i];
    for (int k = 0; k < g.h; k++) acc = dev::mad(g.a * g.A[(long)k * g.lda + i], g.x[k], acc);
    g.out[i] = acc;
}

// trans: output(i), i < h, from column i of A: V lane chains over k of mad(A(kV + j, i), x(kV + j), .), their sum from +0 in lane
// order, the tail on top of the sum, then mad2(b, y(i), a, s).  Lane l: output 16 * block + l / 4, chain l % 4.
__global__ __launch_bounds__(GEMV_WG) void ld_gemv_t(VGeom g) {
    const int lane = threadIdx.x, j = lane & (V - 1);
    const int o = blockIdx.x * (GEMV_WG / V) + lane / V;
    const double *col = g.A + (long)min(o, g.h - 1) * g.lda;   // the lanes past the last output repeat it and store nothing
    const int nvec = g.w / V;
    double acc = 0.0;
    int k = 0;
    if (nvec >= GEMV_U) {
        double ca[GEMV_U], cx[GEMV_U], na[GEMV_U], nx[GEMV_U];
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
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < V; i++) s = s + __shfl(acc, i, V);
    for (int t = nvec * V; t < g.w; t++) s = dev::mad(col[t], g.x[t], s);
    if (j == 0 && o < g.h) g.out[o] = dev::mad2(g.b, g.y[o], g.a, s);
}

__global__ __launch_bounds__(256) void ld_gemv_t_general(VGeom g) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= g.h) return;
    const double *col = g.A + (long)o * g.lda;
    double lanes[V];
#pragma unroll
    for (int i = 0; i < V; i++) lanes[i] = 0.0;
    const int nvec = g.w / V;
    for (int k = 0; k < nvec; k++)
#pragma unroll
        for (int i = 0; i < V; i++) lanes[i] = dev::mad(col[k * V + i], g.x[k * V + i], lanes[i]);
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < V; i++) s = s + lanes[i];
    for (int t = nvec * V; t < g.w; t++) s = dev::mad(col[t], g.x[t], s);
    g.out[o] = dev::mad2(g.b, g.y[o], g.a, s);
}

// ---------------------------------------------------------------------------------------------------------------- dgemm
struct GGeom {
    const double *A, *B, *C;
    double *out;
    int M, N, K;             // result is M x N (i < M contiguous), the sum runs over K
    long sa, sb, sc, so;     // column strides in elements
    double a, b;
};

// x = i (contiguous in C and the result), y = j.  Operand X[k][x] = opA(x, k): A[k * sa + x] (straight) or, TA, A[x * sa + k] (turned).
// Operand Y[k][y] = opB(k, y): B[y * sb + k] (turned) or, TB, B[k * sb + y] (straight).  Thread (tx, ty) of 16 x 16 holds the outputs
// x = 2 tx + {0, 1} + 32 r (r < TM / 2), y = 2 ty + {0, 1} + 32 s (s < 2): a 16-byte LDS read brings two X or two Y values, the 16
// lanes of one ty read 256 contiguous bytes, and the lanes of one tx read the same address.
template<int TM, bool FAST, bool TA, bool TB>
__global__ __launch_bounds__(256) void dgemm_tile(GGeom g) {
    constexpr int TX = 16 * TM;        // tile extent along x
    constexpr int TY = TILE_N;         // tile extent along y
    constexpr int RX = TM / 2, RY = 2; // double2 per thread along x and along y
    constexpr bool XTURN = TA, YTURN = !TB;
    constexpr int XP = XTURN ? TX + 2 : TX, YP = YTURN ? TY + 2 : TY;   // LDS pitches: even, so that rows stay 16-byte aligned
    constexpr int NX = KC * TX / 2 / 256, NY = KC * TY / 2 / 256;      // double2 per thread, operand and chunk
    static_assert(KC * TX / 2 % 256 == 0 && KC * TY / 2 % 256 == 0, "whole double2 per thread");
    __shared__ __attribute__((aligned(16))) double sX[2][KC * XP];  // [k][x]
    __shared__ __attribute__((aligned(16))) double sY[2][KC * YP];  // [k][y]
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
    const int K = g.K;

    // double2 number f of a chunk of one operand: `t0` the tile's origin in the operand's tile dimension, `tn` that dimension's extent,
    // `td` the tile's extent
    auto load_op = [&](auto turned, const double *base, long stride, int t0, int tn, int td, int k0, int f) -> double2 {
        if constexpr (decltype(turned)::value) {
            const int tt = f / (KC / 2), kk = 2 * (f % (KC / 2));   // tile row tt, first k
            if constexpr (FAST) {
                return *reinterpret_cast<const double2 *>(base + (long)(t0 + tt) * stride + k0 + kk);
            } else {   // clamped: what lies past the matrix is loaded from its last row / column and never reaches a stored result
                const double *r = base + (long)min(t0 + tt, tn - 1) * stride;
                return make_double2(r[min(k0 + kk, K - 1)], r[min(k0 + kk + 1, K - 1)]);
            }
        } else {
            const int kk = f / (td / 2), tc = 2 * (f % (td / 2));   // row k, first tile column
            if constexpr (FAST) {
                return *reinterpret_cast<const double2 *>(base + (long)(k0 + kk) * stride + t0 + tc);
            } else {
                const double *r = base + (long)min(k0 + kk, K - 1) * stride;
                return make_double2(r[min(t0 + tc, tn - 1)], r[min(t0 + tc + 1, tn - 1)]);
            }
        }
    };
    auto stage_op = [&](auto turned, double *buf, int pitch, int td, int f, const double2 p) {
        if constexpr (decltype(turned)::value) {
            const int tt = f / (KC / 2), kk = 2 * (f % (KC / 2));
            buf[(kk + 0) * pitch + tt] = p.x;
            buf[(kk + 1) * pitch + tt] = p.y;
        } else {
            const int kk = f / (td / 2), tc = 2 * (f % (td / 2));
            *reinterpret_cast<double2 *>(&buf[kk * pitch + tc]) = p;
        }
    };
    constexpr std::integral_constant<bool, XTURN> xturn{};
    constexpr std::integral_constant<bool, YTURN> yturn{};

    double2 px[NX], py[NY];   // the chunk in flight
    auto load = [&](int k0) {
#pragma unroll
        for (int q = 0; q < NX; q++) px[q] = load_op(xturn, g.A, g.sa, x0, g.M, TX, k0, tid + 256 * q);
#pragma unroll
        for (int q = 0; q < NY; q++) py[q] = load_op(yturn, g.B, g.sb, y0, g.N, TY, k0, tid + 256 * q);
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int q = 0; q < NX; q++) stage_op(xturn, sX[buf], XP, TX, tid + 256 * q, px[q]);
#pragma unroll
        for (int q = 0; q < NY; q++) stage_op(yturn, sY[buf], YP, TY, tid + 256 * q, py[q]);
    };

    double acc[2 * RX][2 * RY];   // [x index 2 r + e][y index 2 s + e]
#pragma unroll
    for (int a = 0; a < 2 * RX; a++)
#pragma unroll
        for (int b = 0; b < 2 * RY; b++) acc[a][b] = 0.0;

    // one k step: every output's chain takes its next product, k strictly upward
    auto step = [&](const double *bx, const double *by, int kk) {
        double2 xv[RX], yv[RY];
#pragma unroll
        for (int r = 0; r < RX; r++) xv[r] = *reinterpret_cast<const double2 *>(bx + kk * XP + 32 * r);
#pragma unroll
        for (int s = 0; s < RY; s++) yv[s] = *reinterpret_cast<const double2 *>(by + kk * YP + 32 * s);
#pragma unroll
        for (int r = 0; r < RX; r++)
#pragma unroll
            for (int s = 0; s < RY; s++) {
                acc[2 * r][2 * s] = dev::mad(xv[r].x, yv[s].x, acc[2 * r][2 * s]);
                acc[2 * r + 1][2 * s] = dev::mad(xv[r].y, yv[s].x, acc[2 * r + 1][2 * s]);
                acc[2 * r][2 * s + 1] = dev::mad(xv[r].x, yv[s].y, acc[2 * r][2 * s + 1]);
                acc[2 * r + 1][2 * s + 1] = dev::mad(xv[r].y, yv[s].y, acc[2 * r + 1][2 * s + 1]);
            }
    };
    auto compute = [&](int c) {
        const double *bx = sX[c & 1] + 2 * tx, *by = sY[c & 1] + 2 * ty;
        if (FAST) {
#pragma unroll
            for (int kk = 0; kk < KC; kk++) step(bx, by, kk);
        } else {
            const int kc = min(KC, K - c * KC);   // the K edge is a loop bound: no zero-padded step
            if (kc == KC) {
#pragma unroll
                for (int kk = 0; kk < KC; kk++) step(bx, by, kk);
            } else {
#pragma unroll 1
                for (int kk = 0; kk < kc; kk++) step(bx, by, kk);
            }
        }
    };

    // Chunk c is computed from LDS buffer c & 1 while the loads of chunk c + 1 are in flight; after the fmas chunk c + 1 goes to the
    // other buffer, last read in iteration c - 1 behind that iteration's barrier.
    const int nchunk = (K + KC - 1) / KC;
    load(0);
    stage(0);
    __syncthreads();
#pragma unroll 1
    for (int c = 0; c + 1 < nchunk; c++) {
        load((c + 1) * KC);
        compute(c);
        stage((c + 1) & 1);
        __syncthreads();
    }

    // ---- the last chunk, with the C loads of the epilogue in flight under it.  What lies past the matrix is read from its last row /
    // column and not stored.
    double2 cv[RX][2 * RY];
#pragma unroll
    for (int r = 0; r < RX; r++)
#pragma unroll
        for (int b = 0; b < 2 * RY; b++) {
            const int x = x0 + 2 * tx + 32 * r, y = y0 + 2 * ty + 32 * (b >> 1) + (b & 1);
            if constexpr (FAST) {
                cv[r][b] = *reinterpret_cast<const double2 *>(g.C + (long)y * g.sc + x);
            } else {
                const double *row = g.C + (long)min(y, g.N - 1) * g.sc;
                cv[r][b] = make_double2(row[min(x, g.M - 1)], row[min(x + 1, g.M - 1)]);
            }
        }
    compute(nchunk - 1);

    // ---- epilogue: result(x, y) = mad2(a, ab, b, C(x, y))
#pragma unroll
    for (int r = 0; r < RX; r++)
#pragma unroll
        for (int b = 0; b < 2 * RY; b++) {
            const int x = x0 + 2 * tx + 32 * r, y = y0 + 2 * ty + 32 * (b >> 1) + (b & 1);
            const double v0 = dev::mad2(g.a, acc[2 * r][b], g.b, cv[r][b].x), v1 = dev::mad2(g.a, acc[2 * r + 1][b], g.b, cv[r][b].y);
            if constexpr (FAST) {
                *reinterpret_cast<double2 *>(g.out + (long)y * g.so + x) = make_double2(v0, v1);
            } else if (y < g.N) {
                if (x < g.M) g.out[(long)y * g.so + x] = v0;
                if (x + 1 < g.M) g.out[(long)y * g.so + x + 1] = v1;
            }
        }
}

// The second implementation: one thread per output, the chain as written.
template<bool TA, bool TB>
__global__ __launch_bounds__(256) void dgemm_general(GGeom g) {
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= g.M) return;
    const double *pa = TA ? g.A + (long)i * g.sa : g.A + i;
    const double *pb = TB ? g.B + j : g.B + (long)j * g.sb;
    const long da = TA ? 1 : g.sa, db = TB ? g.sb : 1;
    double ab = 0.0;
    for (int k = 0; k < g.K; k++) ab = dev::mad(pa[k * da], pb[k * db], ab);
    g.out[(long)j * g.so + i] = dev::mad2(g.a, ab, g.b, g.C[(long)j * g.sc + i]);
}

// ---------------------------------------------------------------------------------------------------------------- host: tables
// no estimates: the generators declare none
const ArgTable dcopy_table("halide_dcopy_impl", {scalar_f64("a"), in_buf("x", T_F64, 1), in_buf("y", T_F64, 1), out_buf("result", T_F64, 1)});
const ArgTable dscal_table("halide_dscal_impl", {scalar_f64("a"), in_buf("x", T_F64, 1), in_buf("y", T_F64, 1), out_buf("result", T_F64, 1)});
const ArgTable daxpy_table("halide_daxpy_impl", {scalar_f64("a"), in_buf("x", T_F64, 1), in_buf("y", T_F64, 1), out_buf("result", T_F64, 1)});
const ArgTable ddot_table("halide_ddot", {in_buf("x", T_F64, 1), in_buf("y", T_F64, 1), out_buf("result", T_F64, 0)});
const ArgTable dasum_table("halide_dasum", {in_buf("x", T_F64, 1), out_buf("result", T_F64, 0)});
const ArgTable dgemv_n_table("halide_dgemv_notrans", {scalar_f64("a"), in_buf("A", T_F64, 2), in_buf("x", T_F64, 1), scalar_f64("b"),
                                                      in_buf("y", T_F64, 1), out_buf("output", T_F64, 1)});
const ArgTable dgemv_t_table("halide_dgemv_trans", {scalar_f64("a"), in_buf("A", T_F64, 2), in_buf("x", T_F64, 1), scalar_f64("b"),
                                                    in_buf("y", T_F64, 1), out_buf("output", T_F64, 1)});
const ArgTable dger_table("halide_dger_impl", {scalar_f64("a"), in_buf("x", T_F64, 1), in_buf("y", T_F64, 1), out_buf("result", T_F64, 2)});
#define HLMI_DGEMM_ARGS {scalar_f64("a_"), in_buf("A_", T_F64, 2), in_buf("B_", T_F64, 2), scalar_f64("b_"), in_buf("C_", T_F64, 2), out_buf("result", T_F64, 2)}
const ArgTable dgemm_tables[4] = {{"halide_dgemm_notrans", HLMI_DGEMM_ARGS}, {"halide_dgemm_transA", HLMI_DGEMM_ARGS},
                                  {"halide_dgemm_transB", HLMI_DGEMM_ARGS}, {"halide_dgemm_transAB", HLMI_DGEMM_ARGS}};   // index: tA + 2 * tB

// ---------------------------------------------------------------------------------------------------------------- host: dcopy, dscal, daxpy, dger
enum ElemLaunch { EL_VEC2, EL_SCALAR, EL_GENERAL };
const char *const elem_names[4][3] = {{"dcopy_vec2", "dcopy_scalar", "dcopy_general"},
                                      {"dscal_vec2", "dscal_scalar", "dscal_general"},
                                      {"daxpy_vec2", "daxpy_scalar", "daxpy_general"},
                                      {"dger_vec2", "dger_scalar", "dger_general"}};

// THE predicate of the four elementwise pipelines: 16-byte accesses where every address a lane forms is a multiple of 16 bytes — x, the
// result, daxpy's y and, for dger, the result's column stride — and one element per thread otherwise.
ElemLaunch elem_plan(int mode, const EGeom &g, bool general_only) {
    if (general_only) return EL_GENERAL;
    const bool vec = aligned16(g.x) && aligned16(g.r) && (mode != E_AXPY || aligned16(g.y)) && (mode != E_GER || g.ldr % 2 == 0);
    return vec ? EL_VEC2 : EL_SCALAR;
}

template<int MODE>
int elem_launch_mode(void *uc, hipStream_t st, const EGeom &g, ElemLaunch l) {
    const char *name = elem_names[MODE][l];
    const double elems = (double)g.n * g.rows;
    timing_note_bytes(MODE == E_COPY || MODE == E_SCAL ? 16.0 * elems : MODE == E_AXPY ? 24.0 * elems : 16.0 * elems + 8.0 * (g.n + g.rows));
    const long per_block = l == EL_VEC2 ? ELEM_BLOCK : 256;
    const dim3 grid((unsigned)((g.n + per_block - 1) / per_block), (unsigned)g.rows);
    if (l == EL_VEC2) HLMI_LAUNCH(uc, name, st, (ld_elem<MODE, true>), grid, dim3(256), 0, g);
    else HLMI_LAUNCH(uc, name, st, (ld_elem<MODE, false>), grid, dim3(256), 0, g);
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

// dcopy / dscal / daxpy.  y is looked at by daxpy only: the reference's wrappers pass a null pointer for it to the other two.
int vec_entry(int mode, double a, halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result, bool general_only) {
    void *uc = nullptr;
    const ArgTable &table = mode == E_COPY ? dcopy_table : mode == E_SCAL ? dscal_table : daxpy_table;
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
    // the wrappers' calls: dscal's result is x, daxpy's result is y
    if (overlap(result, x, mode == E_SCAL)) return report(uc, halide_error_code_constraint_violated, "Constraint violated: result may not overlap x");
    if (mode == E_AXPY && overlap(result, y, true))
        return report(uc, halide_error_code_constraint_violated, "Constraint violated: result may overlap y only where it is y");
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, n))) return r;
    const EGeom g = {dev_ptr<double>(x), mode == E_AXPY ? dev_ptr<double>(y) : nullptr, dev_ptr<double>(result), size, 0, 1, a};
    if ((r = elem_launch(uc, ctx.stream, mode, g, elem_plan(mode, g, general_only)))) return r;
    mark_output_written(result);
    return 0;
}

// dger: the result is read and written in place
int ger_entry(double a, halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result, bool general_only) {
    void *uc = nullptr;
    BufArg args[3];
    dger_table.bufs(args, {x, y, result});
    int r = prologue(uc, args, 3);
    if (r < 0) return r;
    const int m = derive({{x, 0}, {result, 0}}), n = derive({{y, 0}, {result, 1}});
    if (r == 1) {
        answer1(x, m), answer1(y, n), answer2(result, m, n);
        return 0;
    }
    if ((r = limit(uc, "halide_dger_impl", "x.extent.0", m, MAX_EXTENT)) || (r = limit(uc, "halide_dger_impl", "y.extent.0", n, MAX_EXTENT))) return r;
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
    const EGeom g = {dev_ptr<double>(x), dev_ptr<double>(y), dev_ptr<double>(result), m, result->dim[1].stride, n, a};
    if ((r = elem_launch(uc, ctx.stream, E_GER, g, elem_plan(E_GER, g, general_only)))) return r;
    mark_output_written(result);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- host: ddot, dasum
int red_entry(bool asum, halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result, bool general_only) {
    void *uc = nullptr;
    BufArg args[3];
    int n = 0;
    if (asum) {
        BufArg two[2];
        dasum_table.bufs(two, {x, result});
        args[0] = two[0], args[1] = two[1], n = 2;
    } else {
        ddot_table.bufs(args, {x, y, result});
        n = 3;
    }
    const char *entry = asum ? "halide_dasum" : "halide_ddot";
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
    double *out = dev_ptr<double>(result);
    if (size == 0) {
        HLMI_HIP(uc, hipMemsetAsync(out, 0, 8, ctx.stream));   // a zero extent launches nothing: +0, all eight bytes of it
    } else {
        const double *px = dev_ptr<double>(x), *py = asum ? nullptr : dev_ptr<double>(y);
        timing_note_bytes((asum ? 8.0 : 16.0) * size + 8.0);
        // THE predicate: the staged wave everywhere; one thread only where the caller asks for it by name
        const char *name = asum ? (general_only ? "dasum_general" : "dasum_wave") : (general_only ? "ddot_general" : "ddot_wave");
        const long ln = size;
        if (asum && general_only) HLMI_LAUNCH(uc, name, ctx.stream, ld_reduce_general<true>, dim3(1), dim3(64), 0, px, py, out, ln);
        else if (asum) HLMI_LAUNCH(uc, name, ctx.stream, ld_reduce<true>, dim3(1), dim3(64), 0, px, py, out, ln);
        else if (general_only) HLMI_LAUNCH(uc, name, ctx.stream, ld_reduce_general<false>, dim3(1), dim3(64), 0, px, py, out, ln);
        else HLMI_LAUNCH(uc, name, ctx.stream, ld_reduce<false>, dim3(1), dim3(64), 0, px, py, out, ln);
    }
    mark_output_written(result);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- host: dgemv
// A is w x h as stored.  notrans: x[h], y[w], output[w].  trans: x[w], y[h], output[h].
int gemv_entry(bool trans, double a, halide_buffer_t *A, halide_buffer_t *x, double b, halide_buffer_t *y, halide_buffer_t *output, bool general_only) {
    void *uc = nullptr;
    BufArg args[4];
    (trans ? dgemv_t_table : dgemv_n_table).bufs(args, {A, x, y, output});
    const char *entry = trans ? "halide_dgemv_trans" : "halide_dgemv_notrans";
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
        const VGeom g = {dev_ptr<double>(A), dev_ptr<double>(x), dev_ptr<double>(y), dev_ptr<double>(output), w, h, A->dim[1].stride, a, b};
        timing_note_bytes(8.0 * ((double)w * h + nx + 2.0 * ny));
        // THE predicate: the wave kernels everywhere; one thread per output only where the caller asks for it by name
        hipStream_t st = ctx.stream;
        if (!trans && !general_only) HLMI_LAUNCH(uc, "dgemv_notrans_wave", st, ld_gemv_n, dim3((unsigned)((w + GEMV_WG - 1) / GEMV_WG)), dim3(GEMV_WG), 0, g);
        else if (!trans) HLMI_LAUNCH(uc, "dgemv_notrans_general", st, ld_gemv_n_general, dim3((unsigned)((w + 255) / 256)), dim3(256), 0, g);
        else if (!general_only) HLMI_LAUNCH(uc, "dgemv_trans_wave", st, ld_gemv_t, dim3((unsigned)((h + GEMV_WG / V - 1) / (GEMV_WG / V))), dim3(GEMV_WG), 0, g);
        else HLMI_LAUNCH(uc, "dgemv_trans_general", st, ld_gemv_t_general, dim3((unsigned)((h + 255) / 256)), dim3(256), 0, g);
    }
    mark_output_written(output);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- host: dgemm
enum GemmLaunch { GM_TILE, GM_TILE_EDGE, GM_GENERAL };
const char *const gemm_names[3] = {"dgemm_tile", "dgemm_tile_edge", "dgemm_general"};

struct GemmPlan {
    GemmLaunch launch;
    int tile;   // workgroup tile extent along i of the two tiled launches; along j it is TILE_N
};

// the large tile (half the B reads per fma) only where it still leaves a workgroup for every CU
constexpr int gemm_tile(int M, int N) {
    return ((M + LARGE_TILE - 1) / LARGE_TILE) * ((N + TILE_N - 1) / TILE_N) >= LARGE_FROM_WGS ? LARGE_TILE : SMALL_TILE;
}

// THE predicate.  The register-tiled kernel steps dev::mad, so it is the contract's chain in both canonical forms; it needs one step at
// least.  The aligned kernel takes a call whose M is a multiple of its tile, whose N is one of TILE_N and whose K is one of KC, with all
// four buffers on 16 bytes and column strides a multiple of 16 bytes; the edge variant takes every other call; the general kernel runs
// where the caller asks for it by name and for K == 0.
GemmPlan gemm_plan(const GGeom &g, bool general_only) {
    const int tile = gemm_tile(g.M, g.N);
    if (general_only || g.K == 0) return {GM_GENERAL, tile};
    const bool fast = g.M % tile == 0 && g.N % TILE_N == 0 && g.K % KC == 0 && aligned16(g.A, g.sa, 2) && aligned16(g.B, g.sb, 2) && aligned16(g.C, g.sc, 2) &&
                      aligned16(g.out, g.so, 2);
    return {fast ? GM_TILE : GM_TILE_EDGE, tile};
}

int gemm_launch(void *uc, hipStream_t st, bool tA, bool tB, const GGeom &g, const GemmPlan &p) {
    timing_note_bytes(8.0 * ((double)g.M * g.K + (double)g.K * g.N + 2.0 * g.M * g.N));   // each matrix read or written once
    const char *name = gemm_names[p.launch];
    if (p.launch == GM_GENERAL) {
        const dim3 grid((unsigned)((g.M + 255) / 256), (unsigned)g.N);
        return with_flags([&](auto ta, auto tb) {
            HLMI_LAUNCH(uc, name, st, (dgemm_general<ta.value, tb.value>), grid, dim3(256), 0, g);
            return 0;
        }, tA, tB);
    }
    const dim3 grid((unsigned)((g.M + p.tile - 1) / p.tile), (unsigned)((g.N + TILE_N - 1) / TILE_N));
    return with_flags([&](auto large, auto fast, auto ta, auto tb) {
        HLMI_LAUNCH(uc, name, st, (dgemm_tile<large.value ? LARGE_TILE / 16 : SMALL_TILE / 16, fast.value, ta.value, tb.value>), grid, dim3(256), 0, g);
        return 0;
    }, p.tile == LARGE_TILE, p.launch == GM_TILE, tA, tB);
}

// The shapes (blas_l3_generators.cpp:37-53, :167-171): num_rows = A_.width(), num_cols = B_.height() and sum_size = A_.height() are
// taken from the STORED A and B whatever the flags, B_.extent.0 is pinned to sum_size, C_ and result to num_rows x num_cols; a
// transposed operand is read inside its matrix only where that matrix is square (linear_algebra.hip has the derivation).
int gemm_entry(bool tA, bool tB, double a, halide_buffer_t *A, halide_buffer_t *B, double b, halide_buffer_t *C, halide_buffer_t *result, bool general_only) {
    void *uc = nullptr;
    const ArgTable &table = dgemm_tables[(tA ? 1 : 0) + (tB ? 2 : 0)];
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
        const GGeom g = {dev_ptr<double>(A), dev_ptr<double>(B), dev_ptr<double>(C), dev_ptr<double>(result), M, N, K,
                         A->dim[1].stride, B->dim[1].stride, C->dim[1].stride, result->dim[1].stride, a, b};
        if ((r = gemm_launch(uc, ctx.stream, tA, tB, g, gemm_plan(g, general_only)))) return r;
    }
    mark_output_written(result);
    return 0;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------- entry points
extern "C" int halide_dcopy_impl(double a, halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result) { return vec_entry(E_COPY, a, x, y, result, false); }
HLMI_ENTRY(halide_dcopy_impl, dcopy_table.md)
extern "C" int halide_dscal_impl(double a, halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result) { return vec_entry(E_SCAL, a, x, y, result, false); }
HLMI_ENTRY(halide_dscal_impl, dscal_table.md)
extern "C" int halide_daxpy_impl(double a, halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result) { return vec_entry(E_AXPY, a, x, y, result, false); }
HLMI_ENTRY(halide_daxpy_impl, daxpy_table.md)
extern "C" int halide_ddot(halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result) { return red_entry(false, x, y, result, false); }
HLMI_ENTRY(halide_ddot, ddot_table.md)
extern "C" int halide_dasum(halide_buffer_t *x, halide_buffer_t *result) { return red_entry(true, x, nullptr, result, false); }
HLMI_ENTRY(halide_dasum, dasum_table.md)
extern "C" int halide_dgemv_notrans(double a, halide_buffer_t *A, halide_buffer_t *x, double b, halide_buffer_t *y, halide_buffer_t *output) {
    return gemv_entry(false, a, A, x, b, y, output, false);
}
HLMI_ENTRY(halide_dgemv_notrans, dgemv_n_table.md)
extern "C" int halide_dgemv_trans(double a, halide_buffer_t *A, halide_buffer_t *x, double b, halide_buffer_t *y, halide_buffer_t *output) {
    return gemv_entry(true, a, A, x, b, y, output, false);
}
HLMI_ENTRY(halide_dgemv_trans, dgemv_t_table.md)
extern "C" int halide_dger_impl(double a, halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result) { return ger_entry(a, x, y, result, false); }
HLMI_ENTRY(halide_dger_impl, dger_table.md)
extern "C" int halide_dgemm_notrans(double a, halide_buffer_t *A, halide_buffer_t *B, double b, halide_buffer_t *C, halide_buffer_t *result) {
    return gemm_entry(false, false, a, A, B, b, C, result, false);
}
HLMI_ENTRY(halide_dgemm_notrans, dgemm_tables[0].md)
extern "C" int halide_dgemm_transA(double a, halide_buffer_t *A, halide_buffer_t *B, double b, halide_buffer_t *C, halide_buffer_t *result) {
    return gemm_entry(true, false, a, A, B, b, C, result, false);
}
HLMI_ENTRY(halide_dgemm_transA, dgemm_tables[1].md)
extern "C" int halide_dgemm_transB(double a, halide_buffer_t *A, halide_buffer_t *B, double b, halide_buffer_t *C, halide_buffer_t *result) {
    return gemm_entry(false, true, a, A, B, b, C, result, false);
}
HLMI_ENTRY(halide_dgemm_transB, dgemm_tables[2].md)
extern "C" int halide_dgemm_transAB(double a, halide_buffer_t *A, halide_buffer_t *B, double b, halide_buffer_t *C, halide_buffer_t *result) {
    return gemm_entry(true, true, a, A, B, b, C, result, false);
}
HLMI_ENTRY(halide_dgemm_transAB, dgemm_tables[3].md)

// Measurement and test hook (hlmi_internal.h): the named entry point with one thread per output.  p0 .. p3 are the entry point's
// buffers in its own order (the unused trailing ones null); a and b are read where the entry point has them.
extern "C" int hlmi_linear_algebra_general_f64(const char *name, double a, double b, halide_buffer_t *p0, halide_buffer_t *p1, halide_buffer_t *p2,
                                               halide_buffer_t *p3) {
    const char *n = name ? name : "(null)";
    if (!strcmp(n, "halide_dcopy_impl")) return vec_entry(E_COPY, a, p0, p1, p2, true);
    if (!strcmp(n, "halide_dscal_impl")) return vec_entry(E_SCAL, a, p0, p1, p2, true);
    if (!strcmp(n, "halide_daxpy_impl")) return vec_entry(E_AXPY, a, p0, p1, p2, true);
    if (!strcmp(n, "halide_ddot")) return red_entry(false, p0, p1, p2, true);
    if (!strcmp(n, "halide_dasum")) return red_entry(true, p0, nullptr, p1, true);
    if (!strcmp(n, "halide_dgemv_notrans")) return gemv_entry(false, a, p0, p1, b, p2, p3, true);
    if (!strcmp(n, "halide_dgemv_trans")) return gemv_entry(true, a, p0, p1, b, p2, p3, true);
    if (!strcmp(n, "halide_dger_impl")) return ger_entry(a, p0, p1, p2, true);
    if (!strcmp(n, "halide_dgemm_notrans")) return gemm_entry(false, false, a, p0, p1, b, p2, p3, true);
    if (!strcmp(n, "halide_dgemm_transA")) return gemm_entry(true, false, a, p0, p1, b, p2, p3, true);
    if (!strcmp(n, "halide_dgemm_transB")) return gemm_entry(false, true, a, p0, p1, b, p2, p3, true);
    if (!strcmp(n, "halide_dgemm_transAB")) return gemm_entry(true, true, a, p0, p1, b, p2, p3, true);
    return report(nullptr, halide_error_code_constraint_violated, "hlmi_linear_algebra_general_f64: no entry point named %s", n);
}

// ---------------------------------------------------------------------------------------------------------------- hblas_d*
// include/hlmi_blas.h states the interface and where it departs from the reference's.  Each call wraps the caller's host arrays in
// buffers, runs the entry point, brings the result home and lets go of the device side.
namespace {

struct HostVec {
    halide_dimension_t dim[2];
    halide_buffer_t buf;
    HostVec(const double *p, int w, int h = -1, int ld = 0) {
        dim[0] = {0, w, 1, 0};
        dim[1] = {0, h, ld, 0};
        memset(&buf, 0, sizeof buf);
        buf.host = (uint8_t *)const_cast<double *>(p);
        buf.flags = halide_buffer_flag_host_dirty;
        buf.type.code = halide_type_float, buf.type.bits = 64;
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

extern "C" void hblas_dcopy(const int N, const double *X, const int incX, double *Y, const int incY) {
    if (bad_inc("hblas_dcopy", incX, incY)) return;
    HostVec x(X, N), y(Y, N);
    finish("hblas_dcopy", halide_dcopy(&x.buf, &y.buf), &y.buf);
}

extern "C" void hblas_dscal(const int N, const double alpha, double *X, const int incX) {
    if (bad_inc("hblas_dscal", incX)) return;
    HostVec x(X, N);
    finish("hblas_dscal", halide_dscal(alpha, &x.buf), &x.buf);
}

extern "C" void hblas_daxpy(const int N, const double alpha, const double *X, const int incX, double *Y, const int incY) {
    if (bad_inc("hblas_daxpy", incX, incY)) return;
    HostVec x(X, N), y(Y, N);
    finish("hblas_daxpy", halide_daxpy(alpha, &x.buf, &y.buf), &y.buf);
}

extern "C" double hblas_ddot(const int N, const double *X, const int incX, const double *Y, const int incY) {
    if (bad_inc("hblas_ddot", incX, incY)) return NAN;
    double result = NAN;
    HostVec x(X, N), y(Y, N), r(&result, 0);
    r.buf.dimensions = 0;
    return finish("hblas_ddot", halide_ddot(&x.buf, &y.buf, &r.buf), &r.buf) == 0 ? result : NAN;
}

extern "C" double hblas_dnrm2(const int N, const double *X, const int incX) {
    if (bad_inc("hblas_dnrm2", incX)) return NAN;
    double result = NAN;
    HostVec x(X, N), r(&result, 0);
    r.buf.dimensions = 0;
    return finish("hblas_dnrm2", halide_ddot(&x.buf, &x.buf, &r.buf), &r.buf) == 0 ? sqrt(result) : NAN;
}

extern "C" double hblas_dasum(const int N, const double *X, const int incX) {
    if (bad_inc("hblas_dasum", incX)) return NAN;
    double result = NAN;
    HostVec x(X, N), r(&result, 0);
    r.buf.dimensions = 0;
    return finish("hblas_dasum", halide_dasum(&x.buf, &r.buf), &r.buf) == 0 ? result : NAN;
}

extern "C" void hblas_dgemv(const enum HBLAS_ORDER order, const enum HBLAS_TRANSPOSE TransA, const int M, const int N, const double alpha, const double *A,
                            const int lda, const double *X, const int incX, const double beta, double *Y, const int incY) {
    if (bad_order("hblas_dgemv", order) || bad_inc("hblas_dgemv", incX, incY)) return;
    const bool t = TransA != HblasNoTrans;
    HostVec a(A, M, N, lda), x(X, t ? M : N), y(Y, t ? N : M);
    finish("hblas_dgemv", halide_dgemv(t, alpha, &a.buf, &x.buf, beta, &y.buf), &y.buf);
}

extern "C" void hblas_dger(const enum HBLAS_ORDER order, const int M, const int N, const double alpha, const double *X, const int incX, const double *Y,
                           const int incY, double *A, const int lda) {
    if (bad_order("hblas_dger", order) || bad_inc("hblas_dger", incX, incY)) return;
    HostVec x(X, M), y(Y, N), a(A, M, N, lda);
    finish("hblas_dger", halide_dger(alpha, &x.buf, &y.buf, &a.buf), &a.buf);
}

extern "C" void hblas_dgemm(const enum HBLAS_ORDER Order, const enum HBLAS_TRANSPOSE TransA, const enum HBLAS_TRANSPOSE TransB, const int M, const int N,
                            const int K, const double alpha, const double *A, const int lda, const double *B, const int ldb, const double beta, double *C,
                            const int ldc) {
    if (bad_order("hblas_dgemm", Order)) return;
    const bool tA = TransA != HblasNoTrans, tB = TransB != HblasNoTrans;
    // the generator's shapes (hlmi_pipelines.h): a transposed operand is square
    if (((tA && M != K) || (tB && N != K)) && hblas_refuse("hblas_dgemm", "a transposed operand must be square (M == K for TransA, N == K for TransB)")) return;
    HostVec a(A, tA ? K : M, tA ? M : K, lda), b(B, tB ? N : K, tB ? K : N, ldb), c(C, M, N, ldc);
    finish("hblas_dgemm", halide_dgemm(tA, tB, alpha, &a.buf, &b.buf, beta, &c.buf), &c.buf);
}
