// linear_algebra_f64.hip — gfx950 implementation of the twelve f64 AOT pipelines of apps/linear_algebra (the `halide_d*` objects behind
// halide_blas.h) and of the CBLAS-shaped hblas_d* calls over them (include/hlmi_blas.h): linear_algebra_core.h at T = double.
//
// Algorithms: apps/linear_algebra/src/blas_l1_generators.cpp, blas_l2_generators.cpp, blas_l3_generators.cpp.  The contract, the checks,
// the entry points' bodies and every kernel but the one below are in linear_algebra_core.h.  What differs from
// the f32 half: elements are 8 bytes, the scalars a and b are doubles, and a vectorised reduction keeps V = 4 lane sums —
// natural_vector_size(double) of the reference's x86-64 AVX2 build.  This file holds the named constants, the extern "C" surface and
//   dgemm (four variants)          dgemm_tile<TM, FAST, TA, TB>: 256 threads as 16 x 16, each with a TM x 4 register block of outputs
//                                  stepped by v_fma_f64 (or v_mul_f64 + v_add_f64) strictly upward in k: the contract's chain by
//                                  construction, in BOTH canonical forms.  Both operands are staged k-major in LDS — an operand
//                                  contiguous along its tile dimension is copied straight in with 16-byte stores, one contiguous
//                                  along k is turned on the way in (pitch + 2) — double-buffered, the next chunk's global loads in
//                                  flight under this chunk's fmas.  One 16-byte LDS read per two A values and per two B values.  No
//                                  zero-padded k step: the K edge is a loop bound.  The C loads of the mad2 epilogue are issued
//                                  under the last chunk.  The f64 MFMA is not used (an open question).
#include "linear_algebra_core.h"

using namespace hlmi;
using namespace hlmi::la_host;

namespace {

constexpr int V = 4;                     // natural_vector_size(double) of the reference's x86-64 AVX2 target
constexpr int MAX_VECTOR = 134217728;    // vector lengths 0 .. 2^27
constexpr int MAX_EXTENT = 8192;         // matrix extents 0 .. 8192
constexpr int ELEM_BLOCK = 1024;         // elements a 256-thread workgroup of la_elem<., ., true> moves: two double2 per lane
constexpr int RED_BLOCK = 128;           // elements of each operand la_reduce stages per step of its pipeline: 32 chain steps
constexpr int RED_PITCH = 40;            // doubles between the chain lanes' rows in LDS: rows 16-byte aligned, 16 banks apart
constexpr int GEMV_WG = 64;              // threads of a gemv workgroup: one wave
constexpr int GEMV_U = 8;                // k steps per unrolled group of the two gemv kernels
constexpr int TILE_N = 64;               // dgemm workgroup tile along j: 16 threads x 4 outputs
constexpr int SMALL_TILE = 64;           // dgemm workgroup tile along i with 4 x 4 outputs per thread
constexpr int LARGE_TILE = 128;          // dgemm workgroup tile along i with 8 x 4 outputs per thread
constexpr int LARGE_FROM_WGS = 256;      // the large tile where it still leaves a workgroup for every CU
constexpr int KC = 16;                   // k steps per staged chunk

using GGeom = la::GGeom<double>;

// the configuration of linear_algebra_core.h
struct F64 {
    using T = double;
    static constexpr int V = ::V, MAX_VECTOR = ::MAX_VECTOR, MAX_EXTENT = ::MAX_EXTENT, ELEM_ACCESSES = ELEM_BLOCK / (256 * 2), RED_BLOCK = ::RED_BLOCK,
                         RED_PITCH = ::RED_PITCH, GEMV_WG = ::GEMV_WG, GEMV_U = ::GEMV_U;
    static constexpr uint32_t TYPE = T_F64;
    static constexpr auto scalar = scalar_f64;
    static constexpr la::Names NAMES = HLMI_LA_NAMES("d", "vec2");
    static int gemm(void *uc, hipStream_t st, bool tA, bool tB, const GGeom &g, bool general_only);
};
const auto &tables = la::tables<F64>;

// ---------------------------------------------------------------------------------------------------------------- dgemm
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
            HLMI_LAUNCH(uc, name, st, (la::la_gemm_general<double, ta.value, tb.value>), grid, dim3(256), 0, g);
            return 0;
        }, tA, tB);
    }
    const dim3 grid((unsigned)((g.M + p.tile - 1) / p.tile), (unsigned)((g.N + TILE_N - 1) / TILE_N));
    return with_flags([&](auto large, auto fast, auto ta, auto tb) {
        HLMI_LAUNCH(uc, name, st, (dgemm_tile<large.value ? LARGE_TILE / 16 : SMALL_TILE / 16, fast.value, ta.value, tb.value>), grid, dim3(256), 0, g);
        return 0;
    }, p.tile == LARGE_TILE, p.launch == GM_TILE, tA, tB);
}

int F64::gemm(void *uc, hipStream_t st, bool tA, bool tB, const GGeom &g, bool general_only) { return gemm_launch(uc, st, tA, tB, g, gemm_plan(g, general_only)); }

}  // namespace

// ---------------------------------------------------------------------------------------------------------------- entry points
extern "C" int halide_dcopy_impl(double a, halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result) {
    return la::vec_entry<F64>(la::E_COPY, a, x, y, result, false);
}
HLMI_ENTRY(halide_dcopy_impl, tables[la::N_COPY].md)
extern "C" int halide_dscal_impl(double a, halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result) {
    return la::vec_entry<F64>(la::E_SCAL, a, x, y, result, false);
}
HLMI_ENTRY(halide_dscal_impl, tables[la::N_SCAL].md)
extern "C" int halide_daxpy_impl(double a, halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result) {
    return la::vec_entry<F64>(la::E_AXPY, a, x, y, result, false);
}
HLMI_ENTRY(halide_daxpy_impl, tables[la::N_AXPY].md)
extern "C" int halide_ddot(halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result) { return la::red_entry<F64>(false, x, y, result, false); }
HLMI_ENTRY(halide_ddot, tables[la::N_DOT].md)
extern "C" int halide_dasum(halide_buffer_t *x, halide_buffer_t *result) { return la::red_entry<F64>(true, x, nullptr, result, false); }
HLMI_ENTRY(halide_dasum, tables[la::N_ASUM].md)
extern "C" int halide_dgemv_notrans(double a, halide_buffer_t *A, halide_buffer_t *x, double b, halide_buffer_t *y, halide_buffer_t *output) {
    return la::gemv_entry<F64>(false, a, A, x, b, y, output, false);
}
HLMI_ENTRY(halide_dgemv_notrans, tables[la::N_GEMV_N].md)
extern "C" int halide_dgemv_trans(double a, halide_buffer_t *A, halide_buffer_t *x, double b, halide_buffer_t *y, halide_buffer_t *output) {
    return la::gemv_entry<F64>(true, a, A, x, b, y, output, false);
}
HLMI_ENTRY(halide_dgemv_trans, tables[la::N_GEMV_T].md)
extern "C" int halide_dger_impl(double a, halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result) { return la::ger_entry<F64>(a, x, y, result, false); }
HLMI_ENTRY(halide_dger_impl, tables[la::N_GER].md)
extern "C" int halide_dgemm_notrans(double a, halide_buffer_t *A, halide_buffer_t *B, double b, halide_buffer_t *C, halide_buffer_t *result) {
    return la::gemm_entry<F64>(false, false, a, A, B, b, C, result, false);
}
HLMI_ENTRY(halide_dgemm_notrans, tables[la::N_GEMM + 0].md)
extern "C" int halide_dgemm_transA(double a, halide_buffer_t *A, halide_buffer_t *B, double b, halide_buffer_t *C, halide_buffer_t *result) {
    return la::gemm_entry<F64>(true, false, a, A, B, b, C, result, false);
}
HLMI_ENTRY(halide_dgemm_transA, tables[la::N_GEMM + 1].md)
extern "C" int halide_dgemm_transB(double a, halide_buffer_t *A, halide_buffer_t *B, double b, halide_buffer_t *C, halide_buffer_t *result) {
    return la::gemm_entry<F64>(false, true, a, A, B, b, C, result, false);
}
HLMI_ENTRY(halide_dgemm_transB, tables[la::N_GEMM + 2].md)
extern "C" int halide_dgemm_transAB(double a, halide_buffer_t *A, halide_buffer_t *B, double b, halide_buffer_t *C, halide_buffer_t *result) {
    return la::gemm_entry<F64>(true, true, a, A, B, b, C, result, false);
}
HLMI_ENTRY(halide_dgemm_transAB, tables[la::N_GEMM + 3].md)

// Measurement and test hook (hlmi_internal.h): the named entry point with one thread per output
extern "C" int hlmi_linear_algebra_general_f64(const char *name, double a, double b, halide_buffer_t *p0, halide_buffer_t *p1, halide_buffer_t *p2,
                                               halide_buffer_t *p3) {
    return la::general_entry<F64>("hlmi_linear_algebra_general_f64", name, a, b, p0, p1, p2, p3);
}

// ---------------------------------------------------------------------------------------------------------------- hblas_d*
extern "C" void hblas_dcopy(const int N, const double *X, const int incX, double *Y, const int incY) { la::hblas_copy<F64>("hblas_dcopy", N, X, incX, Y, incY); }

extern "C" void hblas_dscal(const int N, const double alpha, double *X, const int incX) { la::hblas_scal<F64>("hblas_dscal", N, alpha, X, incX); }

extern "C" void hblas_daxpy(const int N, const double alpha, const double *X, const int incX, double *Y, const int incY) {
    la::hblas_axpy<F64>("hblas_daxpy", N, alpha, X, incX, Y, incY);
}

extern "C" double hblas_ddot(const int N, const double *X, const int incX, const double *Y, const int incY) {
    return la::hblas_dot<F64>("hblas_ddot", N, X, incX, Y, incY);
}

extern "C" double hblas_dnrm2(const int N, const double *X, const int incX) { return la::hblas_nrm2<F64>("hblas_dnrm2", N, X, incX); }

extern "C" double hblas_dasum(const int N, const double *X, const int incX) { return la::hblas_asum<F64>("hblas_dasum", N, X, incX); }

extern "C" void hblas_dgemv(const enum HBLAS_ORDER order, const enum HBLAS_TRANSPOSE TransA, const int M, const int N, const double alpha, const double *A,
                            const int lda, const double *X, const int incX, const double beta, double *Y, const int incY) {
    la::hblas_gemv<F64>("hblas_dgemv", order, TransA, M, N, alpha, A, lda, X, incX, beta, Y, incY);
}

extern "C" void hblas_dger(const enum HBLAS_ORDER order, const int M, const int N, const double alpha, const double *X, const int incX, const double *Y,
                           const int incY, double *A, const int lda) {
    la::hblas_ger<F64>("hblas_dger", order, M, N, alpha, X, incX, Y, incY, A, lda);
}

extern "C" void hblas_dgemm(const enum HBLAS_ORDER Order, const enum HBLAS_TRANSPOSE TransA, const enum HBLAS_TRANSPOSE TransB, const int M, const int N,
                            const int K, const double alpha, const double *A, const int lda, const double *B, const int ldb, const double beta, double *C,
                            const int ldc) {
    la::hblas_gemm<F64>("hblas_dgemm", Order, TransA, TransB, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc);
}
