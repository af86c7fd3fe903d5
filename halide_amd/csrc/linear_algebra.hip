// linear_algebra.hip — gfx950 implementation of the twelve f32 AOT pipelines of apps/linear_algebra (the `halide_s*` objects behind
// halide_blas.h) and of the CBLAS-shaped hblas_s* calls over them (include/hlmi_blas.h): linear_algebra_core.h at T = float.
//
// Algorithms: apps/linear_algebra/src/blas_l1_generators.cpp (AXPY :27-70, Dot :90-124, AbsSum :144-176), blas_l2_generators.cpp
// (GEMV :27-196, GER :217-242), blas_l3_generators.cpp (GEMM :25-172); which generator parameters make which entry point:
// src/CMakeLists.txt.  The contract, the checks, the entry points' bodies and every kernel but the one below are in
// linear_algebra_core.h; a vectorised reduction keeps the V = 8 lane sums of the reference's x86-64 AVX2 build.
// This file holds the named constants, the extern "C" surface and
//   sgemm (four variants)          sgemm_mfma<W, FAST, TA, TB>: chain::tile() of f32_chain_gemm.h, the tile loop mat_mul.hip shares,
//                                  for M != N != K.  The variants are the 2 x 2 of "opA is i-contiguous or k-contiguous" x "opB is
//                                  k-contiguous or j-contiguous", which is the tile's "straight or turned" per operand.  transAB
//                                  needs no swap of roles here: the product commutes, and k still runs upward.  The epilogue is
//                                  mad2 on the accumulator registers.  v_mfma_f32_32x32x2_f32 is a chain of fused steps, so these
//                                  kernels exist in the default build only: with HLMI_CANON_FMA=0 (each product rounded before
//                                  the add) the plan always answers the one-thread-per-output kernel.
#include "f32_chain_gemm.h"
#include "linear_algebra_core.h"

using namespace hlmi;
using namespace hlmi::la_host;

namespace {

constexpr int V = 8;                     // natural_vector_size(float) of the reference's x86-64 AVX2 target: a choice
constexpr int MAX_VECTOR = 134217728;    // vector lengths 0 .. 2^27
constexpr int MAX_EXTENT = 8192;         // matrix extents 0 .. 8192
constexpr int ELEM_ACCESSES = 1;         // 16-byte accesses per lane of la_elem<., ., true>: one float4, 1024 elements per workgroup
constexpr int RED_BLOCK = 256;           // elements of each operand la_reduce stages per step of its pipeline: 32 chain steps
constexpr int RED_PITCH = 36;            // floats between the chain lanes' rows in LDS: 32 steps + 4, rows stay 16-byte aligned
constexpr int GEMV_WG = 64;              // threads of a gemv workgroup: one wave
constexpr int GEMV_U = 8;                // k steps per unrolled group of the two gemv kernels
constexpr int SMALL_TILE = 64;           // sgemm workgroup tile with one accumulator per wave
constexpr int LARGE_TILE = 128;          // sgemm workgroup tile with 2 x 2 accumulators per wave
constexpr int LARGE_FROM_WGS = 256;      // the large tile where it still leaves this many workgroups (x 4 waves = 256 CUs x 4 SIMDs)
constexpr int KC = 32;                   // the tile loop's chunk, as gemm_plan() and the tests read it: a K that is no multiple of it has a short last chunk
static_assert(KC == chain::KC, "gemm_plan() plans for the chunk that chain::tile() stages");

using GGeom = la::GGeom<float>;

// the configuration of linear_algebra_core.h
struct F32 {
    using T = float;
    static constexpr int V = ::V, MAX_VECTOR = ::MAX_VECTOR, MAX_EXTENT = ::MAX_EXTENT, ELEM_ACCESSES = ::ELEM_ACCESSES, RED_BLOCK = ::RED_BLOCK,
                         RED_PITCH = ::RED_PITCH, GEMV_WG = ::GEMV_WG, GEMV_U = ::GEMV_U;
    static constexpr uint32_t TYPE = T_F32;
    static constexpr auto scalar = scalar_f32;
    static constexpr la::Names NAMES = HLMI_LA_NAMES("s", "vec4");
    static int gemm(void *uc, hipStream_t st, bool tA, bool tB, const GGeom &g, bool general_only);
};
const auto &tables = la::tables<F32>;

// ---------------------------------------------------------------------------------------------------------------- sgemm
#if HLMI_CANON_FMA
// chain::tile() with x = i (the MFMA's column, contiguous in C and the result), y = j.  Operand X[k][x] = opA(x, k): A[k * sa + x]
// (straight) or, TA, A[x * sa + k] (turned).  Operand Y[k][y] = opB(k, y): B[y * sb + k] (turned) or, TB, B[k * sb + y] (straight).
struct SgemmOps {
    static __device__ __forceinline__ int M(const GGeom &g) { return g.M; }
    static __device__ __forceinline__ int N(const GGeom &g) { return g.N; }
    static __device__ __forceinline__ int K(const GGeom &g) { return g.K; }
    // result(x, y) = mad2(a, ab, b, C(x, y)): C is read where the result is written, in the 128-byte half-wave rows the store uses
    static __device__ __forceinline__ void store(const GGeom &g, int x, int y, float acc) {
        g.out[(long)y * g.so + x] = dev::mad2(g.a, acc, g.b, g.C[(long)y * g.sc + x]);
    }
};

template<int W, bool FAST, bool TA, bool TB>
__global__ __launch_bounds__(256) void sgemm_mfma(GGeom g) {
    chain::tile<W, FAST, TA, !TB, SgemmOps>(g);
}
#endif   // HLMI_CANON_FMA

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
            HLMI_LAUNCH(uc, name, st, (la::la_gemm_general<float, ta.value, tb.value>), grid, dim3(256), 0, g);
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

int F32::gemm(void *uc, hipStream_t st, bool tA, bool tB, const GGeom &g, bool general_only) { return gemm_launch(uc, st, tA, tB, g, gemm_plan(g, general_only)); }

}  // namespace

// ---------------------------------------------------------------------------------------------------------------- entry points
extern "C" int halide_scopy_impl(float a, halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result) {
    return la::vec_entry<F32>(la::E_COPY, a, x, y, result, false);
}
HLMI_ENTRY(halide_scopy_impl, tables[la::N_COPY].md)
extern "C" int halide_sscal_impl(float a, halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result) {
    return la::vec_entry<F32>(la::E_SCAL, a, x, y, result, false);
}
HLMI_ENTRY(halide_sscal_impl, tables[la::N_SCAL].md)
extern "C" int halide_saxpy_impl(float a, halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result) {
    return la::vec_entry<F32>(la::E_AXPY, a, x, y, result, false);
}
HLMI_ENTRY(halide_saxpy_impl, tables[la::N_AXPY].md)
extern "C" int halide_sdot(halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result) { return la::red_entry<F32>(false, x, y, result, false); }
HLMI_ENTRY(halide_sdot, tables[la::N_DOT].md)
extern "C" int halide_sasum(halide_buffer_t *x, halide_buffer_t *result) { return la::red_entry<F32>(true, x, nullptr, result, false); }
HLMI_ENTRY(halide_sasum, tables[la::N_ASUM].md)
extern "C" int halide_sgemv_notrans(float a, halide_buffer_t *A, halide_buffer_t *x, float b, halide_buffer_t *y, halide_buffer_t *output) {
    return la::gemv_entry<F32>(false, a, A, x, b, y, output, false);
}
HLMI_ENTRY(halide_sgemv_notrans, tables[la::N_GEMV_N].md)
extern "C" int halide_sgemv_trans(float a, halide_buffer_t *A, halide_buffer_t *x, float b, halide_buffer_t *y, halide_buffer_t *output) {
    return la::gemv_entry<F32>(true, a, A, x, b, y, output, false);
}
HLMI_ENTRY(halide_sgemv_trans, tables[la::N_GEMV_T].md)
extern "C" int halide_sger_impl(float a, halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result) { return la::ger_entry<F32>(a, x, y, result, false); }
HLMI_ENTRY(halide_sger_impl, tables[la::N_GER].md)
extern "C" int halide_sgemm_notrans(float a, halide_buffer_t *A, halide_buffer_t *B, float b, halide_buffer_t *C, halide_buffer_t *result) {
    return la::gemm_entry<F32>(false, false, a, A, B, b, C, result, false);
}
HLMI_ENTRY(halide_sgemm_notrans, tables[la::N_GEMM + 0].md)
extern "C" int halide_sgemm_transA(float a, halide_buffer_t *A, halide_buffer_t *B, float b, halide_buffer_t *C, halide_buffer_t *result) {
    return la::gemm_entry<F32>(true, false, a, A, B, b, C, result, false);
}
HLMI_ENTRY(halide_sgemm_transA, tables[la::N_GEMM + 1].md)
extern "C" int halide_sgemm_transB(float a, halide_buffer_t *A, halide_buffer_t *B, float b, halide_buffer_t *C, halide_buffer_t *result) {
    return la::gemm_entry<F32>(false, true, a, A, B, b, C, result, false);
}
HLMI_ENTRY(halide_sgemm_transB, tables[la::N_GEMM + 2].md)
extern "C" int halide_sgemm_transAB(float a, halide_buffer_t *A, halide_buffer_t *B, float b, halide_buffer_t *C, halide_buffer_t *result) {
    return la::gemm_entry<F32>(true, true, a, A, B, b, C, result, false);
}
HLMI_ENTRY(halide_sgemm_transAB, tables[la::N_GEMM + 3].md)

// Measurement and test hook (hlmi_internal.h): the named entry point with one thread per output
extern "C" int hlmi_linear_algebra_general(const char *name, float a, float b, halide_buffer_t *p0, halide_buffer_t *p1, halide_buffer_t *p2,
                                           halide_buffer_t *p3) {
    return la::general_entry<F32>("hlmi_linear_algebra_general", name, a, b, p0, p1, p2, p3);
}

// ---------------------------------------------------------------------------------------------------------------- hblas_s*
extern "C" void hblas_scopy(const int N, const float *X, const int incX, float *Y, const int incY) { la::hblas_copy<F32>("hblas_scopy", N, X, incX, Y, incY); }

extern "C" void hblas_sscal(const int N, const float alpha, float *X, const int incX) { la::hblas_scal<F32>("hblas_sscal", N, alpha, X, incX); }

extern "C" void hblas_saxpy(const int N, const float alpha, const float *X, const int incX, float *Y, const int incY) {
    la::hblas_axpy<F32>("hblas_saxpy", N, alpha, X, incX, Y, incY);
}

extern "C" float hblas_sdot(const int N, const float *X, const int incX, const float *Y, const int incY) {
    return la::hblas_dot<F32>("hblas_sdot", N, X, incX, Y, incY);
}

extern "C" float hblas_snrm2(const int N, const float *X, const int incX) { return la::hblas_nrm2<F32>("hblas_snrm2", N, X, incX); }

extern "C" float hblas_sasum(const int N, const float *X, const int incX) { return la::hblas_asum<F32>("hblas_sasum", N, X, incX); }

extern "C" void hblas_sgemv(const enum HBLAS_ORDER order, const enum HBLAS_TRANSPOSE TransA, const int M, const int N, const float alpha, const float *A,
                            const int lda, const float *X, const int incX, const float beta, float *Y, const int incY) {
    la::hblas_gemv<F32>("hblas_sgemv", order, TransA, M, N, alpha, A, lda, X, incX, beta, Y, incY);
}

extern "C" void hblas_sger(const enum HBLAS_ORDER order, const int M, const int N, const float alpha, const float *X, const int incX, const float *Y,
                           const int incY, float *A, const int lda) {
    la::hblas_ger<F32>("hblas_sger", order, M, N, alpha, X, incX, Y, incY, A, lda);
}

extern "C" void hblas_sgemm(const enum HBLAS_ORDER Order, const enum HBLAS_TRANSPOSE TransA, const enum HBLAS_TRANSPOSE TransB, const int M, const int N,
                            const int K, const float alpha, const float *A, const int lda, const float *B, const int ldb, const float beta, float *C,
                            const int ldc) {
    la::hblas_gemm<F32>("hblas_sgemm", Order, TransA, TransB, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc);
}
