// linear_algebra.hip — gfx950 implementation of the twelve f32 AOT pipelines of apps/linear_algebra (the `halide_s*` objects behind
// halide_blas.h) and of the CBLAS-shaped hblas_s* calls over them (include/hlmi_blas.h): linear_algebra_core.h at T = float.
//
// Algorithms: apps/linear_algebra/src/blas_l1_generators.cpp (AXPY :27-70, Dot :90-124, AbsSum :144-176), blas_l2_generators.cpp
// (GEMV :27-196, GER :217-242), blas_l3_generators.cpp (GEMM :25-172); which generator parameters make which entry point:
// src/CMakeLists.txt.  The contract, the checks, the entry points' bodies and every kernel but the one below are in
// linear_algebra_core.h; a vectorised reduction keeps the V = 8 lane sums of the reference's x86-64 AVX2 build.
// This file holds the named constants, the extern "C" surface and
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
#include "linear_algebra_core.h"

using namespace hlmi;
using namespace hlmi::la_host;

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));

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
constexpr int KC = 32;                   // k steps per staged chunk of the small tile; the large tile stages KC / 2

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
