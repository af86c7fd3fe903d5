// linear_algebra_core.h — what linear_algebra.hip (f32) and linear_algebra_f64.hip (f64) share, written once: the reference's generators
// are templates on the element type, and so is everything here.  Each file instantiates it with a configuration struct built from its
// own named constants:
//     struct Cfg {
//         using T = float;                                   // the element type, and the type of the scalars a and b
//         static constexpr int V, MAX_VECTOR, MAX_EXTENT;    // lane sums of a vectorised reduction; the limits of the entry points
//         static constexpr int ELEM_ACCESSES;                // 16-byte accesses per lane of la_elem<., ., true>
//         static constexpr int RED_BLOCK, RED_PITCH;         // la_reduce: elements staged per step, elements between the chain lanes' LDS rows
//         static constexpr int GEMV_WG, GEMV_U;              // threads of a gemv workgroup, k steps per unrolled group
//         static constexpr uint32_t TYPE;                    // T_F32 / T_F64 ...
//         static constexpr auto scalar;                      // ... with scalar_f32 / scalar_f64
//         static constexpr la::Names NAMES;                  // HLMI_LA_NAMES(routine prefix, suffix of the vector elementwise launch)
//         static int gemm(void *uc, hipStream_t st, bool tA, bool tB, const la::GGeom<T> &g, bool general_only);   // the file's gemm_plan + gemm_launch
//     };
// What stays in the two files: those constants, the tiled gemm kernel with its plan and launch, and the extern "C" surface.
//
// The contract the kernels share with the checkers (tests/cpp/linear_algebra_check.c, linear_algebra_f64_check.c) is restated in
// include/hlmi_pipelines.h and DESIGN.md sections 5.8 and 5.10.  In short: dimension 0 is innermost with stride 1 and min 0, matrices
// are column-major, every reduction runs its index strictly upward, a vectorised reduction keeps the V lane sums of the reference's
// x86-64 AVX2 build, and the float forms are dev::mad / dev::mad2 of hlmi_device_math.h.
//
// Every pipeline has two implementations.  The second one — one thread per output running the chain as written — is reached only
// through the general hook; `<family>_plan()` (or the line marked THE predicate) is the one place that chooses a launch:
//   copy / scal / axpy / ger   la_elem<C, MODE, VEC>: 16-byte accesses where every address (and the matrix's column stride) allows — 1024
//                              elements per workgroup: one float4, or two double2 at pairs tid and tid + 256, per lane — and one element
//                              per thread otherwise
//   dot / asum                 la_reduce: ONE wave.  The contract is V chains of n / V dependent steps, so the only job is that loads
//                              never stall the chains: the wave loads RED_BLOCK elements of each operand with coalesced loads, one block
//                              ahead, hands them through LDS to the V chain lanes (each reads its 32 steps as 16-byte LDS loads), and
//                              lanes 0 .. V - 1 step the chains
//   gemv_notrans               la_gemv_n: one sequential chain per output, lanes along i (coalesced), 64-thread workgroups so that a
//                              small M still spreads over CUs, k unrolled by GEMV_U with the next GEMV_U loads in flight under the
//                              fmas; x(k) is wave-uniform
//   gemv_trans                 la_gemv_t: a wave owns 64 / V outputs x V chains; the lanes of a chain group read 32 contiguous bytes of
//                              their column per step, GEMV_U steps ahead; the lane sum is __shfl with width V
//   gemm (four variants)       the file's own tiled kernel; here only la_gemm_general
#pragma once

#include "hlmi_blas.h"
#include "hlmi_device_math.h"
#include "hlmi_internal.h"

#include <math.h>

namespace hlmi {

// ---------------------------------------------------------------------------------------------------------------- host: checks
// alignment, overlap of byte ranges (by each buffer's own element size), the pinned shapes, derived extents, limits and bounds-query answers.
// Ordinary inline functions under the namespace they have had since the f64 half: pin() and overlap() are emitted out of line, and the
// library's dynamic symbol table lists them under these names.
namespace la_host {

inline bool aligned16(const void *p) { return (uintptr_t)p % 16 == 0; }
// a matrix whose every column starts on 16 bytes: `per16` elements fill 16 bytes
inline bool aligned16(const void *p, long col_stride, int per16) { return aligned16(p) && col_stride % per16 == 0; }

inline uintptr_t elem_bytes(const halide_buffer_t *b) { return (b->type.bits + 7) / 8; }

// elements from a buffer's first to one past its last, 0 for an empty one (dimension 0 has stride 1)
inline uintptr_t span_elems(const halide_buffer_t *b) {
    uintptr_t n = 1;
    for (int d = 0; d < b->dimensions; d++) {
        if (b->dim[d].extent <= 0) return 0;
        n += (uintptr_t)(b->dim[d].extent - 1) * (uintptr_t)b->dim[d].stride;
    }
    return n;
}

inline bool same_layout(const halide_buffer_t *a, const halide_buffer_t *b) {
    if (a->dimensions != b->dimensions) return false;
    for (int d = 0; d < a->dimensions; d++)
        if (a->dim[d].extent != b->dim[d].extent || a->dim[d].stride != b->dim[d].stride) return false;
    return true;
}

// mat_mul.hip's overlap() for any shape: do the byte ranges of a and b meet, in host or in device memory.  With `exact_ok`, a that IS
// b — the same first element and the same layout, the call every wrapper of halide_blas.h makes — does not count.
inline bool overlap(const halide_buffer_t *a, const halide_buffer_t *b, bool exact_ok) {
    if (a == b) return !exact_ok;
    const uintptr_t na = elem_bytes(a) * span_elems(a), nb = elem_bytes(b) * span_elems(b);
    auto hit = [&](uintptr_t pa, uintptr_t pb) {
        if (!pa || !pb || !na || !nb) return false;
        if (exact_ok && pa == pb && same_layout(a, b)) return false;
        return pa < pb + nb && pb < pa + na;
    };
    return hit((uintptr_t)a->host, (uintptr_t)b->host) || hit((uintptr_t)a->device, (uintptr_t)b->device);
}

// records: min == 0, extent == the named value, and for a matrix a column stride that keeps columns apart
inline void pin(void *uc, const BufArg &a, int d, int extent, const char *extent_name) {
    char what[40], expect[64];
    snprintf(what, sizeof what, "%s.min.%d", a.name, d);
    check_equal(uc, what, a.buf->dim[d].min, "0", 0);
    snprintf(what, sizeof what, "%s.extent.%d", a.name, d);
    check_equal(uc, what, a.buf->dim[d].extent, extent_name, extent);
    if (d == 1) {
        snprintf(what, sizeof what, "%s.stride.1", a.name);
        snprintf(expect, sizeof expect, "max(%s.stride.1, %s.extent.0)", a.name, a.name);
        check_equal(uc, what, a.buf->dim[1].stride, expect, std::max(a.buf->dim[1].stride, a.buf->dim[0].extent));
    }
}

// an extent the call derives its sizes from: the first of `cands` (buffer, dimension) that is real or, in a query, shaped; else 0
struct Cand {
    const halide_buffer_t *b;
    int d;
};
inline int derive(std::initializer_list<Cand> cands) {
    for (const Cand &c : cands)
        if (c.b && buffer_known(c.b)) return c.b->dim[c.d].extent;
    return 0;
}

inline int limit(void *uc, const char *entry, const char *what, int v, int max) {
    if (v >= 0 && v <= max) return 0;
    return report(uc, halide_error_code_constraint_violated, "Constraint violated: %s %s (%d) must be 0 .. %d", entry, what, v, max);
}

inline void answer1(halide_buffer_t *b, int n) {
    const int mins[1] = {0}, ext[1] = {n};
    answer_query(b, mins, ext);
}
inline void answer2(halide_buffer_t *b, int w, int h) {
    const int mins[2] = {0, 0}, ext[2] = {w, h};
    answer_query(b, mins, ext);
}

// null, type, dimensionality; returns 1 for a bounds query (the caller answers it), < 0 for an error
inline int prologue(void *uc, const BufArg *args, int n) {
    int r = check_not_null(uc, args, n);
    if (r) return r;
    if ((r = check_type_and_dims(uc, args, n))) return r;
    return any_bounds_query(args, n) ? 1 : 0;
}

}  // namespace la_host

namespace la {
using namespace la_host;
namespace {   // internal linkage, as when each file held its own copy: the library exports the C ABI only

// ---------------------------------------------------------------------------------------------------------------- names
enum Entry { N_COPY, N_SCAL, N_AXPY, N_DOT, N_ASUM, N_GEMV_N, N_GEMV_T, N_GER, N_GEMM /* + tA + 2 * tB */, N_ENTRIES = N_GEMM + 4 };
enum ElemMode { E_COPY, E_SCAL, E_AXPY, E_GER };   // the first three are their own Entry
enum ElemLaunch { EL_VEC, EL_SCALAR, EL_GENERAL };

// every routine-name string of one element type: string literals, so that what HLMI_LAUNCH is handed has static storage
struct Names {
    const char *entry[N_ENTRIES];   // [Entry]
    const char *elem[4][3];         // [ElemMode][ElemLaunch]
    const char *red[2][2];          // [asum][general_only]
    const char *gemv[2][2];         // [trans][general_only]
};
// p: "s" or "d"; vec: "vec4" or "vec2", the elements of a 16-byte access
#define HLMI_LA_NAMES(p, vec)                                                                                                                          \
    {{"halide_" p "copy_impl", "halide_" p "scal_impl", "halide_" p "axpy_impl", "halide_" p "dot", "halide_" p "asum", "halide_" p "gemv_notrans",     \
      "halide_" p "gemv_trans", "halide_" p "ger_impl", "halide_" p "gemm_notrans", "halide_" p "gemm_transA", "halide_" p "gemm_transB",               \
      "halide_" p "gemm_transAB"},                                                                                                                      \
     {{p "copy_" vec, p "copy_scalar", p "copy_general"}, {p "scal_" vec, p "scal_scalar", p "scal_general"},                                           \
      {p "axpy_" vec, p "axpy_scalar", p "axpy_general"}, {p "ger_" vec, p "ger_scalar", p "ger_general"}},                                             \
     {{p "dot_wave", p "dot_general"}, {p "asum_wave", p "asum_general"}},                                                                              \
     {{p "gemv_notrans_wave", p "gemv_notrans_general"}, {p "gemv_trans_wave", p "gemv_trans_general"}}}

// the correctly rounded call of each type
__device__ __forceinline__ float abs_of(float x) { return fabsf(x); }
__device__ __forceinline__ double abs_of(double x) { return fabs(x); }
inline float sqrt_of(float x) { return sqrtf(x); }
inline double sqrt_of(double x) { return sqrt(x); }

template<typename T>
using Vec16 = T __attribute__((ext_vector_type(16 / sizeof(T))));   // float4 / double2

// ---------------------------------------------------------------------------------------------------------------- elementwise
template<typename T>
struct EGeom {
    const T *x;   // [n]
    const T *y;   // AXPY: [n], read at i; GER: [rows], read at j
    T *r;         // [n] or [n x rows]; GER reads it too
    long n, ldr;
    int rows;
    T a;
};

template<int MODE, typename T>
__device__ __forceinline__ T elem_value(T a, T x, T y, T r) {
    if (MODE == E_COPY) return x;
    if (MODE == E_SCAL) return a * x;
    if (MODE == E_AXPY) return dev::mad(a, x, y);
    return dev::mad(a * y, x, r);   // GER: (a * y(j)) * x(i) + result(i, j)
}

// the 16-byte group at element i of one row, or what is left of it at the end of the row
template<typename C, int MODE, typename T>
__device__ __forceinline__ void elem_group(const EGeom<T> &g, T *row, T yj, long i) {
    constexpr int PER = 16 / sizeof(T);
    if (C::ELEM_ACCESSES == 1 && i >= g.n) return;   // a lane with a single access and nothing to do leaves first
    if (i + PER <= g.n) {
        const Vec16<T> xv = *reinterpret_cast<const Vec16<T> *>(g.x + i);
        Vec16<T> yv = (Vec16<T>)(yj), rv = (Vec16<T>)(T(0)), out;
        if (MODE == E_AXPY) yv = *reinterpret_cast<const Vec16<T> *>(g.y + i);
        if (MODE == E_GER) rv = *reinterpret_cast<const Vec16<T> *>(row + i);
#pragma unroll
        for (int e = 0; e < PER; e++) out[e] = elem_value<MODE>(g.a, xv[e], yv[e], rv[e]);
        *reinterpret_cast<Vec16<T> *>(row + i) = out;
    } else if (PER == 2) {   // the last element of an odd n
        if (i < g.n) row[i] = elem_value<MODE>(g.a, g.x[i], MODE == E_AXPY ? g.y[i] : yj, MODE == E_GER ? row[i] : T(0));
    } else {
        for (long e = i; e < g.n; e++)   // the last, partial group
            row[e] = elem_value<MODE>(g.a, g.x[e], MODE == E_AXPY ? g.y[e] : yj, MODE == E_GER ? row[e] : T(0));
    }
}

template<typename C, int MODE, bool VEC>
__global__ __launch_bounds__(256) void la_elem(EGeom<typename C::T> g) {
    using T = typename C::T;
    constexpr int PER = 16 / sizeof(T);
    const long j = blockIdx.y;
    T *row = g.r + j * g.ldr;
    const T yj = MODE == E_GER ? g.y[j] : T(0);
    if (VEC) {
        // group p of the workgroup's 256 * ELEM_ACCESSES: a lane moves groups tid and, with two accesses, tid + 256, so each access of a wave is 1 KiB
        const long i0 = (long)blockIdx.x * (256 * C::ELEM_ACCESSES * PER);
        if (C::ELEM_ACCESSES == 1) {   // not a one-trip loop: inside one the compiler gives saxpy_vec4 and sger_vec4 another schedule and 4 and 3 VGPRs more
            elem_group<C, MODE>(g, row, yj, i0 + PER * threadIdx.x);
        } else {
#pragma unroll
            for (int h = 0; h < C::ELEM_ACCESSES; h++) elem_group<C, MODE>(g, row, yj, i0 + PER * (threadIdx.x + 256 * h));
        }
    } else {
        const long idx = (long)blockIdx.x * 256 + threadIdx.x;
        if (idx >= g.n) return;
        row[idx] = elem_value<MODE>(g.a, g.x[idx], MODE == E_AXPY ? g.y[idx] : yj, MODE == E_GER ? row[idx] : T(0));
    }
}

// ---------------------------------------------------------------------------------------------------------------- dot, asum
template<bool ASUM, typename T>
__device__ __forceinline__ T red_step(T x, T y, T acc) { return ASUM ? acc + abs_of(x) : dev::mad(x, y, acc); }

// one wave; y is not read by asum
template<typename C, bool ASUM>
__global__ __launch_bounds__(64) void la_reduce(const typename C::T *x, const typename C::T *y, typename C::T *result, long n) {
    using T = typename C::T;
    constexpr int V = C::V, RED_BLOCK = C::RED_BLOCK, RED_PITCH = C::RED_PITCH;
    constexpr int PER_LANE = RED_BLOCK / 64;     // loads per lane, operand and block
    constexpr int STEPS = RED_BLOCK / V;         // chain steps per block
    constexpr int PER = 16 / sizeof(T), NQ = STEPS / PER;   // a chain lane's steps of a block: NQ 16-byte LDS reads
    __shared__ __attribute__((aligned(16))) T sx[2][V * RED_PITCH];
    __shared__ __attribute__((aligned(16))) T sy[2][V * RED_PITCH];
    const int lane = threadIdx.x;
    const long nblk = n / RED_BLOCK;
    T px[PER_LANE], py[PER_LANE];   // the block in flight: element 64 c + lane of it
    auto load = [&](long blk) {
#pragma unroll
        for (int c = 0; c < PER_LANE; c++) {
            px[c] = x[blk * RED_BLOCK + 64 * c + lane];
            if (!ASUM) py[c] = y[blk * RED_BLOCK + 64 * c + lane];
        }
    };
    // element e of a block belongs to chain e % V, step e / V: chain lane i finds its steps in row i
    auto stage = [&](int buf) {
#pragma unroll
        for (int c = 0; c < PER_LANE; c++) {
            sx[buf][(lane & (V - 1)) * RED_PITCH + (64 / V) * c + lane / V] = px[c];
            if (!ASUM) sy[buf][(lane & (V - 1)) * RED_PITCH + (64 / V) * c + lane / V] = py[c];
        }
    };
    T acc = T(0);   // lanes 0 .. V - 1: the chains
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
            const Vec16<T> *rx = reinterpret_cast<const Vec16<T> *>(&sx[buf][lane * RED_PITCH]);
            const Vec16<T> *ry = reinterpret_cast<const Vec16<T> *>(&sy[buf][lane * RED_PITCH]);
            Vec16<T> vx[NQ], vy[NQ];
#pragma unroll
            for (int q = 0; q < NQ; q++) {
                vx[q] = rx[q];
                vy[q] = ASUM ? vx[q] : ry[q];
            }
#pragma unroll
            for (int q = 0; q < NQ; q++)
#pragma unroll
                for (int e = 0; e < PER; e++) acc = red_step<ASUM>(vx[q][e], vy[q][e], acc);
        }
        __syncthreads();
    }
    // the whole steps past the last block, straight from global memory
    const long nvec = n / V;
    if (lane < V)
        for (long k = nblk * STEPS; k < nvec; k++) acc = red_step<ASUM>(x[k * V + lane], ASUM ? T(0) : y[k * V + lane], acc);
    T s = T(0);
#pragma unroll
    for (int i = 0; i < V; i++) s = s + __shfl(acc, i);
    T t = T(0);
    for (long e = nvec * V; e < n; e++) t = red_step<ASUM>(x[e], ASUM ? T(0) : y[e], t);
    if (lane == 0) *result = s + t;
}

template<typename C, bool ASUM>
__global__ __launch_bounds__(64) void la_reduce_general(const typename C::T *x, const typename C::T *y, typename C::T *result, long n) {
    using T = typename C::T;
    constexpr int V = C::V;
    if (threadIdx.x != 0) return;
    T lanes[V];
#pragma unroll
    for (int i = 0; i < V; i++) lanes[i] = T(0);
    const long nvec = n / V;
    for (long k = 0; k < nvec; k++)
#pragma unroll
        for (int i = 0; i < V; i++) lanes[i] = red_step<ASUM>(x[k * V + i], ASUM ? T(0) : y[k * V + i], lanes[i]);
    T s = T(0);
#pragma unroll
    for (int i = 0; i < V; i++) s = s + lanes[i];
    T t = T(0);
    for (long e = nvec * V; e < n; e++) t = red_step<ASUM>(x[e], ASUM ? T(0) : y[e], t);
    *result = s + t;
}

// ---------------------------------------------------------------------------------------------------------------- gemv
template<typename T>
struct VGeom {
    const T *A, *x, *y;
    T *out;
    int w, h;   // A's extents: dimension 0 (contiguous) and dimension 1
    long lda;
    T a, b;
};

// notrans: output(i) = the chain over k of mad(a * A(i, k), x(k), .) from b * y(i); i < w, k < h
template<typename C>
__global__ __launch_bounds__(C::GEMV_WG) void la_gemv_n(VGeom<typename C::T> g) {
    using T = typename C::T;
    constexpr int GEMV_WG = C::GEMV_WG, GEMV_U = C::GEMV_U;
    const int i = blockIdx.x * GEMV_WG + threadIdx.x;
    if (i >= g.w) return;
    T acc = g.b * g.y[i];
    const T *col = g.A + i;
    int k = 0;
    if (g.h >= GEMV_U) {
        T cur[GEMV_U], nxt[GEMV_U];
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

template<typename T>
__global__ __launch_bounds__(256) void la_gemv_n_general(VGeom<T> g) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.w) return;
    T acc = g.b * g.y[i];
    for (int k = 0; k < g.h; k++) acc = dev::mad(g.a * g.A[(long)k * g.lda + i], g.x[k], acc);
    g.out[i] = acc;
}

// trans: output(i), i < h, from column i of A: V lane chains over k of mad(A(kV + j, i), x(kV + j), .), their sum from +0 in lane
// order, the tail on top of the sum, then mad2(b, y(i), a, s).  Lane l: output (GEMV_WG / V) * block + l / V, chain l % V.
template<typename C>
__global__ __launch_bounds__(C::GEMV_WG) void la_gemv_t(VGeom<typename C::T> g) {
    using T = typename C::T;
    constexpr int V = C::V, GEMV_WG = C::GEMV_WG, GEMV_U = C::GEMV_U;
    const int lane = threadIdx.x, j = lane & (V - 1);
    const int o = blockIdx.x * (GEMV_WG / V) + lane / V;
    const T *col = g.A + (long)min(o, g.h - 1) * g.lda;   // the lanes past the last output repeat it and store nothing
    const int nvec = g.w / V;
    T acc = T(0);
    int k = 0;
    if (nvec >= GEMV_U) {
        T ca[GEMV_U], cx[GEMV_U], na[GEMV_U], nx[GEMV_U];
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
    T s = T(0);
#pragma unroll
    for (int i = 0; i < V; i++) s = s + __shfl(acc, i, V);
    for (int t = nvec * V; t < g.w; t++) s = dev::mad(col[t], g.x[t], s);
    if (j == 0 && o < g.h) g.out[o] = dev::mad2(g.b, g.y[o], g.a, s);
}

template<typename C>
__global__ __launch_bounds__(256) void la_gemv_t_general(VGeom<typename C::T> g) {
    using T = typename C::T;
    constexpr int V = C::V;
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= g.h) return;
    const T *col = g.A + (long)o * g.lda;
    T lanes[V];
#pragma unroll
    for (int i = 0; i < V; i++) lanes[i] = T(0);
    const int nvec = g.w / V;
    for (int k = 0; k < nvec; k++)
#pragma unroll
        for (int i = 0; i < V; i++) lanes[i] = dev::mad(col[k * V + i], g.x[k * V + i], lanes[i]);
    T s = T(0);
#pragma unroll
    for (int i = 0; i < V; i++) s = s + lanes[i];
    for (int t = nvec * V; t < g.w; t++) s = dev::mad(col[t], g.x[t], s);
    g.out[o] = dev::mad2(g.b, g.y[o], g.a, s);
}

// ---------------------------------------------------------------------------------------------------------------- gemm
template<typename T>
struct GGeom {
    const T *A, *B, *C;
    T *out;
    int M, N, K;             // result is M x N (i < M contiguous), the sum runs over K
    long sa, sb, sc, so;     // column strides in elements
    T a, b;
};

// The second implementation: one thread per output, the chain as written.
template<typename T, bool TA, bool TB>
__global__ __launch_bounds__(256) void la_gemm_general(GGeom<T> g) {
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= g.M) return;
    const T *pa = TA ? g.A + (long)i * g.sa : g.A + i;
    const T *pb = TB ? g.B + j : g.B + (long)j * g.sb;
    const long da = TA ? 1 : g.sa, db = TB ? g.sb : 1;
    T ab = T(0);
    for (int k = 0; k < g.K; k++) ab = dev::mad(pa[k * da], pb[k * db], ab);
    g.out[(long)j * g.so + i] = dev::mad2(g.a, ab, g.b, g.C[(long)j * g.sc + i]);
}

// ---------------------------------------------------------------------------------------------------------------- host: tables
// no estimates: the generators declare none
template<typename C>
struct Tables {
#define HLMI_LA_VEC_ARGS {C::scalar("a"), in_buf("x", C::TYPE, 1), in_buf("y", C::TYPE, 1), out_buf("result", C::TYPE, 1)}
#define HLMI_LA_GEMV_ARGS {C::scalar("a"), in_buf("A", C::TYPE, 2), in_buf("x", C::TYPE, 1), C::scalar("b"), in_buf("y", C::TYPE, 1), out_buf("output", C::TYPE, 1)}
#define HLMI_LA_GEMM_ARGS {C::scalar("a_"), in_buf("A_", C::TYPE, 2), in_buf("B_", C::TYPE, 2), C::scalar("b_"), in_buf("C_", C::TYPE, 2), out_buf("result", C::TYPE, 2)}
    const ArgTable t[N_ENTRIES] = {   // [Entry]
        {C::NAMES.entry[N_COPY], HLMI_LA_VEC_ARGS},
        {C::NAMES.entry[N_SCAL], HLMI_LA_VEC_ARGS},
        {C::NAMES.entry[N_AXPY], HLMI_LA_VEC_ARGS},
        {C::NAMES.entry[N_DOT], {in_buf("x", C::TYPE, 1), in_buf("y", C::TYPE, 1), out_buf("result", C::TYPE, 0)}},
        {C::NAMES.entry[N_ASUM], {in_buf("x", C::TYPE, 1), out_buf("result", C::TYPE, 0)}},
        {C::NAMES.entry[N_GEMV_N], HLMI_LA_GEMV_ARGS},
        {C::NAMES.entry[N_GEMV_T], HLMI_LA_GEMV_ARGS},
        {C::NAMES.entry[N_GER], {C::scalar("a"), in_buf("x", C::TYPE, 1), in_buf("y", C::TYPE, 1), out_buf("result", C::TYPE, 2)}},
        {C::NAMES.entry[N_GEMM + 0], HLMI_LA_GEMM_ARGS},
        {C::NAMES.entry[N_GEMM + 1], HLMI_LA_GEMM_ARGS},
        {C::NAMES.entry[N_GEMM + 2], HLMI_LA_GEMM_ARGS},
        {C::NAMES.entry[N_GEMM + 3], HLMI_LA_GEMM_ARGS}};
#undef HLMI_LA_VEC_ARGS
#undef HLMI_LA_GEMV_ARGS
#undef HLMI_LA_GEMM_ARGS
    const ArgTable &operator[](int e) const { return t[e]; }
};
template<typename C>
const Tables<C> tables{};

// ---------------------------------------------------------------------------------------------------------------- host: copy, scal, axpy, ger
// THE predicate of the four elementwise pipelines: 16-byte accesses where every address a lane forms is a multiple of 16 bytes — x, the
// result, axpy's y and, for ger, the result's column stride — and one element per thread otherwise.
template<typename T>
ElemLaunch elem_plan(int mode, const EGeom<T> &g, bool general_only) {
    if (general_only) return EL_GENERAL;
    const bool vec = aligned16(g.x) && aligned16(g.r) && (mode != E_AXPY || aligned16(g.y)) && (mode != E_GER || g.ldr % (16 / sizeof(T)) == 0);
    return vec ? EL_VEC : EL_SCALAR;
}

template<typename C, int MODE>
int elem_launch_mode(void *uc, hipStream_t st, const EGeom<typename C::T> &g, ElemLaunch l) {
    const char *name = C::NAMES.elem[MODE][l];
    const double elems = (double)g.n * g.rows, bytes = sizeof(typename C::T);
    timing_note_bytes(MODE == E_COPY || MODE == E_SCAL ? 2 * bytes * elems : MODE == E_AXPY ? 3 * bytes * elems : 2 * bytes * elems + bytes * (g.n + g.rows));
    const long per_block = l == EL_VEC ? 256 * C::ELEM_ACCESSES * (16 / sizeof(typename C::T)) : 256;
    const dim3 grid((unsigned)((g.n + per_block - 1) / per_block), (unsigned)g.rows);
    if (l == EL_VEC) HLMI_LAUNCH(uc, name, st, (la_elem<C, MODE, true>), grid, dim3(256), 0, g);
    else HLMI_LAUNCH(uc, name, st, (la_elem<C, MODE, false>), grid, dim3(256), 0, g);
    return 0;
}

template<typename C>
int elem_launch(void *uc, hipStream_t st, int mode, const EGeom<typename C::T> &g, ElemLaunch l) {
    if (g.n <= 0 || g.rows <= 0) return 0;   // a zero extent launches nothing
    switch (mode) {
    case E_COPY: return elem_launch_mode<C, E_COPY>(uc, st, g, l);
    case E_SCAL: return elem_launch_mode<C, E_SCAL>(uc, st, g, l);
    case E_AXPY: return elem_launch_mode<C, E_AXPY>(uc, st, g, l);
    default: return elem_launch_mode<C, E_GER>(uc, st, g, l);
    }
}

// copy / scal / axpy.  y is looked at by axpy only: the reference's wrappers pass a null pointer for it to the other two.
template<typename C>
int vec_entry(int mode, typename C::T a, halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result, bool general_only) {
    using T = typename C::T;
    void *uc = nullptr;
    const ArgTable &table = tables<C>[mode];
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
    if ((r = limit(uc, table.md.name, "x.extent.0", size, C::MAX_VECTOR))) return r;
    check_shapes(uc, args, n);
    for (int i = 0; i < n; i++) pin(uc, args[i], 0, size, "x.extent.0");
    if ((r = checks_done(uc))) return r;
    // the wrappers' calls: scal's result is x, axpy's result is y
    if (overlap(result, x, mode == E_SCAL)) return report(uc, halide_error_code_constraint_violated, "Constraint violated: result may not overlap x");
    if (mode == E_AXPY && overlap(result, y, true))
        return report(uc, halide_error_code_constraint_violated, "Constraint violated: result may overlap y only where it is y");
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, n))) return r;
    const EGeom<T> g = {dev_ptr<T>(x), mode == E_AXPY ? dev_ptr<T>(y) : nullptr, dev_ptr<T>(result), size, 0, 1, a};
    if ((r = elem_launch<C>(uc, ctx.stream, mode, g, elem_plan(mode, g, general_only)))) return r;
    mark_output_written(result);
    return 0;
}

// ger: the result is read and written in place
template<typename C>
int ger_entry(typename C::T a, halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result, bool general_only) {
    using T = typename C::T;
    void *uc = nullptr;
    const char *entry = tables<C>[N_GER].md.name;
    BufArg args[3];
    tables<C>[N_GER].bufs(args, {x, y, result});
    int r = prologue(uc, args, 3);
    if (r < 0) return r;
    const int m = derive({{x, 0}, {result, 0}}), n = derive({{y, 0}, {result, 1}});
    if (r == 1) {
        answer1(x, m), answer1(y, n), answer2(result, m, n);
        return 0;
    }
    if ((r = limit(uc, entry, "x.extent.0", m, C::MAX_EXTENT)) || (r = limit(uc, entry, "y.extent.0", n, C::MAX_EXTENT))) return r;
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
    const EGeom<T> g = {dev_ptr<T>(x), dev_ptr<T>(y), dev_ptr<T>(result), m, result->dim[1].stride, n, a};
    if ((r = elem_launch<C>(uc, ctx.stream, E_GER, g, elem_plan(E_GER, g, general_only)))) return r;
    mark_output_written(result);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- host: dot, asum
template<typename C>
int red_entry(bool asum, halide_buffer_t *x, halide_buffer_t *y, halide_buffer_t *result, bool general_only) {
    using T = typename C::T;
    void *uc = nullptr;
    const ArgTable &table = tables<C>[asum ? N_ASUM : N_DOT];
    BufArg args[3];
    int n = 0;
    if (asum) {
        BufArg two[2];
        table.bufs(two, {x, result});
        args[0] = two[0], args[1] = two[1], n = 2;
    } else {
        table.bufs(args, {x, y, result});
        n = 3;
    }
    int r = prologue(uc, args, n);
    if (r < 0) return r;
    const int size = derive({{x, 0}, {asum ? nullptr : y, 0}});
    if (r == 1) {
        answer1(x, size);
        if (!asum) answer1(y, size);
        return 0;   // the 0-dimensional result has nothing to answer
    }
    if ((r = limit(uc, table.md.name, "x.extent.0", size, C::MAX_VECTOR))) return r;
    check_shapes(uc, args, n);
    for (int i = 0; i < n - 1; i++) pin(uc, args[i], 0, size, "x.extent.0");
    if ((r = checks_done(uc))) return r;
    if (overlap(result, x, false) || (!asum && overlap(result, y, false)))
        return report(uc, halide_error_code_constraint_violated, "Constraint violated: result may not overlap %s", overlap(result, x, false) ? "x" : "y");
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, n))) return r;
    T *out = dev_ptr<T>(result);
    if (size == 0) {
        HLMI_HIP(uc, hipMemsetAsync(out, 0, sizeof(T), ctx.stream));   // a zero extent launches nothing: +0, every byte of it
    } else {
        const T *px = dev_ptr<T>(x), *py = asum ? nullptr : dev_ptr<T>(y);
        const double bytes = sizeof(T);
        timing_note_bytes((asum ? bytes : 2 * bytes) * size + bytes);
        // THE predicate: the staged wave everywhere; one thread only where the caller asks for it by name
        const char *name = C::NAMES.red[asum][general_only];
        const long ln = size;
        if (asum && general_only) HLMI_LAUNCH(uc, name, ctx.stream, (la_reduce_general<C, true>), dim3(1), dim3(64), 0, px, py, out, ln);
        else if (asum) HLMI_LAUNCH(uc, name, ctx.stream, (la_reduce<C, true>), dim3(1), dim3(64), 0, px, py, out, ln);
        else if (general_only) HLMI_LAUNCH(uc, name, ctx.stream, (la_reduce_general<C, false>), dim3(1), dim3(64), 0, px, py, out, ln);
        else HLMI_LAUNCH(uc, name, ctx.stream, (la_reduce<C, false>), dim3(1), dim3(64), 0, px, py, out, ln);
    }
    mark_output_written(result);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- host: gemv
// A is w x h as stored.  notrans: x[h], y[w], output[w].  trans: x[w], y[h], output[h].
template<typename C>
int gemv_entry(bool trans, typename C::T a, halide_buffer_t *A, halide_buffer_t *x, typename C::T b, halide_buffer_t *y, halide_buffer_t *output,
               bool general_only) {
    using T = typename C::T;
    constexpr int V = C::V, GEMV_WG = C::GEMV_WG;
    void *uc = nullptr;
    const ArgTable &table = tables<C>[trans ? N_GEMV_T : N_GEMV_N];
    const char *entry = table.md.name;
    BufArg args[4];
    table.bufs(args, {A, x, y, output});
    int r = prologue(uc, args, 4);
    if (r < 0) return r;
    const int w = trans ? derive({{A, 0}, {x, 0}}) : derive({{A, 0}, {y, 0}, {output, 0}});
    const int h = trans ? derive({{A, 1}, {y, 0}, {output, 0}}) : derive({{A, 1}, {x, 0}});
    const int nx = trans ? w : h, ny = trans ? h : w;
    if (r == 1) {
        answer2(A, w, h), answer1(x, nx), answer1(y, ny), answer1(output, ny);
        return 0;
    }
    if ((r = limit(uc, entry, "A.extent.0", w, C::MAX_EXTENT)) || (r = limit(uc, entry, "A.extent.1", h, C::MAX_EXTENT))) return r;
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
        const VGeom<T> g = {dev_ptr<T>(A), dev_ptr<T>(x), dev_ptr<T>(y), dev_ptr<T>(output), w, h, A->dim[1].stride, a, b};
        timing_note_bytes(sizeof(T) * ((double)w * h + nx + 2.0 * ny));
        // THE predicate: the wave kernels everywhere; one thread per output only where the caller asks for it by name
        const char *name = C::NAMES.gemv[trans][general_only];
        hipStream_t st = ctx.stream;
        if (!trans && !general_only) HLMI_LAUNCH(uc, name, st, la_gemv_n<C>, dim3((unsigned)((w + GEMV_WG - 1) / GEMV_WG)), dim3(GEMV_WG), 0, g);
        else if (!trans) HLMI_LAUNCH(uc, name, st, la_gemv_n_general<T>, dim3((unsigned)((w + 255) / 256)), dim3(256), 0, g);
        else if (!general_only) HLMI_LAUNCH(uc, name, st, la_gemv_t<C>, dim3((unsigned)((h + GEMV_WG / V - 1) / (GEMV_WG / V))), dim3(GEMV_WG), 0, g);
        else HLMI_LAUNCH(uc, name, st, la_gemv_t_general<C>, dim3((unsigned)((h + 255) / 256)), dim3(256), 0, g);
    }
    mark_output_written(output);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- host: gemm
// The shapes (blas_l3_generators.cpp:37-53, :167-171): num_rows = A_.width(), num_cols = B_.height() and sum_size = A_.height() are
// taken from the STORED A and B whatever the flags, B_.extent.0 is pinned to sum_size, C_ and result to num_rows x num_cols.  transA
// reads A_(k, i) for i < A_.width() and k < A_.height(): inside A_ only where A_ is square (elsewhere constant_exterior's zeros or
// nothing).  transB reads B_(j, k) for j < B_.height(), k < sum_size == B_.width(): square B_.  transAB swaps the two inputs and
// reads B_(i, k) and A_(k, j) over i < A_.width(), j < B_.height(), k < A_.height(): all three extents equal.
template<typename C>
int gemm_entry(bool tA, bool tB, typename C::T a, halide_buffer_t *A, halide_buffer_t *B, typename C::T b, halide_buffer_t *Cb, halide_buffer_t *result,
               bool general_only) {
    using T = typename C::T;
    void *uc = nullptr;
    const ArgTable &table = tables<C>[N_GEMM + (tA ? 1 : 0) + (tB ? 2 : 0)];
    const char *entry = table.md.name;
    BufArg args[4];
    table.bufs(args, {A, B, Cb, result});
    int r = prologue(uc, args, 4);
    if (r < 0) return r;
    const int M = derive({{A, 0}, {Cb, 0}, {result, 0}}), K = derive({{A, 1}, {B, 0}}), N = derive({{B, 1}, {Cb, 1}, {result, 1}});
    if (r == 1) {
        answer2(A, M, K), answer2(B, K, N), answer2(Cb, M, N), answer2(result, M, N);
        return 0;
    }
    if ((r = limit(uc, entry, "A_.extent.0", M, C::MAX_EXTENT)) || (r = limit(uc, entry, "A_.extent.1", K, C::MAX_EXTENT)) ||
        (r = limit(uc, entry, "B_.extent.1", N, C::MAX_EXTENT)))
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
    if (overlap(result, Cb, true)) return report(uc, halide_error_code_constraint_violated, "Constraint violated: result may overlap C_ only where it is C_");
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, 4))) return r;
    if (M > 0 && N > 0) {   // an empty sum still leaves mad2(a, +0, b, C)
        const GGeom<T> g = {dev_ptr<T>(A), dev_ptr<T>(B), dev_ptr<T>(Cb), dev_ptr<T>(result), M, N, K,
                            A->dim[1].stride, B->dim[1].stride, Cb->dim[1].stride, result->dim[1].stride, a, b};
        if ((r = C::gemm(uc, ctx.stream, tA, tB, g, general_only))) return r;
    }
    mark_output_written(result);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- host: the hook
// Measurement and test hook (hlmi_internal.h): the named entry point with one thread per output.  p0 .. p3 are the entry point's
// buffers in its own order (the unused trailing ones null); a and b are read where the entry point has them.
template<typename C>
int general_entry(const char *hook, const char *name, typename C::T a, typename C::T b, halide_buffer_t *p0, halide_buffer_t *p1, halide_buffer_t *p2,
                  halide_buffer_t *p3) {
    const char *n = name ? name : "(null)";
    int e = 0;
    while (e < N_ENTRIES && strcmp(n, C::NAMES.entry[e])) e++;
    switch (e) {
    case N_COPY:
    case N_SCAL:
    case N_AXPY: return vec_entry<C>(e, a, p0, p1, p2, true);
    case N_DOT: return red_entry<C>(false, p0, p1, p2, true);
    case N_ASUM: return red_entry<C>(true, p0, nullptr, p1, true);
    case N_GEMV_N:
    case N_GEMV_T: return gemv_entry<C>(e == N_GEMV_T, a, p0, p1, b, p2, p3, true);
    case N_GER: return ger_entry<C>(a, p0, p1, p2, true);
    case N_ENTRIES: return report(nullptr, halide_error_code_constraint_violated, "%s: no entry point named %s", hook, n);
    default: return gemm_entry<C>((e - N_GEMM) & 1, (e - N_GEMM) & 2, a, p0, p1, b, p2, p3, true);
    }
}

// ---------------------------------------------------------------------------------------------------------------- hblas_*
// include/hlmi_blas.h states the interface and where it departs from the reference's.  Each call wraps the caller's host arrays in
// buffers, runs the entry point as the wrappers of hlmi_blas.h call it (the one buffer that is both read and written passed twice),
// brings the result home and lets go of the device side.  `fn`: the exported call's own name.
template<typename T>
struct HostVec {
    halide_dimension_t dim[2];
    halide_buffer_t buf;
    HostVec(const T *p, int w, int h = -1, int ld = 0) {
        dim[0] = {0, w, 1, 0};
        dim[1] = {0, h, ld, 0};
        memset(&buf, 0, sizeof buf);
        buf.host = (uint8_t *)const_cast<T *>(p);
        buf.flags = halide_buffer_flag_host_dirty;
        buf.type.code = halide_type_float, buf.type.bits = 8 * sizeof(T);
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

template<typename C, typename T = typename C::T>
void hblas_copy(const char *fn, int N, const T *X, int incX, T *Y, int incY) {
    if (bad_inc(fn, incX, incY)) return;
    HostVec<T> x(X, N), y(Y, N);
    finish(fn, vec_entry<C>(E_COPY, T(0), &x.buf, nullptr, &y.buf, false), &y.buf);
}

template<typename C, typename T = typename C::T>
void hblas_scal(const char *fn, int N, T alpha, T *X, int incX) {
    if (bad_inc(fn, incX)) return;
    HostVec<T> x(X, N);
    finish(fn, vec_entry<C>(E_SCAL, alpha, &x.buf, nullptr, &x.buf, false), &x.buf);
}

template<typename C, typename T = typename C::T>
void hblas_axpy(const char *fn, int N, T alpha, const T *X, int incX, T *Y, int incY) {
    if (bad_inc(fn, incX, incY)) return;
    HostVec<T> x(X, N), y(Y, N);
    finish(fn, vec_entry<C>(E_AXPY, alpha, &x.buf, &y.buf, &y.buf, false), &y.buf);
}

template<typename C, typename T = typename C::T>
T hblas_dot(const char *fn, int N, const T *X, int incX, const T *Y, int incY) {
    if (bad_inc(fn, incX, incY)) return NAN;
    T result = NAN;
    HostVec<T> x(X, N), y(Y, N), r(&result, 0);
    r.buf.dimensions = 0;
    return finish(fn, red_entry<C>(false, &x.buf, &y.buf, &r.buf, false), &r.buf) == 0 ? result : NAN;
}

template<typename C, typename T = typename C::T>
T hblas_nrm2(const char *fn, int N, const T *X, int incX) {
    if (bad_inc(fn, incX)) return NAN;
    T result = NAN;
    HostVec<T> x(X, N), r(&result, 0);
    r.buf.dimensions = 0;
    return finish(fn, red_entry<C>(false, &x.buf, &x.buf, &r.buf, false), &r.buf) == 0 ? sqrt_of(result) : NAN;
}

template<typename C, typename T = typename C::T>
T hblas_asum(const char *fn, int N, const T *X, int incX) {
    if (bad_inc(fn, incX)) return NAN;
    T result = NAN;
    HostVec<T> x(X, N), r(&result, 0);
    r.buf.dimensions = 0;
    return finish(fn, red_entry<C>(true, &x.buf, nullptr, &r.buf, false), &r.buf) == 0 ? result : NAN;
}

template<typename C, typename T = typename C::T>
void hblas_gemv(const char *fn, enum HBLAS_ORDER order, enum HBLAS_TRANSPOSE TransA, int M, int N, T alpha, const T *A, int lda, const T *X, int incX, T beta,
                T *Y, int incY) {
    if (bad_order(fn, order) || bad_inc(fn, incX, incY)) return;
    const bool t = TransA != HblasNoTrans;
    HostVec<T> a(A, M, N, lda), x(X, t ? M : N), y(Y, t ? N : M);
    finish(fn, gemv_entry<C>(t, alpha, &a.buf, &x.buf, beta, &y.buf, &y.buf, false), &y.buf);
}

template<typename C, typename T = typename C::T>
void hblas_ger(const char *fn, enum HBLAS_ORDER order, int M, int N, T alpha, const T *X, int incX, const T *Y, int incY, T *A, int lda) {
    if (bad_order(fn, order) || bad_inc(fn, incX, incY)) return;
    HostVec<T> x(X, M), y(Y, N), a(A, M, N, lda);
    finish(fn, ger_entry<C>(alpha, &x.buf, &y.buf, &a.buf, false), &a.buf);
}

template<typename C, typename T = typename C::T>
void hblas_gemm(const char *fn, enum HBLAS_ORDER Order, enum HBLAS_TRANSPOSE TransA, enum HBLAS_TRANSPOSE TransB, int M, int N, int K, T alpha, const T *A,
                int lda, const T *B, int ldb, T beta, T *Cm, int ldc) {
    if (bad_order(fn, Order)) return;
    const bool tA = TransA != HblasNoTrans, tB = TransB != HblasNoTrans;
    // the generator's shapes (hlmi_pipelines.h): a transposed operand is square
    if (((tA && M != K) || (tB && N != K)) && hblas_refuse(fn, "a transposed operand must be square (M == K for TransA, N == K for TransB)")) return;
    HostVec<T> a(A, tA ? K : M, tA ? M : K, lda), b(B, tB ? N : K, tB ? K : N, ldb), c(Cm, M, N, ldc);
    finish(fn, gemm_entry<C>(tA, tB, alpha, &a.buf, &b.buf, beta, &c.buf, &c.buf, false), &c.buf);
}

}  // namespace
}  // namespace la
}  // namespace hlmi
