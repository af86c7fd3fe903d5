// fft.hip — gfx950 implementation of the reference's fft AOT pipelines: the 2-D f32 transforms c2c forward, c2c inverse, r2c and c2r.
//
// Algorithm: apps/fft/fft.cpp (fft_dim1 :295-421, the codelets :109-229, fft2d_c2c :481-552, fft2d_r2c :667-883, fft2d_c2r :886-1061,
// radix_factor :1066-1097), complex.h, boundary fft_generator.cpp:84-152; the four entry points and their sizes and gains are those of
// apps/fft/CMakeLists.txt:22-47.  The contract, with every choice made where the reference defines nothing (the f32 form of the twiddle
// angle, the signs of zero of * j, * sign, -j *, 0.5f * and conj, the vector width V = 8 that pairs real columns), is derived line by
// line in tests/cpp/fft_check.c and stated in DESIGN.md section 5.9; include/hlmi_pipelines.h restates it for callers.
//
// Every transform is two LINE PASSES through a scratch image, a pass being a set of independent 1-D Stockham transforms whose points
// are fetched by load_elem<MODE> and delivered by store_elem<MODE>: zip, unzip, the conjugate extension and the DC / Nyquist row are
// part of those two functions, never a launch of their own.
//   kind         pass A (lines, along)                               pass B
//   c2c          N1 rows, dimension 0, gain 1                        N0 columns, dimension 1, the gain
//   r2c, skip    the same on (r, +0)                                 the same, rows 0 .. N1/2 stored
//   c2r, skip    the same on the conjugate extension                 the same, the real part stored
//   r2c          N0/2 zipped columns, dimension 1, gain 1            N1/2 rows of the unzipped image (row 0 = DC + j Nyquist), dimension
//                                                                    0, gain / 2; row 0 unzips into rows 0 and N1/2 on the way out
//   c2r          N1/2 rows (row 0 = DC + j Nyquist), dim 0, gain 1   N0/2 zipped columns, dimension 1, the gain; re / im to two columns
// Launches (fft_plan() is the one place that chooses):
//   fft_whole, fft_whole_elem     the whole transform in ONE workgroup and one launch, where the N0 x N1 complex image fits
//                                 ONE_GROUP_BYTES (the reference's 16 x 16 is 2 KB): pass A, a barrier, pass B, the scratch image in
//                                 LDS in front of the two exchange buffers.  The same pass code as below (line_pass).
//   fft_rows, fft_cols            a workgroup holds a batch of lines; each lane runs one radix-R codelet per pass in registers; the
//                                 first pass reads global memory and the last one writes it, the passes between exchange through LDS
//                                 (two buffers, at most four passes for N <= 4096).  Rows are contiguous lines; fft_cols takes a tile
//                                 of adjacent columns by all N1 rows, so every global access of a pass is one contiguous run of
//                                 lines x 8 bytes and no global transpose exists.  The tile is 8 columns (64 bytes) up to N1 = 1024, 4
//                                 at 2048 and 2 at 4096: two exchange buffers of LDS_COMPLEX elements hold no more.
//   fft_rows_elem, fft_cols_elem  the same with 4-byte accesses to the caller's complex buffer, for a pointer or a row stride that is
//                                 no multiple of 8 bytes
//   fft_general_a, fft_general_b  pass A and pass B with one thread per line, the passes as the checker writes them, through two line
//                                 buffers in the scratch arena (hlmi_fft2d_general only)
// LDS layout: element n of line b at pad(n * lines + b) (columns) or pad(b * N + n) (rows), pad(a) = a + (a >> 3); an element is 2
// dwords.  Consecutive lanes take consecutive codelets: consecutive s within a line (rows), consecutive lines b, then s (columns).
// The conflict arithmetic, with the lane groups of MI355X_MICROARCH.md (LDS):
//   reads (ds_read_b64: two halves of 32 lanes, 64 banks).  In both layouts a half reads x[s + r N/R] at 32 consecutive elements.
//     Unpadded that is exactly the 64 banks; padded, the 32 elements hold 3 or 4 pad slots and span 70 or 72 dwords, so the last 3 or
//     4 lanes fall on the banks of the first: 2-way, one extra cycle per half.  THE PAD COSTS THE READS THAT MUCH.
//   writes (ds_write_b64: four groups of 16 lanes, 32 banks), y[(s / S) R S + s % S + r S].
//     rows, S = 1: stride R elements.  R = 8 unpadded is 16 dwords, 2 of 32 banks, 16-way; padded it is 18 dwords, 16 distinct even
//       banks, conflict-free.  R = 4: dwords 8 s + 2 (s / 2), 2-way; R = 2: 4 s + 2 (s / 4), 2-way; R = 6: 12 s + 2 (3 s / 4), 2-way.
//     rows, S >= 8: runs of min(S, 16) consecutive elements R S apart; a run of 8 aligned elements has no pad inside (16 dwords) and the
//       next run starts 2 R S + 2 (R S / 8) dwords on, 16 mod 32 for R S = 64: conflict-free; a run of 16 holds 1 or 2 pads: 2-way.
//     columns: every element index above times `lines`.  lines = 8, S = 1, R = 8: a group is two s of 8 lines each, two aligned runs
//       of 8 elements 64 elements = 144 padded dwords apart, 16 mod 32: conflict-free.  lines = 4 (N1 = 2048): four runs of 4 elements
//       72 dwords apart, 8 mod 32: conflict-free.  lines = 2 (4096): eight runs of 2 elements 36 dwords apart, 4 mod 32:
//       conflict-free.  Later passes as for rows.
//   So the pad removes the 16-way write conflict of the first pass and leaves 2-way conflicts on the reads and on some writes; it
//   does NOT make the exchange conflict-free.  The counters (profiles/NOTES.md) show 7 extra cycles per LDS instruction in the row
//   kernel and 10 in the column kernel at 4096, several times what this arithmetic gives (about 1): the difference is not explained,
//   and no layout was found in the time that is better in both measurements.
// Twiddle tables are built on the host by hlmi_fft_twiddles (cosf / sinf of an f32 angle), one blob per call shape (the two N, sign, gain) holding
// the table of every pass with S > 1, kept on the device in the shared cache of derived data (hlmi_internal.h).
#include "hlmi_internal.h"

#include <math.h>
#include <atomic>
#include <vector>

#include "hlmi_device_math.h"

using namespace hlmi;

namespace {

constexpr int V = 8;                // natural_vector_size of f32 on the reference's x86-64 AVX2 build, vector_width = 0
constexpr int MAX_N = 4096;         // each dimension 2 .. MAX_N
constexpr int MAX_STAGES = 4;       // passes of a 1-D transform of N <= MAX_N whose factors are 8, 6, 4, 2
constexpr int LINE_THREADS = 1024;  // lanes of a line workgroup at most: one per radix-8 codelet of the batch, in whole waves
constexpr int LDS_COMPLEX = 8192;   // complex elements a line workgroup holds (per LDS buffer, before the pad)
constexpr int MAX_LINES = 16;       // lines per workgroup at most
constexpr int MIN_COLS = 8;         // columns per fft_cols workgroup at least, where LDS_COMPLEX allows: 64-byte runs
constexpr int WANT_GROUPS = 512;    // workgroups a pass is cut into before lines are batched: two per CU
constexpr int ONE_GROUP_BYTES = 16384;   // a transform whose N0 x N1 complex image fits this runs in one workgroup, one launch (52 KB of LDS with the exchange buffers)

enum Kind { K_C2C_FWD = 0, K_C2C_INV = 1, K_R2C = 2, K_C2R = 3 };
enum Mode { M_C2C_A, M_R2CS_A, M_C2RS_A, M_C2C_B, M_R2CS_B, M_C2RS_B, M_R2C_A, M_R2C_B, M_C2R_A, M_C2R_B };
// a mode's lines run along dimension 1 (columns: adjacent lines are adjacent in memory) or along dimension 0 (rows)
constexpr bool mode_cols(int m) { return m == M_C2C_B || m == M_R2CS_B || m == M_C2RS_B || m == M_R2C_A || m == M_C2R_B; }

struct FGeom {
    const float *in;
    float *out;
    float2 *scr;
    long irs, ors;   // row strides in floats
    int N0, N1, zw;
};

struct LinePlan {
    int N, n, sign, lines;
    int R[MAX_STAGES];
    float g_in[MAX_STAGES];        // pass i, S > 1: the table's gain and the factor of the r = 0 point
    float g_out[MAX_STAGES];       // the factor of the pass's results (the gain of a one-pass transform)
    const float2 *W[MAX_STAGES];   // device table of (R S, sign, g_in), null for S = 1
};

// ------------------------------------------------------------------------------------------------------------ complex arithmetic
__device__ __forceinline__ float2 c_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 c_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 c_mul(float2 a, float2 b) { return make_float2(dev::mulsub(a.x, b.x, a.y * b.y), dev::mad2(a.x, b.y, a.y, b.x)); }
__device__ __forceinline__ float2 c_scale(float2 a, float g) { return g == 1.0f ? a : make_float2(a.x * g, a.y * g); }
__device__ __forceinline__ float2 c_conj(float2 a) { return make_float2(a.x, -a.y); }
__device__ __forceinline__ float2 c_jsign(float2 a, int sign) { return sign > 0 ? make_float2(-a.y, a.x) : make_float2(a.y, -a.x); }   // a * j * sign
__device__ __forceinline__ float2 c_zipj(float2 x, float2 y) { return make_float2(x.x - y.y, x.y + y.x); }                            // x + j y

template<int R>
__device__ __forceinline__ void dft(float2 (&x)[R], int sign) {
    if constexpr (R == 2) {
        const float2 a = c_add(x[0], x[1]), b = c_sub(x[0], x[1]);
        x[0] = a, x[1] = b;
    } else if constexpr (R == 4) {
        const float2 t0 = c_add(x[0], x[2]), t2 = c_add(x[1], x[3]);
        const float2 t1 = c_sub(x[0], x[2]), t3 = c_jsign(c_sub(x[1], x[3]), sign);
        x[0] = c_add(t0, t2), x[2] = c_sub(t0, t2), x[1] = c_add(t1, t3), x[3] = c_sub(t1, t3);
    } else if constexpr (R == 6) {
        const float wi = (float)sign * 0.866025404f;
        const float2 W1 = make_float2(-0.5f, wi), W2 = make_float2(-0.5f, -wi);
        const float2 t0 = c_add(x[0], x[3]), t3 = c_sub(x[0], x[3]), t1 = c_add(x[1], x[4]), t4 = c_sub(x[1], x[4]);
        const float2 t2 = c_add(x[2], x[5]), t5 = c_sub(x[2], x[5]);
        x[0] = c_add(c_add(t0, t2), t1);
        x[4] = c_add(c_add(t0, c_mul(t2, W1)), c_mul(t1, W2));
        x[2] = c_add(c_add(t0, c_mul(t2, W2)), c_mul(t1, W1));
        x[3] = c_sub(c_add(t3, t5), t4);
        x[1] = c_sub(c_add(t3, c_mul(t5, W1)), c_mul(t4, W2));
        x[5] = c_sub(c_add(t3, c_mul(t5, W2)), c_mul(t4, W1));
    } else {
        static_assert(R == 8, "codelets: 2, 4, 6, 8");
        const float q = 0.70710678f;
        const float2 Wa = make_float2(q, (float)sign * q), Wb = make_float2(-q, (float)sign * q);
        float2 X[8], T[8];
        X[0] = c_add(x[0], x[4]), X[2] = c_add(x[2], x[6]);
        T[0] = c_add(X[0], X[2]), T[2] = c_sub(X[0], X[2]);
        X[1] = c_sub(x[0], x[4]), X[3] = c_jsign(c_sub(x[2], x[6]), sign);
        T[1] = c_add(X[1], X[3]), T[3] = c_sub(X[1], X[3]);
        X[4] = c_add(x[1], x[5]), X[6] = c_add(x[3], x[7]);
        T[4] = c_add(X[4], X[6]), T[6] = c_jsign(c_sub(X[4], X[6]), sign);
        X[5] = c_sub(x[1], x[5]), X[7] = c_jsign(c_sub(x[3], x[7]), sign);
        T[5] = c_mul(c_add(X[5], X[7]), Wa), T[7] = c_mul(c_sub(X[5], X[7]), Wb);
#pragma unroll
        for (int i = 0; i < 4; i++) x[i] = c_add(T[i], T[i + 4]), x[i + 4] = c_sub(T[i], T[i + 4]);
    }
}

// ------------------------------------------------------------------------------------------------------- the two ends of a pass
__device__ __forceinline__ int zx(int u, int zw) { return (u / zw) * zw * 2 + u % zw; }
__device__ __forceinline__ int ux(int n0, int zw) { return (n0 / (2 * zw)) * zw + n0 % zw; }

template<bool VEC>
__device__ __forceinline__ float2 in_c(const FGeom &g, int n0, int n1) {
    const float *p = g.in + (long)n1 * g.irs + 2 * (long)n0;
    if constexpr (VEC) return *reinterpret_cast<const float2 *>(p);
    else return make_float2(p[0], p[1]);
}
__device__ __forceinline__ float in_r(const FGeom &g, int n0, int n1) { return g.in[(long)n1 * g.irs + n0]; }
template<bool VEC>
__device__ __forceinline__ void out_c(const FGeom &g, int n0, int n1, float2 v) {
    float *p = g.out + (long)n1 * g.ors + 2 * (long)n0;
    if constexpr (VEC) *reinterpret_cast<float2 *>(p) = v;
    else p[0] = v.x, p[1] = v.y;
}
__device__ __forceinline__ void out_r(const FGeom &g, int n0, int n1, float v) { g.out[(long)n1 * g.ors + n0] = v; }

// r2c: unzipped(n0, m) from the zipped columns' transform scr[m][u]
__device__ __forceinline__ float2 r2c_unzipped(const FGeom &g, int n0, int m) {
    const int H0 = g.N0 / 2, u = ux(n0, g.zw);
    const float2 Z = g.scr[(long)m * H0 + u], Zs = g.scr[(long)((g.N1 - m) % g.N1) * H0 + u];
    if (n0 % (2 * g.zw) < g.zw) return make_float2(Z.x + Zs.x, Z.y - Zs.y);
    const float2 D = make_float2(Z.x - Zs.x, Z.y + Zs.y);
    return make_float2(D.y, -D.x);
}

// c2r: U(n0, m) of the rows' transform scr[m][n0]
__device__ __forceinline__ float2 c2r_u(const FGeom &g, int n0, int n1) {
    const int H1 = g.N1 / 2, m = n1 < H1 ? n1 : (g.N1 - n1) % g.N1;
    float2 U;
    if (m <= 0) U = make_float2(g.scr[n0].x, 0.0f);
    else if (m >= H1) U = make_float2(g.scr[n0].y, 0.0f);
    else U = g.scr[(long)m * g.N0 + n0];
    return n1 < H1 ? U : c_conj(U);
}

// point n of line l
template<int MODE, bool VEC>
__device__ __forceinline__ float2 load_elem(const FGeom &g, int l, int n) {
    if constexpr (MODE == M_C2C_A) return in_c<VEC>(g, n, l);
    else if constexpr (MODE == M_R2CS_A) return make_float2(in_r(g, n, l), 0.0f);
    else if constexpr (MODE == M_C2RS_A) return l <= g.N1 / 2 ? in_c<VEC>(g, n, l) : c_conj(in_c<VEC>(g, (g.N0 - n) % g.N0, g.N1 - l));
    else if constexpr (MODE == M_C2C_B || MODE == M_R2CS_B || MODE == M_C2RS_B) return g.scr[(long)n * g.N0 + l];
    else if constexpr (MODE == M_R2C_A) return make_float2(in_r(g, zx(l, g.zw), n), in_r(g, zx(l, g.zw) + g.zw, n));
    else if constexpr (MODE == M_R2C_B) {
        const float2 a = r2c_unzipped(g, n, l);
        return l > 0 ? a : make_float2(a.x, r2c_unzipped(g, n, g.N1 / 2).x);
    } else if constexpr (MODE == M_C2R_A) return l > 0 ? in_c<VEC>(g, n, l) : c_zipj(in_c<VEC>(g, n, 0), in_c<VEC>(g, n, g.N1 / 2));
    else return c_zipj(c2r_u(g, zx(l, g.zw), n), c2r_u(g, zx(l, g.zw) + g.zw, n));
}

// result k of line l.  M_R2C_B delivers through r2c_store() instead: its line 0 needs the whole line.
template<int MODE, bool VEC>
__device__ __forceinline__ void store_elem(const FGeom &g, int l, int k, float2 v) {
    if constexpr (MODE == M_C2C_A || MODE == M_R2CS_A || MODE == M_C2RS_A || MODE == M_C2R_A) g.scr[(long)l * g.N0 + k] = v;
    else if constexpr (MODE == M_C2C_B) out_c<VEC>(g, l, k, v);
    else if constexpr (MODE == M_R2CS_B) {
        if (k <= g.N1 / 2) out_c<VEC>(g, l, k, v);
    } else if constexpr (MODE == M_C2RS_B) out_r(g, l, k, v.x);
    else if constexpr (MODE == M_R2C_A) g.scr[(long)k * (g.N0 / 2) + l] = v;
    else if constexpr (MODE == M_C2R_B) out_r(g, zx(l, g.zw), k, v.x), out_r(g, zx(l, g.zw) + g.zw, k, v.y);
    else static_assert(MODE != M_R2C_B, "r2c_store");
}

// r2c, the way out of pass B: result k of line l, `at(i)` being result i of the same line.  Lines 1 .. N1/2 - 1 are rows of the output;
// line 0 is the transform D of DC + j Nyquist and unzips into row 0 and row N1/2 (Q) by the reference's six updates, which read D as
// the pass left it and, written per element with i = min(k, N0 - k):  Q[0] = (D[0].im, +0), D'[0] = (D[0].re, +0);
// q = (0.5f (D[i].im + D[N0-i].im), -(0.5f (D[i].re - D[N0-i].re))), d = (0.5f (D[i].re + D[N0-i].re), 0.5f (D[i].im - D[N0-i].im));
// Q[k] = q, D'[k] = d for k < N0/2 and their conjugates for k >= N0/2 (k = N0/2 is conjugated by updates 2 and 5 in place).
template<bool VEC, typename At>
__device__ __forceinline__ void r2c_store(const FGeom &g, int l, int k, At at) {
    if (l > 0) {
        out_c<VEC>(g, k, l, at(k));
        return;
    }
    const int H0 = g.N0 / 2, H1 = g.N1 / 2;
    if (k == 0) {
        const float2 D0 = at(0);
        out_c<VEC>(g, 0, 0, make_float2(D0.x, 0.0f));
        out_c<VEC>(g, 0, H1, make_float2(D0.y, 0.0f));
        return;
    }
    const int i = k <= H0 ? k : g.N0 - k;
    const float2 a = at(i), b = at(g.N0 - i);
    float2 q = make_float2(0.5f * (a.y + b.y), -(0.5f * (a.x - b.x)));
    float2 d = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y - b.y));
    if (k >= H0) q = c_conj(q), d = c_conj(d);
    out_c<VEC>(g, k, 0, d);
    out_c<VEC>(g, k, H1, q);
}

// ------------------------------------------------------------------------------------------------------------------- one codelet
// Codelet s of pass i of one line: `get(n)` is point n of the pass's input, `put(k, v)` takes result k.
template<int R, typename Get, typename Put>
__device__ __forceinline__ void codelet(const LinePlan &p, int i, int S, int s, Get get, Put put) {
    const int M = p.N / R;
    float2 v[R];
#pragma unroll
    for (int r = 0; r < R; r++) v[r] = get(s + r * M);
    if (S > 1) {
        const int t = s % S;
        v[0] = c_scale(v[0], p.g_in[i]);
#pragma unroll
        for (int r = 1; r < R; r++) v[r] = c_mul(v[r], p.W[i][r * t]);
    }
    dft<R>(v, p.sign);
    const int k0 = (s / S) * R * S + s % S;
#pragma unroll
    for (int r = 0; r < R; r++) put(k0 + r * S, c_scale(v[r], p.g_out[i]));
}

template<typename Get, typename Put>
__device__ __forceinline__ void codelet_any(const LinePlan &p, int i, int S, int s, Get get, Put put) {
    switch (p.R[i]) {
    case 2: codelet<2>(p, i, S, s, get, put); break;
    case 4: codelet<4>(p, i, S, s, get, put); break;
    case 6: codelet<6>(p, i, S, s, get, put); break;
    default: codelet<8>(p, i, S, s, get, put); break;
    }
}

__device__ __forceinline__ int lds_pad(int a) { return a + (a >> 3); }

// ------------------------------------------------------------------------------------------------------------- the line kernels
// One pass over lines [l0, l0 + nl) by the whole workgroup.  Pass 0 reads through load_elem, the last pass writes through store_elem,
// the passes between exchange through the two LDS buffers of `half` elements at `lds`; M_R2C_B's last pass ends in LDS too, because
// its line 0 leaves through r2c_store.  Ends behind a barrier.
template<int MODE, bool VEC>
__device__ __forceinline__ void line_pass(const FGeom &g, const LinePlan &p, int l0, int nl, float2 *lds, int half) {
    constexpr bool COL = mode_cols(MODE);
    const int N = p.N;
    auto at = [&](int b, int n) { return COL ? lds_pad(n * nl + b) : lds_pad(b * N + n); };   // element n of line b
    const bool last_in_lds = MODE == M_R2C_B;
    int S = 1;
    for (int i = 0; i < p.n; i++) {
        const int R = p.R[i], M = N / R, ncod = nl * M;
        const bool first = i == 0, last = i == p.n - 1 && !last_in_lds;
        const float2 *src = lds + ((i + 1) & 1) * half;
        float2 *dst = lds + (i & 1) * half;
        for (int c = threadIdx.x; c < ncod; c += blockDim.x) {
            const int b = COL ? c % nl : c / M, s = COL ? c / nl : c % M;
            auto get = [&](int n) { return first ? load_elem<MODE, VEC>(g, l0 + b, n) : src[at(b, n)]; };
            auto put = [&](int k, float2 v) {
                if constexpr (MODE != M_R2C_B) {
                    if (last) {
                        store_elem<MODE, VEC>(g, l0 + b, k, v);
                        return;
                    }
                }
                dst[at(b, k)] = v;
            };
            codelet_any(p, i, S, s, get, put);
        }
        S *= R;
        __syncthreads();
    }
    if constexpr (MODE == M_R2C_B) {
        const float2 *res = lds + ((p.n - 1) & 1) * half;
        for (int c = threadIdx.x; c < nl * N; c += blockDim.x) {
            const int b = c / N, k = c % N;
            r2c_store<VEC>(g, l0 + b, k, [&](int n) { return res[at(b, n)]; });
        }
    }
}

// A workgroup takes lines [l0, l0 + nl), nl <= B, of one pass.
template<int MODE, bool VEC>
__global__ __launch_bounds__(LINE_THREADS) void fft_lines(FGeom g, LinePlan p, int B) {
    extern __shared__ float2 lds[];
    const int l0 = blockIdx.x * B;
    line_pass<MODE, VEC>(g, p, l0, min(B, p.lines - l0), lds, lds_pad(B * p.N));
}

// pass B's mode of pass A's
constexpr int mode_b_of(int a) { return a == M_C2C_A ? M_C2C_B : a == M_R2CS_A ? M_R2CS_B : a == M_C2RS_A ? M_C2RS_B : a == M_R2C_A ? M_R2C_B : M_C2R_B; }

// The whole transform in one workgroup, one launch: both passes over all their lines, the scratch image in LDS in front of the two
// exchange buffers (N0 N1 elements, then two of pad(N0 N1)).  Chosen where N0 N1 complex elements fit ONE_GROUP_BYTES.
template<int MODE_A, bool VEC_A, bool VEC_B>
__global__ __launch_bounds__(LINE_THREADS) void fft_whole(FGeom g, LinePlan pa, LinePlan pb) {
    extern __shared__ float2 lds[];
    const int n = g.N0 * g.N1;
    g.scr = lds;
    line_pass<MODE_A, VEC_A>(g, pa, 0, pa.lines, lds + n, lds_pad(n));
    line_pass<mode_b_of(MODE_A), VEC_B>(g, pb, 0, pb.lines, lds + n, lds_pad(n));
}

// The second implementation: one thread per line, every pass in full before the next, through two line buffers of the scratch arena
// (element n of line l at buf[n * lines + l]).
template<int MODE>
__global__ __launch_bounds__(64) void fft_general(FGeom g, LinePlan p, float2 *buf0, float2 *buf1) {
    const int l = blockIdx.x * 64 + threadIdx.x;
    if (l >= p.lines) return;
    const long L = p.lines;
    const bool last_in_buf = MODE == M_R2C_B;
    int S = 1;
    for (int i = 0; i < p.n; i++) {
        const int R = p.R[i], M = p.N / R;
        const bool first = i == 0, last = i == p.n - 1 && !last_in_buf;
        const float2 *src = (i & 1) ? buf0 : buf1;
        float2 *dst = (i & 1) ? buf1 : buf0;
        for (int s = 0; s < M; s++) {
            auto get = [&](int n) { return first ? load_elem<MODE, false>(g, l, n) : src[n * L + l]; };
            auto put = [&](int k, float2 v) {
                if constexpr (MODE != M_R2C_B) {
                    if (last) {
                        store_elem<MODE, false>(g, l, k, v);
                        return;
                    }
                }
                dst[k * L + l] = v;
            };
            codelet_any(p, i, S, s, get, put);
        }
        S *= R;
    }
    if constexpr (MODE == M_R2C_B) {
        const float2 *res = ((p.n - 1) & 1) ? buf1 : buf0;
        for (int k = 0; k < p.N; k++) r2c_store<false>(g, l, k, [&](int n) { return res[n * L + l]; });
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
int radix_factor(int N, int *R) {   // fft.cpp:1066-1097; room for 16
    switch (N) {
    case 16: R[0] = 4, R[1] = 4; return 2;
    case 32: R[0] = 8, R[1] = 4; return 2;
    case 64: R[0] = 8, R[1] = 8; return 2;
    case 128: R[0] = 8, R[1] = 4, R[2] = 4; return 3;
    case 256: R[0] = 8, R[1] = 8, R[2] = 4; return 3;
    }
    int n = 0;
    for (int r : {8, 6, 4, 2})
        while (N > 0 && N % r == 0 && n < 15) R[n++] = r, N /= r;
    if (N != 1 || n == 0) R[n++] = N;
    return n;
}

bool size_ok(int N) {
    int R[16];
    if (N < 2 || N > MAX_N) return false;
    const int n = radix_factor(N, R);
    for (int i = 0; i < n; i++)
        if (R[i] != 8 && R[i] != 6 && R[i] != 4 && R[i] != 2) return false;
    return n <= MAX_STAGES;
}

int gcd(int x, int y) {
    while (y) {
        const int r = x % y;
        x = y, y = r;
    }
    return x;
}

// the zip width of r2c and c2r, 0 where the reference goes through c2c (skip_zip)
int zip_width(int kind, int N0, int N1) {
    if (kind == K_R2C) return (N0 < 2 * V || (N0 < 4 * V && N0 % (2 * V) != 0)) ? 0 : gcd(V, N0 / 2);
    if (kind == K_C2R) return N0 < 2 * V ? 0 : gcd(gcd(V, N1 / 2), N0 / 2);
    return 0;
}

struct TwiddleKey {
    int device, Na, Nb, sign;
    float gain;
};
static_assert(sizeof(TwiddleKey) <= DERIVED_KEY_BYTES, "key does not fit an entry");
DerivedCache g_twiddles(8);

// The 1-D plan of (N, sign, gain) over `lines` lines, without its tables; returns the complex elements its tables take and notes
// in off[] where each begins
size_t line_plan(int N, int sign, float gain, int lines, LinePlan *p, size_t *off) {
    int R[16];
    memset(p, 0, sizeof *p);
    p->N = N, p->sign = sign, p->lines = lines, p->n = radix_factor(N, R);
    size_t total = 0;
    int S = 1;
    for (int i = 0; i < p->n; i++) {
        p->R[i] = R[i];
        p->g_in[i] = i == 1 ? gain : 1.0f;
        p->g_out[i] = p->n == 1 ? gain : 1.0f;
        off[i] = total;
        if (S > 1) total += (size_t)R[i] * S;
        S *= R[i];
    }
    return total;
}

// The tables of the two passes of one call: one blob per (N of pass A, N of pass B, sign, gain of pass B), pass A's tables first (its
// gain is always 1), from the cache of derived data, or in `spare` (room for 4 MAX_N complex) where every slot is pinned.
int line_tables(void *uc, const DeviceCtx &ctx, LinePlan *a, LinePlan *b, const size_t *off_a, const size_t *off_b, size_t n_a, size_t n_b, float gain_b,
                float2 *spare, DerivedUse *use) {
    const size_t total = n_a + n_b;
    if (total == 0) return 0;
    TwiddleKey key;
    memset(&key, 0, sizeof key);
    key.device = ctx.device, key.Na = a->N, key.Nb = b->N, key.sign = a->sign, key.gain = gain_b;
    int r = derived_acquire(uc, ctx, g_twiddles, &key, sizeof key, total * sizeof(float2), true, use);
    if (r) return r;
    float2 *tab = use->ptr ? (float2 *)use->ptr : spare;
    LinePlan *pl[2] = {a, b};
    const size_t *offs[2] = {off_a, off_b}, base[2] = {0, n_a};
    if (use->fill) {
        std::vector<float> host(2 * total);
        for (int j = 0; j < 2; j++) {
            int S = 1;
            for (int i = 0; i < pl[j]->n; i++) {
                if (S > 1) hlmi_fft_twiddles(pl[j]->R[i] * S, pl[j]->sign, pl[j]->g_in[i], host.data() + 2 * (base[j] + offs[j][i]));
                S *= pl[j]->R[i];
            }
        }
        HLMI_HIP(uc, hipMemcpyAsync(tab, host.data(), total * sizeof(float2), hipMemcpyHostToDevice, ctx.stream));
        HLMI_HIP(uc, hipStreamSynchronize(ctx.stream));   // `host` goes out of scope
        if (use->ptr) use->filled(ctx.stream);
    }
    for (int j = 0; j < 2; j++) {
        int S = 1;
        for (int i = 0; i < pl[j]->n; i++) {
            if (S > 1) pl[j]->W[i] = tab + base[j] + offs[j][i];
            S *= pl[j]->R[i];
        }
    }
    return 0;
}

enum FftLaunch { F_ROWS, F_ROWS_ELEM, F_COLS, F_COLS_ELEM, F_GENERAL_A, F_GENERAL_B, F_WHOLE, F_WHOLE_ELEM };
const char *const fft_names[8] = {"fft_rows", "fft_rows_elem", "fft_cols", "fft_cols_elem", "fft_general_a", "fft_general_b", "fft_whole", "fft_whole_elem"};

struct PassPlan {
    int mode;
    FftLaunch launch;
    int lines_per_group;   // lines a workgroup holds
    int threads;           // lanes of a line workgroup: one per radix-8 codelet of its batch, in whole waves, LINE_THREADS at most
};
struct FftPlan {
    PassPlan a, b;
    bool whole;              // both passes in one launch of one workgroup (fft_whole), a.launch its name
    bool vec_a, vec_b;       // 8-byte accesses to the caller's complex input / output
    int whole_threads;
};

bool aligned8(const void *p, long row_stride) { return (uintptr_t)p % 8 == 0 && row_stride % 2 == 0; }

// lines per workgroup: as many as leave WANT_GROUPS workgroups, within LDS_COMPLEX and MAX_LINES; columns at least MIN_COLS
int lines_per_group(bool cols, int N, int lines) {
    const int cap = std::max(1, std::min(MAX_LINES, LDS_COMPLEX / N));
    int b = std::max(1, std::min(cap, lines / WANT_GROUPS));
    if (cols) b = std::max(b, std::min(cap, MIN_COLS));
    return std::min(b, lines);
}

// THE predicate.  The modes follow from the kind and the zip width; a pass runs on fft_rows or fft_cols as its lines lie, on the _elem
// variant where the complex buffer it touches (pass A: the input, pass B: the output) is not 8-byte aligned with even rows; the general
// kernel runs only where the caller asks for it by name (hlmi_fft2d_general).  A transform whose image fits ONE_GROUP_BYTES takes one
// launch of one workgroup instead of the two passes: fft_whole, or fft_whole_elem where either buffer is off 8 bytes.
FftPlan fft_plan(int kind, const FGeom &g, bool general_only) {
    const bool zip = g.zw > 0;
    FftPlan p;
    p.a.mode = kind == K_R2C ? (zip ? M_R2C_A : M_R2CS_A) : kind == K_C2R ? (zip ? M_C2R_A : M_C2RS_A) : M_C2C_A;
    p.b.mode = kind == K_R2C ? (zip ? M_R2C_B : M_R2CS_B) : kind == K_C2R ? (zip ? M_C2R_B : M_C2RS_B) : M_C2C_B;
    const bool vec_a = kind == K_R2C || aligned8(g.in, g.irs), vec_b = kind == K_C2R || aligned8(g.out, g.ors);
    PassPlan *pp[2] = {&p.a, &p.b};
    for (int i = 0; i < 2; i++) {
        const bool cols = mode_cols(pp[i]->mode), vec = i ? vec_b : vec_a;
        const bool along0 = !cols;
        const int N = along0 ? g.N0 : g.N1;
        int lines;
        switch (pp[i]->mode) {
        case M_R2C_A: case M_C2R_B: lines = g.N0 / 2; break;
        case M_R2C_B: case M_C2R_A: lines = g.N1 / 2; break;
        default: lines = along0 ? g.N1 : g.N0; break;
        }
        pp[i]->launch = general_only ? (i ? F_GENERAL_B : F_GENERAL_A) : cols ? (vec ? F_COLS : F_COLS_ELEM) : (vec ? F_ROWS : F_ROWS_ELEM);
        pp[i]->lines_per_group = general_only ? 1 : lines_per_group(cols, N, lines);
        pp[i]->threads = std::min(LINE_THREADS, std::max(64, (pp[i]->lines_per_group * N / 8 + 63) / 64 * 64));
    }
    p.vec_a = vec_a, p.vec_b = vec_b;
    p.whole = !general_only && (size_t)g.N0 * g.N1 * sizeof(float2) <= (size_t)ONE_GROUP_BYTES;
    p.whole_threads = std::min(LINE_THREADS, std::max(64, (g.N0 * g.N1 / 8 + 63) / 64 * 64));
    if (p.whole) p.a.launch = p.b.launch = vec_a && vec_b ? F_WHOLE : F_WHOLE_ELEM;
    return p;
}

// a mode whose pass touches a complex buffer of the caller's: only these have an _elem variant
constexpr bool mode_has_elem(int m) { return !(m == M_R2C_A || m == M_R2CS_A || m == M_C2R_B || m == M_C2RS_B); }
constexpr size_t MAX_LDS_BYTES = 2 * (size_t)(LDS_COMPLEX + LDS_COMPLEX / 8) * sizeof(float2);   // what a line workgroup asks for at most

// the dynamic-LDS ceiling of a kernel instantiation, raised once per device (`done`: one bit per device)
template<typename K>
int raise_lds_once(void *uc, K kernel, std::atomic<uint64_t> &done) {
    int dev = 0;
    HLMI_HIP(uc, hipGetDevice(&dev));
    const uint64_t bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return 0;
    HLMI_HIP(uc, hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)MAX_LDS_BYTES));
    done.fetch_or(bit, std::memory_order_release);
    return 0;
}

template<int MODE>
int launch_pass(void *uc, hipStream_t st, const FGeom &g, const LinePlan &lp, const PassPlan &pp, float2 *buf0, float2 *buf1) {
    const char *name = fft_names[pp.launch];
    if (pp.launch == F_GENERAL_A || pp.launch == F_GENERAL_B) {
        HLMI_LAUNCH(uc, name, st, fft_general<MODE>, dim3((unsigned)((lp.lines + 63) / 64)), dim3(64), 0, g, lp, buf0, buf1);
        return 0;
    }
    const int B = pp.lines_per_group;
    const int nbuf = std::min(2, MODE == M_R2C_B ? lp.n : lp.n - 1);
    const size_t lds = (size_t)nbuf * (size_t)(B * lp.N + (B * lp.N >> 3)) * sizeof(float2);
    const dim3 grid((unsigned)((lp.lines + B - 1) / B));
    const bool vec = pp.launch == F_ROWS || pp.launch == F_COLS;
    return with_flags([&](auto v) {
        constexpr bool VEC = decltype(v)::value || !mode_has_elem(MODE);   // (no second instantiation where the flag changes nothing)
        static std::atomic<uint64_t> raised{0};
        if (lds > 48 * 1024) {
            const int e = raise_lds_once(uc, fft_lines<MODE, VEC>, raised);
            if (e) return e;
        }
        HLMI_LAUNCH(uc, name, st, (fft_lines<MODE, VEC>), grid, dim3((unsigned)pp.threads), lds, g, lp, B);
        return 0;
    }, vec);
}

template<int MODE_A>
int launch_whole_mode(void *uc, hipStream_t st, const FGeom &g, const LinePlan &la, const LinePlan &lb, const FftPlan &plan) {
    const char *name = fft_names[plan.a.launch];
    const size_t n = (size_t)g.N0 * g.N1, lds = (n + 2 * (n + (n >> 3))) * sizeof(float2);
    return with_flags([&](auto va, auto vb) {
        constexpr bool VA = decltype(va)::value || !mode_has_elem(MODE_A), VB = decltype(vb)::value || !mode_has_elem(mode_b_of(MODE_A));
        static std::atomic<uint64_t> raised{0};
        if (lds > 48 * 1024) {
            const int e = raise_lds_once(uc, fft_whole<MODE_A, VA, VB>, raised);
            if (e) return e;
        }
        HLMI_LAUNCH(uc, name, st, (fft_whole<MODE_A, VA, VB>), dim3(1), dim3((unsigned)plan.whole_threads), lds, g, la, lb);
        return 0;
    }, plan.vec_a, plan.vec_b);
}

int launch_whole(void *uc, hipStream_t st, const FGeom &g, const LinePlan &la, const LinePlan &lb, const FftPlan &plan) {
    switch (plan.a.mode) {
    case M_C2C_A: return launch_whole_mode<M_C2C_A>(uc, st, g, la, lb, plan);
    case M_R2CS_A: return launch_whole_mode<M_R2CS_A>(uc, st, g, la, lb, plan);
    case M_C2RS_A: return launch_whole_mode<M_C2RS_A>(uc, st, g, la, lb, plan);
    case M_R2C_A: return launch_whole_mode<M_R2C_A>(uc, st, g, la, lb, plan);
    default: return launch_whole_mode<M_C2R_A>(uc, st, g, la, lb, plan);
    }
}

int launch_mode(void *uc, hipStream_t st, const FGeom &g, const LinePlan &lp, const PassPlan &pp, float2 *buf0, float2 *buf1) {
    switch (pp.mode) {
    case M_C2C_A: return launch_pass<M_C2C_A>(uc, st, g, lp, pp, buf0, buf1);
    case M_R2CS_A: return launch_pass<M_R2CS_A>(uc, st, g, lp, pp, buf0, buf1);
    case M_C2RS_A: return launch_pass<M_C2RS_A>(uc, st, g, lp, pp, buf0, buf1);
    case M_C2C_B: return launch_pass<M_C2C_B>(uc, st, g, lp, pp, buf0, buf1);
    case M_R2CS_B: return launch_pass<M_R2CS_B>(uc, st, g, lp, pp, buf0, buf1);
    case M_C2RS_B: return launch_pass<M_C2RS_B>(uc, st, g, lp, pp, buf0, buf1);
    case M_R2C_A: return launch_pass<M_R2C_A>(uc, st, g, lp, pp, buf0, buf1);
    case M_R2C_B: return launch_pass<M_R2C_B>(uc, st, g, lp, pp, buf0, buf1);
    case M_C2R_A: return launch_pass<M_C2R_A>(uc, st, g, lp, pp, buf0, buf1);
    default: return launch_pass<M_C2R_B>(uc, st, g, lp, pp, buf0, buf1);
    }
}

const ArgTable t_fwd_r2c = {"fft_forward_r2c", {in_buf("input", T_F32, 3), out_buf("output", T_F32, 3)}};
const ArgTable t_inv_c2r = {"fft_inverse_c2r", {in_buf("input", T_F32, 3), out_buf("output", T_F32, 3)}};
const ArgTable t_fwd_c2c = {"fft_forward_c2c", {in_buf("input", T_F32, 3), out_buf("output", T_F32, 3)}};
const ArgTable t_inv_c2c = {"fft_inverse_c2c", {in_buf("input", T_F32, 3), out_buf("output", T_F32, 3)}};

// [first, last) floats of the rows x N0 x comps block a buffer describes, in host or in device memory
bool overlap(const halide_buffer_t *a, long na, const halide_buffer_t *b, long nb) {
    auto hit = [&](uintptr_t pa, uintptr_t pb) {
        if (!pa || !pb) return false;
        return pa < pb + 4 * (uintptr_t)nb && pb < pa + 4 * (uintptr_t)na;
    };
    return hit((uintptr_t)a->host, (uintptr_t)b->host) || hit((uintptr_t)a->device, (uintptr_t)b->device);
}

int entry(const ArgTable &table, int kind, int N0, int N1, float gain, halide_buffer_t *input, halide_buffer_t *output, bool general_only) {
    void *uc = nullptr;
    BufArg args[2];
    table.bufs(args, {input, output});
    int r = check_not_null(uc, args, 2);
    if (r) return r;
    if (kind < K_C2C_FWD || kind > K_C2R) return report(uc, halide_error_code_constraint_violated, "Constraint violated: fft kind (%d) must be 0 .. 3", kind);
    const bool real_kind = kind == K_R2C || kind == K_C2R;
    if (!size_ok(N0) || !size_ok(N1) || (real_kind && ((N0 | N1) & 1)))
        return report(uc, halide_error_code_constraint_violated,
                      "Constraint violated: fft sizes (%d, %d) must be 2 .. %d with radix factors 8, 6, 4 and 2%s", N0, N1, MAX_N, real_kind ? ", and even" : "");
    if ((r = check_type_and_dims(uc, args, 2))) return r;
    const int comps[2] = {kind == K_R2C ? 1 : 2, kind == K_C2R ? 1 : 2};
    const int rows[2] = {kind == K_C2R ? N1 / 2 + 1 : N1, kind == K_R2C ? N1 / 2 + 1 : N1};
    if (any_bounds_query(args, 2)) {
        for (int i = 0; i < 2; i++) {
            halide_buffer_t *b = args[i].buf;
            if (buffer_is_real(b)) continue;
            b->dim[0] = {0, N0, comps[i], 0};
            b->dim[1] = {0, rows[i], comps[i] * N0, 0};
            b->dim[2] = {0, comps[i], 1, 0};
        }
        return 0;
    }
    char what[32], expect[64];
    for (int i = 0; i < 2; i++) {
        const BufArg &a = args[i];
        const halide_buffer_t *b = a.buf;
        snprintf(what, sizeof what, "%s.stride.0", a.name);
        check_equal(uc, what, b->dim[0].stride, i ? "output components" : "input components", comps[i]);
        snprintf(what, sizeof what, "%s.stride.2", a.name);
        check_equal(uc, what, b->dim[2].stride, "1", 1);
        snprintf(what, sizeof what, "%s.min.2", a.name);
        check_equal(uc, what, b->dim[2].min, "0", 0);
        snprintf(what, sizeof what, "%s.extent.2", a.name);
        check_equal(uc, what, b->dim[2].extent, i ? "output components" : "input components", comps[i]);
        snprintf(what, sizeof what, "%s.stride.1", a.name);
        snprintf(expect, sizeof expect, "max(%s.stride.1, components * size0)", a.name);
        check_equal(uc, what, b->dim[1].stride, expect, std::max(b->dim[1].stride, comps[i] * N0));
        if (i) {   // the output is exactly the transform's domain
            for (int d = 0; d < 2; d++) {
                snprintf(what, sizeof what, "%s.min.%d", a.name, d);
                check_equal(uc, what, b->dim[d].min, "0", 0);
                snprintf(what, sizeof what, "%s.extent.%d", a.name, d);
                check_equal(uc, what, b->dim[d].extent, d ? "output rows" : "size0", d ? rows[1] : N0);
            }
        }
        for (int d = 0; d < 3; d++) {
            if (b->dim[d].extent < 0)
                return report(uc, halide_error_code_buffer_extents_negative, "The extents for buffer %s dimension %d is negative (%d)", a.name, d, b->dim[d].extent);
            if ((int64_t)b->dim[d].extent * b->dim[d].stride > 0x7fffffffLL)
                return report(uc, halide_error_code_buffer_allocation_too_large, "Total allocation for buffer %s exceeds the maximum size", a.name);
        }
        check_covers(uc, a, 0, 0, N0);
        check_covers(uc, a, 1, 0, rows[i]);
    }
    if ((r = checks_done(uc))) return r;
    // the blocks the call reads and writes, from element (0, 0, 0)
    const long in_off = -(long)input->dim[1].min * input->dim[1].stride - (long)input->dim[0].min * input->dim[0].stride;
    const long in_n = (long)(rows[0] - 1) * input->dim[1].stride + (long)comps[0] * N0, out_n = (long)(rows[1] - 1) * output->dim[1].stride + (long)comps[1] * N0;
    {
        halide_buffer_t in0 = *input;
        if (in0.host) in0.host += 4 * in_off;
        if (in0.device) in0.device += 4 * in_off;
        if (overlap(output, out_n, &in0, in_n)) return report(uc, halide_error_code_constraint_violated, "Constraint violated: output may not alias input");
    }
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, 2))) return r;

    FGeom g;
    g.in = dev_ptr<float>(input) + in_off, g.out = dev_ptr<float>(output), g.irs = input->dim[1].stride, g.ors = output->dim[1].stride;
    g.N0 = N0, g.N1 = N1, g.zw = zip_width(kind, N0, N1);
    const FftPlan plan = fft_plan(kind, g, general_only);
    // arena: the scratch image | a spare table blob | the general path's two line buffers
    const size_t n_scr = (size_t)N0 * N1, n_spare = 4 * (size_t)MAX_N, n_buf = general_only ? n_scr : 0;
    void *ws = nullptr;
    if ((r = get_workspace(uc, ctx, sizeof(float2) * (n_scr + n_spare + 2 * n_buf), &ws))) return r;
    g.scr = (float2 *)ws;
    float2 *spare = g.scr + n_scr, *buf0 = spare + n_spare, *buf1 = buf0 + n_buf;

    const int sign = (kind == K_C2C_INV || kind == K_C2R) ? 1 : -1;
    const bool a_along0 = !mode_cols(plan.a.mode);
    const int lines_a = plan.a.mode == M_R2C_A ? N0 / 2 : plan.a.mode == M_C2R_A ? N1 / 2 : N1;
    const int lines_b = plan.b.mode == M_R2C_B ? N1 / 2 : plan.b.mode == M_C2R_B ? N0 / 2 : N0;
    const float gain_b = plan.b.mode == M_R2C_B ? gain * 0.5f : gain;
    LinePlan la, lb;
    size_t off_a[MAX_STAGES], off_b[MAX_STAGES];
    const size_t n_a = line_plan(a_along0 ? N0 : N1, sign, 1.0f, lines_a, &la, off_a);
    const size_t n_b = line_plan(a_along0 ? N1 : N0, sign, gain_b, lines_b, &lb, off_b);
    DerivedUse use;
    if ((r = line_tables(uc, ctx, &la, &lb, off_a, off_b, n_a, n_b, gain_b, spare, &use))) return r;
    // pass A reads the input and writes the scratch image (half the size where columns are zipped), pass B reads that and writes the output
    const double in_bytes = 4.0 * comps[0] * N0 * rows[0], out_bytes = 4.0 * comps[1] * N0 * rows[1], scr_bytes = 8.0 * n_scr / (g.zw > 0 ? 2 : 1);
    if (plan.whole) {
        timing_note_bytes(in_bytes + out_bytes);
        if ((r = launch_whole(uc, ctx.stream, g, la, lb, plan))) return r;
    } else {
        timing_note_bytes(in_bytes + scr_bytes);
        if ((r = launch_mode(uc, ctx.stream, g, la, plan.a, buf0, buf1))) return r;
        timing_note_bytes(scr_bytes + out_bytes);
        if ((r = launch_mode(uc, ctx.stream, g, lb, plan.b, buf0, buf1))) return r;
    }
    if (use.ptr) use.done(ctx.stream);
    mark_output_written(output);
    return 0;
}

const ArgTable &table_of(int kind) { return kind == K_R2C ? t_fwd_r2c : kind == K_C2R ? t_inv_c2r : kind == K_C2C_INV ? t_inv_c2c : t_fwd_c2c; }

}  // namespace

// The host function behind every twiddle table, exported so that the checker builds its tables with it (tests/fft_checker.py):
// out[2 k], out[2 k + 1] = (cosf(a_k), sinf(a_k)) * gain, a_k = ((float)(sign * 2) * (float)M_PI * (float)k) / (float)n in f32, k < n;
// no multiplication where gain == 1.0f.
extern "C" void hlmi_fft_twiddles(int32_t n, int32_t sign, float gain, float *out) {
    const float kPi = (float)3.14159265358979310000;
    const float two_pi = (float)(sign * 2) * kPi;
    for (int k = 0; k < n; k++) {
        const float ang = (two_pi * (float)k) / (float)n;
        float c = cosf(ang), s = sinf(ang);
        if (gain != 1.0f) c = c * gain, s = s * gain;
        out[2 * k] = c, out[2 * k + 1] = s;
    }
}

// radix_factor as the library holds it: the factors into R (room for 16), their number returned; and the size predicate of one dimension
extern "C" int hlmi_fft_radix_factor(int32_t N, int32_t *R) { return radix_factor(N, R); }
extern "C" int hlmi_fft_size_ok(int32_t N) { return size_ok(N) ? 1 : 0; }

// Internal entry points (hlmi_internal.h): the generator instantiated at other sizes and gains, and the second implementation.
extern "C" int hlmi_fft2d(int32_t kind, int32_t N0, int32_t N1, float gain, halide_buffer_t *input, halide_buffer_t *output) {
    return entry(table_of(kind), kind, N0, N1, gain, input, output, false);
}
extern "C" int hlmi_fft2d_general(int32_t kind, int32_t N0, int32_t N1, float gain, halide_buffer_t *input, halide_buffer_t *output) {
    return entry(table_of(kind), kind, N0, N1, gain, input, output, true);
}

extern "C" int fft_forward_r2c(halide_buffer_t *input, halide_buffer_t *output) { return hlmi_fft2d(K_R2C, 16, 16, 1.0f / 256.0f, input, output); }
HLMI_ENTRY(fft_forward_r2c, t_fwd_r2c.md)
extern "C" int fft_inverse_c2r(halide_buffer_t *input, halide_buffer_t *output) { return hlmi_fft2d(K_C2R, 16, 16, 1.0f, input, output); }
HLMI_ENTRY(fft_inverse_c2r, t_inv_c2r.md)
extern "C" int fft_forward_c2c(halide_buffer_t *input, halide_buffer_t *output) { return hlmi_fft2d(K_C2C_FWD, 16, 16, 1.0f / 256.0f, input, output); }
HLMI_ENTRY(fft_forward_c2c, t_fwd_c2c.md)
extern "C" int fft_inverse_c2c(halide_buffer_t *input, halide_buffer_t *output) { return hlmi_fft2d(K_C2C_INV, 16, 16, 1.0f, input, output); }
HLMI_ENTRY(fft_inverse_c2c, t_inv_c2c.md)
