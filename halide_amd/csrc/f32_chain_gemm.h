// f32_chain_gemm.h — the exact f32 MFMA tile loop: one workgroup's T x T tile of sum_k X[k][x] * Y[k][y] as the k-ordered fmaf chain,
// shared by mat_mul.hip (mm_mfma) and linear_algebra.hip (sgemm_mfma).  Nobody launches it: each user is a __global__ wrapper that
// names its geometry and what to do with a finished sum.  Also the C/D-map row of the 32 x 32 MFMA for every file that walks it.
//
// `v_mfma_f32_32x32x2_f32` evaluates D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)), a k-ordered fmaf chain with one rounding per product,
// so feeding k upward reproduces acc_{k+1} = fmaf(X[k][x], Y[k][y], acc_k), acc_0 = +0.0f, bit for bit at the f32 matrix rate.
//   D[i][j]: i = y, j = x = lane & 31, so that a half-wave stores 128 contiguous bytes; register r of a lane holds row
//   cd_row(r) + 4 * (lane >> 5), column lane & 31 (the C/D map).  MFMA operand "A"[i][k] is Y, operand "B"[k][j] is X.
//   Both operands lie k-major in LDS.  One that is contiguous along its tile dimension in memory is copied straight (float4 stores,
//   pitch T); one that is contiguous along k is TURNED k-major on the way in (scalar stores, odd pitch T + 1).
//   workgroup = 4 waves = T x T outputs, wave = W x W accumulators of 32 x 32, T = 64 W.  K cannot be split, so output tiles are the
//   only parallelism; which W a call gets is its user's plan.
// Chunk schedule.  A chunk is KCH = KC / W k steps (the same LDS and the same loads per thread for either W).  One accumulator chain
//   per wave hides nothing, so the global loads of the next TWO chunks are in flight during this chunk's MFMAs and LDS is
//   double-buffered: chunk c is computed from buffer c & 1 while the loads of chunk c + 2 are issued and, after the MFMAs, chunk c + 1
//   (loaded one whole chunk earlier) goes to the other buffer, last read in iteration c - 1 behind that iteration's barrier: one
//   barrier per chunk.  The load of chunk c + 2 is unconditional; past the end it fetches the last chunk again, which is never staged
//   into a buffer that is read.
// Named registers.  The two chunks in flight are eight named float4 (set a: even chunks, set b: odd chunks) handed to the lambdas by
//   reference, and the chunk loop is unrolled by two so that each set keeps its role.  Arrays of them, or a struct of them, end up in
//   scratch.
// A whole chunk reads every operand from LDS first, so that the reads of later steps are in flight under the MFMAs of earlier ones (a
//   wave that is alone on its SIMD has nothing else to hide them); the sched_barrier between the reads and the MFMAs keeps the
//   scheduler from sinking each read to its MFMA again to save registers.
// FAST = false: scalar loads from clamped addresses (what lies past the matrix is loaded from its last row / column, computed in
//   padded rows and columns and never stored), and a last chunk of K % KCH steps: its pairs run as MFMAs, and the last step of an odd
//   K, which has no partner, as a VALU fmaf on each accumulator register with its operands picked through the C/D map.  No zero-padded
//   step exists in either dimension of k: fmaf(0, 0, -0.0f) is +0.0f, so one would turn a chain that ends in -0 into +0.
// FAST = true is its user's promise: M, N multiples of T, K one of KC, every address and stride a multiple of 16 bytes: float4 loads.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

namespace hlmi {
namespace chain {

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int KC = 32;   // k steps per staged chunk of the small tile (W = 1); the large tile (W = 2) stages KC / 2

// C/D map of v_mfma_f32_32x32x2_f32: accumulator register r of a lane holds row cd_row(r) + 4 * (lane >> 5), column lane & 31
constexpr int cd_row(int r) { return (r & 3) + 8 * (r >> 2); }

// One workgroup (256 threads, blockIdx = tile) of the product.  x is the MFMA's column, contiguous in the result; G has the operands
// as X = (A, sa) and Y = (B, sb): X[k][x] = A[k * sa + x] or, XTURN, A[x * sa + k]; Y[k][y] = B[k * sb + y] or, YTURN, B[y * sb + k].
// P names the rest: P::M(g), P::N(g), P::K(g) the extents of x, y and k, and P::store(g, x, y, sum), called for every output of the
// tile that lies inside the result.  g comes BY VALUE, as a kernel's own argument does: the compiler optimises this function before
// it inlines it, and behind a reference it cannot know that no store of the loop changes g (profiles/NOTES.md has the figures).
template<int W, bool FAST, bool XTURN, bool YTURN, typename P, typename G>
__device__ __forceinline__ void tile(const G g) {
    constexpr int T = 64 * W;          // tile edge
    constexpr int KCH = KC / W;        // k per chunk
    constexpr int XP = XTURN ? T + 1 : T, YP = YTURN ? T + 1 : T;   // LDS pitches: conflict-light scalar stores / float4 stores
    constexpr int TQ = T / 4;          // float4 per LDS row of a straight operand
    constexpr int KQ = KCH / 4;        // float4 per tile row of a turned operand
    static_assert(KCH * T / 4 == 512, "two float4 per thread and operand");
    __shared__ __attribute__((aligned(16))) float sX[2][KCH * XP];  // [k][x]
    __shared__ __attribute__((aligned(16))) float sY[2][KCH * YP];  // [k][y]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wy = (wave >> 1) * 32 * W, wx = (wave & 1) * 32 * W;   // wave tile origin inside the workgroup tile
    const int x0 = blockIdx.x * T, y0 = blockIdx.y * T;
    const int K = P::K(g);

    // float4 number f of a chunk of one operand: `t0` the tile's origin in the operand's tile dimension, `tn` that dimension's extent
    auto load_op = [&](auto turned, const float *base, long stride, int t0, int tn, int k0, int f, float4 &p) {
        if constexpr (decltype(turned)::value) {
            const int tt = f / KQ, kk = 4 * (f % KQ);   // tile row tt, first k
            if constexpr (FAST) {
                p = *reinterpret_cast<const float4 *>(base + (long)(t0 + tt) * stride + k0 + kk);
            } else {
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

    // two float4 of each operand per thread and chunk: float4 number f = tid and tid + 256 of the chunk
    float4 ax0, ax1, ay0, ay1, bx0, bx1, by0, by1;
    auto load = [&](int k0, float4 &rx0, float4 &rx1, float4 &ry0, float4 &ry1) {
        load_op(xturn, g.A, g.sa, x0, P::M(g), k0, tid, rx0);
        load_op(yturn, g.B, g.sb, y0, P::N(g), k0, tid, ry0);
        load_op(xturn, g.A, g.sa, x0, P::M(g), k0, tid + 256, rx1);
        load_op(yturn, g.B, g.sb, y0, P::N(g), k0, tid + 256, ry1);
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

    const int nchunk = (K + KCH - 1) / KCH;
    auto chunk = [&](int c, float4 &nx0, float4 &nx1, float4 &ny0, float4 &ny1, const float4 &sx0, const float4 &sx1, const float4 &sy0, const float4 &sy1) {
        const int buf = c & 1;
        load(min(c + 2, nchunk - 1) * KCH, nx0, nx1, ny0, ny1);
        const float *pa = sY[buf] + (lane >> 5) * YP + wy + (lane & 31);
        const float *pb = sX[buf] + (lane >> 5) * XP + wx + (lane & 31);
        const int kc = FAST ? KCH : min(KCH, K - c * KCH);   // k steps this chunk holds
        if (FAST || kc == KCH) {
            float av[KCH / 2][W], bv[KCH / 2][W];
#pragma unroll
            for (int s = 0; s < KCH / 2; s++) {
#pragma unroll
                for (int a = 0; a < W; a++) av[s][a] = pa[2 * s * YP + 32 * a];
#pragma unroll
                for (int b = 0; b < W; b++) bv[s][b] = pb[2 * s * XP + 32 * b];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s = 0; s < KCH / 2; s++)
#pragma unroll
                for (int a = 0; a < W; a++)
#pragma unroll
                    for (int b = 0; b < W; b++) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s][a], bv[s][b], acc[a][b], 0, 0, 0);
        } else {
#pragma unroll 1
            for (int s = 0; s < kc / 2; s++) step(pa, pb, s);
            if (kc & 1) {   // the odd last step, on the VALU
                const float *ky = sY[buf] + (kc - 1) * YP + wy + 4 * (lane >> 5);
                const float *kx = sX[buf] + (kc - 1) * XP + wx + (lane & 31);
#pragma unroll
                for (int a = 0; a < W; a++)
#pragma unroll
                    for (int b = 0; b < W; b++) {
                        const float xv = kx[32 * b];
#pragma unroll
                        for (int r = 0; r < 16; r++) acc[a][b][r] = __builtin_fmaf(xv, ky[32 * a + cd_row(r)], acc[a][b][r]);
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

    // ---- epilogue: x = lane & 31 contiguous
#pragma unroll
    for (int a = 0; a < W; a++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int y = y0 + wy + 32 * a + cd_row(r) + 4 * (lane >> 5);
#pragma unroll
            for (int b = 0; b < W; b++) {
                const int x = x0 + wx + 32 * b + (lane & 31);
                if (FAST || (y < P::N(g) && x < P::M(g))) P::store(g, x, y, acc[a][b][r]);
            }
        }
}

}  // namespace chain
}  // namespace hlmi
