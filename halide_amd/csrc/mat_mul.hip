// mat_mul.hip — gfx950 implementation of the reference's cuda_mat_mul AOT pipeline (square f32 matrix product).
//
// Algorithm: apps/cuda_mat_mul/mat_mul_generator.cpp:27-32; boundary: `int mat_mul(halide_buffer_t *A,
// halide_buffer_t *B, halide_buffer_t *out)` (:18-21, :74), built with size = 1024 (apps/cuda_mat_mul/CMakeLists.txt).
//   out(x, y) = acc_size,  acc_0 = +0.0f,  acc_{r+1} = fmaf(A(x, r), B(r, y), acc_r),  r = 0 .. size - 1
// Dimension 0 is innermost: in memory out[y][x] = sum_r B[y][r] * A[r][x], i.e. the row-major product B @ A.  The chain is the
// contract in BOTH canonical float forms: k runs strictly upward for every output, no step is padded with
// zeros (fmaf(0, 0, -0.0f) is +0.0f), subnormals are kept.
//
// Exact MFMA path: `v_mfma_f32_32x32x2_f32` evaluates D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)), a k-ordered fmaf chain with one
// rounding per product (as conv_layer.hip), so feeding k upward reproduces the chain bit for bit at the f32 matrix rate.
//   D[i][j]: i = y, j = x = lane & 31, so that a half-wave stores 128 contiguous bytes (C/D map: row = (reg & 3) + 8 * (reg >> 2)
//   + 4 * (lane >> 5), col = lane & 31).  MFMA operand "A"[i][k] is B(r, y) = B[y][r]: r contiguous in memory, turned k-major on
//   the way into LDS (sY, odd pitch).  MFMA operand "B"[k][j] is A(x, r) = A[r][x]: x contiguous, copied straight (sX).
//   workgroup = 4 waves = TILE x TILE outputs, wave = W x W accumulators of 32 x 32, W = TILE / 64.  K cannot be split, so output
//   tiles are the only parallelism: mm_tile() picks the smallest tile while that is what it takes to have a wave on every SIMD.
//   Latency: one accumulator chain per wave hides nothing, so the global loads of the next two chunks are in flight during this
//   chunk's MFMAs and LDS is double-buffered: one barrier per chunk.
// Three launches (mm_plan() is the one place that chooses):
//   mat_mul_mfma       size a multiple of the tile and of KC; every device address and row stride a multiple of 16 bytes: float4 loads
//   mat_mul_mfma_edge  the same template with scalar loads from clamped addresses (padded rows and columns are computed and never
//                      stored), a last chunk of size % KC steps, and for an odd size the last step as a VALU fmaf on the
//                      accumulator registers through the C/D map: no padded k step exists
//   mat_mul_general    one thread per output, a plain fmaf loop (hlmi_mat_mul_general only)
#include "hlmi_internal.h"

using namespace hlmi;

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int MAX_SIZE = 8192;     // hlmi_mat_mul_sized takes 1 .. MAX_SIZE
constexpr int SMALL_TILE = 64;     // workgroup tile with one accumulator per wave
constexpr int LARGE_TILE = 128;    // workgroup tile with 2 x 2 accumulators per wave
constexpr int LARGE_FROM = 2048;   // (LARGE_FROM / LARGE_TILE)^2 workgroups x 4 waves = 1024 waves = 256 CUs x 4 SIMDs
constexpr int KC = 32;             // k steps per staged chunk of the small tile; the large tile stages KC / 2 (same LDS, same loads per thread)

struct MGeom {
    const float *A, *B;
    float *out;
    int n;
    long sa, sb, so;   // row strides in elements
};

// The wave tile follows from the size: the large tile (LDS reuse 2 x) only where it still leaves a wave for every SIMD.
constexpr int mm_tile(int size) { return size >= LARGE_FROM ? LARGE_TILE : SMALL_TILE; }

template<int W, bool FAST>
__global__ __launch_bounds__(256) void mm_mfma(MGeom g) {
    constexpr int T = 64 * W;          // tile edge
    constexpr int KCH = KC / W;        // k per chunk
    constexpr int XP = T, YP = T + 1;  // LDS pitches: float4 stores / conflict-light scalar stores
    constexpr int XQ = T / 4;          // float4 per sX row
    constexpr int YQ = KCH / 4;        // float4 per tile row of B
    static_assert(KCH * T / 4 == 512, "two float4 per thread and operand");
    __shared__ float sX[2][KCH * XP];  // [k][x] = A(x0 + x, k0 + k)
    __shared__ float sY[2][KCH * YP];  // [k][y] = B(k0 + k, y0 + y)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wy = (wave >> 1) * 32 * W, wx = (wave & 1) * 32 * W;   // wave tile origin inside the workgroup tile
    const int x0 = blockIdx.x * T, y0 = blockIdx.y * T;
    const int n = g.n;

    // Two chunks in flight: two float4 of each operand per thread and chunk, float4 number f = tid and tid + 256 of the chunk
    float4 ax0, ax1, ay0, ay1, bx0, bx1, by0, by1;   // set a: even chunks, set b: odd chunks (named registers: arrays or a struct of them end up in scratch)
    auto load_one = [&](int k0, int f, float4 &px, float4 &py) {
        const int xk = f / XQ, xc = 4 * (f % XQ);   // sX: row k, first column
        const int yy = f / YQ, yk = 4 * (f % YQ);   // sY: tile row y, first k
        if constexpr (FAST) {
            px = *reinterpret_cast<const float4 *>(g.A + (long)(k0 + xk) * g.sa + x0 + xc);
            py = *reinterpret_cast<const float4 *>(g.B + (long)(y0 + yy) * g.sb + k0 + yk);
        } else {   // clamped: what lies past the matrix is loaded from its last row / column and never reaches a stored result
            const float *ra = g.A + (long)min(k0 + xk, n - 1) * g.sa;
            const float *rb = g.B + (long)min(y0 + yy, n - 1) * g.sb;
            px = make_float4(ra[min(x0 + xc, n - 1)], ra[min(x0 + xc + 1, n - 1)], ra[min(x0 + xc + 2, n - 1)], ra[min(x0 + xc + 3, n - 1)]);
            py = make_float4(rb[min(k0 + yk, n - 1)], rb[min(k0 + yk + 1, n - 1)], rb[min(k0 + yk + 2, n - 1)], rb[min(k0 + yk + 3, n - 1)]);
        }
    };
    auto stage_one = [&](float *bx, float *by, int f, const float4 &px, const float4 &py) {
        const int xk = f / XQ, xc = 4 * (f % XQ);
        const int yy = f / YQ, yk = 4 * (f % YQ);
        *reinterpret_cast<float4 *>(&bx[xk * XP + xc]) = px;
        by[(yk + 0) * YP + yy] = py.x;
        by[(yk + 1) * YP + yy] = py.y;
        by[(yk + 2) * YP + yy] = py.z;
        by[(yk + 3) * YP + yy] = py.w;
    };
    auto load = [&](int k0, float4 &rx0, float4 &rx1, float4 &ry0, float4 &ry1) {
        load_one(k0, tid, rx0, ry0);
        load_one(k0, tid + 256, rx1, ry1);
    };
    auto stage = [&](int buf, const float4 &rx0, const float4 &rx1, const float4 &ry0, const float4 &ry1) {
        stage_one(sX[buf], sY[buf], tid, rx0, ry0);
        stage_one(sX[buf], sY[buf], tid + 256, rx1, ry1);
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
    const int nchunk = (n + KCH - 1) / KCH;
    auto chunk = [&](int c, float4 &nx0, float4 &nx1, float4 &ny0, float4 &ny1, const float4 &sx0, const float4 &sx1, const float4 &sy0, const float4 &sy1) {
        const int buf = c & 1;
        load(min(c + 2, nchunk - 1) * KCH, nx0, nx1, ny0, ny1);   // unconditional (past the end: the last chunk again, never staged into a buffer that is read)
        const float *pa = sY[buf] + (lane >> 5) * YP + wy + (lane & 31);
        const float *pb = sX[buf] + (lane >> 5) * XP + wx + (lane & 31);
        const int kc = FAST ? KCH : min(KCH, n - c * KCH);   // k steps this chunk holds
        if (FAST || kc == KCH) {
            // a whole chunk: every operand read from LDS first, so that the reads of later steps are in flight under the MFMAs of
            // earlier ones (a wave that is alone on its SIMD has nothing else to hide them)
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
                // The last step of an odd size has no partner: a zero-padded one would turn a chain that ends in -0 into +0.  It is
                // a VALU fmaf on each accumulator register instead, operands picked through the C/D map.
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

    // ---- epilogue: out[y][x], x = lane & 31 contiguous
#pragma unroll
    for (int a = 0; a < W; a++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int y = y0 + wy + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
#pragma unroll
            for (int b = 0; b < W; b++) {
                const int x = x0 + wx + 32 * b + (lane & 31);
                if (FAST || (y < n && x < n)) g.out[(long)y * g.so + x] = acc[a][b][r];
            }
        }
}

// The second implementation: one thread per output, the chain as written.
__global__ __launch_bounds__(256) void mm_general(MGeom g) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= g.n) return;
    const float *a = g.A + x, *b = g.B + (long)y * g.sb;
    float acc = 0.0f;
    for (int r = 0; r < g.n; r++) acc = __builtin_fmaf(a[(long)r * g.sa], b[r], acc);
    g.out[(long)y * g.so + x] = acc;
}

// ---------------------------------------------------------------------------------------------------------------- host
const ArgTable mm_table = {"mat_mul", {in_buf("A", T_F32, 2, {0, 1024, 0, 1024}), in_buf("B", T_F32, 2, {0, 1024, 0, 1024}),
                                       out_buf("out", T_F32, 2, {0, 1024, 0, 1024})}};

enum MmLaunch { MM_MFMA, MM_MFMA_EDGE, MM_GENERAL };
const char *const mm_names[3] = {"mat_mul_mfma", "mat_mul_mfma_edge", "mat_mul_general"};

struct MmPlan {
    MmLaunch launch;
    int tile;   // workgroup tile edge of the two MFMA launches
};

bool aligned16(const void *p, long row_stride) { return (uintptr_t)p % 16 == 0 && row_stride % 4 == 0; }

// THE predicate.  The aligned kernel takes a call whose size is a multiple of its tile and of KC (no ragged tile, no short chunk, no
// odd last step) and whose three buffers start on 16 bytes with rows a multiple of 16 bytes; the edge variant takes every other call;
// the general kernel runs only where the caller asks for it by name (hlmi_mat_mul_general).
MmPlan mm_plan(const MGeom &g, bool general_only) {
    const int tile = mm_tile(g.n);
    if (general_only) return {MM_GENERAL, tile};
    const bool fast = g.n % tile == 0 && g.n % KC == 0 && aligned16(g.A, g.sa) && aligned16(g.B, g.sb) && aligned16(g.out, g.so);
    return {fast ? MM_MFMA : MM_MFMA_EDGE, tile};
}

int mm_launch(void *uc, hipStream_t st, const MGeom &g, const MmPlan &p) {
    timing_note_bytes(3.0 * 4.0 * g.n * g.n);   // each matrix read or written once
    const char *name = mm_names[p.launch];
    if (p.launch == MM_GENERAL) {
        HLMI_LAUNCH(uc, name, st, mm_general, dim3((unsigned)((g.n + 255) / 256), (unsigned)g.n), dim3(256), 0, g);
        return 0;
    }
    const unsigned nt = (unsigned)((g.n + p.tile - 1) / p.tile);
    const dim3 grid(nt, nt);
    if (p.tile == LARGE_TILE) {
        if (p.launch == MM_MFMA) HLMI_LAUNCH(uc, name, st, (mm_mfma<2, true>), grid, dim3(256), 0, g);
        else HLMI_LAUNCH(uc, name, st, (mm_mfma<2, false>), grid, dim3(256), 0, g);
    } else {
        if (p.launch == MM_MFMA) HLMI_LAUNCH(uc, name, st, (mm_mfma<1, true>), grid, dim3(256), 0, g);
        else HLMI_LAUNCH(uc, name, st, (mm_mfma<1, false>), grid, dim3(256), 0, g);
    }
    return 0;
}

// [first, last) bytes of the square a buffer describes, in host or in device memory
bool overlap(const halide_buffer_t *a, const halide_buffer_t *b, int n) {
    auto hit = [&](uintptr_t pa, uintptr_t pb) {
        if (!pa || !pb) return false;
        const uintptr_t ea = pa + 4 * ((uintptr_t)(n - 1) * a->dim[1].stride + n), eb = pb + 4 * ((uintptr_t)(n - 1) * b->dim[1].stride + n);
        return pa < eb && pb < ea;
    };
    return hit((uintptr_t)a->host, (uintptr_t)b->host) || hit((uintptr_t)a->device, (uintptr_t)b->device);
}

int entry(int32_t size, halide_buffer_t *A, halide_buffer_t *B, halide_buffer_t *out, bool general_only) {
    void *uc = nullptr;
    if (size < 1 || size > MAX_SIZE)
        return report(uc, halide_error_code_constraint_violated, "Constraint violated: mat_mul size (%d) must be 1 .. %d", size, MAX_SIZE);
    BufArg args[3];
    mm_table.bufs(args, {A, B, out});
    int r = check_not_null(uc, args, 3);
    if (r) return r;
    if ((r = check_type_and_dims(uc, args, 3))) return r;
    if (any_bounds_query(args, 3)) {
        const int mins[2] = {0, 0}, ext[2] = {size, size};
        for (const BufArg &a : args) answer_query(a.buf, mins, ext);
        return 0;
    }
    if ((r = check_shapes(uc, args, 3))) return r;
    char what[32], expect[48];
    for (const BufArg &a : args) {
        for (int d = 0; d < 2; d++) {
            snprintf(what, sizeof what, "%s.min.%d", a.name, d);
            check_equal(uc, what, a.buf->dim[d].min, "0", 0);
            snprintf(what, sizeof what, "%s.extent.%d", a.name, d);
            check_equal(uc, what, a.buf->dim[d].extent, "size", size);
        }
        // rows may be padded (the reference pins stride.1 == size), never overlapping
        snprintf(what, sizeof what, "%s.stride.1", a.name);
        snprintf(expect, sizeof expect, "max(%s.stride.1, size)", a.name);
        check_equal(uc, what, a.buf->dim[1].stride, expect, std::max(a.buf->dim[1].stride, size));
        for (int d = 0; d < 2; d++) check_covers(uc, a, d, 0, size);
    }
    if ((r = checks_done(uc))) return r;
    if (overlap(out, A, size) || overlap(out, B, size))
        return report(uc, halide_error_code_constraint_violated, "Constraint violated: out may not alias %s", overlap(out, A, size) ? "A" : "B");
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, 3))) return r;
    const MGeom g = {dev_ptr<float>(A), dev_ptr<float>(B), dev_ptr<float>(out), size, A->dim[1].stride, B->dim[1].stride, out->dim[1].stride};
    if ((r = mm_launch(uc, ctx.stream, g, mm_plan(g, general_only)))) return r;
    mark_output_written(out);
    return 0;
}

}  // namespace

// Internal entry points (hlmi_internal.h): the generator instantiated at another size, and the second implementation.
extern "C" int hlmi_mat_mul_sized(int32_t size, halide_buffer_t *A, halide_buffer_t *B, halide_buffer_t *out) { return entry(size, A, B, out, false); }
extern "C" int hlmi_mat_mul_general(int32_t size, halide_buffer_t *A, halide_buffer_t *B, halide_buffer_t *out) { return entry(size, A, B, out, true); }

extern "C" int mat_mul(halide_buffer_t *A, halide_buffer_t *B, halide_buffer_t *out) { return hlmi_mat_mul_sized(1024, A, B, out); }
HLMI_ENTRY(mat_mul, mm_table.md)
