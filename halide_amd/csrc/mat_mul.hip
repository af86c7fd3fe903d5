// mat_mul.hip — gfx950 implementation of the reference's cuda_mat_mul AOT pipeline (square f32 matrix product).
//
// Algorithm: apps/cuda_mat_mul/mat_mul_generator.cpp:27-32; boundary: `int mat_mul(halide_buffer_t *A,
// halide_buffer_t *B, halide_buffer_t *out)` (:18-21, :74), built with size = 1024 (apps/cuda_mat_mul/CMakeLists.txt).
//   out(x, y) = acc_size,  acc_0 = +0.0f,  acc_{r+1} = fmaf(A(x, r), B(r, y), acc_r),  r = 0 .. size - 1
// Dimension 0 is innermost: in memory out[y][x] = sum_r B[y][r] * A[r][x], i.e. the row-major product B @ A.  The chain is the
// contract in BOTH canonical float forms: k runs strictly upward for every output, no step is padded with
// zeros (fmaf(0, 0, -0.0f) is +0.0f), subnormals are kept.
//
// Exact MFMA path: chain::tile() of f32_chain_gemm.h, the k-ordered chain on `v_mfma_f32_32x32x2_f32` that sgemm shares; the tile
// loop, its chunk schedule and the rule for an odd size are described there, once.  Here X[k][x] = A(x, r) = A[r][x]: x contiguous,
// copied straight into LDS; Y[k][y] = B(r, y) = B[y][r]: r contiguous, turned k-major on the way in; M = N = K = size; a finished
// sum is stored as it is.  workgroup = TILE x TILE outputs, wave = W x W accumulators, W = TILE / 64: mm_tile() picks the smallest
// tile while that is what it takes to have a wave on every SIMD.
// Three launches (mm_plan() is the one place that chooses):
//   mat_mul_mfma       size a multiple of the tile and of KC; every device address and row stride a multiple of 16 bytes: float4 loads
//   mat_mul_mfma_edge  the same template with scalar loads from clamped addresses (padded rows and columns are computed and never
//                      stored), a last chunk of size % KC steps, and for an odd size the last step as a VALU fmaf on the
//                      accumulator registers through the C/D map: no padded k step exists
//   mat_mul_general    one thread per output, a plain fmaf loop (hlmi_mat_mul_general only)
#include "f32_chain_gemm.h"
#include "hlmi_internal.h"

using namespace hlmi;

namespace {

constexpr int MAX_SIZE = 8192;     // hlmi_mat_mul_sized takes 1 .. MAX_SIZE
constexpr int SMALL_TILE = 64;     // workgroup tile with one accumulator per wave
constexpr int LARGE_TILE = 128;    // workgroup tile with 2 x 2 accumulators per wave
constexpr int LARGE_FROM = 2048;   // (LARGE_FROM / LARGE_TILE)^2 workgroups x 4 waves = 1024 waves = 256 CUs x 4 SIMDs
constexpr int KC = 32;             // the tile loop's chunk, as mm_plan() and the tests read it: a size that is no multiple of it has a short last chunk
static_assert(KC == chain::KC, "mm_plan() plans for the chunk that chain::tile() stages");

struct MGeom {
    const float *A, *B;
    float *out;
    int n;
    long sa, sb, so;   // row strides in elements
};

// The wave tile follows from the size: the large tile (LDS reuse 2 x) only where it still leaves a wave for every SIMD.
constexpr int mm_tile(int size) { return size >= LARGE_FROM ? LARGE_TILE : SMALL_TILE; }

// chain::tile() with X = A straight, Y = B turned, M = N = K = n and a plain store.
struct MmOps {
    static __device__ __forceinline__ int M(const MGeom &g) { return g.n; }
    static __device__ __forceinline__ int N(const MGeom &g) { return g.n; }
    static __device__ __forceinline__ int K(const MGeom &g) { return g.n; }
    static __device__ __forceinline__ void store(const MGeom &g, int x, int y, float acc) { g.out[(long)y * g.so + x] = acc; }
};

template<int W, bool FAST>
__global__ __launch_bounds__(256) void mm_mfma(MGeom g) {
    chain::tile<W, FAST, false, true, MmOps>(g);
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
    return with_flags([&](auto large, auto fast) {
        HLMI_LAUNCH(uc, name, st, (mm_mfma<large.value ? 2 : 1, fast.value>), grid, dim3(256), 0, g);
        return 0;
    }, p.tile == LARGE_TILE, p.launch == MM_MFMA);
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
