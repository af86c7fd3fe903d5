// compositing.hip — apps/compositing: Porter-Duff blending of six u8 RGBA layers by five run-time op codes, a small interpreter.
// Reference semantics: apps/compositing/compositing_generator.cpp:25-154 in its INTEGER form (uint16 colour, uint8 alpha: the branch
// of a target without a GPU feature); the float form is undefined at alpha 0 and is not built.  The contract the kernels share with
// the checker (tests/cpp/compositing_check.c) is restated in include/hlmi_pipelines.h and DESIGN.md §5.5.  No float operation: the
// default and the _nofma build give the same bytes.
//
//   comp_blend     one launch, every shape.  A workgroup is 4 waves, a wave owns 512 consecutive pixels of one row, a lane 8 of them:
//                  one 8-byte load from each of a layer's 4 planes, one 8-byte store to each of the 4 output planes.  Layers are
//                  folded one at a time (the next layer's loads are in flight while the current one is folded); the op code of a
//                  layer is wave-uniform, so the interpreter's switch is a scalar branch per layer.  A wave takes the 8-byte
//                  accesses only where all of its 512 pixels lie inside the row and all 28 plane rows are 8-byte aligned there (a
//                  wave-uniform choice); any other wave — a row's partial last wave, a row that starts unaligned in any buffer —
//                  fills the same registers from per-byte loads and stores per byte.
//   comp_general   hlmi_compositing_general: one thread per pixel, byte loads, the normalise division as the machine's integer divide.
// Both form a pixel through the same scale() / blend<OP>(), so they agree bit for bit.
#include "hlmi_internal.h"

using namespace hlmi;

namespace {

constexpr int LAYERS = 6, NOPS = 5;
constexpr int ROWS = 4;            // rows per workgroup: one per wave
constexpr int PX = 8;              // pixels per lane
constexpr int WAVE_PX = 64 * PX;   // pixels per wave

struct CGeom {
    const uint8_t *src[LAYERS];       // element (ox, oy, 0) of each layer
    long s_sy[LAYERS], s_sc[LAYERS];
    const int32_t *ops;               // element 0
    uint8_t *dst;                     // the output's first element
    long d_sy, d_sc;
    int ow, oh;
};

// The normalise division: numerators below 2^16, denominators 1 .. 255.  With m = ceil(2^24 / d) and e = m d - 2^24 (0 <= e < d),
// floor(n m / 2^24) = floor(n / d + n e / (d 2^24)), and n e <= 65535 * 254 < 2^24 keeps the second term below 1 / d: the floor is
// that of n / d, for every pair.  m <= 2^24 and n << 8 < 2^24, so the quotient is the high word of one 32 x 32 product.  m(0) = 0:
// a zero denominator gives 0, as fast_integer_divide does (src/FastIntegerDivide.cpp:302-307).
struct RecipTable {
    uint32_t m[256];
    constexpr RecipTable() : m() {
        for (uint32_t d = 1; d < 256; d++) m[d] = ((1u << 24) + d - 1) / d;
    }
};
__device__ const RecipTable kRecip{};

__device__ __forceinline__ uint32_t quotient(uint32_t n, uint32_t m) { return __umulhi(n << 8, m); }   // n < 2^16, m = kRecip.m[d]

// scale16 and scale8 (:58-69): c = a * s; c += (c + 128) >> 8; c = (c + 128) >> 8.  a < 2^16, s < 2^8: the product fits 24 bits, the
// result 16 (8 for a < 2^8), so the casts of the generator change nothing.  NOT (c + 127) / 255 for a >= 2^8.
__device__ __forceinline__ uint32_t scale(uint32_t a, uint32_t s) {
    uint32_t c = __umul24(a, s);
    c += (c + 128u) >> 8;
    return (c + 128u) >> 8;
}

struct Px {
    uint32_t c[3], a;   // uint16 colours, uint8 alpha
};

// layer 0 (:139): premultiply_alpha
__device__ __forceinline__ void first(Px &s, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t b3) {
    s.c[0] = __umul24(v0, b3), s.c[1] = __umul24(v1, b3), s.c[2] = __umul24(v2, b3), s.a = b3;
}

// one operator of :80-123 on the layer (v0, v1, v2, b3), every result from the old state; additions wrap in uint16 / uint8
template<int OP>
__device__ __forceinline__ void blend(Px &s, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t b3) {
    const uint32_t v[3] = {v0, v1, v2};
    const uint32_t a = s.a, na = 255u - a, nb = 255u - b3;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const uint32_t bc = __umul24(v[i], b3), old = s.c[i];
        uint32_t r;
        if (OP == 0) r = bc + scale(old, nb);
        else if (OP == 1) r = scale(bc, a) + scale(old, nb);
        else if (OP == 2) r = scale(bc, na) + scale(old, nb);
        else if (OP == 3) r = scale(old, b3);
        else r = scale(old, nb);
        s.c[i] = r & 0xffffu;
    }
    uint32_t ra;
    if (OP == 0) ra = b3 + scale(a, nb);
    else if (OP == 1) ra = a;
    else if (OP == 2) ra = scale(b3, na) + scale(a, nb);
    else if (OP == 3) ra = scale(a, b3);
    else ra = scale(a, nb);
    s.a = ra & 0xffu;
}

__device__ __forceinline__ uint32_t byte_of(const uint2 &w, int i) { return ((i < 4 ? w.x : w.y) >> (8 * (i & 3))) & 0xffu; }

// one layer folded into the PX pixels of a lane; op is wave-uniform, any code outside 0 .. 4 changes nothing (:146-147)
template<int OP>
__device__ __forceinline__ void fold(Px (&st)[PX], const uint2 (&w)[4]) {
#pragma unroll
    for (int i = 0; i < PX; i++) blend<OP>(st[i], byte_of(w[0], i), byte_of(w[1], i), byte_of(w[2], i), byte_of(w[3], i));
}

// the PX bytes from x0 on of the four plane rows of layer l; wide: one 8-byte load each, otherwise bytes, 0 past the row's end
__device__ __forceinline__ void load_layer(const CGeom &g, int l, long y, long x0, bool wide, uint2 (&w)[4]) {
    const uint8_t *row = g.src[l] + y * g.s_sy[l] + x0;
    const long sc = g.s_sc[l];
    if (wide) {
#pragma unroll
        for (int c = 0; c < 4; c++) w[c] = *reinterpret_cast<const uint2 *>(row + c * sc);
    } else {
#pragma unroll
        for (int c = 0; c < 4; c++) {
            uint32_t lo = 0, hi = 0;
#pragma unroll
            for (int i = 0; i < PX; i++) {
                const uint32_t b = x0 + i < g.ow ? row[c * sc + i] : 0u;
                if (i < 4) lo |= b << (8 * i);
                else hi |= b << (8 * (i - 4));
            }
            w[c] = make_uint2(lo, hi);
        }
    }
}

__global__ __launch_bounds__(256) void comp_blend(CGeom g) {
    const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const long y = (long)blockIdx.y * ROWS + wave;
    if (y >= g.oh) return;   // scalar: no barrier follows
    const long xw = (long)blockIdx.x * WAVE_PX, x0 = xw + PX * lane;
    // wave-uniform: all of the wave's pixels inside the row, and the 28 plane rows 8-byte aligned (xw is a multiple of 512)
    uintptr_t bits = 0;
#pragma unroll
    for (int l = 0; l < LAYERS; l++)
#pragma unroll
        for (int c = 0; c < 4; c++) bits |= (uintptr_t)(g.src[l] + y * g.s_sy[l] + c * g.s_sc[l]);
#pragma unroll
    for (int c = 0; c < 4; c++) bits |= (uintptr_t)(g.dst + y * g.d_sy + c * g.d_sc);
    const bool wide = xw + WAVE_PX <= g.ow && (bits & 7) == 0;
    if (!wide && x0 >= g.ow) return;

    uint2 cur[4], nxt[4];
    load_layer(g, 0, y, x0, wide, cur);
    load_layer(g, 1, y, x0, wide, nxt);
    Px st[PX];
#pragma unroll
    for (int i = 0; i < PX; i++) first(st[i], byte_of(cur[0], i), byte_of(cur[1], i), byte_of(cur[2], i), byte_of(cur[3], i));
#pragma unroll 1
    for (int k = 1; k < LAYERS; k++) {
#pragma unroll
        for (int c = 0; c < 4; c++) cur[c] = nxt[c];
        if (k + 1 < LAYERS) load_layer(g, k + 1, y, x0, wide, nxt);
        const int op = __builtin_amdgcn_readfirstlane(g.ops[k - 1]);
        switch (op) {
            case 0: fold<0>(st, cur); break;
            case 1: fold<1>(st, cur); break;
            case 2: fold<2>(st, cur); break;
            case 3: fold<3>(st, cur); break;
            case 4: fold<4>(st, cur); break;
            default: break;
        }
    }
    // normalize (:42-56): out[i] = sat_u8(u16(C[i] + A / 2) / A), 0 for A == 0; out[3] = A
    uint32_t o[4][2] = {};
#pragma unroll
    for (int i = 0; i < PX; i++) {
        const uint32_t a = st[i].a, m = kRecip.m[a], h = a >> 1;
#pragma unroll
        for (int c = 0; c < 3; c++) o[c][i >> 2] |= min(quotient((st[i].c[c] + h) & 0xffffu, m), 255u) << (8 * (i & 3));
        o[3][i >> 2] |= a << (8 * (i & 3));
    }
    uint8_t *orow = g.dst + y * g.d_sy + x0;
    if (wide) {
#pragma unroll
        for (int c = 0; c < 4; c++) *reinterpret_cast<uint2 *>(orow + c * g.d_sc) = make_uint2(o[c][0], o[c][1]);
    } else {
#pragma unroll
        for (int c = 0; c < 4; c++)
#pragma unroll
            for (int i = 0; i < PX; i++)
                if (x0 + i < g.ow) orow[c * g.d_sc + i] = (uint8_t)(o[c][i >> 2] >> (8 * (i & 3)));
    }
}

// ---------------------------------------------------------------------------------------------------------------- general path
__global__ __launch_bounds__(256) void comp_general(CGeom g) {
    const long x = (long)blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= g.ow) return;
    Px s;
    {
        const uint8_t *p = g.src[0] + y * g.s_sy[0] + x;
        const long sc = g.s_sc[0];
        first(s, p[0], p[sc], p[2 * sc], p[3 * sc]);
    }
    for (int k = 1; k < LAYERS; k++) {
        const uint8_t *p = g.src[k] + y * g.s_sy[k] + x;
        const long sc = g.s_sc[k];
        const uint32_t v0 = p[0], v1 = p[sc], v2 = p[2 * sc], b3 = p[3 * sc];
        switch (g.ops[k - 1]) {
            case 0: blend<0>(s, v0, v1, v2, b3); break;
            case 1: blend<1>(s, v0, v1, v2, b3); break;
            case 2: blend<2>(s, v0, v1, v2, b3); break;
            case 3: blend<3>(s, v0, v1, v2, b3); break;
            case 4: blend<4>(s, v0, v1, v2, b3); break;
            default: break;
        }
    }
    uint8_t *o = g.dst + y * g.d_sy + x;
    for (int c = 0; c < 3; c++) o[c * g.d_sc] = (uint8_t)(s.a == 0 ? 0u : min(((s.c[c] + (s.a >> 1)) & 0xffffu) / s.a, 255u));
    o[3 * g.d_sc] = (uint8_t)s.a;
}

// test hook: fn 0 the normalise quotient of (a, b) before the saturation, fn 1 scale16(a, b)
__global__ __launch_bounds__(256) void dbg_compositing(int fn, const uint16_t *__restrict__ a, const uint8_t *__restrict__ b, uint16_t *__restrict__ out,
                                                       size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = (uint16_t)(fn == 0 ? quotient(a[i], kRecip.m[b[i]]) : scale(a[i], b[i]));
}

// ---------------------------------------------------------------------------------------------------------------- host
// estimates: generator :157-161
#define HLMI_COMP_LAYER(i) in_buf("layer_rgba_" #i, T_U8, 3, {0, 1536, 0, 2560, 0, 4})
const ArgTable comp_table("compositing", {HLMI_COMP_LAYER(0), HLMI_COMP_LAYER(1), HLMI_COMP_LAYER(2), HLMI_COMP_LAYER(3), HLMI_COMP_LAYER(4),
                                          HLMI_COMP_LAYER(5), in_buf("ops", T_I32, 1, {0, NOPS}),
                                          out_buf("output", T_U8, 3, {0, 1536, 0, 2560, 0, 4})});
#undef HLMI_COMP_LAYER

int blocks_ok(void *uc, size_t gx, size_t gy) {
    if (gx <= 0x7fffffffu && gy <= 65535u) return 0;
    return report(uc, halide_error_code_buffer_extents_too_large, "compositing: %zu x %zu workgroups exceed one launch", gx, gy);
}

int entry(halide_buffer_t *const (&b)[LAYERS + 2], bool general_only) {
    void *uc = nullptr;
    constexpr int N = LAYERS + 2;
    BufArg args[N];
    comp_table.bufs(args, b);
    int r = check_not_null(uc, args, N);
    if (r) return r;
    if ((r = check_type_and_dims(uc, args, N))) return r;
    halide_buffer_t *ops = b[LAYERS], *out = b[LAYERS + 1];
    const halide_dimension_t *od = out->dim;
    // bound(c, 0, 4) (:179): all four channels are produced together
    check_equal(uc, "output.min.2", od[2].min, "0", 0);
    check_equal(uc, "output.extent.2", od[2].extent, "4", 4);
    if ((r = checks_done(uc))) return r;
    const int ox = od[0].min, oy = od[1].min, ow = od[0].extent, oh = od[1].extent;
    if (any_bounds_query(args, N)) {
        // nothing is clamped: every layer is read over the output's x, y box and channels [0, 4), ops over [0, 5); the output stays
        const int lmin[3] = {ox, oy, 0}, lext[3] = {ow, oh, 4}, omin[1] = {0}, oext[1] = {NOPS};
        for (int l = 0; l < LAYERS; l++) answer_query(b[l], lmin, lext);
        answer_query(ops, omin, oext);
        return 0;
    }
    if ((r = check_shapes(uc, args, N))) return r;
    const bool empty = ow <= 0 || oh <= 0;   // nothing is read where the output is empty
    if (!empty) {
        for (int l = 0; l < LAYERS; l++)
            if ((r = check_covers(uc, args[l], 0, ox, ow)) || (r = check_covers(uc, args[l], 1, oy, oh)) || (r = check_covers(uc, args[l], 2, 0, 4))) return r;
        if ((r = check_covers(uc, args[LAYERS], 0, 0, NOPS))) return r;
    }
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, N))) return r;
    if (!empty) {
        CGeom g = {};
        for (int l = 0; l < LAYERS; l++) {
            const halide_dimension_t *d = b[l]->dim;
            g.s_sy[l] = d[1].stride, g.s_sc[l] = d[2].stride;
            g.src[l] = dev_ptr<uint8_t>(b[l]) + ((long)ox - d[0].min) + ((long)oy - d[1].min) * g.s_sy[l] + (0L - d[2].min) * g.s_sc[l];
        }
        g.ops = dev_ptr<int32_t>(ops) + (0L - ops->dim[0].min);   // read by the kernel: no host read, no synchronisation
        g.dst = dev_ptr<uint8_t>(out), g.d_sy = od[1].stride, g.d_sc = od[2].stride;
        g.ow = ow, g.oh = oh;
        hipStream_t st = ctx.stream;
        const double bytes = 28.0 * ow * oh;   // 24 layer bytes read, 4 written
        if (!general_only) {
            const size_t gx = ((size_t)ow + WAVE_PX - 1) / WAVE_PX, gy = ((size_t)oh + ROWS - 1) / ROWS;
            if ((r = blocks_ok(uc, gx, gy))) return r;
            timing_note_bytes(bytes);
            HLMI_LAUNCH(uc, "comp_blend", st, comp_blend, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, g);
        } else {
            const size_t gx = ((size_t)ow + 255) / 256;
            if ((r = blocks_ok(uc, gx, oh))) return r;
            timing_note_bytes(bytes);
            HLMI_LAUNCH(uc, "comp_general", st, comp_general, dim3((unsigned)gx, (unsigned)oh), dim3(256), 0, g);
        }
    }
    mark_output_written(out);
    return 0;
}

}  // namespace

extern "C" int compositing(halide_buffer_t *layer_rgba_0, halide_buffer_t *layer_rgba_1, halide_buffer_t *layer_rgba_2, halide_buffer_t *layer_rgba_3,
                           halide_buffer_t *layer_rgba_4, halide_buffer_t *layer_rgba_5, halide_buffer_t *ops, halide_buffer_t *output) {
    return entry({layer_rgba_0, layer_rgba_1, layer_rgba_2, layer_rgba_3, layer_rgba_4, layer_rgba_5, ops, output}, false);
}
HLMI_ENTRY(compositing, comp_table.md)

// Measurement and test hook (hlmi_internal.h): the same call with one thread per pixel, whatever the sizes.  Its grid takes one
// output row per workgroup row, so it refuses an output of more than 65535 rows (-6) that the default path, at 4 rows per workgroup
// row, accepts.
extern "C" int hlmi_compositing_general(halide_buffer_t *layer_rgba_0, halide_buffer_t *layer_rgba_1, halide_buffer_t *layer_rgba_2,
                                        halide_buffer_t *layer_rgba_3, halide_buffer_t *layer_rgba_4, halide_buffer_t *layer_rgba_5,
                                        halide_buffer_t *ops, halide_buffer_t *output) {
    return entry({layer_rgba_0, layer_rgba_1, layer_rgba_2, layer_rgba_3, layer_rgba_4, layer_rgba_5, ops, output}, true);
}

// a, b, out: host pointers to n elements.  One launch.
extern "C" int hlmi_debug_compositing(int fn, const uint16_t *a, const uint8_t *b, uint16_t *out, size_t n) {
    if (fn < 0 || fn > 1 || !a || !b || !out || n == 0 || (n + 255) / 256 > 0x7fffffffu) return -1;
    void *d[3] = {nullptr, nullptr, nullptr};
    const void *h[2] = {a, b};
    const size_t bytes[3] = {2 * n, n, 2 * n};
    int rc = 0;
    for (int i = 0; i < 3 && !rc; i++) {
        if (hipMalloc(&d[i], bytes[i]) != hipSuccess) rc = -2;
        else if (i < 2 && hipMemcpy(d[i], h[i], bytes[i], hipMemcpyHostToDevice) != hipSuccess) rc = -3;
    }
    if (!rc) {
        hipLaunchKernelGGL(dbg_compositing, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, fn, (const uint16_t *)d[0], (const uint8_t *)d[1],
                           (uint16_t *)d[2], n);
        if (hipGetLastError() != hipSuccess || hipMemcpy(out, d[2], bytes[2], hipMemcpyDeviceToHost) != hipSuccess) rc = -4;
    }
    for (int i = 0; i < 3; i++) {
        if (d[i]) (void)hipFree(d[i]);
    }
    return rc;
}
