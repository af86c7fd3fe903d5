// reaction_diffusion.hip — apps/HelloWasm's reaction_diffusion: init, update and render, f32 [x, y, 3] (render: -> u32 [x, y]), 3 AOT
// entry points, and hlmi_reaction_diffusion_run, a library extension that runs several updates and one render in as few launches
// as its plan allows.  Reference semantics: apps/HelloWasm/generator/reaction_diffusion_generator.cpp:10-12 (init), :34-105
// (update), :150-174 (render); the contract the kernels share with the checker (tests/cpp/reaction_diffusion_check.c) is restated in
// DESIGN.md §5.16, the random hash in hlmi_random.h.
//
//   rd_steps<S, RENDER>  the hot path: S time steps in one launch.  A workgroup owns 64 x 32 pixels of all three channels (the
//                        reaction couples them): it stages them with a halo of 2 S into LDS and runs the S steps between two LDS
//                        buffers, step k on the region 2 (S - k) wider than the tile on every side, cut to the state's rectangle;
//                        the last step goes to new_state and, with RENDER, to the packed pixel.  Cells outside the rectangle are never
//                        made or read: every tap clamps its COORDINATE into the rectangle and reads the cell that step made there, so
//                        the border a step reads is the post-edge-noise, post-clobber border of the step before.  S = 1, 2, 4 are the
//                        instances of the one template.  Full frames only (output box == state box).  In the one run that measured them
//                         no instance beat rd_update_general, per step, at 1024^2 or at 4096^2, so by the project's rule
//                        they stay behind the switch HLMI_RD_STEPS_PER_LAUNCH (1, 2, 4) and the plan's default is rd_update_general
//   rd_update_general    one thread per output pixel, every tap a clamped load from global memory: any output box; the plan's default
//   rd_init, rd_render   four pixels of a row per thread, 16-byte accesses where the addresses allow; *_general: one thread per output
// Every path evaluates rd_cell / rd_pack / init_value, so all of them agree bit for bit.
#include "hlmi_device_math.h"
#include "hlmi_internal.h"
#include "hlmi_random.h"

using namespace hlmi;

namespace {

constexpr int TW = 64, TH = 32;   // pixels per workgroup

// The (call id, definition tag) of every random_float call: the ONE table the kernels read.  Derivation: DESIGN.md §5.16 — ids count
// the calls in generate() from 0, tags count every Func definition of the generator before the one that holds the call (init: none;
// update: state_im, repeat_edge, blur_x, blur_y, blur, new_state's pure definition = 0 .. 5, then the four edge updates 6 .. 9, noise 10).
// Not confirmed against a Halide build: a correction is a change of this table (and of the checker's).
struct RandomCall {
    uint32_t id, tag;
};
enum { RC_INIT, RC_ROW_MIN, RC_ROW_MAX, RC_COL_MIN, RC_COL_MAX, RC_NOISE };
__device__ constexpr RandomCall RD_RANDOM[6] = {{0, 0}, {0, 6}, {1, 7}, {2, 8}, {3, 9}, {4, 10}};

struct RDGeom {
    const float *src;       // state(sx0, sy0, 0)
    long s_sy, s_sc;
    int sx0, sy0, sw, sh;   // the state's box in x and y: the clamp and the edges
    float *dst;             // new_state(ox, oy, 0)
    long d_sy, d_sc;
    int ox, oy, ow, oh;     // the output's box
    uint32_t *pix;          // RENDER: render(ox, oy)
    long p_sy;
    int mouse_x, mouse_y, frame;
    int cx0, cx1, cy0, cy1;   // the clobber box, absolute coordinates 0 .. W - 1, 0 .. H - 1
};

// x / 10 -> x * fold(1 / 10) (src/Simplify_Div.cpp:204)
constexpr float TENTH = 1.0f / 10.0f;

// int32 arithmetic wraps (the contract for coordinates and mouse positions near the ends of the range)
__host__ __device__ __forceinline__ int wrap_sub(int a, int b) { return (int)((uint32_t)a - (uint32_t)b); }
__host__ __device__ __forceinline__ int wrap_add(int a, int b) { return (int)((uint32_t)a + (uint32_t)b); }
__device__ __forceinline__ int sq_sum(int a, int b) { return (int)((uint32_t)a * (uint32_t)a + (uint32_t)b * (uint32_t)b); }

// init: [id, tag, c, y, x]
__device__ __forceinline__ uint32_t init_prefix(int c, int y) {
    uint32_t r = rnd::random_begin(RD_RANDOM[RC_INIT].id);
    r = rnd::random_next(r, RD_RANDOM[RC_INIT].tag);
    r = rnd::random_next(r, (uint32_t)c);
    return rnd::random_next(r, (uint32_t)y);
}
__device__ __forceinline__ float init_value(uint32_t prefix, int x) { return rnd::random_float_end(rnd::random_next(prefix, (uint32_t)x)); }

// [frame, id, tag, c, ...]
__device__ __forceinline__ uint32_t frame_prefix(int which, int frame, int c) {
    uint32_t r = rnd::random_begin((uint32_t)frame);
    r = rnd::random_next(r, RD_RANDOM[which].id);
    r = rnd::random_next(r, RD_RANDOM[which].tag);
    return rnd::random_next(r, (uint32_t)c);
}
// the edge rows hash x, the edge columns y: random_float(frame) * 0.2f
__device__ __forceinline__ float edge_noise(int which, int frame, int c, int v) {
    return rnd::random_float_end(rnd::random_next(frame_prefix(which, frame, c), (uint32_t)v)) * 0.2f;
}
__device__ __forceinline__ float noise_at(uint32_t prefix, int x, int y) {
    return rnd::random_float_end(rnd::random_next(rnd::random_next(prefix, (uint32_t)y), (uint32_t)x));
}

// new_state(X, Y, 0 .. 2) of one update with `frame`; tap(c, dx, dy) = repeat_edge(state)(X + dx, Y + dy, c), asked for on the cross only
template<typename Tap>
__device__ __forceinline__ void rd_cell(const RDGeom &g, int frame, int X, int Y, Tap tap, float v[3]) {
    float bl[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float m = tap(c, 0, 0);
        const float bx = (((tap(c, -2, 0) + tap(c, -1, 0)) + m) + tap(c, 1, 0)) + tap(c, 2, 0);
        const float by = (((tap(c, 0, -2) + tap(c, 0, -1)) + m) + tap(c, 0, 1)) + tap(c, 0, 2);
        bl[c] = (bx + by) * TENTH;
    }
    // the sigmoid push: R *= (1 - s) + s * R * (3 - 2 * R), s = 0.5f; (s * R) * (3 - 2 R) is the multiply that feeds the add
    float p[3];
#pragma unroll
    for (int c = 0; c < 3; c++) p[c] = bl[c] * dev::mad(0.5f * bl[c], dev::msub(3.0f, 2.0f, bl[c]), 0.5f);
    float R = p[0], G = p[1], B = p[2];
    const float dR = B * ((1.0f - R) - G);
    const float dG = (1.0f - B) * (R - G);
    const float dB = (dev::mad(2.0f * G, R, 1.0f - B) - R) - G;
    // 5 * max(0, 1.f - (mx * mx + my * my) * 0.001f) + 1, the squared distance int32
    const float d2 = (float)sq_sum(wrap_sub(g.mouse_x, X), wrap_sub(g.mouse_y, Y));
    const float fall = dev::msub(1.0f, d2, 0.001f);
    const float boost = dev::mad(5.0f, 0.0f > fall ? 0.0f : fall, 1.0f);
    R = dev::mad(dR * 0.14f, boost, R);
    G = dev::mad(dG * 0.05f, boost, G);
    B = dev::mad(dB * 0.065f, boost, B);
    v[0] = dev::clampf(R, 0.0f, 1.0f), v[1] = dev::clampf(G, 0.0f, 1.0f), v[2] = dev::clampf(B, 0.0f, 1.0f);
    // the update definitions, in the generator's order: row min, row max, column min, column max, the clobber
    const int xmax = g.sx0 + g.sw - 1, ymax = g.sy0 + g.sh - 1;
    if (X == g.sx0 || X == xmax || Y == g.sy0 || Y == ymax) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            if (Y == g.sy0) v[c] = edge_noise(RC_ROW_MIN, frame, c, X);
            if (Y == ymax) v[c] = edge_noise(RC_ROW_MAX, frame, c, X);
            if (X == g.sx0) v[c] = edge_noise(RC_COL_MIN, frame, c, Y);
            if (X == xmax) v[c] = edge_noise(RC_COL_MAX, frame, c, Y);
        }
    }
    if (X >= g.cx0 && X <= g.cx1 && Y >= g.cy0 && Y <= g.cy1) {
        const float radius = (float)sq_sum(wrap_sub(X, g.mouse_x), wrap_sub(Y, g.mouse_y));
        if (radius < 100.0f) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const uint32_t pre = frame_prefix(RC_NOISE, frame, c);
                const int X1 = wrap_add(X, 1), Y1 = wrap_add(Y, 1);
                v[c] = 0.25f * (((noise_at(pre, X, Y) + noise_at(pre, X1, Y)) + noise_at(pre, X1, Y1)) + noise_at(pre, X, Y1));
            }
        }
    }
}

// render: min(a, b) = a < b ? a : b, max(a, b) = a > b ? a : b; the cast of a value outside [0, 2^32) is not defined (a NaN state)
__device__ __forceinline__ uint32_t rd_pack(const float s[3]) {
    float k[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float v = (s[c] * (1.01f - s[c])) * 4.0f;
        v = v * v;
        v = v * v;
        k[c] = v < 1.0f ? v : 1.0f;
    }
    const float half = (k[1] + k[2]) * 0.5f;
    const float R = k[0] < half ? k[0] : half;
    const float G = dev::clampf(((k[1] + k[0]) + k[2]) * 0.5f, 0.0f, 1.0f);
    const float m12 = k[1] > k[2] ? k[1] : k[2];
    const float B = k[0] > m12 ? k[0] : m12;
    const uint32_t r = (uint32_t)(R * 255.0f) & 0xffu, gg = (uint32_t)(G * 255.0f) & 0xffu, b = (uint32_t)(B * 255.0f) & 0xffu;
    return b | (gg << 8) | (r << 16) | (255u << 24);
}

// ---------------------------------------------------------------------------------------------------------------- the time-tiled kernel
// Step K of S (1 .. S) with frame g.frame + K - 1: reads the state with halo HS = 2 (S - K + 1) from one LDS buffer, makes the one with
// halo HS - 2 in the other, or, K == S, in new_state.  x, y are relative to the state's min; a holds the halo-2S layout (and every
// later even one), b the halo-(2S - 2) layout.
template<int S, int K, bool RENDER>
__device__ __forceinline__ void rd_step(const RDGeom &g, float *a, float *b, int tx0, int ty0, int tid) {
    constexpr int HS = 2 * (S - K + 1), HD = HS - 2;
    constexpr int LWS = TW + 2 * HS, PS = LWS * (TH + 2 * HS);
    constexpr int LWD = TW + 2 * HD, LHD = TH + 2 * HD, PD = LWD * LHD;
    const float *cur = (K & 1) ? a : b;
    float *nxt = (K & 1) ? b : a;
    const int frame = wrap_add(g.frame, K - 1);
    for (int idx = tid; idx < PD; idx += 256) {
        const int lx = idx % LWD, ly = idx / LWD;
        const int x = tx0 - HD + lx, y = ty0 - HD + ly;
        if (x < 0 || x >= g.sw || y < 0 || y >= g.sh) continue;
        int xi[5], yi[5];
#pragma unroll
        for (int j = 0; j < 5; j++) {
            xi[j] = dev::clampi(x + j - 2, 0, g.sw - 1) - (tx0 - HS);
            yi[j] = (dev::clampi(y + j - 2, 0, g.sh - 1) - (ty0 - HS)) * LWS;
        }
        float v[3];
        rd_cell(g, frame, g.sx0 + x, g.sy0 + y, [&](int c, int dx, int dy) { return cur[c * PS + yi[dy + 2] + xi[dx + 2]]; }, v);
        if constexpr (K < S) {
#pragma unroll
            for (int c = 0; c < 3; c++) nxt[c * PD + ly * LWD + lx] = v[c];
        } else {
            float *o = g.dst + (long)y * g.d_sy + x;
#pragma unroll
            for (int c = 0; c < 3; c++) o[c * g.d_sc] = v[c];
            if constexpr (RENDER) g.pix[(long)y * g.p_sy + x] = rd_pack(v);
        }
    }
    if constexpr (K < S) {
        __syncthreads();
        rd_step<S, K + 1, RENDER>(g, a, b, tx0, ty0, tid);
    }
}

constexpr size_t steps_lds_bytes(int S) {
    const size_t a = (size_t)(TW + 4 * S) * (TH + 4 * S), b = S > 1 ? (size_t)(TW + 4 * S - 4) * (TH + 4 * S - 4) : 0;
    return 3 * sizeof(float) * (a + b);
}

template<int S, bool RENDER>
__global__ __launch_bounds__(256) void rd_steps(RDGeom g) {
    extern __shared__ __align__(16) float rd_lds[];
    constexpr int H0 = 2 * S, LW = TW + 2 * H0, LH = TH + 2 * H0, P0 = LW * LH;
    float *a = rd_lds, *b = rd_lds + 3 * P0;
    const int tid = (int)threadIdx.x;
    const int tx0 = (int)blockIdx.x * TW, ty0 = (int)blockIdx.y * TH;
    for (int idx = tid; idx < P0; idx += 256) {
        const int lx = idx % LW, ly = idx / LW;
        const int x = tx0 - H0 + lx, y = ty0 - H0 + ly;
        if (x < 0 || x >= g.sw || y < 0 || y >= g.sh) continue;
        const float *p = g.src + (long)y * g.s_sy + x;
#pragma unroll
        for (int c = 0; c < 3; c++) a[c * P0 + idx] = p[c * g.s_sc];
    }
    __syncthreads();
    rd_step<S, 1, RENDER>(g, a, b, tx0, ty0, tid);
}

// ---------------------------------------------------------------------------------------------------------------- one thread per output
__global__ __launch_bounds__(256) void rd_update_general(RDGeom g) {
    const int x = (int)blockIdx.x * 256 + (int)threadIdx.x, y = (int)blockIdx.y;
    if (x >= g.ow) return;
    const int X = g.ox + x, Y = g.oy + y;
    long xo[5], yo[5];
#pragma unroll
    for (int j = 0; j < 5; j++) {
        xo[j] = max(min((long)X + j - 2, (long)g.sx0 + g.sw - 1), (long)g.sx0) - g.sx0;
        yo[j] = (max(min((long)Y + j - 2, (long)g.sy0 + g.sh - 1), (long)g.sy0) - g.sy0) * g.s_sy;
    }
    float v[3];
    rd_cell(g, g.frame, X, Y, [&](int c, int dx, int dy) { return g.src[c * g.s_sc + yo[dy + 2] + xo[dx + 2]]; }, v);
    float *o = g.dst + (long)y * g.d_sy + x;
#pragma unroll
    for (int c = 0; c < 3; c++) o[c * g.d_sc] = v[c];
}

struct IGeom {
    float *dst;
    long d_sy, d_sc;
    int ox, oy, oc, ow;
};

__global__ __launch_bounds__(256) void rd_init(IGeom g) {
    const int x = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4, y = (int)blockIdx.y, c = (int)blockIdx.z;
    if (x >= g.ow) return;
    const uint32_t pre = init_prefix(g.oc + c, g.oy + y);
    float *o = g.dst + (long)c * g.d_sc + (long)y * g.d_sy + x;
    if (x + 4 <= g.ow && ((uintptr_t)o & 15) == 0) {
        *(float4 *)o = make_float4(init_value(pre, g.ox + x), init_value(pre, g.ox + x + 1), init_value(pre, g.ox + x + 2), init_value(pre, g.ox + x + 3));
    } else {
        for (int j = 0; j < 4 && x + j < g.ow; j++) o[j] = init_value(pre, g.ox + x + j);
    }
}

__global__ __launch_bounds__(256) void rd_init_general(IGeom g) {
    const int x = (int)blockIdx.x * 256 + (int)threadIdx.x, y = (int)blockIdx.y, c = (int)blockIdx.z;
    if (x >= g.ow) return;
    g.dst[(long)c * g.d_sc + (long)y * g.d_sy + x] = init_value(init_prefix(g.oc + c, g.oy + y), g.ox + x);
}

struct PGeom {
    const float *src;   // state(render's x min, render's y min, 0)
    long s_sy, s_sc;
    uint32_t *pix;
    long p_sy;
    int ow;
};

__global__ __launch_bounds__(256) void rd_render(PGeom g) {
    const int x = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4, y = (int)blockIdx.y;
    if (x >= g.ow) return;
    const float *p = g.src + (long)y * g.s_sy + x;
    uint32_t *o = g.pix + (long)y * g.p_sy + x;
    const bool wide = x + 4 <= g.ow && (((uintptr_t)p | (uintptr_t)(p + g.s_sc) | (uintptr_t)(p + 2 * g.s_sc) | (uintptr_t)o) & 15) == 0;
    if (wide) {
        const float4 r = *(const float4 *)p, gr = *(const float4 *)(p + g.s_sc), bl = *(const float4 *)(p + 2 * g.s_sc);
        const float s0[3] = {r.x, gr.x, bl.x}, s1[3] = {r.y, gr.y, bl.y}, s2[3] = {r.z, gr.z, bl.z}, s3[3] = {r.w, gr.w, bl.w};
        *(uint4 *)o = make_uint4(rd_pack(s0), rd_pack(s1), rd_pack(s2), rd_pack(s3));
    } else {
        for (int j = 0; j < 4 && x + j < g.ow; j++) {
            const float s[3] = {p[j], p[g.s_sc + j], p[2 * g.s_sc + j]};
            o[j] = rd_pack(s);
        }
    }
}

__global__ __launch_bounds__(256) void rd_render_general(PGeom g) {
    const int x = (int)blockIdx.x * 256 + (int)threadIdx.x, y = (int)blockIdx.y;
    if (x >= g.ow) return;
    const float *p = g.src + (long)y * g.s_sy + x;
    const float s[3] = {p[0], p[g.s_sc], p[2 * g.s_sc]};
    g.pix[(long)y * g.p_sy + x] = rd_pack(s);
}

// ---------------------------------------------------------------------------------------------------------------- host
// the generators declare no estimates
const ArgTable init_table("reaction_diffusion_init", {out_buf("output", T_F32, 3)});
const ArgTable update_table("reaction_diffusion_update", {in_buf("state", T_F32, 3), scalar_i32("mouse_x"), scalar_i32("mouse_y"), scalar_i32("frame"),
                                                          out_buf("new_state", T_F32, 3)});
const ArgTable render_table("reaction_diffusion_render", {in_buf("state", T_F32, 3), out_buf("render", T_U32, 2)});

int blocks_ok(void *uc, size_t gx, size_t gy, size_t gz) {
    if (gx <= 0x7fffffffu && gy <= 65535u && gz <= 65535u) return 0;
    return report(uc, halide_error_code_buffer_extents_too_large, "reaction_diffusion: %zu x %zu x %zu workgroups exceed one launch", gx, gy, gz);
}

int host_clamp(int v, int lo, int hi) { return std::max(std::min(v, hi), lo); }   // clamp(v, lo, hi) = max(min(v, hi), lo)

// What the update definitions write, whatever the output's box (reaction_diffusion_generator.cpp:80-83, 93-104): rows state.min(1) and
// state.max(1), columns state.min(0) and state.max(0), and the clobber box, which is in EXTENT coordinates 0 .. W - 1, 0 .. H - 1
struct Written {
    int cx0, cx1, cy0, cy1;   // the clobber box
    int x0, x1, y0, y1;       // the box that holds all of it
};
Written written_by_updates(const halide_dimension_t *sd, int mouse_x, int mouse_y) {
    Written w;
    const int W = sd[0].extent, H = sd[1].extent;
    w.cx0 = host_clamp(wrap_sub(mouse_x, 10), 0, W - 1), w.cx1 = host_clamp(wrap_add(mouse_x, 10), 0, W - 1);
    w.cy0 = host_clamp(wrap_sub(mouse_y, 10), 0, H - 1), w.cy1 = host_clamp(wrap_add(mouse_y, 10), 0, H - 1);
    w.x0 = std::min(sd[0].min, w.cx0), w.x1 = std::max(sd[0].min + W - 1, w.cx1);
    w.y0 = std::min(sd[1].min, w.cy0), w.y1 = std::max(sd[1].min + H - 1, w.cy1);
    return w;
}

void fill_state(RDGeom &g, const halide_buffer_t *state, const float *base) {
    const halide_dimension_t *sd = state->dim;
    g.src = base, g.s_sy = sd[1].stride, g.s_sc = sd[2].stride;
    g.sx0 = sd[0].min, g.sy0 = sd[1].min, g.sw = sd[0].extent, g.sh = sd[1].extent;
}

template<int S>
int launch_steps_s(void *uc, hipStream_t st, const RDGeom &g, bool render) {
    constexpr size_t lds = steps_lds_bytes(S);
    const size_t tx = ((size_t)g.sw + TW - 1) / TW, ty = ((size_t)g.sh + TH - 1) / TH;
    int r = blocks_ok(uc, tx, ty, 1);
    if (r) return r;
    const dim3 grid((unsigned)tx, (unsigned)ty), block(256);
    return with_flags([&](auto R) {
        if (lds > 64 * 1024) HLMI_HIP(uc, hipFuncSetAttribute((const void *)rd_steps<S, R.value>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        static const char *const names[2] = {S == 1 ? "rd_steps1" : S == 2 ? "rd_steps2" : "rd_steps4",
                                             S == 1 ? "rd_steps1_render" : S == 2 ? "rd_steps2_render" : "rd_steps4_render"};
        HLMI_LAUNCH(uc, names[R.value], st, (rd_steps<S, R.value>), grid, block, lds, g);
        return 0;
    }, render);
}
// s steps (1, 2 or 4) of the full frame in one launch
int launch_steps(void *uc, hipStream_t st, const RDGeom &g, int s, bool render) {
    timing_note_bytes((24.0 + (render ? 4.0 : 0.0)) * g.sw * g.sh);
    return s == 4 ? launch_steps_s<4>(uc, st, g, render) : s == 2 ? launch_steps_s<2>(uc, st, g, render) : launch_steps_s<1>(uc, st, g, render);
}

int launch_update_general(void *uc, hipStream_t st, const RDGeom &g) {
    const size_t gx = ((size_t)g.ow + 255) / 256;
    int r = blocks_ok(uc, gx, g.oh, 1);
    if (r) return r;
    timing_note_bytes(24.0 * g.ow * g.oh);
    HLMI_LAUNCH(uc, "rd_update_general", st, rd_update_general, dim3((unsigned)gx, (unsigned)g.oh), dim3(256), 0, g);
    return 0;
}

int launch_render(void *uc, hipStream_t st, const PGeom &g, int oh, bool general_only) {
    const size_t gx = general_only ? ((size_t)g.ow + 255) / 256 : ((size_t)g.ow + 1023) / 1024;
    int r = blocks_ok(uc, gx, oh, 1);
    if (r) return r;
    timing_note_bytes(16.0 * g.ow * oh);
    if (general_only) HLMI_LAUNCH(uc, "rd_render_general", st, rd_render_general, dim3((unsigned)gx, (unsigned)oh), dim3(256), 0, g);
    else HLMI_LAUNCH(uc, "rd_render", st, rd_render, dim3((unsigned)gx, (unsigned)oh), dim3(256), 0, g);
    return 0;
}

bool same_box_xy(const halide_dimension_t *a, const halide_dimension_t *b) {
    return a[0].min == b[0].min && a[0].extent == b[0].extent && a[1].min == b[1].min && a[1].extent == b[1].extent;
}

void pin_channels(void *uc, const halide_buffer_t *b, const char *min_what, const char *extent_what) {
    check_equal(uc, min_what, b->dim[2].min, "0", 0);
    check_equal(uc, extent_what, b->dim[2].extent, "3", 3);
}

// ---- init
int init_entry(halide_buffer_t *output, bool general_only) {
    void *uc = nullptr;
    BufArg args[1];
    init_table.bufs(args, {output});
    int r = check_not_null(uc, args, 1);
    if (r) return r;
    if ((r = check_type_and_dims(uc, args, 1))) return r;
    if (any_bounds_query(args, 1)) return 0;   // the output's region is the request and stays as passed
    if ((r = check_shapes(uc, args, 1))) return r;
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, 1))) return r;
    const halide_dimension_t *od = output->dim;
    if (od[0].extent > 0 && od[1].extent > 0 && od[2].extent > 0) {
        IGeom g = {dev_ptr<float>(output), od[1].stride, od[2].stride, od[0].min, od[1].min, od[2].min, od[0].extent};
        const size_t gx = general_only ? ((size_t)g.ow + 255) / 256 : ((size_t)g.ow + 1023) / 1024;
        if ((r = blocks_ok(uc, gx, od[1].extent, od[2].extent))) return r;
        const dim3 grid((unsigned)gx, (unsigned)od[1].extent, (unsigned)od[2].extent);
        timing_note_bytes(4.0 * g.ow * od[1].extent * od[2].extent);
        if (general_only) HLMI_LAUNCH(uc, "rd_init_general", ctx.stream, rd_init_general, grid, dim3(256), 0, g);
        else HLMI_LAUNCH(uc, "rd_init", ctx.stream, rd_init, grid, dim3(256), 0, g);
    }
    mark_output_written(output);
    return 0;
}

int steps_per_launch(void *uc, int w, int h, int *S);

// ---- update
int update_entry(halide_buffer_t *state, int32_t mouse_x, int32_t mouse_y, int32_t frame, halide_buffer_t *new_state, bool general_only) {
    void *uc = nullptr;
    BufArg args[2];
    update_table.bufs(args, {state, new_state});
    int r = check_not_null(uc, args, 2);
    if (r) return r;
    if ((r = check_type_and_dims(uc, args, 2))) return r;
    const halide_dimension_t *sd = state->dim, *od = new_state->dim;
    const bool state_ok = sd[0].extent > 0 && sd[1].extent > 0;
    const Written w = written_by_updates(sd, mouse_x, mouse_y);
    if (any_bounds_query(args, 2)) {
        // new_state: the box that holds its own region as passed and everything the update definitions write (they depend on the state's
        // box: a state without a shape adds nothing); channels [0, 3).  state: every read clamps into whatever the state is, so x and y
        // stay as passed (as for linear_blur); channels [0, 3)
        int mins[3] = {od[0].min, od[1].min, 0}, ext[3] = {od[0].extent, od[1].extent, 3};
        if (state_ok) {
            const bool shaped = od[0].extent > 0 && od[1].extent > 0;
            const int x0 = shaped ? std::min(od[0].min, w.x0) : w.x0, x1 = shaped ? std::max(od[0].min + od[0].extent - 1, w.x1) : w.x1;
            const int y0 = shaped ? std::min(od[1].min, w.y0) : w.y0, y1 = shaped ? std::max(od[1].min + od[1].extent - 1, w.y1) : w.y1;
            mins[0] = x0, ext[0] = x1 - x0 + 1, mins[1] = y0, ext[1] = y1 - y0 + 1;
        }
        int smins[3] = {sd[0].min, sd[1].min, 0}, sext[3] = {sd[0].extent, sd[1].extent, 3};
        answer_query(new_state, mins, ext);
        answer_query(state, smins, sext);
        return 0;
    }
    if ((r = check_shapes(uc, args, 2))) return r;
    pin_channels(uc, state, "state.min.2", "state.extent.2");
    pin_channels(uc, new_state, "new_state.min.2", "new_state.extent.2");
    const bool out_some = od[0].extent > 0 && od[1].extent > 0;
    if (state_ok) {
        check_covers(uc, args[1], 0, w.x0, w.x1 - w.x0 + 1);
        check_covers(uc, args[1], 1, w.y0, w.y1 - w.y0 + 1);
    }
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, 2))) return r;
    if (!state_ok && out_some)
        return report(uc, halide_error_code_access_out_of_bounds, "Input buffer state is empty in dimension %d: there is no edge to repeat", sd[0].extent > 0 ? 1 : 0);
    if (out_some) {
        RDGeom g = {};
        fill_state(g, state, dev_ptr<float>(state));
        g.dst = dev_ptr<float>(new_state), g.d_sy = od[1].stride, g.d_sc = od[2].stride;
        g.ox = od[0].min, g.oy = od[1].min, g.ow = od[0].extent, g.oh = od[1].extent;
        g.mouse_x = mouse_x, g.mouse_y = mouse_y, g.frame = frame;
        g.cx0 = w.cx0, g.cx1 = w.cx1, g.cy0 = w.cy0, g.cy1 = w.cy1;
        // the time-tiled kernel takes full frames only, and runs where the plan or the switch asks for it
        int S = 0;
        if (!general_only && same_box_xy(sd, od) && (r = steps_per_launch(uc, g.sw, g.sh, &S))) return r;
        if (S > 0) r = launch_steps(uc, ctx.stream, g, 1, false);
        else r = launch_update_general(uc, ctx.stream, g);
        if (r) return r;
    }
    mark_output_written(new_state);
    return 0;
}

// ---- render
int render_entry(halide_buffer_t *state, halide_buffer_t *render, bool general_only) {
    void *uc = nullptr;
    BufArg args[2];
    render_table.bufs(args, {state, render});
    int r = check_not_null(uc, args, 2);
    if (r) return r;
    if ((r = check_type_and_dims(uc, args, 2))) return r;
    const halide_dimension_t *sd = state->dim, *od = render->dim;
    if (any_bounds_query(args, 2)) {
        // render is the request; the state gets its x and y and channels [0, 3)
        int mins[3] = {od[0].min, od[1].min, 0}, ext[3] = {od[0].extent, od[1].extent, 3};
        if (!buffer_known(render)) mins[0] = sd[0].min, mins[1] = sd[1].min, ext[0] = sd[0].extent, ext[1] = sd[1].extent;
        answer_query(state, mins, ext);
        return 0;
    }
    if ((r = check_shapes(uc, args, 2))) return r;
    check_covers(uc, args[0], 0, od[0].min, od[0].extent);
    check_covers(uc, args[0], 1, od[1].min, od[1].extent);
    check_covers(uc, args[0], 2, 0, 3);
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, 2))) return r;
    if (od[0].extent > 0 && od[1].extent > 0) {
        PGeom g;
        g.src = dev_ptr<float>(state) + (long)(0 - sd[2].min) * sd[2].stride + (long)(od[1].min - sd[1].min) * sd[1].stride + (od[0].min - sd[0].min);
        g.s_sy = sd[1].stride, g.s_sc = sd[2].stride;
        g.pix = dev_ptr<uint32_t>(render), g.p_sy = od[1].stride, g.ow = od[0].extent;
        if ((r = launch_render(uc, ctx.stream, g, od[1].extent, general_only))) return r;
    }
    mark_output_written(render);
    return 0;
}

// ---- run
// The plan's steps per launch for a W x H frame: 0 = one rd_update_general launch per step.  DESIGN.md §5.16 has the measurements: no
// rd_steps instance beat that chain at either size measured, so every instance stays behind the switch.
int plan_steps_per_launch(int w, int h) {
    (void)w, (void)h;
    return 0;
}

// HLMI_RD_STEPS_PER_LAUNCH, read once per call: *S = 1, 2 or 4, or the plan's choice where it is unset; any other value is refused
int steps_per_launch(void *uc, int w, int h, int *S) {
    *S = plan_steps_per_launch(w, h);
    if (const auto sw = env_int("HLMI_RD_STEPS_PER_LAUNCH")) {
        if (*sw != 1 && *sw != 2 && *sw != 4)
            return report(uc, halide_error_code_constraint_violated, "HLMI_RD_STEPS_PER_LAUNCH (%d) must be 1, 2 or 4", *sw);
        *S = *sw;
    }
    return 0;
}

bool ranges_overlap(uintptr_t a, size_t na, uintptr_t b, size_t nb) { return a && b && a < b + nb && b < a + na; }
// bytes from the first to one past the last element of a buffer with non-negative strides
size_t span_bytes(const halide_buffer_t *b) {
    size_t last = 0;
    for (int d = 0; d < b->dimensions; d++) {
        if (b->dim[d].extent <= 0) return 0;
        last += (size_t)(b->dim[d].extent - 1) * (size_t)std::abs(b->dim[d].stride);
    }
    return (last + 1) * (size_t)((b->type.bits + 7) / 8);
}

int run_entry(halide_buffer_t *state, int32_t mouse_x, int32_t mouse_y, int32_t frame0, int32_t steps, halide_buffer_t *new_state, halide_buffer_t *render,
              bool general_only) {
    void *uc = nullptr;
    BufArg args[3] = {{"state", state, T_F32, 3, false}, {"new_state", new_state, T_F32, 3, true}, {"render", render, T_U32, 2, true}};
    const int n = render ? 3 : 2;
    int r = check_not_null(uc, args, n);
    if (r) return r;
    if ((r = check_type_and_dims(uc, args, n))) return r;
    const halide_dimension_t *sd = state->dim, *od = new_state->dim;
    if (steps < 1) return report(uc, halide_error_code_constraint_violated, "hlmi_reaction_diffusion_run: steps (%d) must be at least 1", steps);
    if (!same_box_xy(sd, od)) return report(uc, halide_error_code_constraint_violated, "hlmi_reaction_diffusion_run: state and new_state must have the same box in x and y");
    if (render && !same_box_xy(sd, render->dim))
        return report(uc, halide_error_code_constraint_violated, "hlmi_reaction_diffusion_run: render must have the state's box in x and y");
    if (state == new_state || ranges_overlap((uintptr_t)state->host, span_bytes(state), (uintptr_t)new_state->host, span_bytes(new_state)) ||
        ranges_overlap((uintptr_t)state->device, span_bytes(state), (uintptr_t)new_state->device, span_bytes(new_state)))
        return report(uc, halide_error_code_constraint_violated, "hlmi_reaction_diffusion_run: state and new_state overlap");
    if ((r = check_shapes(uc, args, n))) return r;
    pin_channels(uc, state, "state.min.2", "state.extent.2");
    pin_channels(uc, new_state, "new_state.min.2", "new_state.extent.2");
    const bool some = sd[0].extent > 0 && sd[1].extent > 0;
    const Written w = written_by_updates(sd, mouse_x, mouse_y);
    if (some) {
        check_covers(uc, args[1], 0, w.x0, w.x1 - w.x0 + 1);
        check_covers(uc, args[1], 1, w.y0, w.y1 - w.y0 + 1);
    }
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, n))) return r;
    if (some) {
        const int W = sd[0].extent, H = sd[1].extent;
        int S = 0;
        if (!general_only && (r = steps_per_launch(uc, W, H, &S))) return r;
        const bool tiled = S > 0;
        if (!tiled) S = 1;
        // launches of S steps, then the remainder in launches of the next smaller instances: 5 with S = 2 is 2 + 2 + 1, 7 with S = 4 is 4 + 2 + 1
        int launches = 0;
        for (int left = steps, s = S; left > 0; s >>= 1) launches += left / s, left %= s;
        // the intermediate states alternate between one dense frame in the stream's workspace and new_state, so that the last lands in new_state
        float *ws = nullptr;
        if (launches > 1) {
            void *p = nullptr;
            if ((r = get_workspace(uc, ctx, sizeof(float) * 3 * (size_t)W * H, &p))) return r;
            ws = (float *)p;
        }
        RDGeom g = {};
        fill_state(g, state, dev_ptr<float>(state));
        g.ox = sd[0].min, g.oy = sd[1].min, g.ow = W, g.oh = H;
        g.mouse_x = mouse_x, g.mouse_y = mouse_y;
        g.cx0 = w.cx0, g.cx1 = w.cx1, g.cy0 = w.cy0, g.cy1 = w.cy1;
        if (render) g.pix = dev_ptr<uint32_t>(render), g.p_sy = render->dim[1].stride;
        int frame = frame0, i = 0;
        for (int left = steps, s = S; left > 0; s >>= 1) {
            for (; left >= s; left -= s, i++, frame = wrap_add(frame, s)) {
                const bool to_out = (launches - 1 - i) % 2 == 0, last = i == launches - 1;
                if (to_out) g.dst = dev_ptr<float>(new_state), g.d_sy = od[1].stride, g.d_sc = od[2].stride;
                else g.dst = ws, g.d_sy = W, g.d_sc = (long)W * H;
                g.frame = frame;
                if (!tiled) r = launch_update_general(uc, ctx.stream, g);
                else r = launch_steps(uc, ctx.stream, g, s, last && render);
                if (r) return r;
                g.src = g.dst, g.s_sy = g.d_sy, g.s_sc = g.d_sc;
            }
        }
        if (!tiled && render) {
            PGeom p = {dev_ptr<float>(new_state), od[1].stride, od[2].stride, g.pix, g.p_sy, W};
            if ((r = launch_render(uc, ctx.stream, p, H, general_only))) return r;
        }
    }
    mark_output_written(new_state);
    if (render) mark_output_written(render);
    return 0;
}

}  // namespace

extern "C" int reaction_diffusion_init(halide_buffer_t *output) { return init_entry(output, false); }
HLMI_ENTRY(reaction_diffusion_init, init_table.md)

extern "C" int reaction_diffusion_update(halide_buffer_t *state, int32_t mouse_x, int32_t mouse_y, int32_t frame, halide_buffer_t *new_state) {
    return update_entry(state, mouse_x, mouse_y, frame, new_state, false);
}
HLMI_ENTRY(reaction_diffusion_update, update_table.md)

extern "C" int reaction_diffusion_render(halide_buffer_t *state, halide_buffer_t *render) { return render_entry(state, render, false); }
HLMI_ENTRY(reaction_diffusion_render, render_table.md)

extern "C" int hlmi_reaction_diffusion_run(halide_buffer_t *state, int32_t mouse_x, int32_t mouse_y, int32_t frame0, int32_t steps, halide_buffer_t *new_state,
                                           halide_buffer_t *render) {
    return run_entry(state, mouse_x, mouse_y, frame0, steps, new_state, render, false);
}

// Measurement and test hook (hlmi_internal.h): the named entry point, or "run", with one thread per output and one launch per step.
extern "C" int hlmi_reaction_diffusion_general(const char *name, halide_buffer_t *state, int32_t mouse_x, int32_t mouse_y, int32_t frame, int32_t steps,
                                               halide_buffer_t *out, halide_buffer_t *render) {
    if (name && strcmp(name, "reaction_diffusion_init") == 0) return init_entry(out, true);
    if (name && strcmp(name, "reaction_diffusion_update") == 0) return update_entry(state, mouse_x, mouse_y, frame, out, true);
    if (name && strcmp(name, "reaction_diffusion_render") == 0) return render_entry(state, render, true);
    if (name && strcmp(name, "run") == 0) return run_entry(state, mouse_x, mouse_y, frame, steps, out, render, true);
    return report(nullptr, halide_error_code_constraint_violated, "hlmi_reaction_diffusion_general: no entry point named %s", name ? name : "(null)");
}
