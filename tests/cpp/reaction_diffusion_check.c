/* reaction_diffusion_check.c — the checker of reaction_diffusion_init, reaction_diffusion_update and reaction_diffusion_render: the
 * arithmetic of apps/HelloWasm/generator/reaction_diffusion_generator.cpp restated in plain C, one rounding per operator (no contraction
 * by the compiler), the fused operations written out.  tests/reaction_diffusion_checker.py declares the object (tests/checker_lib.py
 * links this file with check_canon.c into a shared object of its own) and drives it through ctypes.  Written from the generator's text:
 *
 *   :10-12    init: output(x, y, c) = random_float()
 *   :35-47    clamped = repeat_edge(state) over the state's own min and extent; blur_x, blur_y the five-tap sums, left to right as
 *             written; blur = (blur_x + blur_y) / 10 -> * fold(1 / 10) (src/Simplify_Div.cpp:204)
 *   :53-57    R *= (1 - s) + s * R * (3 - 2 * R), s = 0.5f: R * (0.5f + (0.5f * R) * (3 - 2 * R))
 *   :60-62    dR = B * ((1 - R) - G), dG = (1 - B) * (R - G), dB = (((1 - B) + (2 * G) * R) - R) - G
 *   :65-67    boost = 5 * max(0, 1.f - (mx * mx + my * my) * 0.001f) + 1, mx = mouse_x - x, my = mouse_y - y, the squared distance
 *             int32 (wrapping here) converted to float
 *   :69-75    R += (dR * 0.14f) * boost, G += (dG * 0.05f) * boost, B += (dB * 0.065f) * boost; clamp(., 0, 1) = max(min(., 1), 0)
 *   :80-83    the four edge updates, in this order: row state.min(1), row state.max(1), column state.min(0), column state.max(0), each
 *             random_float(frame) * 0.2f over the output's range in the other dimension
 *   :85-90    noise = random_float(frame); blurry_noise = 0.25f * (((n(x, y) + n(x + 1, y)) + n(x + 1, y + 1)) + n(x, y + 1))
 *   :93-104   the clobber: x in [clamp(mouse_x - 10, 0, W - 1), clamp(mouse_x + 10, 0, W - 1)], y alike, W and H the state's EXTENTS;
 *             where float(dx * dx + dy * dy) < 100.0f the pixel becomes blurry_noise
 *   :150-174  render
 *
 * Two canonical float forms, those of oracle/oracle_common.h (ck_set_canon in check_canon.c selects one).  The multiplies with one use
 * that feed an add or a subtract, and so fuse in canon 1: (0.5f * R) * (3 - 2 R) into + 0.5f; 2 * R into 3 - (exact either way);
 * (2 * G) * R into + (1 - B); d2 * 0.001f into 1.f -; 5 * max into + 1; (d * rate) * boost into R +=.  Everything else is a multiply
 * that feeds a multiply, a subtract of two values, or a sum.  Render has no multiply that feeds an add: its two forms agree.
 *
 * The random hash (src/Random.cpp:14-98) is restated here independently of halide_amd/csrc/hlmi_random.h; the (call id, definition
 * tag) pairs are the ONE table rdc_random below, derived in DESIGN.md 5.16 and not confirmed against a Halide build. */
#include <stddef.h>
#include <stdint.h>

#include "oracle_common.h"

/* ---- the hash */
static uint32_t rdc_rng32(uint32_t x) { return (1040796640u * x + 1121052041u) * x + 576942909u; }

/* random_int of an argument list (src/Random.cpp:66-90) */
uint32_t rdc_random_int(const int32_t *e, int n) {
    uint32_t r = rdc_rng32((uint32_t)e[0]);
    for (int i = 1; i < n; i++) r = rdc_rng32(r + (uint32_t)e[i]);
    return r ^ (r >> 16);
}

/* random_float of an argument list (src/Random.cpp:92-98) */
float rdc_random_float(const int32_t *e, int n) {
    const float f = o_bits2f((127u << 23) | (rdc_random_int(e, n) >> 9)) - 1.0f;
    return o_clampf(f, 0.0f, 1.0f);
}

/* (call id, definition tag): init; row min, row max, column min, column max; noise */
enum { RC_INIT, RC_ROW_MIN, RC_ROW_MAX, RC_COL_MIN, RC_COL_MAX, RC_NOISE };
static const int32_t rdc_random[6][2] = {{0, 0}, {0, 6}, {1, 7}, {2, 8}, {3, 9}, {4, 10}};

int rdc_table(int which, int field) { return rdc_random[which][field]; }

static int32_t wrap_sub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
static int32_t wrap_add(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
static int32_t sq_sum(int32_t a, int32_t b) { return (int32_t)((uint32_t)a * (uint32_t)a + (uint32_t)b * (uint32_t)b); }

/* init: [id, tag, c, y, x] */
float rdc_init_value(int x, int y, int c) {
    const int32_t e[5] = {rdc_random[RC_INIT][0], rdc_random[RC_INIT][1], c, y, x};
    return rdc_random_float(e, 5);
}
/* edge rows: [frame, id, tag, c, x]; edge columns: [frame, id, tag, c, y] */
float rdc_edge_value(int which, int frame, int c, int v) {
    const int32_t e[5] = {frame, rdc_random[which][0], rdc_random[which][1], c, v};
    return rdc_random_float(e, 5) * 0.2f;
}
/* noise: [frame, id, tag, c, y, x] */
float rdc_noise(int frame, int x, int y, int c) {
    const int32_t e[6] = {frame, rdc_random[RC_NOISE][0], rdc_random[RC_NOISE][1], c, y, x};
    return rdc_random_float(e, 6);
}
float rdc_blurry_noise(int frame, int x, int y, int c) {
    const int x1 = wrap_add(x, 1), y1 = wrap_add(y, 1);
    return 0.25f * (((rdc_noise(frame, x, y, c) + rdc_noise(frame, x1, y, c)) + rdc_noise(frame, x1, y1, c)) + rdc_noise(frame, x, y1, c));
}

/* out[c][y][x] dense over [ox, ox + ow) x [oy, oy + oh) x [oc, oc + on) */
int rdc_init(float *out, int ox, int oy, int oc, int ow, int oh, int on) {
    for (int c = 0; c < on; c++)
        for (int y = 0; y < oh; y++)
            for (int x = 0; x < ow; x++) out[((size_t)c * oh + y) * ow + x] = rdc_init_value(ox + x, oy + y, oc + c);
    return 0;
}

static int64_t rdc_clamp(int64_t v, int64_t lo, int64_t hi) { /* max(min(v, hi), lo) */
    const int64_t m = v < hi ? v : hi;
    return m > lo ? m : lo;
}

/* the clobber box of a W x H state: {x0, x1, y0, y1} */
void rdc_clobber_box(int W, int H, int mouse_x, int mouse_y, int *box) {
    box[0] = (int)rdc_clamp(wrap_sub(mouse_x, 10), 0, (int64_t)W - 1), box[1] = (int)rdc_clamp(wrap_add(mouse_x, 10), 0, (int64_t)W - 1);
    box[2] = (int)rdc_clamp(wrap_sub(mouse_y, 10), 0, (int64_t)H - 1), box[3] = (int)rdc_clamp(wrap_add(mouse_y, 10), 0, (int64_t)H - 1);
}

/* the pure stage at (X, Y): v[0 .. 2] */
static void rdc_pure(const float *state, int sx0, int sy0, int sw, int sh, int mouse_x, int mouse_y, int X, int Y, float *v) {
    float p[3];
    for (int c = 0; c < 3; c++) {
        const float *pl = state + (size_t)c * sh * sw;
        float t[2][5];
        for (int j = 0; j < 5; j++) {
            const int64_t xx = rdc_clamp((int64_t)X + j - 2, sx0, (int64_t)sx0 + sw - 1) - sx0, yy = rdc_clamp((int64_t)Y + j - 2, sy0, (int64_t)sy0 + sh - 1) - sy0;
            const int64_t x0 = rdc_clamp(X, sx0, (int64_t)sx0 + sw - 1) - sx0, y0 = rdc_clamp(Y, sy0, (int64_t)sy0 + sh - 1) - sy0;
            t[0][j] = pl[y0 * sw + xx], t[1][j] = pl[yy * sw + x0];
        }
        const float bx = (((t[0][0] + t[0][1]) + t[0][2]) + t[0][3]) + t[0][4];
        const float by = (((t[1][0] + t[1][1]) + t[1][2]) + t[1][3]) + t[1][4];
        const float b = (bx + by) * (1.0f / 10.0f);
        p[c] = b * o_mad(0.5f * b, o_msub(3.0f, 2.0f, b), 0.5f);
    }
    float R = p[0], G = p[1], B = p[2];
    const float dR = B * ((1.0f - R) - G);
    const float dG = (1.0f - B) * (R - G);
    const float dB = (o_mad(2.0f * G, R, 1.0f - B) - R) - G;
    const float d2 = (float)sq_sum(wrap_sub(mouse_x, X), wrap_sub(mouse_y, Y));
    const float fall = o_msub(1.0f, d2, 0.001f);
    const float boost = o_mad(5.0f, 0.0f > fall ? 0.0f : fall, 1.0f);
    R = o_mad(dR * 0.14f, boost, R);
    G = o_mad(dG * 0.05f, boost, G);
    B = o_mad(dB * 0.065f, boost, B);
    v[0] = o_clampf(R, 0.0f, 1.0f), v[1] = o_clampf(G, 0.0f, 1.0f), v[2] = o_clampf(B, 0.0f, 1.0f);
}

/* state[c][y][x] dense over [sx0, sx0 + sw) x [sy0, sy0 + sh) x [0, 3); out[c][y][x] dense over [ox, ox + ow) x [oy, oy + oh) x [0, 3).
 * stage: 0 the pure stage alone, 1 + the four edge updates, 2 everything.  Returns -4, and writes nothing, for an output that does
 * not hold what the update definitions write, and for an empty state under an output that is not empty. */
int rdc_update(const float *state, int sx0, int sy0, int sw, int sh, int mouse_x, int mouse_y, int frame, int stage, float *out, int ox, int oy, int ow,
               int oh) {
    if (ow <= 0 || oh <= 0) return 0;
    if (sw <= 0 || sh <= 0) return -4;
    const int xmax = sx0 + sw - 1, ymax = sy0 + sh - 1;
    int box[4];
    rdc_clobber_box(sw, sh, mouse_x, mouse_y, box);
    const int64_t ox1 = (int64_t)ox + ow - 1, oy1 = (int64_t)oy + oh - 1;
    if (sx0 < ox || xmax > ox1 || box[0] < ox || box[1] > ox1 || sy0 < oy || ymax > oy1 || box[2] < oy || box[3] > oy1) return -4;
    for (int y = 0; y < oh; y++)
        for (int x = 0; x < ow; x++) {
            const int X = ox + x, Y = oy + y;
            float v[3];
            rdc_pure(state, sx0, sy0, sw, sh, mouse_x, mouse_y, X, Y, v);
            for (int c = 0; c < 3 && stage >= 1; c++) {
                if (Y == sy0) v[c] = rdc_edge_value(RC_ROW_MIN, frame, c, X);
                if (Y == ymax) v[c] = rdc_edge_value(RC_ROW_MAX, frame, c, X);
                if (X == sx0) v[c] = rdc_edge_value(RC_COL_MIN, frame, c, Y);
                if (X == xmax) v[c] = rdc_edge_value(RC_COL_MAX, frame, c, Y);
            }
            if (stage >= 2 && X >= box[0] && X <= box[1] && Y >= box[2] && Y <= box[3] &&
                (float)sq_sum(wrap_sub(X, mouse_x), wrap_sub(Y, mouse_y)) < 100.0f)
                for (int c = 0; c < 3; c++) v[c] = rdc_blurry_noise(frame, X, Y, c);
            for (int c = 0; c < 3; c++) out[((size_t)c * oh + y) * ow + x] = v[c];
        }
    return 0;
}

/* one packed pixel from the three state values */
uint32_t rdc_pack(float s0, float s1, float s2) {
    const float s[3] = {s0, s1, s2};
    float k[3];
    for (int c = 0; c < 3; c++) {
        float v = (s[c] * (1.01f - s[c])) * 4.0f;
        v = v * v;
        v = v * v;
        k[c] = v < 1.0f ? v : 1.0f;
    }
    const float half = (k[1] + k[2]) * 0.5f;
    const float R = k[0] < half ? k[0] : half;
    const float G = o_clampf(((k[1] + k[0]) + k[2]) * 0.5f, 0.0f, 1.0f);
    const float m12 = k[1] > k[2] ? k[1] : k[2];
    const float B = k[0] > m12 ? k[0] : m12;
    const uint32_t r = (uint32_t)(R * 255.0f) & 0xffu, g = (uint32_t)(G * 255.0f) & 0xffu, b = (uint32_t)(B * 255.0f) & 0xffu;
    return b | (g << 8) | (r << 16) | (255u << 24);
}

/* state[c][y][x] dense, w x h x 3; out[y][x] */
int rdc_render(const float *state, uint32_t *out, int w, int h) {
    const size_t n = (size_t)w * h;
    for (size_t i = 0; i < n; i++) out[i] = rdc_pack(state[i], state[n + i], state[2 * n + i]);
    return 0;
}
