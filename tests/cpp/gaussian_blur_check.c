/* gaussian_blur_check.c — the checker of the gaussian_blur pipelines: the arithmetic of
 * apps/gaussian_blur/gaussian_blur_generator.cpp restated in plain C, one rounding per operator (no contraction by the
 * compiler), every fused operation written out.  tests/checker_lib.py holds the build line: it links this file, with the other
 * *_check.c files, into one shared object and drives it through ctypes.  Written from the generator's text:
 *
 *   :18-63    direct_gaussian_blur: the kernel table, its sum, the normalised table, the two passes
 *   :68-100   gaussian_blur_direct: repeat_edge of the input in front of it
 *   :117-150  make_resampling_kernel: `order` boxes of width `factor` and order - 1 [1 1] filters, and its variance
 *   :160-214  the resampled blur: down_y in phases, down_x, sigma_lo, the second row clamp, the small blur, the two expansions
 *
 * Two canonical float forms, those of oracle/oracle_common.h, whose o_mad / o_mad2 / o_mulsub and o_halide_exp are used as they
 * are (the device's halide_exp is held to that one bit for bit by tests/test_device_math.py): ck_set_canon(0) (check_canon.c)
 * rounds every operator on its own, ck_set_canon(1) contracts a multiply with one use that feeds an add or a subtract.
 *
 * Zero folding.  The expansions are written `e = 0.f; e += t_0; e += t_1; ...` on Exprs (:197-200, :207-210), and Halide's
 * simplifier folds `0.f + t_0` to `t_0`; this checker follows it: e = t_0 + t_1 + ... with no leading zero, so a result of -0
 * stays -0, and in form 1 the first add sees two products and contracts the first (o_mad2), every later one its own product
 * (o_mad).  The sums of the reductions (sum(), `+=` on a Func) are stores of 0 followed by updates and keep their zero:
 * s = mad(a, b, s) from 0.0f, and down_y = 0 + phase_0 + phase_1 + ... */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "oracle_common.h"

static int gc_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
static int gc_div_up(int a, int b) { return o_fdiv(a + b - 1, b); }

/* ------------------------------------------------------------------------------------------------ the direct blur (:18-63) */
int gc_radius(float sigma, int trunc) { return (int)ceilf((float)trunc * sigma); }

/* kn[0 .. 2 * radius] = kernel_normalized(-radius .. radius); *sum = kernel_sum (may be NULL) */
void gc_kernel_table(float sigma, int radius, float *kn, float *sum) {
    const float denom = (2.0f * sigma) * sigma;
    float s = 0.0f;
    for (int x = -radius; x <= radius; x++) {
        kn[x + radius] = o_halide_exp((float)(-(x * x)) / denom);
        s = s + kn[x + radius];
    }
    for (int i = 0; i <= 2 * radius; i++) kn[i] = kn[i] / s;
    if (sum) *sum = s;
}

/* The two passes over a dense source src[sh][sw] whose rows AND columns are clamped (the direct blur's repeat_edge; the small
 * blur's callers pass a source that covers every column it reads, so that its column clamp never acts).  The output region
 * [x0, x0 + ow) x [y0, y0 + oh) is in the source's own coordinates.  blur_y is evaluated on the source's columns only: at a
 * column outside them it is blur_y at the clamped column. */
static int gc_blur(const float *src, int sw, int sh, const float *kn, int radius, float *out, int x0, int y0, int ow, int oh) {
    float *mid = malloc(sizeof(float) * (size_t)sw * (size_t)oh);
    if (!mid) return -1;
    for (int y = 0; y < oh; y++)
        for (int x = 0; x < sw; x++) {
            float s = 0.0f;
            for (int r = -radius; r <= radius; r++) s = o_mad(kn[r + radius], src[(size_t)gc_clampi(y0 + y + r, 0, sh - 1) * sw + x], s);
            mid[(size_t)y * sw + x] = s;
        }
    for (int y = 0; y < oh; y++)
        for (int x = 0; x < ow; x++) {
            float s = 0.0f;
            for (int r = -radius; r <= radius; r++) s = o_mad(kn[r + radius], mid[(size_t)y * sw + gc_clampi(x0 + x + r, 0, sw - 1)], s);
            out[(size_t)y * ow + x] = s;
        }
    free(mid);
    return 0;
}

/* in: dense [H][W] at absolute (ix0, iy0); out: dense [oh][ow] at absolute (ox0, oy0).  Returns 0, -1 out of memory. */
int gc_direct(const float *in, int ix0, int iy0, int W, int H, float sigma, int trunc, float *out, int ox0, int oy0, int ow, int oh) {
    if (ow <= 0 || oh <= 0) return 0;
    const int radius = gc_radius(sigma, trunc);
    float *kn = malloc(sizeof(float) * (2 * (size_t)radius + 1));
    if (!kn) return -1;
    gc_kernel_table(sigma, radius, kn, NULL);
    const int r = gc_blur(in, W, H, kn, radius, out, ox0 - ix0, oy0 - iy0, ow, oh);
    free(kn);
    return r;
}

/* ------------------------------------------------------------------------------------------------ resampling kernels (:117-150)
 * k[0 .. order * F): the generator's own evaluation in f32.  Every value is a dyadic rational with a numerator below 2^12, so
 * each operation here is exact. */
#define GC_DOM 256
#define GC_OFF 96
void gc_resampling_kernel(int order, int F, float *k) {
    float box[GC_DOM], cur[GC_DOM], next[GC_DOM];
    for (int i = 0; i < GC_DOM; i++) box[i] = (i - GC_OFF >= 0 && i - GC_OFF < F) ? 1.0f / (float)F : 0.0f;
    memcpy(cur, box, sizeof cur);
    for (int i = 1; i < order; i++) {
        for (int x = 0; x < GC_DOM; x++) {   /* next(x) = sum over r_box of kernel(x - r) * box(r); outside the array: zeros */
            float s = 0.0f;
            for (int r = 0; r < F; r++) s = s + (x - r >= 0 ? cur[x - r] : 0.0f) * box[r + GC_OFF];
            next[x] = s;
        }
        for (int x = 0; x < GC_DOM; x++) cur[x] = (next[x] + (x >= 1 ? next[x - 1] : 0.0f)) * 0.5f;
    }
    for (int x = 0; x < order * F; x++) k[x] = cur[x + GC_OFF];
}

float gc_variance(int order, int F) {
    float variance = (float)order * ((float)F * (float)F - 1.0f) / 12.0f;
    variance += (float)(order - 1) / 4.0f;
    return variance;
}

float gc_sigma_lo(int U, int D, int F, float sigma) {
    const float t = o_mulsub(sigma, sigma, gc_variance(U, F)) - gc_variance(D, F);
    return sqrtf(t > 1e-4f ? t : 1e-4f) / (float)F;
}

/* ------------------------------------------------------------------------------------------------ the resampled blur (:160-214)
 * in: dense [H][W] at absolute (ix0, iy0); out: dense [oh][ow] at (0, 0).  Returns 0, -1 out of memory. */
int gc_resampled(int U, int D, int F, const float *in, int ix0, int iy0, int W, int H, float sigma, int trunc, float *out, int ow, int oh) {
    if (ow <= 0 || oh <= 0) return 0;
    float dk[64], uk[64];
    gc_resampling_kernel(D, F, dk);
    gc_resampling_kernel(U, F, uk);
    const int shift = o_fdiv((U - D) * F, 2);
    const float sigma_lo = gc_sigma_lo(U, D, F, sigma);
    const int radius = gc_radius(sigma_lo, trunc);
    /* the low-resolution region the expansions read: blurred on [bx0, bx1] x [by0, by1]; the small blur reads down_x on the
     * columns [bx0 - radius, bx1 + radius] and on the rows [by0 - radius, by1 + radius] clamped to [-U, div_up(H, F)] (:191) */
    const int bx0 = -(U - 1), bx1 = o_fdiv(ow - 1, F), by0 = -(U - 1), by1 = o_fdiv(oh - 1, F);
    const int lx0 = bx0 - radius, lw = bx1 + radius - lx0 + 1;
    const int ly0 = gc_clampi(by0 - radius, -U, gc_div_up(H, F)), ly1 = gc_clampi(by1 + radius, -U, gc_div_up(H, F));
    const int lh = ly1 - ly0 + 1, bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
    float *kn = malloc(sizeof(float) * (2 * (size_t)radius + 1));
    float *dy = malloc(sizeof(float) * (size_t)W), *lo = malloc(sizeof(float) * (size_t)lw * lh);
    float *bl = malloc(sizeof(float) * (size_t)bw * bh), *ux = malloc(sizeof(float) * (size_t)ow * bh);
    if (!kn || !dy || !lo || !bl || !ux) return -1;
    gc_kernel_table(sigma_lo, radius, kn, NULL);
    for (int yl = ly0; yl <= ly1; yl++) {
        for (int x = 0; x < W; x++) {   /* down_y on the input's columns */
            float d = 0.0f;
            for (int p = 0; p < D; p++) {
                float s = 0.0f;
                for (int rf = 0; rf < F; rf++) {
                    const int y = gc_clampi(F * (yl + p) + rf + shift, iy0, iy0 + H - 1);
                    s = o_mad(in[(size_t)(y - iy0) * W + x], dk[rf + p * F], s);
                }
                d = d + s;
            }
            dy[x] = d;
        }
        for (int xl = lx0; xl < lx0 + lw; xl++) {
            float s = 0.0f;
            for (int rx = 0; rx < F * D; rx++) s = o_mad(dy[gc_clampi(F * xl + rx + shift, ix0, ix0 + W - 1) - ix0], dk[rx], s);
            lo[(size_t)(yl - ly0) * lw + (xl - lx0)] = s;
        }
    }
    /* clamping the rows to [ly0, ly1] is clamping them to [-U, div_up(H, F)]: both ends are images of that clamp */
    if (gc_blur(lo, lw, lh, kn, radius, bl, bx0 - lx0, by0 - ly0, bw, bh)) return -1;
    float c[4];
    for (int yl = 0; yl < bh; yl++)
        for (int x = 0; x < ow; x++) {
            const int xl = o_fdiv(x, F), p = o_fmod(x, F);
            const float *b = bl + (size_t)yl * bw + (xl - bx0);
            for (int i = 0; i < U; i++) c[i] = uk[i * F + p] * (float)F;
            float e = o_mad2(b[0], c[0], b[-1], c[1]);
            for (int i = 2; i < U; i++) e = o_mad(b[-i], c[i], e);
            ux[(size_t)yl * ow + x] = e;
        }
    for (int y = 0; y < oh; y++) {
        const int yl = o_fdiv(y, F), p = o_fmod(y, F);
        for (int i = 0; i < U; i++) c[i] = uk[i * F + p] * (float)F;
        for (int x = 0; x < ow; x++) {
            const float *u = ux + (size_t)(yl - by0) * ow + x;
            float e = o_mad2(u[0], c[0], u[-(ptrdiff_t)ow], c[1]);
            for (int i = 2; i < U; i++) e = o_mad(u[-(ptrdiff_t)i * ow], c[i], e);
            out[(size_t)y * ow + x] = e;
        }
    }
    free(kn), free(dy), free(lo), free(bl), free(ux);
    return 0;
}
