/* resize_check.c — the checker of the resize pipelines: the arithmetic of apps/resize/resize_generator.cpp restated in
 * plain C, one rounding per operator (no contraction by the compiler), every fused operation written out.
 * tests/checker_lib.py holds the build line: it links this file, with the other *_check.c files, into one shared object
 * and drives it through ctypes.
 * Written from the generator's text:
 *
 *   :12-46   the four kernels (box, linear, cubic, lanczos)
 *   :85-147  inverse factor, kernel scaling, radius, taps, source coordinates, begin, weights, the two sums, the cast
 *
 * Two canonical float forms, those of oracle/oracle_common.h, whose o_mad and o_mulsub are used as they are:
 * ck_set_canon(0) (check_canon.c) rounds every operator on its own, ck_set_canon(1) contracts a multiply with one use
 * that feeds an add or a subtract.  The `begin` expression sits under strict_float in the generator and is never
 * contracted.  sin() is rc_halide_sin, the routine the device uses (hlmi_device_math.h: dev::halide_sin), the same in
 * both forms: the reference's CPU targets call libm there, one opaque function, and no device routine can be bit-equal
 * to it.
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "oracle_common.h"

/* ------------------------------------------------------------------------------------------------ sin
 * Specified for |x| <= 3 pi (1 + eps) only (the lanczos window cuts at |x| = 3 before the multiplication by pi).
 * k = nearest integer to x * 2/pi (|k| <= 6), r = x - k * pi/2 with pi/2 = P1 + P2 + P3: P1 and P2 carry 21 bits, so
 * k * P1 and k * P2 are exact, x - k * P1 is exact, and the second subtraction is an error-free two-sum (hi, lo);
 * sin or cos of hi + lo by Taylor polynomials on |r| <= pi/4, first-order correction for lo.  No fused operation. */
float rc_halide_sin(float x) {
    const float two_over_pi = 0x1.45f306p-1f;
    const float P1 = 0x1.921fbp+0f, P2 = 0x1.5110bp-22f, P3 = 0x1.184698p-44f;
    const float kf = rintf(x * two_over_pi);
    const int k = (int)kf;
    const float a = x - kf * P1;
    const float b = kf * P2;
    const float hi = a - b;
    const float bb = hi - a;
    float lo = (a - (hi - bb)) - (b + bb);
    lo = lo - kf * P3;
    const float z = hi * hi;
    float r;
    if (k & 1) {
        float c = 0x1.1eed8ep-29f;                 /* 1/12! */
        c = c * z - 0x1.27e4fcp-22f;               /* 1/10! */
        c = c * z + 0x1.a01a02p-16f;               /* 1/8! */
        c = c * z - 0x1.6c16c2p-10f;               /* 1/6! */
        c = c * z + 0x1.555556p-5f;                /* 1/4! */
        const float h = 0.5f * z, w = 1.0f - h;
        r = w + (((1.0f - w) - h) + ((z * z) * c - hi * lo));
    } else {
        float s = -0x1.ae6456p-26f;                /* 1/11! */
        s = s * z + 0x1.71de3ap-19f;               /* 1/9! */
        s = s * z - 0x1.a01a02p-13f;               /* 1/7! */
        s = s * z + 0x1.111112p-7f;                /* 1/5! */
        s = s * z - 0x1.555556p-3f;                /* 1/3! */
        r = hi + ((hi * z) * s + lo * (1.0f - 0.5f * z));
    }
    return (k & 2) ? -r : r;
}

void rc_sin_array(const float *x, float *out, size_t n) {
    for (size_t i = 0; i < n; i++) out[i] = rc_halide_sin(x[i]);
}

/* The largest error, in units in the last place of the correctly rounded value, of rc_halide_sin and of libm's sinf over
 * every float of both signs with bit patterns in [lo_bits, hi_bits].  worst_x[2] = where each maximum was seen. */
void rc_sin_sweep(uint32_t lo_bits, uint32_t hi_bits, double *max_ulp, float *worst_x) {
    max_ulp[0] = max_ulp[1] = 0.0;
    worst_x[0] = worst_x[1] = 0.0f;
    for (int sign = 0; sign < 2; sign++) {
        for (uint32_t u = lo_bits; u <= hi_bits; u++) {
            const uint32_t bits = u | ((uint32_t)sign << 31);
            float x;
            memcpy(&x, &bits, 4);
            const double exact = sin((double)x);
            const float ref = (float)exact;
            int e;
            frexp((double)ref, &e);                             /* |ref| in [2^(e-1), 2^e): ulp = 2^(e-24) */
            const double ulp = ldexp(1.0, (e - 24 < -149) ? -149 : e - 24);
            const double d0 = fabs((double)rc_halide_sin(x) - exact) / ulp, d1 = fabs((double)sinf(x) - exact) / ulp;
            if (d0 > max_ulp[0]) max_ulp[0] = d0, worst_x[0] = x;
            if (d1 > max_ulp[1]) max_ulp[1] = d1, worst_x[1] = x;
        }
    }
}

/* ------------------------------------------------------------------------------------------------ kernels (:12-46) */
enum { RC_BOX = 0, RC_LINEAR = 1, RC_CUBIC = 2, RC_LANCZOS = 3 };
static const int rc_taps_of[4] = {1, 2, 4, 6};

static float rc_sinc(float x) {
    x = x * 3.14159265359f;
    return rc_halide_sin(x) / x;
}

static float rc_kernel(int kind, float x) {
    const float xx = fabsf(x);
    switch (kind) {
        case RC_BOX: return xx <= 0.5f ? 1.0f : 0.0f;
        case RC_LINEAR: return xx < 1.0f ? 1.0f - xx : 0.0f;
        case RC_CUBIC: {
            const float xx2 = xx * xx, xx3 = xx2 * xx;
            /* a = -0.5: (a + 2) xx3 - (a + 3) xx2 + 1  and  a xx3 - 5a xx2 + 8a xx - 4a, constants folded in C++ */
            const float inner = o_mulsub(1.5f, xx3, 2.5f * xx2) + 1.0f;
            const float outer = o_mad(-4.0f, xx, o_mulsub(-0.5f, xx3, -2.5f * xx2)) - -2.0f;
            return xx < 1.0f ? inner : (xx < 2.0f ? outer : 0.0f);
        }
        default: {
            float value = rc_sinc(x) * rc_sinc(x / 3.0f);
            if (x == 0.0f) value = 1.0f;
            if (x > 3.0f || x < -3.0f) value = 0.0f;
            return value;
        }
    }
}

/* ------------------------------------------------------------------------------------------------ tables (:85-127)
 * taps for (kind, direction, factor); < 1 or not a number when the factor is unusable */
static float rc_inverse(float scale) {
    volatile float one = 1.0f;   /* one correctly rounded division, kept from being folded into a reciprocal */
    return one / scale;
}

float rc_taps_f(int kind, int up, float scale) {
    const float iks = up ? 1.0f : rc_inverse(scale);
    return ceilf((float)rc_taps_of[kind] * iks);
}

/* begin[n], weights w[k * n + i] (k < taps), sums[n] for output coordinates out_min .. out_min + n - 1 along one axis of
 * an input spanning [in_min, in_min + in_extent).  Returns taps, or -4 when !(1 <= taps <= in_extent). */
int rc_tables(int kind, int up, float scale, int out_min, int n, int in_min, int in_extent, int *begin, float *w, float *sums) {
    const float inv = rc_inverse(scale);
    const float ks = up ? 1.0f : scale, iks = up ? 1.0f : inv;
    const float radius = (0.5f * (float)rc_taps_of[kind]) * iks;
    const float taps_f = ceilf((float)rc_taps_of[kind] * iks);
    if (!(taps_f >= 1.0f && taps_f <= (float)in_extent)) return -4;
    const int taps = (int)taps_f;
    for (int i = 0; i < n; i++) {
        const float xf = (float)(out_min + i) + 0.5f;
        /* strict_float: every operation rounded on its own in both forms */
        const float strict_src = xf * inv - 0.5f;
        int b = (int)ceilf(strict_src - radius);
        const int hi = in_min + in_extent - 1 + 1 - taps;
        b = b < hi ? b : hi;
        b = b > in_min ? b : in_min;
        begin[i] = b;
        const float src = o_mulsub(xf, inv, 0.5f);
        float sum = 0.0f;
        for (int k = 0; k < taps; k++) {
            float arg = (float)(k + b) - src;
            if (!up) arg = arg * ks;
            const float u = rc_kernel(kind, arg);
            w[(size_t)k * n + i] = u;
            sum = sum + u;
        }
        for (int k = 0; k < taps; k++) w[(size_t)k * n + i] = w[(size_t)k * n + i] / sum;
        if (sums) sums[i] = sum;
    }
    return taps;
}

/* ------------------------------------------------------------------------------------------------ the pipeline (:129-147)
 * type: 0 f32, 1 u8, 2 u16.  Dense planar buffers [c][y][x]; mins and extents in the order x, y, c.  The output's
 * channel range must lie inside the input's.  Returns 0, -4 as rc_tables, -1 out of memory. */
static float rc_load(const void *p, int type, size_t i) {
    return type == 0 ? ((const float *)p)[i] : type == 1 ? (float)((const uint8_t *)p)[i] : (float)((const uint16_t *)p)[i];
}

static void rc_store(void *p, int type, size_t i, float v) {
    if (type == 0) {
        const float m = v < 1.0f ? v : 1.0f;
        ((float *)p)[i] = m > 0.0f ? m : 0.0f;
    } else {
        const float top = type == 1 ? 255.0f : 65535.0f;
        const float m = v < top ? v : top;
        const float c = m > 0.0f ? m : 0.0f;
        if (type == 1) ((uint8_t *)p)[i] = (uint8_t)(int)c;
        else ((uint16_t *)p)[i] = (uint16_t)(int)c;
    }
}

int rc_resize(int kind, int type, int up, float scale, const void *in, const int *in_min, const int *in_ext, void *out,
              const int *out_min, const int *out_ext) {
    const int ow = out_ext[0], oh = out_ext[1], oc = out_ext[2], W = in_ext[0], H = in_ext[1];
    if (ow <= 0 || oh <= 0 || oc <= 0) return 0;
    const float tf = rc_taps_f(kind, up, scale);
    if (!(tf >= 1.0f && tf <= (float)W && tf <= (float)H)) return -4;
    const int taps = (int)tf;
    int *bx = malloc(sizeof(int) * ow), *by = malloc(sizeof(int) * oh);
    float *wx = malloc(sizeof(float) * (size_t)taps * ow), *wy = malloc(sizeof(float) * (size_t)taps * oh);
    /* intermediate: _up  resized_x over [ow][H rows of the input];  _down  resized_y over [W columns][oh] */
    const size_t mid_w = up ? ow : W, mid_h = up ? H : oh;
    float *mid = malloc(sizeof(float) * mid_w * mid_h);
    if (!bx || !by || !wx || !wy || !mid) return -1;
    rc_tables(kind, up, scale, out_min[0], ow, in_min[0], W, bx, wx, NULL);
    rc_tables(kind, up, scale, out_min[1], oh, in_min[1], H, by, wy, NULL);
    for (int c = 0; c < oc; c++) {
        const size_t plane = (size_t)(out_min[2] + c - in_min[2]) * W * H;
        if (up) {
            for (int y = 0; y < H; y++)
                for (int x = 0; x < ow; x++) {
                    float s = 0.0f;
                    for (int k = 0; k < taps; k++) s = o_mad(wx[(size_t)k * ow + x], rc_load(in, type, plane + (size_t)y * W + (bx[x] + k - in_min[0])), s);
                    mid[(size_t)y * ow + x] = s;
                }
            for (int y = 0; y < oh; y++)
                for (int x = 0; x < ow; x++) {
                    float s = 0.0f;
                    for (int k = 0; k < taps; k++) s = o_mad(wy[(size_t)k * oh + y], mid[(size_t)(by[y] + k - in_min[1]) * ow + x], s);
                    rc_store(out, type, ((size_t)c * oh + y) * ow + x, s);
                }
        } else {
            for (int y = 0; y < oh; y++)
                for (int x = 0; x < W; x++) {
                    float s = 0.0f;
                    for (int k = 0; k < taps; k++) s = o_mad(wy[(size_t)k * oh + y], rc_load(in, type, plane + (size_t)(by[y] + k - in_min[1]) * W + x), s);
                    mid[(size_t)y * W + x] = s;
                }
            for (int y = 0; y < oh; y++)
                for (int x = 0; x < ow; x++) {
                    float s = 0.0f;
                    for (int k = 0; k < taps; k++) s = o_mad(wx[(size_t)k * ow + x], mid[(size_t)y * W + (bx[x] + k - in_min[0])], s);
                    rc_store(out, type, ((size_t)c * oh + y) * ow + x, s);
                }
        }
    }
    free(bx), free(by), free(wx), free(wy), free(mid);
    return 0;
}
