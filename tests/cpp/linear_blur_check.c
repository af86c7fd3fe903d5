/* linear_blur_check.c — the checker of simple_blur and linear_blur: the arithmetic of apps/linear_blur restated in plain C, one
 * rounding per operator (no contraction by the compiler), the one fused operation written out.  tests/checker_lib.py holds the
 * build line: it links this file, with the other *_check.c files, into one shared object and drives it through ctypes.  Written
 * from the generators' text:
 *
 *   simple_blur_generator.cpp:5-22       in = repeat_edge(input, {{0, width}, {0, height}}); blur_x = (in(x) + in(x + 1) + in(x + 2)) / 3;
 *                                        output = (blur_x(y) + blur_x(y + 1) + blur_x(y + 2)) / 3.  The channel is not clamped.
 *   srgb_to_linear_generator.cpp:14-16   select(s <= 0.04045f, s / 12.92f, pow((s + .055f) / (1.0f + .055f), 2.4f))
 *   linear_to_srgb_generator.cpp:14-16   select(l <= .0031308f, l * 12.92f, (1 + .055f) * pow(l, 1.0f / 2.4f) - .055f)
 *   linear_blur_generator.cpp:8-27       to_srgb(simple_blur(to_linear(input), input.width(), input.height()))
 *
 * x / c is x * fold(1 / c) (src/Simplify_Div.cpp:204); 1 + .055f, 1 / 2.4f and the reciprocals are folded in f32.  Two canonical
 * float forms, those of oracle/oracle_common.h (ck_set_canon in check_canon.c selects one), whose o_halide_pow and o_mulsub are
 * used as they are: the only multiply that feeds an add or a subtract is the last step of to_srgb, one fma in form 1 and two
 * roundings in form 0.  blur_x is a Func of its own (a stored value), so its multiply by a third does not contract into the sum
 * that reads it. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "oracle_common.h"

static const float lc_third = 1.0f / 3.0f;

float lc_to_linear(float s) {
    return s <= 0.04045f ? s * (1.0f / 12.92f) : o_halide_pow((s + 0.055f) * (1.0f / (1.0f + 0.055f)), 2.4f);
}

float lc_to_srgb(float l) {
    return l <= 0.0031308f ? l * 12.92f : o_mulsub(1.0f + 0.055f, o_halide_pow(l, 1.0f / 2.4f), 0.055f);
}

static long lc_clamp(long v, long n) {   /* max(min(v, n - 1), 0) */
    const long m = v < n - 1 ? v : n - 1;
    return m > 0 ? m : 0;
}

/* The input is dense, in[c][y][x] over [ix0, ix0 + iw) x [iy0, iy0 + ih) x ic channels that are the output's; the output dense,
 * out[c][y][x] over [ox, ox + ow) x [oy, oy + oh).  linear != 0: width and height are iw and ih and both conversions apply.
 * Returns -4 where a tap leaves the input, as the entry points do, and writes nothing then. */
int lc_blur(int linear, const float *in, int ix0, int iy0, int iw, int ih, int nc, int width, int height, float *out, int ox, int oy, int ow, int oh) {
    if (linear) width = iw, height = ih;
    if (ow <= 0 || oh <= 0 || nc <= 0) return 0;
    const long x_lo = lc_clamp(ox, width), x_hi = lc_clamp((long)ox + ow + 1, width);
    const long y_lo = lc_clamp(oy, height), y_hi = lc_clamp((long)oy + oh + 1, height);
    if (x_lo < ix0 || x_hi > (long)ix0 + iw - 1 || y_lo < iy0 || y_hi > (long)iy0 + ih - 1) return -4;
    for (int c = 0; c < nc; c++)
        for (int y = 0; y < oh; y++)
            for (int x = 0; x < ow; x++) {
                float bx[3];
                for (int j = 0; j < 3; j++) {
                    float v[3];
                    for (int i = 0; i < 3; i++) {
                        const long sx = lc_clamp((long)ox + x + i, width), sy = lc_clamp((long)oy + y + j, height);
                        const float s = in[((size_t)c * ih + (size_t)(sy - iy0)) * iw + (size_t)(sx - ix0)];
                        v[i] = linear ? lc_to_linear(s) : s;
                    }
                    bx[j] = ((v[0] + v[1]) + v[2]) * lc_third;
                }
                const float o = ((bx[0] + bx[1]) + bx[2]) * lc_third;
                out[((size_t)c * oh + y) * ow + x] = linear ? lc_to_srgb(o) : o;
            }
    return 0;
}
