/* wavelet_check.c — the checker of haar_x, inverse_haar_x, daubechies_x and inverse_daubechies_x: the arithmetic of apps/wavelet
 * restated in plain C, one rounding per operator (no contraction by the compiler), the fused operations written out.
 * tests/wavelet_checker.py declares the object (tests/checker_lib.py links this file with check_canon.c into a shared object of its own) and drives
 * it through ctypes.  Written from the generators' text, `in` being repeat_edge of the input over the buffer's own min and extent
 * in every dimension:
 *
 *   haar_x_generator.cpp:15-21                out(x, y, c) = mux(c, {in(2x, y) + in(2x + 1, y), in(2x, y) - in(2x + 1, y)}) / 2
 *   inverse_haar_x_generator.cpp:15-20        out(x, y) = select(x % 2 == 0, in(x/2, y, 0) + in(x/2, y, 1), in(x/2, y, 0) - in(x/2, y, 1))
 *   daubechies_x_generator.cpp:15-20          out(x, y, c) = mux(c, {D0 in(2x - 1) + D1 in(2x) + D2 in(2x + 1) + D3 in(2x + 2),
 *                                                                     D3 in(2x - 1) - D2 in(2x) + D1 in(2x + 1) - D0 in(2x + 2)})
 *   inverse_daubechies_x_generator.cpp:15-20  out(x, y) = select(x % 2 == 0, D2 p + D1 q + D0 r + D3 s, D3 p - D0 q + D1 r - D2 s),
 *                                             p, q, r, s = in(x/2, y, 0), in(x/2, y, 1), in(x/2 + 1, y, 0), in(x/2 + 1, y, 1)
 *   daubechies_constants.h:4-7                D0 .. D3, D3 < 0
 *
 * mux selects the LAST value for every index other than 0.  x / 2 on floats is x * 0.5f (src/Simplify_Div.cpp:204); x / 2 and x % 2
 * on ints are floor and Euclidean (o_fdiv, o_fmod).  2x +- k and x/2 + 1 are formed in 64 bits before the clamp.  Two canonical
 * float forms, those of oracle/oracle_common.h (ck_set_canon in check_canon.c selects one): the sum of four products, written
 * ((A + B) + C) + D, is mad(D, mad(C, mad2(A, B))): the first add has two products and fuses the first, each later add fuses its
 * own; the alternating one, ((A - B) + C) - D, is msub(mad(C, mulsub(A, B)), D).  Haar has no multiply that feeds an add: its two
 * forms agree.  src/Simplify_Sub.cpp:94 rewrites x - y * c0 into x + y * (-c0) only for c0 < 0, and every constant that is
 * subtracted here (D2, D0) is positive.  src/Simplify_Add.cpp has no rule that turns x + y * c0 with c0 < 0 into a subtraction;
 * had it one, `+ D3 * d` read as `- (-D3) * d` would give the same bits in both forms, negation being exact. */
#include <stddef.h>
#include <stdint.h>

#include "oracle_common.h"

static const float wc_d[4] = {0.4829629131445341f, 0.83651630373780772f, 0.22414386804201339f, -0.12940952255126034f};
#define D0 wc_d[0]
#define D1 wc_d[1]
#define D2 wc_d[2]
#define D3 wc_d[3]

float wc_constant(int i) { return wc_d[i & 3]; }

static int64_t wc_clamp(int64_t v, int64_t lo, int64_t n) {   /* max(min(v, lo + n - 1), lo) */
    const int64_t m = v < lo + n - 1 ? v : lo + n - 1;
    return m > lo ? m : lo;
}

/* The forwards.  in[y][x] dense over [ix0, ix0 + iw) x [iy0, iy0 + ih); out[c][y][x] dense over [ox, ox + ow) x [oy, oy + oh) x
 * [oc, oc + on).  Returns -4 for an input with an empty dimension under an output that is not empty, and writes nothing then. */
int wc_forward(int daub, const float *in, int ix0, int iy0, int iw, int ih, float *out, int ox, int oy, int oc, int ow, int oh, int on) {
    if (ow <= 0 || oh <= 0 || on <= 0) return 0;
    if (iw <= 0 || ih <= 0) return -4;
    for (int c = 0; c < on; c++)
        for (int y = 0; y < oh; y++) {
            const float *row = in + (size_t)(wc_clamp((int64_t)oy + y, iy0, ih) - iy0) * iw;
            for (int x = 0; x < ow; x++) {
                const int64_t X = 2 * ((int64_t)ox + x);
                const float a = row[wc_clamp(X - 1, ix0, iw) - ix0], b = row[wc_clamp(X, ix0, iw) - ix0];
                const float c2 = row[wc_clamp(X + 1, ix0, iw) - ix0], d = row[wc_clamp(X + 2, ix0, iw) - ix0];
                const int low = (int64_t)oc + c == 0;
                float v;
                if (!daub) v = low ? (b + c2) * 0.5f : (b - c2) * 0.5f;
                else if (low) v = o_mad(D3, d, o_mad(D2, c2, o_mad2(D0, a, D1, b)));
                else v = o_msub(o_mad(D1, c2, o_mulsub(D3, a, D2 * b)), D0, d);
                out[((size_t)c * oh + y) * ow + x] = v;
            }
        }
    return 0;
}

/* The inverses.  in[c][y][x] dense over [ix0, ix0 + iw) x [iy0, iy0 + ih) x [ic0, ic0 + ic); out[y][x] dense over
 * [ox, ox + ow) x [oy, oy + oh). */
int wc_inverse(int daub, const float *in, int ix0, int iy0, int ic0, int iw, int ih, int ic, float *out, int ox, int oy, int ow, int oh) {
    if (ow <= 0 || oh <= 0) return 0;
    if (iw <= 0 || ih <= 0 || ic <= 0) return -4;
    const float *pl0 = in + (size_t)(wc_clamp(0, ic0, ic) - ic0) * ih * iw, *pl1 = in + (size_t)(wc_clamp(1, ic0, ic) - ic0) * ih * iw;
    for (int y = 0; y < oh; y++) {
        const size_t ro = (size_t)(wc_clamp((int64_t)oy + y, iy0, ih) - iy0) * iw;
        for (int x = 0; x < ow; x++) {
            const int X = (int)((int64_t)ox + x);   /* an output coordinate: it fits */
            const int64_t k = o_fdiv(X, 2);
            const int even = o_fmod(X, 2) == 0;
            const size_t k0 = ro + (size_t)(wc_clamp(k, ix0, iw) - ix0), k1 = ro + (size_t)(wc_clamp(k + 1, ix0, iw) - ix0);
            const float p = pl0[k0], q = pl1[k0], r = pl0[k1], s = pl1[k1];
            float v;
            if (!daub) v = even ? p + q : p - q;
            else if (even) v = o_mad(D3, s, o_mad(D0, r, o_mad2(D2, p, D1, q)));
            else v = o_msub(o_mad(D1, r, o_mulsub(D3, p, D0 * q)), D2, s);
            out[(size_t)y * ow + x] = v;
        }
    }
    return 0;
}
