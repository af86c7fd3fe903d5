/* compositing_check.c — the checker of compositing: apps/compositing/compositing_generator.cpp:25-154 restated in plain C in its
 * INTEGER form (the branch of a target without a GPU feature: uint16 colour, uint8 alpha), every value held in the type the
 * generator gives it so that additions wrap where the generator's do.  tests/compositing_checker.py declares the object (tests/checker_lib.py builds it) and drives
 * this file through ctypes.  No float operation anywhere: there is no canonical form to choose.
 *
 *   premultiply_alpha :34-37     C[i] = widening_mul(v_i, a): u16(v_i) * u16(a); A = a
 *   scale :58-69                 c = widening_mul(a, cast(a.type(), s)); c += rounding_shift_right(c, 8); c = rounding_shift_right(c, 8);
 *                                cast(a.type(), c).  rounding_shift_right(c, 8) is (c + 128) >> 8 without internal overflow.  The
 *                                comment "equivalent to c = (c + 127) / 255" holds for a uint8 a only; cc_scale16_div255 is that
 *                                formula, kept so that a test can count where the two part.
 *   invert :71-77                ~e on uint8: 255 - e
 *   over, atop, xor_, in, out :80-123   written out below, every result from the old state (a Tuple)
 *   :146-151                     r.where(r[0] == ops(r[1])): an op code outside 0 .. 4 selects no operator, the layer is skipped
 *   normalize :50-53             fast_integer_divide(C[i] + A / 2, A) on uint16 / uint8, then saturating_cast to uint8:
 *                                the exact floor quotient, the numerator itself for a denominator of 1, 0 for a denominator of 0
 *                                (src/FastIntegerDivide.cpp:302-307); the sum wraps in uint16
 */
#include <stddef.h>
#include <stdint.h>

uint16_t cc_scale16(uint16_t a, uint8_t s) {
    uint32_t c = (uint32_t)a * (uint32_t)s;
    c += (c + 128u) >> 8;
    c = (c + 128u) >> 8;
    return (uint16_t)c;
}

uint8_t cc_scale8(uint8_t a, uint8_t s) {
    /* the intermediate is at most 65025 + 254 = 65279: uint16 arithmetic does not overflow */
    uint16_t c = (uint16_t)((uint16_t)a * (uint16_t)s);
    c = (uint16_t)(c + (uint16_t)((uint16_t)(c + 128u) >> 8));
    c = (uint16_t)((uint16_t)(c + 128u) >> 8);
    return (uint8_t)c;
}

/* what the generator's comment claims scale to be */
uint16_t cc_scale16_div255(uint16_t a, uint8_t s) { return (uint16_t)(((uint32_t)a * (uint32_t)s + 127u) / 255u); }

/* fast_integer_divide(n, d) for a uint16 numerator and a uint8 denominator */
uint16_t cc_divide(uint16_t n, uint8_t d) {
    if (d == 0) return 0;
    if (d == 1) return n;
    return (uint16_t)(n / d);
}

void cc_scale16_sweep(const uint16_t *a, const uint8_t *s, uint16_t *two_shift, uint16_t *div255, size_t n) {
    for (size_t i = 0; i < n; i++) two_shift[i] = cc_scale16(a[i], s[i]), div255[i] = cc_scale16_div255(a[i], s[i]);
}

typedef struct {
    uint16_t c[3];
    uint8_t a;
} cc_px;

static cc_px cc_premultiply(const uint8_t v[4]) {
    cc_px p;
    for (int i = 0; i < 3; i++) p.c[i] = (uint16_t)((uint16_t)v[i] * (uint16_t)v[3]);
    p.a = v[3];
    return p;
}

static cc_px cc_apply(int32_t op, cc_px a, cc_px b) {
    cc_px r = a;
    const uint8_t nb = (uint8_t)~b.a, na = (uint8_t)~a.a;
    switch (op) {
        case 0: /* over */
            for (int i = 0; i < 3; i++) r.c[i] = (uint16_t)(b.c[i] + cc_scale16(a.c[i], nb));
            r.a = (uint8_t)(b.a + cc_scale8(a.a, nb));
            break;
        case 1: /* atop */
            for (int i = 0; i < 3; i++) r.c[i] = (uint16_t)(cc_scale16(b.c[i], a.a) + cc_scale16(a.c[i], nb));
            r.a = a.a;
            break;
        case 2: /* xor */
            for (int i = 0; i < 3; i++) r.c[i] = (uint16_t)(cc_scale16(b.c[i], na) + cc_scale16(a.c[i], nb));
            r.a = (uint8_t)(cc_scale8(b.a, na) + cc_scale8(a.a, nb));
            break;
        case 3: /* in */
            for (int i = 0; i < 3; i++) r.c[i] = cc_scale16(a.c[i], b.a);
            r.a = cc_scale8(a.a, b.a);
            break;
        case 4: /* out */
            for (int i = 0; i < 3; i++) r.c[i] = cc_scale16(a.c[i], nb);
            r.a = cc_scale8(a.a, nb);
            break;
        default: /* no operator matches: the state stays */
            break;
    }
    return r;
}

/* Six layers, each dense [4][h][w] (planar, x innermost) over the output's own box; ops: five codes; out: dense [4][h][w]. */
void cc_compositing(const uint8_t *const layers[6], const int32_t ops[5], uint8_t *out, int w, int h) {
    const size_t plane = (size_t)w * (size_t)h;
    for (size_t p = 0; p < plane; p++) {
        uint8_t v[4];
        for (int c = 0; c < 4; c++) v[c] = layers[0][c * plane + p];
        cc_px s = cc_premultiply(v);
        for (int k = 1; k < 6; k++) {
            for (int c = 0; c < 4; c++) v[c] = layers[k][c * plane + p];
            s = cc_apply(ops[k - 1], s, cc_premultiply(v));
        }
        for (int i = 0; i < 3; i++) {
            const uint16_t q = cc_divide((uint16_t)(s.c[i] + (uint16_t)(s.a / 2)), s.a);
            out[i * plane + p] = q > 255 ? 255 : (uint8_t)q;
        }
        out[3 * plane + p] = s.a;
    }
}
