/* hannk_nn_check.c — plain-C checker of the pooling, mean, add, mul, softmax and l2_normalization ops of apps/hannk's op library and of
 * the approx_* helpers they use.  TEST INFRASTRUCTURE ONLY: written from the generators' algorithm sections one
 * expression at a time, every value an int64_t that is wrapped (wr) or saturated (st) to the width Halide's type has at that point.
 * Shares no code with the library.  Buffers: u8, the Halide dimensions first (dimension 0 innermost), `min`, `ext`, `str` per dimension,
 * the pointer at the element (min0, min1, ...). */
#include <stdint.h>

typedef int64_t i64;

static i64 wr(i64 v, int bits) { /* signed wrap */
    const i64 m = (i64)1 << bits;
    v = ((v % m) + m) % m;
    return v >= (m >> 1) ? v - m : v;
}
static i64 wru(i64 v, int bits) { /* unsigned wrap */
    const i64 m = (i64)1 << bits;
    return ((v % m) + m) % m;
}
static i64 st(i64 v, int bits) { /* signed saturate */
    const i64 hi = ((i64)1 << (bits - 1)) - 1, lo = -hi - 1;
    return v < lo ? lo : v > hi ? hi : v;
}
static i64 stu(i64 v, int bits) {
    const i64 hi = ((i64)1 << bits) - 1;
    return v < 0 ? 0 : v > hi ? hi : v;
}
static i64 fdiv(i64 a, i64 b) { /* Halide: floor, x / 0 == 0 */
    if (b == 0) return 0;
    i64 q = a / b;
    if (a % b != 0 && ((a < 0) != (b < 0))) q--;
    return q;
}
static i64 asr(i64 a, i64 n) { return n >= 63 ? (a < 0 ? -1 : 0) : a >> n; }
/* a << c in a signed type of `bits`, c signed: negative shifts right; everything is shifted out at |c| >= bits */
static i64 shl(i64 a, i64 c, int bits) {
    if (c >= 0) return c >= bits ? 0 : wr(a * ((i64)1 << c), bits);
    return -c >= bits ? (a < 0 ? -1 : 0) : asr(a, -c);
}
/* rounding_shift_right(a, s) in a signed type of `bits`: s > 0 floor((a + 2^(s-1)) / 2^s), s <= 0 a << -s */
static i64 rsr(i64 a, i64 s, int bits) {
    if (s <= 0) return shl(a, -s, bits);
    if (s > bits) return 0; /* (a + 2^(s-1)) >> s of a `bits`-bit a */
    return asr(a, s) + (asr(a, s - 1) & 1);
}
/* multiply_2x_high = rounding_mul_shift_right(a, b, bits - 1), saturating */
static i64 m2h(i64 a, i64 b, int bits) {
    if (bits == 32) { /* the product needs 63 bits: fits */
        return st((a * b + ((i64)1 << 30)) >> 31, 32);
    }
    return st((a * b + ((i64)1 << (bits - 2))) >> (bits - 1), bits);
}
static int clz32(i64 x) {
    uint32_t u = (uint32_t)wru(x, 32);
    int n = 0;
    if (u == 0) return 32;
    while (!(u & 0x80000000u)) u <<= 1, n++;
    return n;
}

static i64 approx_log2(int q, i64 x, int q_x, int tb) {
    const i64 floor_log2 = 31 - clz32(x);
    const i64 frac1 = wr(shl(x, 15 - floor_log2, 32), 16) & 0x7fff;
    const i64 frac2 = m2h(frac1, frac1, 16), frac3 = m2h(frac2, frac1, 16);
    const i64 poly = wr(m2h(2555, frac3, 16) + m2h(-9421, frac2, 16) + m2h(23249, frac1, 16) + 5, 16);
    i64 frac_result, floor_result;
    if (q < 14) frac_result = wr(rsr(poly, 14 - q, 16), tb);
    else frac_result = shl(wr(poly, tb), q - 14, tb);
    floor_result = shl(wr(wr(floor_log2 - q_x, 16), tb), q, tb);
    return st(floor_result + frac_result, tb);
}
static i64 approx_exp2(int q, i64 x, int xb, i64 q_x, int tb) {
    const i64 floor_x = wr(asr(x, q_x >= xb ? 63 : q_x), tb);
    const i64 exp2_floor_x = st(shl(1, wr(floor_x + q, tb), 32), tb);
    const i64 d = wr(x - (q_x >= 32 ? 0 : floor_x * ((i64)1 << q_x)), 16);
    const i64 frac1 = shl(d, wr(15 - wr(q_x, 16), 16), 16);
    const i64 frac2 = m2h(frac1, frac1, 16), frac3 = m2h(frac2, frac1, 16);
    i64 poly = wr(m2h(2592, frac3, 16) + m2h(7363, frac2, 16) + m2h(22812, frac1, 16), 16);
    poly = shl(poly, tb - 16, tb);
    return st(exp2_floor_x + m2h(exp2_floor_x, poly, tb), tb);
}
static i64 approx_reciprocal(int q, i64 x, int tb) { return approx_exp2(q, wr(-approx_log2(15, x, 0, 32), 32), 32, 15, tb); }
static i64 approx_reciprocal_sqrt(int q, i64 x, int tb) { return approx_exp2(q, wr(-approx_log2(14, x, 0, 32), 32), 32, 15, tb); }

void hkn_approx(int fn, int q, const int32_t *x, long n, int q_x, int bits, int32_t *out) {
    for (long i = 0; i < n; i++) {
        i64 r;
        if (fn == 0) r = approx_log2(q, x[i], q_x, bits);
        else if (fn == 1) r = approx_exp2(q, x[i], 32, q_x, bits);
        else if (fn == 2) r = approx_reciprocal(q, x[i], bits);
        else r = approx_reciprocal_sqrt(q, x[i], bits);
        out[i] = (int32_t)r;
    }
}

static i64 clampu8(i64 v, int lo, int hi) { /* Halide's clamp: max(min(v, hi), lo) */
    v = v < hi ? v : hi;
    return v > lo ? v : lo;
}
static long off(const long *str, const int *min, int nd, const int *at) {
    long o = 0;
    for (int d = 0; d < nd; d++) o += (long)(at[d] - min[d]) * str[d];
    return o;
}

void hkn_pool(int avg, const uint8_t *in, const int *imin, const int *iext, const long *istr, uint8_t *out, const int *omin, const int *oext,
              const long *ostr, int sx, int sy, int fw, int fh, int lo, int hi) {
    const i64 min_x = imin[1], max_x = (i64)imin[1] + iext[1] - 1, min_y = imin[2], max_y = (i64)imin[2] + iext[2] - 1;
    for (int b = omin[3]; b < omin[3] + oext[3]; b++)
        for (int y = omin[2]; y < omin[2] + oext[2]; y++)
            for (int x = omin[1]; x < omin[1] + oext[1]; x++)
                for (int c = omin[0]; c < omin[0] + oext[0]; c++) {
                    i64 sum = 0, mx = lo;
                    for (int ry = 0; ry < fh; ry++)
                        for (int rx = 0; rx < fw; rx++) {
                            const i64 xx = (i64)x * sx + rx, yy = (i64)y * sy + ry;
                            if (!(min_x <= xx && xx <= max_x && min_y <= yy && yy <= max_y)) continue;
                            const int at[4] = {c, (int)xx, (int)yy, b};
                            const i64 v = in[off(istr, imin, 4, at)];
                            sum = wru(sum + v, 16);
                            mx = mx > v ? mx : v;
                        }
                    const int at[4] = {c, x, y, b};
                    i64 r;
                    if (avg) {
                        const i64 x_start = (i64)x * sx > min_x ? (i64)x * sx : min_x, x_end = (i64)x * sx + fw < max_x + 1 ? (i64)x * sx + fw : max_x + 1;
                        const i64 y_start = (i64)y * sy > min_y ? (i64)y * sy : min_y, y_end = (i64)y * sy + fh < max_y + 1 ? (i64)y * sy + fh : max_y + 1;
                        const i64 filter_count = wr((x_end - x_start) * (y_end - y_start), 32);
                        const i64 inv = stu(fdiv(wr(((i64)2 << 16) + filter_count, 32), wr(2 * filter_count, 32)), 16);
                        const i64 average = stu((sum * inv + ((i64)1 << 15)) >> 16, 16);
                        r = clampu8(stu(average, 8), lo, hi);
                    } else {
                        r = mx < hi ? mx : hi;
                    }
                    out[off(ostr, omin, 4, at)] = (uint8_t)r;
                }
}

void hkn_mean(const uint8_t *in, const int *imin, const long *istr, const int *rmin, const int *rext, uint8_t *out, const int *omin, const int *oext,
              const long *ostr) {
    const i64 extent = wr(wr(wr((i64)rext[0] * rext[1], 32) * rext[2], 32) * rext[3], 32);
    int o[4], r[4];
    for (o[3] = omin[3]; o[3] < omin[3] + oext[3]; o[3]++)
        for (o[2] = omin[2]; o[2] < omin[2] + oext[2]; o[2]++)
            for (o[1] = omin[1]; o[1] < omin[1] + oext[1]; o[1]++)
                for (o[0] = omin[0]; o[0] < omin[0] + oext[0]; o[0]++) {
                    i64 sum = 0;
                    for (r[3] = 0; r[3] < rext[3]; r[3]++)
                        for (r[2] = 0; r[2] < rext[2]; r[2]++)
                            for (r[1] = 0; r[1] < rext[1]; r[1]++)
                                for (r[0] = 0; r[0] < rext[0]; r[0]++) {
                                    if (rext[0] <= 0 || rext[1] <= 0 || rext[2] <= 0 || rext[3] <= 0) continue;
                                    const int at[4] = {o[0] + rmin[0] + r[0], o[1] + rmin[1] + r[1], o[2] + rmin[2] + r[2], o[3] + rmin[3] + r[3]};
                                    sum = wru(sum + in[off(istr, imin, 4, at)], 32);
                                }
                    /* u32 + i32 -> i32 (match_types), floor division, the u8 cast wraps */
                    out[off(ostr, omin, 4, o)] = (uint8_t)wru(fdiv(wr(wr(sum, 32) + fdiv(extent, 2), 32), extent), 8);
                }
}

void hkn_add(const uint8_t *a, const int *amin, const long *astr, int zero1, int mul1, const uint8_t *b, const int *bmin, const long *bstr, int zero2,
             int mul2, int out_zero, int lo, int hi, uint8_t *out, const int *omin, const int *oext, const long *ostr) {
    int at[2];
    for (at[1] = omin[1]; at[1] < omin[1] + oext[1]; at[1]++)
        for (at[0] = omin[0]; at[0] < omin[0] + oext[0]; at[0]++) {
            const i64 in1 = shl(wr((i64)a[off(astr, amin, 2, at)] - zero1, 16), 6, 16), in2 = shl(wr((i64)b[off(bstr, bmin, 2, at)] - zero2, 16), 6, 16);
            const i64 sum = wr(wr(in1 * mul1, 32) + wr(in2 * mul2, 32), 32);
            i64 v = st(rsr(sum, 16, 32), 16);
            v = stu(st(v + out_zero, 16), 8);
            out[off(ostr, omin, 2, at)] = (uint8_t)clampu8(v, lo, hi);
        }
}

void hkn_mul(const uint8_t *a, const int *amin, const long *astr, int zero1, const uint8_t *b, const int *bmin, const long *bstr, int zero2, int out_zero,
             int32_t multiplier, uint32_t shift, int lo, int hi, uint8_t *out, const int *omin, const int *oext, const long *ostr) {
    int at[2];
    for (at[1] = omin[1]; at[1] < omin[1] + oext[1]; at[1]++)
        for (at[0] = omin[0]; at[0] < omin[0] + oext[0]; at[0]++) {
            const i64 in1 = shl(wr((i64)a[off(astr, amin, 2, at)] - zero1, 16), 6, 16), in2 = shl(wr((i64)b[off(bstr, bmin, 2, at)] - zero2, 16), 6, 16);
            i64 v = m2h(wr(in1 * in2, 32), multiplier, 32);
            v = st(rsr(v, (i64)shift, 32), 16); /* an unsigned count: only to the right */
            v = stu(st(v + out_zero, 16), 8);
            out[off(ostr, omin, 2, at)] = (uint8_t)clampu8(v, lo, hi);
        }
}

void hkn_softmax(const uint8_t *in, const int *imin, const int *iext, const long *istr, int beta_multiplier, unsigned beta_shift, int out_zero,
                 int out_multiplier, unsigned out_shift, uint8_t *out, const int *omin, const int *oext, const long *ostr) {
    int at[2];
    for (at[1] = omin[1]; at[1] < omin[1] + oext[1]; at[1]++) {
        i64 max_x = 0, sum = 0;
        int r[2] = {0, at[1]};
        for (r[0] = imin[0]; r[0] < imin[0] + iext[0]; r[0]++) {
            const i64 v = in[off(istr, imin, 2, r)];
            max_x = max_x > v ? max_x : v;
        }
        for (r[0] = imin[0]; r[0] < imin[0] + iext[0]; r[0]++) {
            const i64 diff = shl(wr((i64)in[off(istr, imin, 2, r)] - max_x, 16), 6, 16);
            sum = wr(sum + approx_exp2(15, m2h(diff, beta_multiplier, 16), 16, beta_shift, 16), 32);
        }
        const i64 inv = approx_reciprocal(30, sum, 16);
        for (at[0] = omin[0]; at[0] < omin[0] + oext[0]; at[0]++) {
            const i64 diff = shl(wr((i64)in[off(istr, imin, 2, at)] - max_x, 16), 6, 16);
            const i64 e = approx_exp2(15, m2h(diff, beta_multiplier, 16), 16, beta_shift, 16);
            i64 o = m2h(m2h(e, inv, 16), out_multiplier, 16);
            o = rsr(o, (i64)out_shift, 16);
            out[off(ostr, omin, 2, at)] = (uint8_t)stu(st(o + out_zero, 16), 8);
        }
    }
}

void hkn_l2_normalization(const uint8_t *in, const int *imin, const int *iext, const long *istr, int zero, uint8_t *out, const int *omin, const int *oext,
                          const long *ostr) {
    int at[2];
    for (at[1] = omin[1]; at[1] < omin[1] + oext[1]; at[1]++) {
        i64 sum = 0;
        int r[2] = {0, at[1]};
        for (r[0] = imin[0]; r[0] < imin[0] + iext[0]; r[0]++) {
            const i64 z = wr((i64)in[off(istr, imin, 2, r)] - zero, 16);
            sum = wr(sum + wr(z * z, 32), 32);
        }
        const i64 inv = approx_reciprocal_sqrt(15, sum, 32);
        for (at[0] = omin[0]; at[0] < omin[0] + oext[0]; at[0]++) {
            const i64 z = wr((i64)in[off(istr, imin, 2, at)] - zero, 16);
            i64 o = st(rsr(wr(z * inv, 32), 8, 32), 16);
            out[off(ostr, omin, 2, at)] = (uint8_t)stu(st(o + 128, 16), 8);
        }
    }
}
