/* hannk_program_check.c — plain-C checker of the Elementwise interpreter, its approx_logistic / approx_tanh helpers, copy,
 * upsample_channels and the shallow depthwise variant of apps/hannk's op library.  TEST INFRASTRUCTURE ONLY: written from elementwise_generator.cpp:133-200
 * and common_halide.cpp:177-226 one expression at a time, every value an int64_t that is wrapped (wr) or saturated (st) to the width
 * Halide's type has at that point, on the helpers of hannk_nn_check.c (which this file includes and does not change).  Shares no code
 * with the library.
 *
 * cw is the width of the run-time count q_x: a shift by it runs at the wider of its operand's and the count's width (match_bits). */
#include "hannk_nn_check.c"

static i64 shr(i64 a, i64 c, int bits) { return shl(a, -c, bits); }
static int wider(int a, int b) { return a > b ? a : b; }

/* approx_exp2(16, x, q_x, Int(32)) of an i16 x */
static i64 exp2_q16(i64 x, i64 q_x, int cw) {
    const i64 floor_x = shr(x, q_x, wider(16, cw));                 /* cast(Int(32), x >> q_x) */
    const i64 exp2_floor_x = st(shl(1, wr(floor_x + 16, 32), 32), 32);
    const i64 d = wr(x - shl(floor_x, q_x, 32), 16);                /* i16(x - (floor_x << q_x)): floor_x is an i32 */
    const i64 frac1 = shl(d, wr(15 - wr(q_x, 16), 16), 16);
    const i64 frac2 = m2h(frac1, frac1, 16), frac3 = m2h(frac2, frac1, 16);
    i64 poly = wr(m2h(2592, frac3, 16) + m2h(7363, frac2, 16) + m2h(22812, frac1, 16), 16);
    poly = shl(poly, 16, 32);
    return st(exp2_floor_x + m2h(exp2_floor_x, poly, 32), 32);
}
/* approx_log2_exp2_plus_or_minus_one(q, x, sign, q_x, Int(16)) */
static i64 log2pm1_exp2(int q, i64 x, int sign, i64 q_x, int cw) {
    const i64 one_plus_exp2_x = wr((i64)sign * 65536 + exp2_q16(x, q_x, cw), 32);
    const i64 raw = approx_log2(q, one_plus_exp2_x, 16, 16);
    const i64 line = st(rsr(x, wr(wr(q_x, 16) - q, 16), 32), 16);   /* cast(type.widen(), x): an i32 shift */
    return shr(x, q_x, wider(16, cw)) < 14 ? raw : line;
}
static i64 logistic(int q, i64 x, i64 q_x, int cw) {
    const i64 x2 = m2h(x, -23637, 16);
    const i64 log2_d = log2pm1_exp2(11, x2, 1, wr(q_x - 1, cw), cw);
    return approx_exp2(q, wr(-log2_d, 16), 16, 11, 16);
}
static i64 tanh_(int q, i64 x, i64 q_x, int cw) {
    const i64 x2 = m2h(x, 23637, 16);
    const i64 ax = wr(x2 < 0 ? -x2 : x2, 16);
    const i64 log2_n = log2pm1_exp2(11, ax, -1, wr(q_x - 2, cw), cw), log2_d = log2pm1_exp2(11, ax, 1, wr(q_x - 2, cw), cw);
    const i64 abs_output = approx_exp2(q, wr(log2_n - log2_d, 16), 16, 11, 16);
    return x2 < 0 ? wr(-abs_output, 16) : x2 == 0 ? 0 : abs_output;
}
/* fn 0 approx_log2p1_exp2, 1 approx_log2m1_exp2, 2 approx_logistic, 3 approx_tanh, each in Int(16) */
void hkp_approx(int fn, const int32_t *x, const int32_t *q, const int32_t *q_x, long n, int cw, int32_t *out) {
    for (long i = 0; i < n; i++) {
        i64 r;
        if (fn == 0) r = log2pm1_exp2(q[i], x[i], 1, q_x[i], cw);
        else if (fn == 1) r = log2pm1_exp2(q[i], x[i], -1, q_x[i], cw);
        else if (fn == 2) r = logistic(q[i], x[i], q_x[i], cw);
        else r = tanh_(q[i], x[i], q_x[i], cw);
        out[i] = (int32_t)r;
    }
}

/* one instruction: a = slot[arg1], s2 = slot[arg2]; Noop and unknown codes leave 0 (the reference: undef) */
static i64 instruction(int op, i64 a, i64 s2, i64 arg3, i64 arg4) {
    const i64 b = wr(s2 + arg3, 16);
    i64 v;
    switch (op) {
    case 1: return st(a + b, 16);
    case 2: return st(a - b, 16);
    case 3: return st(m2h(a, b, 16) + arg4, 16);
    case 4: return st(rsr(a * b, wru(arg4, 16), 32), 16);           /* widening_mul -> i32, a u16 count widened to u32 */
    case 5: return wr(rsr(a, b, 16), 16);
    case 6: return a < b ? a : b;
    case 7: return a > b ? a : b;
    case 8: v = a < arg4 ? a : arg4; return v > arg3 ? v : arg3;
    case 9: return wr(rsr(logistic(15, a, b, 16), wr(15 - arg4, 16), 16), 16);
    case 10: return wr(rsr(tanh_(15, a, b, 16), wr(15 - arg4, 16), 16), 16);
    default: return 0;
    }
}
void hkp_op(int op, const int32_t *a, const int32_t *s2, const int32_t *arg3, const int32_t *arg4, long n, int32_t *out) {
    for (long i = 0; i < n; i++) out[i] = (int32_t)instruction(op, a[i], s2[i], arg3[i], arg4[i]);
}
/* the interpreter over rank-2 buffers: in[k] points at input k's element of the output's first, strides in elements; program: n rows of
 * (op, arg1, arg2, arg3, arg4), every operand of a live instruction inside [-5, row]; out1 is null for the u8 variant.  Returns -1 where
 * an operand is out of range (nothing is written then) */
int hkp_elementwise(int in_i16, const void *const *in, const long *in_s0, const long *in_s1, const int16_t *program, int n, uint8_t *out0, long o0_s1,
                    int16_t *out1, long o1_s1, int W, int H) {
    if (n > 20) return -2;
    for (int k = 0; k < n; k++)
        if (program[5 * k] >= 1 && program[5 * k] <= 10)
            for (int j = 1; j <= 2; j++)
                if (program[5 * k + j] < -5 || program[5 * k + j] > k) return -1;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            i64 slot[26]; /* slot s at slot[s + 5] */
            for (int k = 0; k < 5; k++) {
                const long at = y * in_s1[k] + x * in_s0[k];
                slot[4 - k] = in_i16 ? (i64)((const int16_t *)in[k])[at] : (i64)((const uint8_t *)in[k])[at];
            }
            slot[5] = 0;
            for (int k = 0; k < n; k++) {
                const int16_t *w = program + 5 * k;
                const int live = w[0] >= 1 && w[0] <= 10;
                slot[5 + k + 1] = live ? instruction(w[0], slot[5 + w[1]], slot[5 + w[2]], w[3], w[4]) : 0;
            }
            if (out1) {
                out0[y * o0_s1 + x] = (uint8_t)stu(slot[5 + n - 1], 8);
                out1[y * o1_s1 + x] = (int16_t)slot[5 + n];
            } else {
                out0[y * o0_s1 + x] = (uint8_t)stu(slot[5 + n], 8);
            }
        }
    return 0;
}

/* copy_uint8_uint8: out(c, x, y, b) = c inside the input's dimension 0 ? in(c, x, y, b) : u8(pad_value) */
void hkp_copy(const uint8_t *in, const int *imin, const int *iext, const long *istr, int pad_value, uint8_t *out, const int *omin, const int *oext,
              const long *ostr) {
    int at[4];
    for (at[3] = omin[3]; at[3] < omin[3] + oext[3]; at[3]++)
        for (at[2] = omin[2]; at[2] < omin[2] + oext[2]; at[2]++)
            for (at[1] = omin[1]; at[1] < omin[1] + oext[1]; at[1]++)
                for (at[0] = omin[0]; at[0] < omin[0] + oext[0]; at[0]++) {
                    const int inside = at[0] >= imin[0] && at[0] < imin[0] + iext[0];
                    out[off(ostr, omin, 4, at)] = inside ? in[off(istr, imin, 4, at)] : (uint8_t)wru(pad_value, 8);
                }
}
/* Halide's division: the remainder is never negative (floor for a positive divisor), x / 0 == 0 */
static i64 hdiv(i64 a, i64 b) {
    i64 q, r;
    if (b == 0) return 0;
    q = a / b, r = a - q * b;
    if (r < 0) q += b < 0 ? 1 : -1;
    return q;
}
/* upsample_channels_uint8: out(c, x, y, b) = in(c / factor, x, y, b) */
void hkp_upsample_channels(const uint8_t *in, const int *imin, const long *istr, int factor, uint8_t *out, const int *omin, const int *oext,
                           const long *ostr) {
    int at[4], src[4];
    for (at[3] = omin[3]; at[3] < omin[3] + oext[3]; at[3]++)
        for (at[2] = omin[2]; at[2] < omin[2] + oext[2]; at[2]++)
            for (at[1] = omin[1]; at[1] < omin[1] + oext[1]; at[1]++)
                for (at[0] = omin[0]; at[0] < omin[0] + oext[0]; at[0]++) {
                    src[0] = (int)hdiv(at[0], factor), src[1] = at[1], src[2] = at[2], src[3] = at[3];
                    out[off(ostr, omin, 4, at)] = in[off(istr, imin, 4, src)];
                }
}

/* depthwise_conv_shallow_uint8 (depthwise_conv_generator.cpp with shallow = true): c is the fused c-x index, the output's x is 0;
 *   acc(c, y, b) = bias((c % 16) % D) + sum over ry, rx of (i16(filter((c % 16) % D, rx, ry)) - filter_zero) *
 *                  (in(c + rx * dilation_x * input_stride_x, y * stride_y + ry * dilation_y, b) - input_zero)      modulo 2^32
 * then quantize_and_relu_u8: i16_sat(rounding_shift_right(multiply_2x_high(acc, multiplier), shift)), u8_sat of the
 * saturating i16 add of output_zero, max(min(., output_max), output_min).
 * in: dense [L, H, B] (the fused row first), filt dense [D, fw, fh], out dense [C, OH, OB]; every min 0 */
void hkp_depthwise_shallow(const uint8_t *in, int L, int H, const uint8_t *filt, int D, int fw, int fh, const int32_t *bias, uint8_t *out, int C, int OH,
                           int OB, int sy, int dx, int dy, int isx, int input_zero, int filter_zero, int32_t multiplier, int32_t shift, int zero, int lo,
                           int hi) {
    for (int b = 0; b < OB; b++)
        for (int y = 0; y < OH; y++)
            for (int c = 0; c < C; c++) {
                const int fc = (c % 16) % D;
                i64 acc = bias[fc], v;
                for (int ry = 0; ry < fh; ry++)
                    for (int rx = 0; rx < fw; rx++) {
                        const i64 a = in[((long)b * H + (long)y * sy + (long)ry * dy) * L + c + (long)rx * dx * isx];
                        const i64 w = filt[((long)ry * fw + rx) * D + fc];
                        acc = wr(acc + (w - filter_zero) * (a - input_zero), 32);
                    }
                v = st(rsr(m2h(acc, multiplier, 32), shift, 32), 16);
                v = stu(st(v + zero, 16), 8);
                out[((long)b * OH + y) * C + c] = (uint8_t)clampu8(v, lo, hi);
            }
}
