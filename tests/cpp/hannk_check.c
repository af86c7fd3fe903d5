/* hannk_check.c — plain-C restatement of the contract of the hannk convolution ops, written from the ALGORITHM sections
 * of the reference's generators (apps/hannk/halide/conv_generator.cpp:84-159 and :341-350, depthwise_conv_generator.cpp:66-135,
 * common_halide.cpp:228-248) and the lowering of the run-time rounding shift (src/FindIntrinsics.cpp:1331-1345); nothing of their
 * schedules.  TEST INFRASTRUCTURE ONLY: built with hannk_program_check.c into one shared object, declared by tests/hannk_checker.py; shares no code with the product.
 *
 * Every buffer comes as a pointer to its element at (min0, min1, ...), its mins, extents and element strides, dimension 0 first.
 * Sums are uint32_t: they wrap modulo 2^32 like the contract's int32. */
#include <stdint.h>

static int32_t sat32(int64_t v) { return v > INT32_MAX ? INT32_MAX : v < INT32_MIN ? INT32_MIN : (int32_t)v; }

/* sat_i32((i64(a) * b + 2^30) >> 31) */
int32_t hk_multiply_2x_high(int32_t a, int32_t b) {
    int64_t p = (int64_t)a * (int64_t)b + ((int64_t)1 << 30);
    /* >> of a negative int64 is an arithmetic shift with every compiler this is built with; spelled as a floor division */
    int64_t q = p >= 0 ? p / ((int64_t)1 << 31) : -((-p + ((int64_t)1 << 31) - 1) / ((int64_t)1 << 31));
    return sat32(q);
}

static int32_t asr(int32_t a, int s) { /* floor(a / 2^s), 0 <= s <= 31 */
    int64_t d = (int64_t)1 << s, v = a;
    return (int32_t)(v >= 0 ? v / d : -((-v + d - 1) / d));
}

/* (a >> s) + (s > 0 ? (a >> (s - 1)) & 1 : 0); a negative s is a wrapping left shift */
int32_t hk_rounding_shift_right(int32_t a, int32_t s) {
    if (s > 0) return asr(a, s) + (asr(a, s - 1) & 1);
    if (s == 0) return a;
    return (int32_t)((uint32_t)a << (-s));
}

int16_t hk_quantize_i16(int32_t acc, int32_t multiplier, int32_t shift) {
    int32_t v = hk_rounding_shift_right(hk_multiply_2x_high(acc, multiplier), shift);
    return (int16_t)(v > 32767 ? 32767 : v < -32768 ? -32768 : v);
}

/* clamp(u8_sat(saturating_add(q, i16(zero))), lo, hi) with Halide's clamp = max(min(v, hi), lo) */
uint8_t hk_quantize_and_relu_u8(int32_t acc, int32_t multiplier, int32_t shift, uint8_t zero, uint8_t lo, uint8_t hi) {
    int32_t s = (int32_t)hk_quantize_i16(acc, multiplier, shift) + (int32_t)zero;
    if (s > 32767) s = 32767;
    int32_t u = s < 0 ? 0 : s > 255 ? 255 : s;
    int32_t m = u < (int32_t)hi ? u : (int32_t)hi;
    return (uint8_t)(m > (int32_t)lo ? m : (int32_t)lo);
}

/* fn 0: int16_t out[n] = quantize_i16; fn 1: uint8_t out[n] = quantize_and_relu_u8 */
void hk_quantize(int fn, const int32_t *acc, long n, int32_t multiplier, int32_t shift, uint8_t zero, uint8_t lo, uint8_t hi, void *out) {
    for (long i = 0; i < n; i++) {
        if (fn == 0) ((int16_t *)out)[i] = hk_quantize_i16(acc[i], multiplier, shift);
        else ((uint8_t *)out)[i] = hk_quantize_and_relu_u8(acc[i], multiplier, shift, zero, lo, hi);
    }
}

/* output(ci, bi, co, bo, x, y) = u8(i16(in(co * 4 + ci, x, y, bo * 16 + bi)) - i16(input_zero) + output_zero), in = input_zero outside */
void hk_tile_filter(const uint8_t *in, const int *imin, const int *iext, const long *istr, uint8_t input_zero, uint8_t output_zero, uint8_t *out,
                    const int *omin, const int *oext, const long *ostr) {
    int p[6];
    for (p[5] = 0; p[5] < oext[5]; p[5]++)
    for (p[4] = 0; p[4] < oext[4]; p[4]++)
    for (p[3] = 0; p[3] < oext[3]; p[3]++)
    for (p[2] = 0; p[2] < oext[2]; p[2]++)
    for (p[1] = 0; p[1] < oext[1]; p[1]++)
    for (p[0] = 0; p[0] < oext[0]; p[0]++) {
        int ci = p[0] + omin[0], bi = p[1] + omin[1], co = p[2] + omin[2], bo = p[3] + omin[3], x = p[4] + omin[4], y = p[5] + omin[5];
        int at[4] = {co * 4 + ci, x, y, bo * 16 + bi};
        int inside = 1;
        long s = 0, o = 0;
        for (int d = 0; d < 4; d++) {
            int r = at[d] - imin[d];
            if (r < 0 || r >= iext[d]) inside = 0;
            s += r * istr[d];
        }
        for (int d = 0; d < 6; d++) o += p[d] * ostr[d];
        int16_t v = (int16_t)((int16_t)(inside ? in[s] : input_zero) - (int16_t)input_zero + (int16_t)output_zero);
        out[o] = (uint8_t)v;
    }
}

static void put(void *out, long o, int out_i16, uint32_t acc, int32_t multiplier, int32_t shift, uint8_t zero, uint8_t lo, uint8_t hi) {
    if (out_i16) ((int16_t *)out)[o] = hk_quantize_i16((int32_t)acc, multiplier, shift);
    else ((uint8_t *)out)[o] = hk_quantize_and_relu_u8((int32_t)acc, multiplier, shift, zero, lo, hi);
}

/* conv: filt is the tiled filter, every min 0, strides fstr[0..5]; bias at [0, C); the output's dimension 0 starts at 0 */
void hk_conv(const uint8_t *in, const int *imin, const long *istr, const uint8_t *filt, const long *fstr, int cq, int fw, int fh, const int32_t *bias,
             void *out, const int *omin, const int *oext, const long *ostr, int out_i16, int sx, int sy, int dx, int dy, uint8_t input_zero,
             uint8_t filter_zero, int32_t multiplier, int32_t shift, uint8_t zero, uint8_t lo, uint8_t hi) {
    for (int b = 0; b < oext[3]; b++)
    for (int y = 0; y < oext[2]; y++)
    for (int x = 0; x < oext[1]; x++)
    for (int c = 0; c < oext[0]; c++) {
        uint32_t acc = (uint32_t)bias[c];
        for (int ry = 0; ry < fh; ry++)
        for (int rx = 0; rx < fw; rx++)
        for (int rz = 0; rz < 4 * cq; rz++) {
            long ix = (long)(x + omin[1]) * sx + (long)rx * dx - imin[1], iy = (long)(y + omin[2]) * sy + (long)ry * dy - imin[2];
            int32_t a = in[(rz - imin[0]) * istr[0] + ix * istr[1] + iy * istr[2] + (long)(b + omin[3] - imin[3]) * istr[3]];
            int32_t w = filt[(rz % 4) * fstr[0] + (c % 16) * fstr[1] + (rz / 4) * fstr[2] + (c / 16) * fstr[3] + rx * fstr[4] + ry * fstr[5]];
            acc += (uint32_t)((a - (int32_t)input_zero) * (w - (int32_t)filter_zero));
        }
        put(out, c * ostr[0] + x * ostr[1] + y * ostr[2] + b * ostr[3], out_i16, acc, multiplier, shift, zero, lo, hi);
    }
}

/* depthwise: filt [c, fx, fy] and bias [c] at min 0; inv = 1 (input channel c) or 0 (input channel 0 feeds every output channel) */
void hk_depthwise(const uint8_t *in, const int *imin, const long *istr, const uint8_t *filt, const long *fstr, int fw, int fh, const int32_t *bias,
                  uint8_t *out, const int *omin, const int *oext, const long *ostr, int inv, int sx, int sy, int dx, int dy, uint8_t input_zero,
                  uint8_t filter_zero, int32_t multiplier, int32_t shift, uint8_t zero, uint8_t lo, uint8_t hi) {
    for (int b = 0; b < oext[3]; b++)
    for (int y = 0; y < oext[2]; y++)
    for (int x = 0; x < oext[1]; x++)
    for (int c = 0; c < oext[0]; c++) {
        uint32_t acc = (uint32_t)bias[c];
        for (int ry = 0; ry < fh; ry++)
        for (int rx = 0; rx < fw; rx++) {
            long ix = (long)(x + omin[1]) * sx + (long)rx * dx - imin[1], iy = (long)(y + omin[2]) * sy + (long)ry * dy - imin[2];
            int32_t a = in[(long)(c * inv - imin[0]) * istr[0] + ix * istr[1] + iy * istr[2] + (long)(b + omin[3] - imin[3]) * istr[3]];
            int32_t w = filt[c * fstr[0] + rx * fstr[1] + ry * fstr[2]];
            acc += (uint32_t)((w - (int32_t)filter_zero) * (a - (int32_t)input_zero));
        }
        put(out, c * ostr[0] + x * ostr[1] + y * ostr[2] + b * ostr[3], 0, acc, multiplier, shift, zero, lo, hi);
    }
}
