/* hexagon_benchmarks_check.c — the checker of the six filters of apps/hexagon_benchmarks, plain C, two restatements per filter:
 *
 *   hb_<name>          from the generator (conv3x3_generator.cpp, dilate3x3_generator.cpp, median3x3_generator.cpp,
 *                      gaussian5x5_generator.cpp, sobel_generator.cpp): separable where the generator is, every value in the type
 *                      the generator gives it
 *   hb_<name>_verify   from the matching verify() of process.h: the window gathered tap by tap, the median by selection, the sums in
 *                      an int16_t or int32_t accumulator
 *
 * tests/hexagon_benchmarks_checker.py declares the object (tests/checker_lib.py builds it) and drives this file through ctypes; tests/test_hexagon_benchmarks.py
 * holds the two to each other and to numpy.  Integer arithmetic only: there is no canonical form to choose.  Wrapping is written
 * out (a sum formed in uint32_t, narrowed through uint16_t), never left to a signed overflow.
 *
 * Every function: `in` is the input plane, iw x ih samples, row stride `is`, whose sample (0, 0) is in[0]; reads are clamped into
 * [0, iw - 1] x [0, ih - 1]; `out` is dense, ow x oh, and holds the output region whose first pixel is (ox, oy).  mask(j, i) is
 * mask[3 * i + j]. */
#include <stddef.h>
#include <stdint.h>

typedef struct {
    const uint8_t *in;
    int iw, ih;
    long is;
} hb_plane;

static int hb_clamp(long v, int n) { return (int)(v < 0 ? 0 : (v > n - 1 ? n - 1 : v)); }
static uint8_t hb_at(const hb_plane *p, long x, long y) { return p->in[(long)hb_clamp(y, p->ih) * p->is + hb_clamp(x, p->iw)]; }

static uint8_t hb_max2(uint8_t a, uint8_t b) { return a > b ? a : b; }
static uint8_t hb_min2(uint8_t a, uint8_t b) { return a < b ? a : b; }
static uint8_t hb_max3(uint8_t a, uint8_t b, uint8_t c) { return hb_max2(hb_max2(a, b), c); }
static uint8_t hb_min3(uint8_t a, uint8_t b, uint8_t c) { return hb_min2(hb_min2(a, b), c); }
static uint8_t hb_mid3(uint8_t a, uint8_t b, uint8_t c) { return hb_max2(hb_min2(hb_max2(a, b), c), hb_min2(a, b)); }

#define HB_ARGS const uint8_t *in, int iw, int ih, long is, uint8_t *out, int ox, int oy, int ow, int oh
#define HB_LOOP                            \
    const hb_plane p = {in, iw, ih, is};   \
    for (int v = 0; v < oh; v++)           \
        for (int u = 0; u < ow; u++)
#define HB_XY const long x = (long)ox + u, y = (long)oy + v
#define HB_OUT out[(size_t)v * (size_t)ow + (size_t)u]

/* ------------------------------------------------------------------------------------------------ dilate3x3 */
static uint8_t hb_dilate_max_y(const hb_plane *p, long x, long y) { return hb_max3(hb_at(p, x, y - 1), hb_at(p, x, y), hb_at(p, x, y + 1)); }

void hb_dilate3x3(HB_ARGS) {
    HB_LOOP {
        HB_XY;
        HB_OUT = hb_max3(hb_dilate_max_y(&p, x - 1, y), hb_dilate_max_y(&p, x, y), hb_dilate_max_y(&p, x + 1, y));
    }
}

void hb_dilate3x3_verify(HB_ARGS) {
    HB_LOOP {
        HB_XY;
        uint8_t m = 0;
        for (int dx = -1; dx <= 1; dx++) {
            const uint8_t col = hb_max3(hb_at(&p, x + dx, y - 1), hb_at(&p, x + dx, y), hb_at(&p, x + dx, y + 1));
            if (col > m) m = col;
        }
        HB_OUT = m;
    }
}

/* ------------------------------------------------------------------------------------------------ median3x3 */
void hb_median3x3(HB_ARGS) {
    HB_LOOP {
        HB_XY;
        uint8_t mx[3], mn[3], md[3];
        for (int j = 0; j < 3; j++) {
            const uint8_t a = hb_at(&p, x + j - 1, y - 1), b = hb_at(&p, x + j - 1, y), c = hb_at(&p, x + j - 1, y + 1);
            mx[j] = hb_max3(a, b, c), mn[j] = hb_min3(a, b, c), md[j] = hb_mid3(a, b, c);
        }
        HB_OUT = hb_mid3(hb_min3(mx[0], mx[1], mx[2]), hb_max3(mn[0], mn[1], mn[2]), hb_mid3(md[0], md[1], md[2]));
    }
}

/* the fifth smallest of the nine, by selection */
void hb_median3x3_verify(HB_ARGS) {
    HB_LOOP {
        HB_XY;
        uint8_t w[9];
        int n = 0;
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) w[n++] = hb_at(&p, x + dx, y + dy);
        for (int k = 0; k <= 4; k++) {
            int least = k;
            for (int t = k + 1; t < 9; t++)
                if (w[t] < w[least]) least = t;
            const uint8_t s = w[k];
            w[k] = w[least], w[least] = s;
        }
        HB_OUT = w[4];
    }
}

/* ------------------------------------------------------------------------------------------------ sobel */
static uint16_t hb_sobel_ax(const hb_plane *p, long x, long y) {
    return (uint16_t)((uint16_t)hb_at(p, x - 1, y) + (uint16_t)(2 * (uint16_t)hb_at(p, x, y)) + (uint16_t)hb_at(p, x + 1, y));
}
static uint16_t hb_sobel_ay(const hb_plane *p, long x, long y) {
    return (uint16_t)((uint16_t)hb_at(p, x, y - 1) + (uint16_t)(2 * (uint16_t)hb_at(p, x, y)) + (uint16_t)hb_at(p, x, y + 1));
}
static uint16_t hb_absd(uint16_t a, uint16_t b) { return (uint16_t)(a > b ? a - b : b - a); }

void hb_sobel(HB_ARGS) {
    HB_LOOP {
        HB_XY;
        const uint16_t sx = hb_absd(hb_sobel_ax(&p, x, y - 1), hb_sobel_ax(&p, x, y + 1));
        const uint16_t sy = hb_absd(hb_sobel_ay(&p, x - 1, y), hb_sobel_ay(&p, x + 1, y));
        const uint16_t s = (uint16_t)(sx + sy);
        HB_OUT = (uint8_t)(s > 255 ? 255 : s);
    }
}

void hb_sobel_verify(HB_ARGS) {
    HB_LOOP {
        HB_XY;
        int t[3][3]; /* t[dy + 1][dx + 1] */
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) t[dy + 1][dx + 1] = hb_at(&p, x + dx, y + dy);
        int gx = (t[0][0] + 2 * t[0][1] + t[0][2]) - (t[2][0] + 2 * t[2][1] + t[2][2]);
        int gy = (t[0][0] + 2 * t[1][0] + t[2][0]) - (t[0][2] + 2 * t[1][2] + t[2][2]);
        if (gx < 0) gx = -gx;
        if (gy < 0) gy = -gy;
        const int s = gx + gy;
        HB_OUT = (uint8_t)(s < 0 ? 0 : (s > 255 ? 255 : s));
    }
}

/* ------------------------------------------------------------------------------------------------ gaussian5x5 */
static int16_t hb_wrap16(uint32_t v) { return (int16_t)(uint16_t)v; }

/* rows(x, y): down the column, int16; at most 16 * 255 */
static int16_t hb_gauss_rows(const hb_plane *p, long x, long y) {
    const uint32_t s = (uint32_t)hb_at(p, x, y - 2) + 4u * hb_at(p, x, y - 1) + 6u * hb_at(p, x, y) + 4u * hb_at(p, x, y + 1) + (uint32_t)hb_at(p, x, y + 2);
    return hb_wrap16(s);
}

void hb_gaussian5x5(HB_ARGS) {
    HB_LOOP {
        HB_XY;
        /* cols(x, y): along the row, int16, wrapping (up to 65280) */
        const uint32_t s = (uint32_t)(uint16_t)hb_gauss_rows(&p, x - 2, y) + 4u * (uint16_t)hb_gauss_rows(&p, x - 1, y) + 6u * (uint16_t)hb_gauss_rows(&p, x, y) +
                           4u * (uint16_t)hb_gauss_rows(&p, x + 1, y) + (uint32_t)(uint16_t)hb_gauss_rows(&p, x + 2, y);
        const int16_t cols = hb_wrap16(s);
        HB_OUT = (uint8_t)(cols >> 8); /* arithmetic shift of a negative int16, then the low byte */
    }
}

void hb_gaussian5x5_verify(HB_ARGS) {
    static const int16_t k[5] = {1, 4, 6, 4, 1};
    HB_LOOP {
        HB_XY;
        int16_t blur = 0;
        for (int dx = -2; dx <= 2; dx++) {
            int16_t blur_y = 0;
            for (int dy = -2; dy <= 2; dy++) blur_y = hb_wrap16((uint32_t)(uint16_t)blur_y + (uint32_t)hb_at(&p, x + dx, y + dy) * (uint32_t)k[dy + 2]);
            blur = hb_wrap16((uint32_t)(uint16_t)blur + (uint32_t)(uint16_t)blur_y * (uint32_t)k[dx + 2]);
        }
        HB_OUT = (uint8_t)(blur >> 8);
    }
}

/* ------------------------------------------------------------------------------------------------ conv3x3a16, conv3x3a32 */
#define HB_CONV_ARGS const uint8_t *in, int iw, int ih, long is, const int8_t *mask, uint8_t *out, int ox, int oy, int ow, int oh

/* the sum modulo 2^32; every product fits int16 */
static uint32_t hb_conv_sum(const hb_plane *p, const int8_t *mask, long x, long y) {
    uint32_t sum = 0;
    for (int i = -1; i <= 1; i++)
        for (int j = -1; j <= 1; j++) {
            const int16_t prod = (int16_t)((int16_t)hb_at(p, x + j, y + i) * (int16_t)mask[3 * (i + 1) + (j + 1)]);
            sum += (uint32_t)(int32_t)prod;
        }
    return sum;
}

static uint8_t hb_shift_clamp(int32_t s) {
    const int32_t q = s >> 4; /* arithmetic */
    return (uint8_t)(q < 0 ? 0 : (q > 255 ? 255 : q));
}

void hb_conv3x3a16(HB_CONV_ARGS) {
    HB_LOOP {
        HB_XY;
        HB_OUT = hb_shift_clamp((int32_t)hb_wrap16(hb_conv_sum(&p, mask, x, y)));
    }
}

void hb_conv3x3a32(HB_CONV_ARGS) {
    HB_LOOP {
        HB_XY;
        HB_OUT = hb_shift_clamp((int32_t)hb_conv_sum(&p, mask, x, y));
    }
}

/* an accumulator of the stated width, added to tap by tap, rows outermost */
void hb_conv3x3a16_verify(HB_CONV_ARGS) {
    HB_LOOP {
        HB_XY;
        int16_t acc = 0;
        for (int ry = -1; ry <= 1; ry++)
            for (int rx = -1; rx <= 1; rx++) {
                const int32_t prod = (int32_t)hb_at(&p, x + rx, y + ry) * (int32_t)mask[3 * (ry + 1) + (rx + 1)];
                acc = hb_wrap16((uint32_t)(uint16_t)acc + (uint32_t)prod);
            }
        acc = (int16_t)(acc >> 4);
        HB_OUT = (uint8_t)(acc < 0 ? 0 : (acc > 255 ? 255 : acc));
    }
}

void hb_conv3x3a32_verify(HB_CONV_ARGS) {
    HB_LOOP {
        HB_XY;
        int32_t acc = 0;
        for (int ry = -1; ry <= 1; ry++)
            for (int rx = -1; rx <= 1; rx++) acc += (int32_t)hb_at(&p, x + rx, y + ry) * (int32_t)mask[3 * (ry + 1) + (rx + 1)];
        acc >>= 4;
        HB_OUT = (uint8_t)(acc < 0 ? 0 : (acc > 255 ? 255 : acc));
    }
}

/* the int32 sum itself, for the tests that ask where conv3x3a16 and conv3x3a32 part; out: ow x oh int32 */
void hb_conv3x3_sum(const uint8_t *in, int iw, int ih, long is, const int8_t *mask, int32_t *out, int ox, int oy, int ow, int oh) {
    HB_LOOP {
        HB_XY;
        HB_OUT = (int32_t)hb_conv_sum(&p, mask, x, y);
    }
}
