// hexagon_benchmarks.hip — apps/hexagon_benchmarks: six single-plane u8 stencils, conv3x3a16, conv3x3a32 (a run-time int8 3x3 mask,
// int16 / int32 accumulator), dilate3x3, median3x3, gaussian5x5 and sobel; 6 AOT entry points from one kernel template.
// Reference semantics: conv3x3_generator.cpp:17-27, dilate3x3_generator.cpp, median3x3_generator.cpp, gaussian5x5_generator.cpp and
// sobel_generator.cpp (generate()), each over repeat_edge of the INPUT's own box; the contract the kernels share with the checker
// (tests/cpp/hexagon_benchmarks_check.c) is restated in include/hlmi_pipelines.h and DESIGN.md §5.6.  Integer arithmetic only: the
// default and the _nofma build give the same bytes.
//
//   hb_slide<F>    one launch, every shape.  A lane owns 8 consecutive pixels of a row, one 8-byte word; lanes 1 .. 62 of a wave
//                  produce output (496 pixels), lanes 0 and 63 hold the words beside them, so that every x +- 1, x +- 2 neighbour is
//                  in an adjacent lane.  A wave slides down 4 rows with a window of 3 (5) rows in registers; a workgroup is 4 waves,
//                  stacked in y.  A row is held as packed u16 pairs — the even pixels (p0, p2), (p4, p6), the odd ones (p1, p3),
//                  (p5, p7) and the pixels beside the word — so that one packed instruction serves two pixels and the pixel at
//                  x +- 1 of a pair is the other stream's pair or one v_alignbit away.  A wave takes the 8-byte accesses only where
//                  every word it touches is whole (inside the row, or wholly left or right of it, where the clamp makes it one
//                  replicated byte) and 8-byte aligned in both buffers, base pointers and row strides counted (a wave-uniform
//                  choice); any other wave fills the same registers from clamped per-byte loads and stores per byte.
//   hb_general<F>  hlmi_hexagon_benchmarks_general: one thread per output pixel, its 9 (25) clamped taps from global memory, the
//                  arithmetic in the contract's own types.
// The packed forms are exact restatements: every intermediate of dilate, median, sobel and gaussian fits 16 bits or is defined
// modulo 2^16 by the contract (gaussian's cols, conv3x3a16's sum); conv3x3a32 splits the mask into 16 * (m >> 4) + (m & 15), whose two
// sums fit int16 and uint16, and floor(sum / 16) is the first plus the second shifted.
#include "hlmi_internal.h"

using namespace hlmi;

namespace {

constexpr int PX = 8;                      // pixels per lane: one 8-byte word
constexpr int OUT_LANES = 62;              // lanes 1 .. 62 produce output
constexpr int WAVE_PX = OUT_LANES * PX;    // output pixels per wave and row
constexpr int ROWS = 4;                    // rows a wave slides over
constexpr int WAVES = 4;                   // waves per workgroup, stacked in y
constexpr int GROUP_ROWS = WAVES * ROWS;   // rows per workgroup

enum { CONV16, CONV32, DILATE, MEDIAN, GAUSSIAN, SOBEL, NFILTERS };

struct HGeom {
    const uint8_t *src;   // in(0, 0): the input's mins are pinned to 0
    long s_sy;
    int iw, ih;           // the clamp: x to [0, iw - 1], y to [0, ih - 1]
    uint8_t *dst;         // out(ox, oy)
    long d_sy;
    int ox, oy, ow, oh;   // the output's region
};

// the nine mask values as the kernels take them, mask(j, i) at [3 * i + j]: v the values themselves (hb_general), a and b splat into
// both halves of a packed pair: conv3x3a16 a = m; conv3x3a32 a = m >> 4, b = m & 15
struct Mask {
    int v[9];
    uint32_t a[9], b[9];
};

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef short i16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u16x2 pk(uint32_t v) { return __builtin_bit_cast(u16x2, v); }
__device__ __forceinline__ uint32_t bits(u16x2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ u16x2 pmax(u16x2 a, u16x2 b) { return __builtin_elementwise_max(a, b); }
__device__ __forceinline__ u16x2 pmin(u16x2 a, u16x2 b) { return __builtin_elementwise_min(a, b); }
__device__ __forceinline__ u16x2 pmid(u16x2 a, u16x2 b, u16x2 c) { return pmax(pmin(pmax(a, b), c), pmin(a, b)); }
// (lo's high half, hi's low half): the pair one place further along a stream
__device__ __forceinline__ u16x2 next(u16x2 hi, u16x2 lo) { return pk(__builtin_amdgcn_alignbit(bits(hi), bits(lo), 16)); }

// One row of a lane, H pixels more on either side.  The even stream is p-2 p0 p2 p4 p6 p8, the odd one p-1 p1 p3 p5 p7 p9:
// v[0] = (p0, p2), v[1] = (p1, p3), v[2] = (p4, p6), v[3] = (p5, p7), low half first; H == 1: v[4] = (p8, p-1); H == 2: v[4] = (p8, p-2),
// v[5] = (p9, p-1).  Whatever is elementwise (the column step) treats all 4 + H alike.
template<int H>
struct Row {
    static constexpr int N = 4 + H;
    u16x2 v[N];
};

// w: the lane's word; lwy: the bytes p-4 .. p-1; rwx: the bytes p8 .. p11
template<int H>
__device__ __forceinline__ Row<H> unpack(uint2 w, uint32_t lwy, uint32_t rwx) {
    constexpr uint32_t M = 0x00ff00ffu;
    Row<H> r;
    r.v[0] = pk(w.x & M), r.v[1] = pk((w.x >> 8) & M), r.v[2] = pk(w.y & M), r.v[3] = pk((w.y >> 8) & M);
    if constexpr (H == 1) {
        r.v[4] = pk((rwx & 0xffu) | ((lwy >> 24) << 16));
    } else {
        r.v[4] = pk((rwx & 0xffu) | (lwy & 0x00ff0000u));
        r.v[5] = pk(((rwx >> 8) & 0xffu) | ((lwy >> 24) << 16));
    }
    return r;
}

// The pairs at x - 1 and x + 1 of v[0 .. 3], from 4 + H values of one kind
template<int N>
__device__ __forceinline__ void beside(const u16x2 (&c)[N], u16x2 (&l)[4], u16x2 (&r)[4]) {
    l[0] = next(c[1], c[N - 1]), l[1] = c[0], l[2] = next(c[3], c[1]), l[3] = c[2];
    r[0] = c[1], r[1] = next(c[2], c[0]), r[2] = c[3], r[3] = next(c[4], c[2]);
}

// ---------------------------------------------------------------------------------------------------------------- the six filters
// Each: H, the halo; packed(): the four output pairs (values 0 .. 255) from the 2 H + 1 rows around the output row; pixel(): the
// same value from a tap(dx, dy) that returns in(x + dx, y + dy), in the contract's own types.
struct Dilate {
    static constexpr int H = 1;
    __device__ __forceinline__ void packed(const Row<1> (&r)[3], u16x2 (&o)[4]) const {
        u16x2 c[5], a[4], b[4];
#pragma unroll
        for (int k = 0; k < 5; k++) c[k] = pmax(pmax(r[0].v[k], r[1].v[k]), r[2].v[k]);
        beside(c, a, b);
#pragma unroll
        for (int k = 0; k < 4; k++) o[k] = pmax(pmax(a[k], c[k]), b[k]);
    }
    template<typename T>
    __device__ __forceinline__ uint8_t pixel(T tap) const {
        int m = 0;
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) m = max(m, tap(dx, dy));
        return (uint8_t)m;
    }
};

__device__ __forceinline__ int mid3(int a, int b, int c) { return max(min(max(a, b), c), min(a, b)); }

struct Median {
    static constexpr int H = 1;
    __device__ __forceinline__ void packed(const Row<1> (&r)[3], u16x2 (&o)[4]) const {
        u16x2 mx[5], mn[5], md[5];
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const u16x2 t = pmax(r[0].v[k], r[1].v[k]), u = pmin(r[0].v[k], r[1].v[k]), c = r[2].v[k];
            mx[k] = pmax(t, c), mn[k] = pmin(u, c), md[k] = pmax(pmin(t, c), u);
        }
        u16x2 xa[4], xb[4], na[4], nb[4], da[4], db[4];
        beside(mx, xa, xb), beside(mn, na, nb), beside(md, da, db);
#pragma unroll
        for (int k = 0; k < 4; k++)
            o[k] = pmid(pmin(pmin(xa[k], mx[k]), xb[k]), pmax(pmax(na[k], mn[k]), nb[k]), pmid(da[k], md[k], db[k]));
    }
    template<typename T>
    __device__ __forceinline__ uint8_t pixel(T tap) const {
        int mx[3], mn[3], md[3];
        for (int j = 0; j < 3; j++) {
            const int a = tap(j - 1, -1), b = tap(j - 1, 0), c = tap(j - 1, 1);
            mx[j] = max(max(a, b), c), mn[j] = min(min(a, b), c), md[j] = mid3(a, b, c);
        }
        return (uint8_t)mid3(min(min(mx[0], mx[1]), mx[2]), max(max(mn[0], mn[1]), mn[2]), mid3(md[0], md[1], md[2]));
    }
};

struct Sobel {
    static constexpr int H = 1;
    // |ax(x, y - 1) - ax(x, y + 1)| is linear in the rows' difference d = in(., y - 1) - in(., y + 1): |d(x - 1) + 2 d(x) + d(x + 1)|,
    // at most 1020 in int16, as is ay; the sum of the two is at most 2040
    __device__ __forceinline__ void packed(const Row<1> (&r)[3], u16x2 (&o)[4]) const {
        u16x2 d[5], ay[5], dl[4], dr[4], al[4], ar[4];
#pragma unroll
        for (int k = 0; k < 5; k++) d[k] = r[0].v[k] - r[2].v[k], ay[k] = r[0].v[k] + r[1].v[k] + r[1].v[k] + r[2].v[k];
        beside(d, dl, dr), beside(ay, al, ar);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const i16x2 sx = __builtin_elementwise_abs((i16x2)(dl[k] + d[k] + d[k] + dr[k]));
            const i16x2 sy = __builtin_elementwise_abs((i16x2)(al[k] - ar[k]));
            o[k] = pmin((u16x2)(sx + sy), pk(0x00ff00ffu));
        }
    }
    template<typename T>
    __device__ __forceinline__ uint8_t pixel(T tap) const {
        auto ax = [&](int dy) { return (uint16_t)(tap(-1, dy) + 2 * tap(0, dy) + tap(1, dy)); };
        auto ay = [&](int dx) { return (uint16_t)(tap(dx, -1) + 2 * tap(dx, 0) + tap(dx, 1)); };
        const int sx = abs((int)ax(-1) - (int)ax(1)), sy = abs((int)ay(-1) - (int)ay(1));
        return (uint8_t)min(sx + sy, 255);
    }
};

struct Gaussian {
    static constexpr int H = 2;
    // rows fit 16 bits (at most 4080); cols is taken modulo 2^16 by the contract, and (cols >> 8) & 255 of the int16 is the
    // logical shift of the uint16
    __device__ __forceinline__ void packed(const Row<2> (&r)[5], u16x2 (&o)[4]) const {
        const u16x2 four = pk(0x00040004u), six = pk(0x00060006u);
        u16x2 c[6];
#pragma unroll
        for (int k = 0; k < 6; k++) c[k] = (r[0].v[k] + r[4].v[k]) + four * (r[1].v[k] + r[3].v[k]) + six * r[2].v[k];
        const u16x2 e0 = next(c[0], c[4]), e1 = next(c[2], c[0]), e2 = next(c[4], c[2]);   // (p-2, p0), (p2, p4), (p6, p8)
        const u16x2 o0 = next(c[1], c[5]), o1 = next(c[3], c[1]), o2 = next(c[5], c[3]);   // (p-1, p1), (p3, p5), (p7, p9)
        o[0] = ((e0 + e1) + four * (o0 + c[1]) + six * c[0]) >> 8;
        o[1] = ((o0 + o1) + four * (c[0] + e1) + six * c[1]) >> 8;
        o[2] = ((e1 + e2) + four * (o1 + c[3]) + six * c[2]) >> 8;
        o[3] = ((o1 + o2) + four * (c[2] + e2) + six * c[3]) >> 8;
    }
    template<typename T>
    __device__ __forceinline__ uint8_t pixel(T tap) const {
        const int w[5] = {1, 4, 6, 4, 1};
        int16_t cols = 0;
        for (int dx = -2; dx <= 2; dx++) {
            int16_t rows = 0;
            for (int dy = -2; dy <= 2; dy++) rows = (int16_t)(rows + w[dy + 2] * tap(dx, dy));
            cols = (int16_t)(uint16_t)((uint32_t)(uint16_t)cols + (uint32_t)w[dx + 2] * (uint32_t)(uint16_t)rows);
        }
        return (uint8_t)(cols >> 8);
    }
};

template<bool A32>
struct Conv {
    static constexpr int H = 1;
    Mask m;
    __device__ __forceinline__ void packed(const Row<1> (&r)[3], u16x2 (&o)[4]) const {
        u16x2 hi[4] = {}, lo[4] = {};
#pragma unroll
        for (int i = 0; i < 3; i++) {
            u16x2 t[3][4];   // the pairs at x - 1, x, x + 1 of row i
            beside(r[i].v, t[0], t[2]);
#pragma unroll
            for (int k = 0; k < 4; k++) t[1][k] = r[i].v[k];
#pragma unroll
            for (int j = 0; j < 3; j++)
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    hi[k] += t[j][k] * pk(m.a[3 * i + j]);
                    if (A32) lo[k] += t[j][k] * pk(m.b[3 * i + j]);
                }
        }
        const i16x2 zero = {0, 0}, top = {255, 255};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const i16x2 s = A32 ? (i16x2)hi[k] + (i16x2)(lo[k] >> 4) : (i16x2)hi[k] >> 4;
            o[k] = (u16x2)__builtin_elementwise_min(__builtin_elementwise_max(s, zero), top);
        }
    }
    template<typename T>
    __device__ __forceinline__ uint8_t pixel(T tap) const {
        uint32_t sum = 0;   // modulo 2^32; narrowed below
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) sum += (uint32_t)(tap(j - 1, i - 1) * m.v[3 * i + j]);
        const int s = A32 ? (int32_t)sum : (int)(int16_t)(uint16_t)sum;
        return (uint8_t)min(max(s >> 4, 0), 255);
    }
};

// ---------------------------------------------------------------------------------------------------------------- the sliding kernel
__device__ __forceinline__ long clamp_to(long v, int n) { return max(min(v, (long)n - 1), 0L); }

template<typename F>
__global__ __launch_bounds__(256) void hb_slide(HGeom g, F f) {
    constexpr int H = F::H, NR = 2 * H + 1;
    const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int y0 = ((int)blockIdx.y * WAVES + wave) * ROWS;
    if (y0 >= g.oh) return;   // scalar: no barrier follows
    const long xw = (long)blockIdx.x * WAVE_PX;
    const long x0 = xw + PX * (lane - 1);   // the lane's first output column; lanes 0 and 63: the words beside the wave's
    const long X0 = g.ox + x0;              // and its first sample column
    const long Xa = g.ox + xw - PX, Xb = Xa + 64 * PX;   // the wave's words cover [Xa, Xb)
    // wave-uniform: every word on the 8-byte grid of both buffers, and whole: the input's inside the row or wholly beside it, the
    // output's inside the row
    const uintptr_t grid = (uintptr_t)g.src | (uintptr_t)g.s_sy | (uintptr_t)g.dst | (uintptr_t)g.d_sy | (uintptr_t)(long)g.ox;
    const bool wide = (grid & 7) == 0 && g.iw >= PX && ((g.iw & 7) == 0 || Xb <= g.iw) && ((g.ow & 7) == 0 || xw + WAVE_PX <= g.ow);
    const bool mine = lane >= 1 && lane <= OUT_LANES && x0 < g.ow;
    Row<H> ring[NR];
    auto emit = [&](int j) {   // output row y0 + j from the ring
        u16x2 o[4];
        f.packed(ring, o);
        const uint2 w = make_uint2(bits(o[0]) | (bits(o[1]) << 8), bits(o[2]) | (bits(o[3]) << 8));
        uint8_t *q = g.dst + (long)(y0 + j) * g.d_sy + x0;
        if (wide) {
            if (mine && x0 + PX <= g.ow) *reinterpret_cast<uint2 *>(q) = w;
        } else if (mine) {
#pragma unroll
            for (int i = 0; i < PX; i++)
                if (x0 + i < g.ow) q[i] = (uint8_t)((i < 4 ? w.x : w.y) >> (8 * (i & 3)));
        }
    };
    if (wide) {
        // every row the wave reads, clamped, so all of them are loads of valid words whatever the region's height
        const long xl = max(min(X0, (long)g.iw - PX), 0L);
        const bool beside_row = Xa < 0 || Xb > g.iw;   // scalar: some lane's word is the clamp's replicated edge byte
        const int up = max(lane - 1, 0) * 4, down = min(lane + 1, 63) * 4;
        uint2 w[ROWS + 2 * H];
#pragma unroll
        for (int r = 0; r < ROWS + 2 * H; r++)
            w[r] = *reinterpret_cast<const uint2 *>(g.src + clamp_to((long)g.oy + y0 - H + r, g.ih) * g.s_sy + xl);
        auto row = [&](int r) {
            uint2 v = w[r];
            if (beside_row) {
                if (X0 < 0) v.x = v.y = (v.x & 0xffu) * 0x01010101u;
                else if (X0 >= g.iw) v.x = v.y = (v.y >> 24) * 0x01010101u;
            }
            const uint32_t lwy = (uint32_t)__builtin_amdgcn_ds_bpermute(up, (int)v.y);
            const uint32_t rwx = (uint32_t)__builtin_amdgcn_ds_bpermute(down, (int)v.x);
            return unpack<H>(v, lwy, rwx);
        };
#pragma unroll
        for (int r = 0; r < NR - 1; r++) ring[r + 1] = row(r);
#pragma unroll
        for (int j = 0; j < ROWS; j++) {
            if (y0 + j >= g.oh) break;   // scalar
#pragma unroll
            for (int r = 0; r < NR - 1; r++) ring[r] = ring[r + 1];
            ring[NR - 1] = row(j + NR - 1);
            emit(j);
        }
    } else {
        if (!mine) return;
        auto row = [&](int r) {
            const uint8_t *p = g.src + clamp_to((long)g.oy + y0 - H + r, g.ih) * g.s_sy;
            auto at = [&](int i) { return (uint32_t)p[clamp_to(X0 + i, g.iw)]; };
            const uint2 v = make_uint2(at(0) | (at(1) << 8) | (at(2) << 16) | (at(3) << 24), at(4) | (at(5) << 8) | (at(6) << 16) | (at(7) << 24));
            const uint32_t lwy = (at(-1) << 24) | (H == 2 ? at(-2) << 16 : 0u), rwx = at(8) | (H == 2 ? at(9) << 8 : 0u);
            return unpack<H>(v, lwy, rwx);
        };
#pragma unroll
        for (int r = 0; r < NR - 1; r++) ring[r + 1] = row(r);
#pragma unroll 1
        for (int j = 0; j < ROWS; j++) {
            if (y0 + j >= g.oh) break;
#pragma unroll
            for (int r = 0; r < NR - 1; r++) ring[r] = ring[r + 1];
            ring[NR - 1] = row(j + NR - 1);
            emit(j);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- general path
template<typename F>
__global__ __launch_bounds__(256) void hb_general(HGeom g, F f) {
    const long x = (long)blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= g.ow) return;
    const long X = g.ox + x, Y = g.oy + y;
    g.dst[y * g.d_sy + x] = f.pixel([&](int dx, int dy) { return (int)g.src[clamp_to(Y + dy, g.ih) * g.s_sy + clamp_to(X + dx, g.iw)]; });
}

// ---------------------------------------------------------------------------------------------------------------- host
// no estimates: the generators declare none
const ArgTable tables[NFILTERS] = {
    {"conv3x3a16", {in_buf("input", T_U8, 2), in_buf("mask", T_I8, 2), out_buf("output", T_U8, 2)}},
    {"conv3x3a32", {in_buf("input", T_U8, 2), in_buf("mask", T_I8, 2), out_buf("output", T_U8, 2)}},
    {"dilate3x3", {in_buf("input", T_U8, 2), out_buf("output", T_U8, 2)}},
    {"median3x3", {in_buf("input", T_U8, 2), out_buf("output", T_U8, 2)}},
    {"gaussian5x5", {in_buf("input", T_U8, 2), out_buf("output", T_U8, 2)}},
    {"sobel", {in_buf("input", T_U8, 2), out_buf("output", T_U8, 2)}},
};
const char *const slide_names[NFILTERS] = {"hb_conv3x3a16", "hb_conv3x3a32", "hb_dilate3x3", "hb_median3x3", "hb_gaussian5x5", "hb_sobel"};
const char *const general_names[NFILTERS] = {"hb_conv3x3a16_general", "hb_conv3x3a32_general", "hb_dilate3x3_general",
                                             "hb_median3x3_general",  "hb_gaussian5x5_general", "hb_sobel_general"};

int host_clamp_to(long v, int n) { return (int)std::max<long>(std::min<long>(v, (long)n - 1), 0); }

int blocks_ok(void *uc, const char *name, size_t gx, size_t gy) {
    if (gx <= 0x7fffffffu && gy <= 65535u) return 0;
    return report(uc, halide_error_code_buffer_extents_too_large, "%s: %zu x %zu workgroups exceed one launch", name, gx, gy);
}

// mask(j, i), j, i in 0 .. 2, read on the host once per call (the reference's drivers keep it in host memory): the kernels take the
// nine values as arguments, so a mask in host memory never goes to the device.  Where only the device holds current values
// (no host pointer, or device_dirty) the buffer goes through the input protocol, which orders the stream behind its producer, and
// the three rows are fetched behind a stream synchronisation
int read_mask(void *uc, const DeviceCtx &ctx, const BufArg &arg, int id, Mask *m) {
    halide_buffer_t *mask = arg.buf;
    const halide_dimension_t *d = mask->dim;
    const long first = (0L - d[0].min) + (0L - d[1].min) * d[1].stride;
    int8_t v[9];
    if (mask->host && !(mask->flags & halide_buffer_flag_device_dirty)) {
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) v[3 * i + j] = ((const int8_t *)mask->host)[first + (long)i * d[1].stride + j];
    } else {
        if (int r = input_to_device(uc, ctx, arg)) return r;
        HLMI_HIP(uc, hipStreamSynchronize(ctx.stream));
        for (int i = 0; i < 3; i++) HLMI_HIP(uc, hipMemcpy(v + 3 * i, dev_ptr<int8_t>(mask) + first + (long)i * d[1].stride, 3, hipMemcpyDeviceToHost));
    }
    for (int k = 0; k < 9; k++) {
        const int a = id == CONV32 ? v[k] >> 4 : v[k], b = v[k] & 15;
        m->v[k] = v[k], m->a[k] = (uint32_t)(uint16_t)a * 0x10001u, m->b[k] = (uint32_t)b * 0x10001u;
    }
    return 0;
}

template<typename F>
int launch(void *uc, int id, hipStream_t st, const HGeom &g, const F &f, bool general_only) {
    timing_note_bytes(2.0 * g.ow * g.oh);   // each pixel read once and written once
    if (!general_only) {
        const size_t gx = ((size_t)g.ow + WAVE_PX - 1) / WAVE_PX, gy = ((size_t)g.oh + GROUP_ROWS - 1) / GROUP_ROWS;
        if (int r = blocks_ok(uc, tables[id].md.name, gx, gy)) return r;
        HLMI_LAUNCH(uc, slide_names[id], st, hb_slide<F>, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, g, f);
    } else {
        const size_t gx = ((size_t)g.ow + 255) / 256;
        if (int r = blocks_ok(uc, tables[id].md.name, gx, g.oh)) return r;
        HLMI_LAUNCH(uc, general_names[id], st, hb_general<F>, dim3((unsigned)gx, (unsigned)g.oh), dim3(256), 0, g, f);
    }
    return 0;
}

int entry(int id, halide_buffer_t *input, halide_buffer_t *mask, halide_buffer_t *output, bool general_only) {
    void *uc = nullptr;
    const bool conv = id == CONV16 || id == CONV32;
    const int n = conv ? 3 : 2, halo = id == GAUSSIAN ? 2 : 1;
    BufArg args[3];
    if (conv) {
        tables[id].bufs(args, {input, mask, output});
    } else {
        BufArg two[2];
        tables[id].bufs(two, {input, output});
        args[0] = two[0], args[1] = two[1];
    }
    int r = check_not_null(uc, args, n);
    if (r) return r;
    if ((r = check_type_and_dims(uc, args, n))) return r;
    const halide_dimension_t *id_ = input->dim, *od = output->dim;
    // the generators pin the input's mins to 0, and all but sobel's the output's
    check_equal(uc, "input.min.0", id_[0].min, "0", 0);
    check_equal(uc, "input.min.1", id_[1].min, "0", 0);
    if (id != SOBEL) {
        check_equal(uc, "output.min.0", od[0].min, "0", 0);
        check_equal(uc, "output.min.1", od[1].min, "0", 0);
    }
    if ((r = checks_done(uc))) return r;
    if (any_bounds_query(args, n)) {
        // the output's region is the request and stays as passed; the clamp's bound is the input's own box, so that stays too
        // (as for linear_blur); the mask is read over [0, 3) x [0, 3)
        const int mins[2] = {0, 0}, ext[2] = {3, 3};
        if (conv) answer_query(mask, mins, ext);
        return 0;
    }
    if ((r = check_shapes(uc, args, n))) return r;
    const int iw = id_[0].extent, ih = id_[1].extent;
    // what the region reads: columns clamp(ox - halo) .. clamp(ox + ow - 1 + halo), rows alike; an empty input holds none of them
    const int rx0 = host_clamp_to((long)od[0].min - halo, iw), rx1 = host_clamp_to((long)od[0].min + od[0].extent - 1 + halo, iw);
    const int ry0 = host_clamp_to((long)od[1].min - halo, ih), ry1 = host_clamp_to((long)od[1].min + od[1].extent - 1 + halo, ih);
    check_covers(uc, args[0], 0, rx0, rx1 - rx0 + 1);
    check_covers(uc, args[0], 1, ry0, ry1 - ry0 + 1);
    if (conv) {
        check_covers(uc, args[1], 0, 0, 3);
        check_covers(uc, args[1], 1, 0, 3);
    }
    DeviceCtx ctx;
    const BufArg io[2] = {args[0], args[n - 1]};   // the mask stays where it is: read_mask
    if ((r = to_device(uc, &ctx, io, 2))) return r;
    HGeom g;
    g.ox = od[0].min, g.oy = od[1].min, g.ow = od[0].extent, g.oh = od[1].extent;
    if (g.ow > 0 && g.oh > 0) {
        g.src = dev_ptr<uint8_t>(input), g.s_sy = id_[1].stride, g.iw = iw, g.ih = ih;
        g.dst = dev_ptr<uint8_t>(output), g.d_sy = od[1].stride;
        hipStream_t st = ctx.stream;
        Mask m = {};
        if (conv && (r = read_mask(uc, ctx, args[1], id, &m))) return r;
        switch (id) {
            case CONV16: r = launch(uc, id, st, g, Conv<false>{m}, general_only); break;
            case CONV32: r = launch(uc, id, st, g, Conv<true>{m}, general_only); break;
            case DILATE: r = launch(uc, id, st, g, Dilate{}, general_only); break;
            case MEDIAN: r = launch(uc, id, st, g, Median{}, general_only); break;
            case GAUSSIAN: r = launch(uc, id, st, g, Gaussian{}, general_only); break;
            default: r = launch(uc, id, st, g, Sobel{}, general_only); break;
        }
        if (r) return r;
    }
    mark_output_written(output);
    return 0;
}

}  // namespace

extern "C" int conv3x3a16(halide_buffer_t *input, halide_buffer_t *mask, halide_buffer_t *output) { return entry(CONV16, input, mask, output, false); }
HLMI_ENTRY(conv3x3a16, tables[CONV16].md)
extern "C" int conv3x3a32(halide_buffer_t *input, halide_buffer_t *mask, halide_buffer_t *output) { return entry(CONV32, input, mask, output, false); }
HLMI_ENTRY(conv3x3a32, tables[CONV32].md)
extern "C" int dilate3x3(halide_buffer_t *input, halide_buffer_t *output) { return entry(DILATE, input, nullptr, output, false); }
HLMI_ENTRY(dilate3x3, tables[DILATE].md)
extern "C" int median3x3(halide_buffer_t *input, halide_buffer_t *output) { return entry(MEDIAN, input, nullptr, output, false); }
HLMI_ENTRY(median3x3, tables[MEDIAN].md)
extern "C" int gaussian5x5(halide_buffer_t *input, halide_buffer_t *output) { return entry(GAUSSIAN, input, nullptr, output, false); }
HLMI_ENTRY(gaussian5x5, tables[GAUSSIAN].md)
extern "C" int sobel(halide_buffer_t *input, halide_buffer_t *output) { return entry(SOBEL, input, nullptr, output, false); }
HLMI_ENTRY(sobel, tables[SOBEL].md)

// Measurement and test hook (hlmi_internal.h): the named entry point with one thread per output pixel, whatever the sizes; `mask` is
// read by the two conv3x3 filters only.  Its grid takes one output row per workgroup row, so it refuses an output of more than 65535
// rows (-6) that the sliding kernel, at 16 rows per workgroup row, accepts.
extern "C" int hlmi_hexagon_benchmarks_general(const char *name, halide_buffer_t *input, halide_buffer_t *mask, halide_buffer_t *output) {
    for (int id = 0; name && id < NFILTERS; id++)
        if (strcmp(name, tables[id].md.name) == 0) return entry(id, input, mask, output, true);
    return report(nullptr, halide_error_code_constraint_violated, "hlmi_hexagon_benchmarks_general: no entry point named %s", name ? name : "(null)");
}
