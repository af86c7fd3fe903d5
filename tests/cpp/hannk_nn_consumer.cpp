// hannk_nn_consumer.cpp — a C++ program that uses the second half of the op library the way apps/hannk's interpreter does, written fresh
// against the headers include/aot/halide/<name>.h: a "same"-padded 3 x 3 stride-2 pool of either kind (what Pool2DOp::execute does: the
// input is translated by compute_padding, nothing is padded), a softmax with the multiplier and shift pairs of SoftmaxOp::execute, and the
// residual add of add_uint8, each through the C++-mangled symbols and each held to plain floating-point loops of its own.
// TEST INFRASTRUCTURE ONLY: tests/test_hannk_nn.py compiles it with the host compiler against libhlmi.so and runs it.
#include "halide/add_uint8_uint8.h"
#include "halide/average_pool_uint8.h"
#include "halide/max_pool_uint8.h"
#include "halide/softmax_uint8.h"

#include "hlmi_runtime.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

struct Buf {
    halide_buffer_t b;
    halide_dimension_t dim[4];
    Buf(void *host, std::initializer_list<int> extents) {
        memset(&b, 0, sizeof b);
        int stride = 1, d = 0;
        for (int e : extents) {
            dim[d].min = 0, dim[d].extent = e, dim[d].stride = stride, dim[d].flags = 0;
            stride *= e, d++;
        }
        const uint32_t v = 1u | (8u << 8) | (1u << 16);   // uint8, one lane
        memcpy(&b.type, &v, 4);
        b.host = (uint8_t *)host, b.dimensions = d, b.dim = dim, b.flags = 1;   // host dirty: the library uploads it
    }
    operator halide_buffer_t *() { return &b; }
};

int fail(const char *what, int code = 0) {
    printf("hannk nn consumer FAILED: %s (%d)\n", what, code);
    return 1;
}

uint32_t rnd() {
    static uint64_t s = 0x9E3779B97F4A7C15ull;
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
}

int compute_padding(int stride, int in_size, int filter_size, int out_size) {
    return std::max(0, (out_size - 1) * stride + filter_size - in_size) / 2;
}

// x = mantissa * 2^exponent / 2^15 (ops.cpp's IntFloat<int16_t>), times 2^power
void int_float16(float x, int power, int16_t *mantissa, int *exponent) {
    int e;
    const float m = std::frexp(x, &e);
    long ml = std::lround(m * 32768.0f);
    if (ml == 32768) ml >>= 1, e++;
    e += power;
    *mantissa = e < -15 ? 0 : (int16_t)ml;
    *exponent = std::min(15, std::max(-15, e));
}

}  // namespace

int main() {
    // ---- Pool2DOp::execute: 13 x 11 x 24, batch 2, 3 x 3 stride 2, padding "same" -> 7 x 6
    const int C = 24, W = 13, H = 11, B = 2, F = 3, S = 2, OW = (W + S - 1) / S, OH = (H + S - 1) / S;
    std::vector<uint8_t> in((size_t)C * W * H * B), avg((size_t)C * OW * OH * B), mx(avg.size());
    for (uint8_t &v : in) v = (uint8_t)rnd();
    const int px = compute_padding(S, W, F, OW), py = compute_padding(S, H, F, OH);
    for (int kind = 0; kind < 2; kind++) {
        Buf ibuf(in.data(), {C, W, H, B}), obuf(kind ? mx.data() : avg.data(), {C, OW, OH, B});
        ibuf.dim[1].min = px, ibuf.dim[2].min = py;   // input_buf.translate(1, ...), (2, ...)
        const int r = kind ? hannk::max_pool_uint8(ibuf, S, S, F, F, 0, 255, obuf) : hannk::average_pool_uint8(ibuf, S, S, F, F, 0, 255, obuf);
        if (r) return fail("pool", r);
        if (int c = halide_copy_to_host(nullptr, obuf)) return fail("copy_to_host", c);
        halide_device_free(nullptr, ibuf), halide_device_free(nullptr, obuf);
    }
    for (int b = 0; b < B; b++)
        for (int y = 0; y < OH; y++)
            for (int x = 0; x < OW; x++)
                for (int c = 0; c < C; c++) {
                    int sum = 0, n = 0, m = 0;
                    for (int ry = 0; ry < F; ry++)
                        for (int rx = 0; rx < F; rx++) {
                            const int xx = x * S + rx - px, yy = y * S + ry - py;
                            if (xx < 0 || xx >= W || yy < 0 || yy >= H) continue;
                            const int v = in[((size_t)(b * H + yy) * W + xx) * C + c];
                            sum += v, n++, m = std::max(m, v);
                        }
                    const size_t o = ((size_t)(b * OH + y) * OW + x) * C + c;
                    if (mx[o] != m) return fail("max pool value", (int)o);
                    if (std::abs((int)avg[o] - (int)std::floor((double)sum / n + 0.5)) > 1) return fail("average pool value", (int)o);
                }

    // ---- SoftmaxOp::execute: 5 rows of 1001, input scale 1/16, beta 1, output scale 1/256, zero 0
    const int N = 1001, R = 5;
    std::vector<uint8_t> logits((size_t)N * R), prob(logits.size());
    for (uint8_t &v : logits) v = (uint8_t)(rnd() % 96);
    const float in_scale = 1.0f / 16, beta2 = 1.0f * std::log2(std::exp(1.0f));
    int16_t bm, om;
    int be, oe;
    int_float16(beta2 * in_scale, -6, &bm, &be);
    int_float16(1.0f / 256, 1, &om, &oe);   // (the extra factor of two of ops.cpp)
    if (be > 0 || oe > 0) return fail("softmax exponents");
    {
        Buf ibuf(logits.data(), {N, R}), obuf(prob.data(), {N, R});
        if (int r = hannk::softmax_uint8(ibuf, bm, (uint16_t)-be, 0, om, (uint16_t)-oe, obuf)) return fail("softmax", r);
        if (int c = halide_copy_to_host(nullptr, obuf)) return fail("copy_to_host", c);
        halide_device_free(nullptr, ibuf), halide_device_free(nullptr, obuf);
    }
    for (int r = 0; r < R; r++) {
        double sum = 0;
        int top = 0;
        for (int i = 0; i < N; i++) top = std::max(top, (int)logits[(size_t)r * N + i]);
        for (int i = 0; i < N; i++) sum += std::exp((logits[(size_t)r * N + i] - top) * (double)in_scale);
        for (int i = 0; i < N; i++) {
            const double want = std::min(255.0, std::floor(256 * std::exp((logits[(size_t)r * N + i] - top) * (double)in_scale) / sum + 0.5));
            if (std::abs(prob[(size_t)r * N + i] - want) > 1) return fail("softmax value", r * N + i);
        }
    }

    // ---- add_uint8: the residual add of two 56 x 56 x 24 tensors as one rank-2 call, ReLU-free
    const int X = 24, Y = 56 * 56;
    std::vector<uint8_t> a((size_t)X * Y), b2(a.size()), sum(a.size());
    for (size_t i = 0; i < a.size(); i++) a[i] = (uint8_t)rnd(), b2[i] = (uint8_t)rnd();
    const float s1 = 0.05f, s2 = 0.03f, so = 0.08f;
    const int z1 = 120, z2 = 7, zo = 100;
    const int m1 = (int)std::lround(s1 * (1 << 16) / (so * (1 << 6))), m2 = (int)std::lround(s2 * (1 << 16) / (so * (1 << 6)));
    {
        Buf abuf(a.data(), {X, Y}), bbuf(b2.data(), {X, Y}), obuf(sum.data(), {X, Y});
        if (int r = hannk::add_uint8_uint8(abuf, (uint8_t)z1, (int16_t)m1, bbuf, (uint8_t)z2, (int16_t)m2, (uint8_t)zo, 0, 255, obuf)) return fail("add", r);
        if (int c = halide_copy_to_host(nullptr, obuf)) return fail("copy_to_host", c);
        halide_device_free(nullptr, abuf), halide_device_free(nullptr, bbuf), halide_device_free(nullptr, obuf);
    }
    for (size_t i = 0; i < a.size(); i++) {
        const double want = std::min(255.0, std::max(0.0, std::floor(((double)s1 * (a[i] - z1) + (double)s2 * (b2[i] - z2)) / so + 0.5) + zo));
        if (std::abs(sum[i] - want) > 1) return fail("add value", (int)i);
    }
    // the argv form and the metadata of one of them
    const halide_filter_metadata_t *md = hannk::softmax_uint8_metadata();
    if (md->num_arguments != 7 || strcmp(md->arguments[1].name, "beta_multiplier") != 0 || md->arguments[1].type.bits != 16) return fail("metadata");
    printf("hannk nn consumer ok\n");
    return 0;
}
