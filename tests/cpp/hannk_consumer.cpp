// hannk_consumer.cpp — a C++ program that uses the op library the way apps/hannk's interpreter does, written fresh against the headers
// include/aot/halide/<name>.h: it learns the filter's tiling from an all-ones bounds query (what ConvOp::prepare does), the filter's
// element type from the metadata (ConvOp::filter_type), the depthwise channel alignment from a second query (DepthwiseConv2DOp::prepare),
// tiles one filter, runs one convolution through the C++-mangled symbols and holds the bytes to loops of its own.
// TEST INFRASTRUCTURE ONLY: tests/test_hannk_conv.py compiles it with the host compiler against libhlmi.so and runs it.
#include "halide/conv_u8_u8_i16.h"
#include "halide/conv_u8_u8_u8.h"
#include "halide/depthwise_conv_broadcast_uint8.h"
#include "halide/depthwise_conv_uint8.h"
#include "halide/tile_conv_filter_uint8.h"

#include "hlmi_runtime.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

// a dense host buffer of up to 6 dimensions; host == nullptr makes a bounds query
struct Buf {
    halide_buffer_t b;
    halide_dimension_t dim[6];
    Buf(halide_type_t type, void *host, std::initializer_list<int> extents) {
        memset(&b, 0, sizeof b);
        int stride = 1, d = 0;
        for (int e : extents) {
            dim[d].min = 0, dim[d].extent = e, dim[d].stride = stride, dim[d].flags = 0;
            stride *= e, d++;
        }
        b.host = (uint8_t *)host, b.type = type, b.dimensions = d, b.dim = dim;
        if (host) b.flags = 1;   // host dirty: the library uploads it
    }
    operator halide_buffer_t *() { return &b; }
};

// a halide_type_t is four bytes: code, bits and 16 bits of lanes (1 for every buffer and scalar)
halide_type_t type_of(uint8_t code, uint8_t bits) {
    const uint32_t v = (uint32_t)code | ((uint32_t)bits << 8) | (1u << 16);
    halide_type_t t;
    memcpy(&t, &v, 4);
    return t;
}
uint32_t type_word(const halide_type_t &t) {
    uint32_t v;
    memcpy(&v, &t, 4);
    return v;
}

int fail(const char *what, int code = 0) {
    printf("hannk consumer FAILED: %s (%d)\n", what, code);
    return 1;
}

uint32_t rnd() {
    static uint64_t s = 0x2545F4914F6CDD1Dull;
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
}

}  // namespace

int main() {
    const halide_type_t u8 = type_of(1, 8), i32 = type_of(0, 32);
    // ---- the filter's element type, from the metadata
    const halide_filter_metadata_t *md = hannk::conv_u8_u8_u8_metadata();
    if (md->num_arguments != 15 || strcmp(md->arguments[2].name, "filter") != 0) return fail("metadata");
    const halide_type_t filter_type = md->arguments[2].type;
    if (type_word(filter_type) != type_word(u8)) return fail("the filter type is not uint8 x 1");
    if (type_word(hannk::conv_u8_u8_i16_metadata()->arguments[14].type) != type_word(type_of(0, 16))) return fail("metadata of conv_u8_u8_i16");

    // ---- the tiling, from minimal unallocated buffers
    int vector_reduction, vector_tile, channel_alignment;
    {
        Buf in(u8, nullptr, {1, 1, 1, 1}), bias(i32, nullptr, {1}), filt(filter_type, nullptr, {1, 1, 1, 1, 1, 1}), out(u8, nullptr, {1, 1, 1, 1});
        if (int r = hannk::conv_u8_u8_u8(in, 0, filt, 0, bias, 1, 1, 1, 1, 0, 0, 0, 0, 0, out)) return fail("the conv query", r);
        vector_reduction = filt.dim[0].extent, vector_tile = filt.dim[1].extent;
    }
    {
        Buf in(u8, nullptr, {1, 1, 1, 1}), bias(i32, nullptr, {1}), filt(u8, nullptr, {1, 1, 1}), out(u8, nullptr, {1, 1, 1, 1});
        if (int r = hannk::depthwise_conv_uint8(in, 0, filt, 0, bias, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, out)) return fail("the depthwise query", r);
        channel_alignment = in.dim[0].extent;
    }
    printf("vector_reduction %d vector_tile %d channel_alignment %d\n", vector_reduction, vector_tile, channel_alignment);
    if (vector_reduction != HLMI_HANNK_VECTOR_REDUCTION || vector_tile != HLMI_HANNK_ACCUM_VECTOR_SIZE || channel_alignment != HLMI_HANNK_DEPTHWISE_VECTOR)
        return fail("the queries disagree with hannk_target.h");

    // ---- one layer: 6 -> 20 channels, 3 x 3, stride 1, 7 x 5 outputs, batch 2
    const int CI = 6, CO = 20, FW = 3, FH = 3, OW = 7, OH = 5, NB = 2, IW = OW + FW - 1, IH = OH + FH - 1;
    const int cq = (CI + vector_reduction - 1) / vector_reduction, co_tiles = (CO + vector_tile - 1) / vector_tile, CP = cq * vector_reduction;
    const uint8_t in_zero = 121, filt_zero = 133, out_zero = 17, out_min = 4, out_max = 251;
    const int32_t multiplier = 1403527424, shift = 7;
    std::vector<uint8_t> filter((size_t)CI * FW * FH * CO), input((size_t)CP * IW * IH * NB, in_zero), output((size_t)CO * OW * OH * NB, 0);
    std::vector<int32_t> bias(CO);
    for (auto &v : filter) v = (uint8_t)rnd();
    for (auto &v : bias) v = (int32_t)(rnd() % 4096) - 2048;
    for (int p = 0; p < IW * IH * NB; p++)
        for (int c = 0; c < CI; c++) input[(size_t)p * CP + c] = (uint8_t)rnd();   // channels CI .. CP stay at the zero point
    // the tiled filter: 64-byte aligned, like the interpreter's allocation
    const size_t tiled_bytes = (size_t)vector_reduction * vector_tile * cq * co_tiles * FW * FH;
    uint8_t *tiled = (uint8_t *)aligned_alloc(64, (tiled_bytes + 63) / 64 * 64);
    Buf fbuf(u8, filter.data(), {CI, FW, FH, CO}), tbuf(filter_type, tiled, {vector_reduction, vector_tile, cq, co_tiles, FW, FH});
    tbuf.b.flags = 0;
    if (int r = hannk::tile_conv_filter_uint8(fbuf, filt_zero, filt_zero, tbuf)) return fail("tile_conv_filter_uint8", r);
    Buf ibuf(u8, input.data(), {CP, IW, IH, NB}), bbuf(i32, bias.data(), {CO}), obuf(u8, output.data(), {CO, OW, OH, NB});
    obuf.b.flags = 0;
    if (int r = hannk::conv_u8_u8_u8(ibuf, in_zero, tbuf, filt_zero, bbuf, 1, 1, 1, 1, multiplier, shift, out_zero, out_min, out_max, obuf))
        return fail("conv_u8_u8_u8", r);
    if (int r = halide_copy_to_host(nullptr, obuf)) return fail("copy_to_host", r);

    // ---- the same layer with plain loops over the UNTILED filter
    int bad = 0;
    for (int b = 0; b < NB; b++)
        for (int y = 0; y < OH; y++)
            for (int x = 0; x < OW; x++)
                for (int c = 0; c < CO; c++) {
                    int64_t acc = bias[c];
                    for (int ry = 0; ry < FH; ry++)
                        for (int rx = 0; rx < FW; rx++)
                            for (int k = 0; k < CI; k++) {
                                const int a = input[(((size_t)b * IH + y + ry) * IW + x + rx) * CP + k];
                                const int w = filter[(((size_t)c * FH + ry) * FW + rx) * CI + k];
                                acc += (a - in_zero) * (w - filt_zero);
                            }
                    int64_t v = (acc * multiplier + (1ll << 30)) >> 31;
                    v = (v >> shift) + ((v >> (shift - 1)) & 1);
                    v = std::min<int64_t>(std::max<int64_t>(v, -32768), 32767) + out_zero;
                    v = std::min<int64_t>(std::max<int64_t>(v, 0), 255);
                    v = std::max<int64_t>(std::min<int64_t>(v, out_max), out_min);
                    bad += output[(((size_t)b * OH + y) * OW + x) * CO + c] != (uint8_t)v;
                }
    halide_device_free(nullptr, fbuf), halide_device_free(nullptr, tbuf), halide_device_free(nullptr, ibuf), halide_device_free(nullptr, bbuf),
        halide_device_free(nullptr, obuf);
    free(tiled);
    if (bad) return fail("outputs differ from the plain loops", bad);
    printf("hannk consumer ok: %d outputs\n", CO * OW * OH * NB);
    return 0;
}
