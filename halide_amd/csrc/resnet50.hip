// resnet50.hip — gfx950 implementation of the reference's resnet_50 AOT pipeline: the f32 ResNet-50 forward pass, 3 x 224 x 224 -> 1000.
//
// Algorithm: apps/resnet_50/Resnet50Generator.cpp:117-218 (the layer list) and :236-379 (the layers); boundary: `int resnet50(269 x
// halide_buffer_t *)` in the generator's declaration order (:31-66).  The contract is stated in include/hlmi_pipelines.h and DESIGN.md
// section 5.11; in short, with mad(a, b, c) = dev::mad (fused in the default build, multiply then add with HLMI_CANON_FMA=0):
//   conv       one chain per output from +0, k = (ky * KW + kx) * CI + ci strictly upward, acc = mad(w(co, kx, ky, ci), padded(ci, s i + kx - p,
//              s j + ky - p), acc); a tap outside the image is a step with the value +0, never a skipped step; no step is added to an odd K
//   norm+scale t = (v - mu(c)) / sqrt(sig(c) + 1e-5f) (IEEE division, correctly rounded sqrt), then mad(t, gamma(c), beta(c))
//   relu       v > 0 ? v : 0 (conv_layer.hip's: a NaN becomes +0);  residual: shortcut + scaled, a plain add, then relu
//   max pool   from -inf (the float type's minimum), r.x fastest: acc = v > acc ? v : acc, the +0 exterior taking part
//   avg pool   from +0, acc = mad(n, v, acc), n = 1.0f / (float)(w h), r.x fastest;   fc: from bias(c), acc = mad(w(c, k), pool(k), acc), k upward
//   softmax    e(c) = halide_exp(fc(c)); S = plain adds from +0 over c upward; out(c) = e(c) / S; no maximum is subtracted
//
// Plan and stages: rn50_plan() turns the fixed layer list into a launch list (57 launches: 53 convolutions, the two pools, fc and
// softmax) with the kernel variant, the geometry and the workspace slot of each; rn50_run() enqueues it in order on the call's stream.
// There is no graph and no second stream.  Activations live in the stream's scratch arena: five slots of the largest activation
// (64 x 112 x 112 = 256 x 56 x 56 floats, 3.2 MB) used in rotation, then the pooled vector, the logits and their exponentials.
//
// Convolution kernels (conv_plan() is the one place that chooses):
//   resnet50_conv_mfma     implicit GEMM on `v_mfma_f32_32x32x2_f32`, a k-ordered chain of fused steps (f32_chain_gemm.h), 4 waves on a tile of
//                          64 co x 64 output pixels.  MFMA operand "B"[k][j] is w(co = j, k): row k of the weights is co-contiguous at
//                          an offset computed from (ky, kx, ci), copied straight.  Operand "A"[i][k] is the activation of pixel i at
//                          tap k: ci-contiguous in memory, +0 where the tap is outside the image, turned k-major on the way into LDS.
//                          k is fed upward in chunks of KC; a short last chunk runs its pairs as MFMAs and an odd last step as a VALU
//                          fmaf on the accumulator registers through the C/D map: no padded k step exists.  The epilogue (normalise,
//                          scale, residual, ReLU) runs on the accumulator registers.  K is never split: the chain is the contract.
//                          A one-wave 32 x 32 tile of the same template, tried for the layers with few 64 x 64 tiles (the last stage has
//                          49 pixels), was slower on every layer class of the network (profiles/NOTES.md) and is not launched.
//   resnet50_conv_general  one thread per output running the chain as written: hlmi_resnet50_general, general_only of the layer hook,
//                          the whole HLMI_CANON_FMA=0 build (an MFMA step is fused by construction), and in the default build the
//                          layers with K <= SHORT_K and CO <= TILE (br2a of the first block, 64 -> 64 at 56 x 56): two chunks at most
//                          leave the tile loop nothing to overlap, and there the plain chain measured faster
// The other kernels are one thread per output: resnet50_maxpool, resnet50_avgpool, resnet50_fc (lanes along c, so the weight loads
// coalesce) and resnet50_softmax (one workgroup per image; the 1000-step sum is one serial chain by contract).
//
// Batches: resnet50_batch is a library extension (the reference's generator has no batch dimension): input [3, 224, 224, N] ->
// final_output [1000, N], column n bit for bit what resnet50 writes for image n.  It is the same entry (rn50_entry), plan and kernels:
// every geometry carries an image count and image strides, and resnet50 is their N = 1 case.  Inside a run of the plan an activation is
// [c, x, y, n], n outermost and dense, so the output pixels of a layer are one flat index p = (n OH + j) OW + i, a tile may lie across
// images, and a layer's weights are staged once for N times the pixels.  THE HAZARD of that layout: images are adjacent, so a tap at
// y = -1 of image n is a real address, the last row of image n - 1; every kernel decides "outside" from the pixel's own (x, y), never
// from an address.  Any N runs as ceil(N / C) runs of the plan over at most C = BATCH_CHUNK images (HLMI_RN50_BATCH_CHUNK, 1 .. 64) on
// the call's stream under the one call lock, 57 launches each.  For a batch conv_plan() has a second tile instance,
//   resnet50_conv_mfma_wide  the same template at 64 co x 128 pixels on 8 waves: the weights of a chunk staged once for twice the pixels,
// and resnet50_fc carries the chains of FC_GROUP images per thread, so that the fc weights are read once per group of images.
#include "f32_chain_gemm.h"
#include "hlmi_internal.h"
#include "hlmi_device_math.h"

#include <vector>

using namespace hlmi;

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int KC = 32;            // k steps per staged chunk
constexpr int TILE = 64;          // co and pixel edge of the workgroup tile (4 waves of 32 x 32)
constexpr int SHORT_K = 64;       // a layer with no more k steps than this and a single column of tiles runs the general kernel
constexpr int SHORT_K_IMAGES = 8; // ... of fewer images than this: from 8 images on the tile loop measured 2.5 x (8) to 4.5 x (32) faster there
constexpr int WIDE = 128;         // pixel edge of the batch's second tile instance, 64 co x 128 pixels on 8 waves
constexpr int WIDE_MIN_TILES = 192;    // fewer 64 x WIDE tiles than this leave compute units idle that 64 x 64 tiles fill (conv_plan)
constexpr int WIDE_ROUND = 768;        // 64 x WIDE workgroups resident at once: 256 compute units x 3 (75 VGPRs: 6 waves per SIMD)
constexpr int CLASSES = 1000;
constexpr int NARGS = 269, NCONV = 53;
constexpr int SLOT = 64 * 112 * 112;   // floats in a workspace slot: the largest activation (conv1's output; 256 x 56 x 56 is as large)
constexpr int NSLOTS = 5;
constexpr int BATCH_CHUNK = 64;   // images per run of the plan in resnet50_batch (HLMI_RN50_BATCH_CHUNK overrides it)
constexpr int MAX_CHUNK = 64;

enum Mode { RAW = 0, SCALED = 1, SCALED_RELU = 2, RESIDUAL_RELU = 3 };

// One convolution: activations (c, x, y) and weights (co, kx, ky, ci), dimension 0 innermost with stride 1; the other strides in elements.
// NI images (resnet50: 1), image n of the input, output and residual isn, osn and rsn elements behind image 0.  The output pixels of
// the NI images are one flat index p = (n OH + j) OW + i; whether a tap is inside its image is decided from the pixel's own (x, y) and
// never from an address: images may lie back to back, and row -1 of image n is then a real address, the last row of image n - 1.
struct CGeom {
    const float *in, *w, *gamma, *beta, *mu, *sig, *res;
    float *out;
    int CI, W, H, CO, KW, KH, S, P, OW, OH, mode;
    int isx, isy, wkx, wky, wci, osx, osy, rsx, rsy;
    int NI, isn, osn, rsn;
};
struct PGeom {   // a pool: max (k x k, stride, pad) or, with avg, the mean over the whole w x h image; NI images as in CGeom
    const float *in;
    float *out;
    int C, W, H, K, S, P, OW, OH, isx, isy, osx, osy;
    int NI, isn, osn;
};
struct TGeom {   // fc and softmax
    const float *pool, *w, *bias;
    float *fc, *e, *out;
    int C, N, ws, omin, oext;   // C inputs, N classes, ws = stride of w's dimension 1; classes [omin, omin + oext) are stored
    int NI, ps, fs, os;         // NI images: pooled vectors ps apart, logits and exponentials fs apart, outputs os apart
};

struct Chan {
    float mu, sd, gamma, beta;
};
__device__ __forceinline__ Chan rn_chan(const CGeom &g, int co) {
    if (g.mode == RAW) return {0.0f, 1.0f, 1.0f, 0.0f};
    return {g.mu[co], sqrtf(g.sig[co] + 1e-5f), g.gamma[co], g.beta[co]};
}
// everything behind the chain of one output; roff: the offset of its residual
__device__ __forceinline__ float rn_finish(const CGeom &g, const Chan &c, float acc, int roff) {
    if (g.mode == RAW) return acc;
    float v = dev::mad((acc - c.mu) / c.sd, c.gamma, c.beta);
    if (g.mode == RESIDUAL_RELU) v = g.res[roff] + v;
    if (g.mode >= SCALED_RELU) v = v > 0.0f ? v : 0.0f;
    return v;
}

// Tile of 32 NCO co x 32 NPX pixels, one wave per 32 x 32.  Per chunk a table of its KC steps (weight row, activation offset, tap
// displacement) is built by KC threads, so that no other thread divides; the pixels' own table is built once.  The global loads of
// chunk c + 1 are in flight under the MFMAs of chunk c; LDS is single-buffered, two barriers per chunk.
template<int NCO, int NPX>
__global__ __launch_bounds__(64 * NCO * NPX) void rn_conv_mfma(CGeom g) {
    constexpr int NT = 64 * NCO * NPX, TC = 32 * NCO, TP = 32 * NPX;
    constexpr int WP = TC, AP = TP + 1;                     // LDS pitches: straight rows / conflict-free turned stores
    constexpr int WSTEP = NT / TC, WN = KC / WSTEP;         // weights: thread t holds rows t / TC + WSTEP r of column t % TC
    constexpr int ASTEP = NT / KC, AN = TP / ASTEP;         // activations: thread t holds pixels t / KC + ASTEP r of step t % KC
    static_assert(TP <= NT && KC <= NT && WN * WSTEP == KC && AN * ASTEP == TP, "staging covers the tile");
    __shared__ float sW[KC * WP];   // [k][co]
    __shared__ float sA[KC * AP];   // [k][pixel]
    __shared__ int sKw[2][KC], sKa[2][KC], sKx[2][KC], sKy[2][KC];
    __shared__ int sPa[TP], sPx[TP], sPy[TP], sPo[TP], sPr[TP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wc = wave % NCO, wp = wave / NCO;
    const int co0 = blockIdx.x * TC, p0 = blockIdx.y * TP, ipix = g.OW * g.OH, npix = g.NI * ipix, K = g.KH * g.KW * g.CI;
    const int nchunk = (K + KC - 1) / KC;

    if (tid < TP) {   // a pixel past the end (of the last image) repeats the last one: loaded, computed, never stored
        const int p = min(p0 + tid, npix - 1), n = g.NI == 1 ? 0 : p / ipix, q = p - n * ipix, j = q / g.OW, i = q - j * g.OW;   // (one image: no division)
        sPx[tid] = i * g.S, sPy[tid] = j * g.S;   // the pixel's own (x, y): what load() tests, whatever lies before and behind the image
        sPa[tid] = n * g.isn + i * g.S * g.isx + j * g.S * g.isy;
        sPo[tid] = n * g.osn + i * g.osx + j * g.osy;
        sPr[tid] = n * g.rsn + i * g.rsx + j * g.rsy;
    }
    auto table = [&](int c) {   // a step past K repeats the last one: loaded, never computed
        if (tid < KC) {
            const int k = min(c * KC + tid, K - 1), tap = k / g.CI, ci = k - tap * g.CI, ky = tap / g.KW, kx = tap - ky * g.KW, b = c & 1;
            sKw[b][tid] = kx * g.wkx + ky * g.wky + ci * g.wci;
            sKx[b][tid] = kx - g.P, sKy[b][tid] = ky - g.P;
            sKa[b][tid] = ci + (kx - g.P) * g.isx + (ky - g.P) * g.isy;
        }
    };
    float rw[WN], ra[AN];
    const int wcol = tid % TC, wrow = tid / TC, akk = tid % KC, apx = tid / KC;
    auto load = [&](int c) {
        const int b = c & 1;
        const float *wcolp = g.w + min(co0 + wcol, g.CO - 1);
#pragma unroll
        for (int r = 0; r < WN; r++) rw[r] = wcolp[sKw[b][wrow + WSTEP * r]];
        const int ao = sKa[b][akk], dx = sKx[b][akk], dy = sKy[b][akk];
#pragma unroll
        for (int r = 0; r < AN; r++) {
            const int px = apx + ASTEP * r, x = sPx[px] + dx, y = sPy[px] + dy;
            ra[r] = ((unsigned)x < (unsigned)g.W && (unsigned)y < (unsigned)g.H) ? g.in[sPa[px] + ao] : 0.0f;
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int r = 0; r < WN; r++) sW[(wrow + WSTEP * r) * WP + wcol] = rw[r];
#pragma unroll
        for (int r = 0; r < AN; r++) sA[akk * AP + apx + ASTEP * r] = ra[r];
    };

    floatx16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.0f;
    // one MFMA: k = 2 s (lanes 0 .. 31) then 2 s + 1 (lanes 32 .. 63), in that order inside the instruction
    const float *pa = sA + (lane >> 5) * AP + wp * 32 + (lane & 31);
    const float *pb = sW + (lane >> 5) * WP + wc * 32 + (lane & 31);
    auto compute = [&](int c) {
        const int kc = min(KC, K - c * KC);
        if (kc == KC) {
#pragma unroll
            for (int s = 0; s < KC / 2; s++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * s * AP], pb[2 * s * WP], acc, 0, 0, 0);
        } else {
#pragma unroll 1
            for (int s = 0; s < kc / 2; s++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * s * AP], pb[2 * s * WP], acc, 0, 0, 0);
            if (kc & 1) {
                // the last step of an odd K has no partner, and a zero-padded one would turn a chain that ends in -0 into +0: a VALU
                // fmaf on each accumulator register, operands picked through the C/D map (row = pixel, column = co)
                const float *ka = sA + (kc - 1) * AP + wp * 32 + 4 * (lane >> 5);
                const float wv = sW[(kc - 1) * WP + wc * 32 + (lane & 31)];
#pragma unroll
                for (int r = 0; r < 16; r++) acc[r] = __builtin_fmaf(wv, ka[chain::cd_row(r)], acc[r]);
            }
        }
    };

    table(0);
    __syncthreads();
    load(0);
    table(1);
    stage();
    __syncthreads();
#pragma unroll 1
    for (int c = 0; c < nchunk; c++) {
        if (c + 1 < nchunk) load(c + 1);
        compute(c);
        __syncthreads();
        if (c + 1 < nchunk) {
            stage();
            table(c + 2);
        }
        __syncthreads();
    }

    // ---- epilogue on the accumulator registers: C/D map row = chain::cd_row(reg) + 4 (lane >> 5) = pixel, col = lane & 31 = co
    const int co = co0 + wc * 32 + (lane & 31);
    if (co < g.CO) {
        const Chan ch = rn_chan(g, co);
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int px = wp * 32 + chain::cd_row(r) + 4 * (lane >> 5);
            if (p0 + px < npix) g.out[sPo[px] + co] = rn_finish(g, ch, acc[r], sPr[px] + co);
        }
    }
}

// The second implementation: one thread per output, the chain as written (co fastest across lanes: the weight loads coalesce and the
// activation loads are one address per pixel).
__global__ __launch_bounds__(256) void rn_conv_general(CGeom g) {
    const long idx = blockIdx.x * 256L + threadIdx.x;
    if (idx >= (long)g.CO * g.OW * g.OH * g.NI) return;
    const int co = (int)(idx % g.CO), p = (int)(idx / g.CO), n = g.NI == 1 ? 0 : p / (g.OW * g.OH), q = p - n * g.OW * g.OH, j = q / g.OW, i = q - j * g.OW;
    float acc = 0.0f;
    for (int ky = 0; ky < g.KH; ky++)
        for (int kx = 0; kx < g.KW; kx++) {
            const int x = g.S * i + kx - g.P, y = g.S * j + ky - g.P;
            const bool inside = (unsigned)x < (unsigned)g.W && (unsigned)y < (unsigned)g.H;
            const float *ip = g.in + (inside ? n * g.isn + x * g.isx + y * g.isy : 0);
            const float *wp = g.w + kx * g.wkx + ky * g.wky + co;
            for (int ci = 0; ci < g.CI; ci++) acc = dev::mad(wp[(long)ci * g.wci], inside ? ip[ci] : 0.0f, acc);
        }
    g.out[n * g.osn + i * g.osx + j * g.osy + co] = rn_finish(g, rn_chan(g, co), acc, n * g.rsn + i * g.rsx + j * g.rsy + co);
}

__global__ __launch_bounds__(256) void rn_maxpool(PGeom g) {
    const long idx = blockIdx.x * 256L + threadIdx.x;
    if (idx >= (long)g.C * g.OW * g.OH * g.NI) return;
    const int c = (int)(idx % g.C), p = (int)(idx / g.C), n = g.NI == 1 ? 0 : p / (g.OW * g.OH), q = p - n * g.OW * g.OH, j = q / g.OW, i = q - j * g.OW;
    float acc = -__builtin_inff();
    for (int ry = 0; ry < g.K; ry++)
        for (int rx = 0; rx < g.K; rx++) {
            const int x = g.S * i + rx - g.P, y = g.S * j + ry - g.P;
            const float v = ((unsigned)x < (unsigned)g.W && (unsigned)y < (unsigned)g.H) ? g.in[n * g.isn + x * g.isx + y * g.isy + c] : 0.0f;
            acc = v > acc ? v : acc;
        }
    g.out[n * g.osn + i * g.osx + j * g.osy + c] = acc;
}

__global__ __launch_bounds__(256) void rn_avgpool(PGeom g) {   // one thread per (c, image)
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= g.C * g.NI) return;
    const int c = idx % g.C, im = idx / g.C;
    const float *in = g.in + im * g.isn + c;
    const float n = 1.0f / (float)(g.W * g.H);
    float acc = 0.0f;
    for (int y = 0; y < g.H; y++)
        for (int x = 0; x < g.W; x++) acc = dev::mad(n, in[x * g.isx + y * g.isy], acc);
    g.out[im * g.osn + c] = acc;
}

// Lanes along classes; a thread carries the chains of the G images of group blockIdx.y, so that one weight load serves all of them:
// the weights are read once per group, not once per image.  Each chain is bias(c), then mad(w(c, k), pool(k), acc), k upward.
constexpr int FC_GROUP = 8;
template<int G>
__global__ __launch_bounds__(64) void rn_fc(TGeom g) {
    const int c = blockIdx.x * 64 + threadIdx.x, n0 = blockIdx.y * G, cnt = min(G, g.NI - n0);
    if (c >= g.N) return;
    float acc[G];
#pragma unroll
    for (int m = 0; m < G; m++) acc[m] = g.bias[c];
    const float *w = g.w + c, *pool = g.pool + (long)n0 * g.ps;
#pragma unroll 8
    for (int k = 0; k < g.C; k++) {
        const float wv = w[(long)k * g.ws];
#pragma unroll
        for (int m = 0; m < G; m++)   // an image past the end repeats the group's first: computed, never stored
            acc[m] = dev::mad(wv, pool[(m < cnt ? m * g.ps : 0) + k], acc[m]);
    }
#pragma unroll
    for (int m = 0; m < G; m++)
        if (m < cnt) g.fc[(long)(n0 + m) * g.fs + c] = acc[m];
}

__global__ __launch_bounds__(1024) void rn_softmax(TGeom g) {   // one workgroup per image
    __shared__ float S;
    const int im = blockIdx.x;
    float *e = g.e + (long)im * g.fs, *out = g.out + (long)im * g.os;
    const float *fc = g.fc + (long)im * g.fs;
    for (int c = threadIdx.x; c < g.N; c += 1024) e[c] = dev::halide_exp(fc[c]);
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.0f;
        for (int c = 0; c < g.N; c++) s = s + e[c];
        S = s;
    }
    __syncthreads();
    for (int c = g.omin + (int)threadIdx.x; c < g.omin + g.oext; c += 1024) out[c - g.omin] = e[c] / S;
}

// ---------------------------------------------------------------------------------------------------------------- plan
enum RnLaunch { RN_MFMA, RN_GENERAL, RN_MAXPOOL, RN_AVGPOOL, RN_FC, RN_SOFTMAX, RN_MFMA_WIDE, RN_LAUNCHES };
const char *const rn_names[RN_LAUNCHES] = {"resnet50_conv_mfma", "resnet50_conv_general", "resnet50_maxpool", "resnet50_avgpool", "resnet50_fc",
                                           "resnet50_softmax", "resnet50_conv_mfma_wide"};
// the (co, pixel) edges of a launch's workgroup tile; the general kernel and the others have none
inline int tile_co(RnLaunch l) { return l == RN_MFMA || l == RN_MFMA_WIDE ? TILE : 0; }
inline int tile_px(RnLaunch l) { return l == RN_MFMA ? TILE : l == RN_MFMA_WIDE ? WIDE : 0; }

// THE predicate.  The general kernel takes the whole HLMI_CANON_FMA=0 build, every call that asks for it by name, and the layers where
// it measured faster than the tile loop: at most SHORT_K steps and at most TILE output channels, over fewer than SHORT_K_IMAGES images
// (measured at one image; at 8 and 32 images the tile loop is far ahead, between them nothing was measured and the one-image rule
// stands).  The MFMA kernel takes the rest on
// its 64 x 64 tile, and a batch on the 64 x WIDE tile where that measured faster in an alternating A/B per layer class (DESIGN.md
// 5.11, "Batches"): with T = the layer's count of wide tiles, from WIDE_MIN_TILES on (fewer leave compute units idle: 8 .. 17 %
// slower), except between one and two rounds of residency, WIDE_ROUND < T < 2 WIDE_ROUND, where the two tiles measured within 4 % of
// each other, the wide one behind on average.  One image keeps the 64 x 64 tile: resnet50's plan is what it was.
RnLaunch conv_plan(const CGeom &g, bool general_only) {
    if (general_only || !dev::CANON_FMA) return RN_GENERAL;
    if (g.KH * g.KW * g.CI <= SHORT_K && g.CO <= TILE && g.NI < SHORT_K_IMAGES) return RN_GENERAL;
    const long T = (long)((g.CO + TILE - 1) / TILE) * (((long)g.NI * g.OW * g.OH + WIDE - 1) / WIDE);
    return g.NI > 1 && T >= WIDE_MIN_TILES && !(T > WIDE_ROUND && T < 2 * WIDE_ROUND) ? RN_MFMA_WIDE : RN_MFMA;
}

struct Step {
    RnLaunch launch;
    CGeom c;
    PGeom p;
    TGeom t;
};

dim3 rn_grid(const Step &s) {
    auto blocks = [](long n, int per) { return dim3((unsigned)((n + per - 1) / per)); };
    switch (s.launch) {
    case RN_MFMA:
    case RN_MFMA_WIDE:
        return dim3((unsigned)((s.c.CO + TILE - 1) / TILE), (unsigned)(((long)s.c.NI * s.c.OW * s.c.OH + tile_px(s.launch) - 1) / tile_px(s.launch)));
    case RN_GENERAL: return blocks((long)s.c.CO * s.c.OW * s.c.OH * s.c.NI, 256);
    case RN_MAXPOOL: return blocks((long)s.p.C * s.p.OW * s.p.OH * s.p.NI, 256);
    case RN_AVGPOOL: return blocks((long)s.p.C * s.p.NI, 256);
    case RN_FC: return dim3((unsigned)((s.t.N + 63) / 64), (unsigned)((s.t.NI + FC_GROUP - 1) / FC_GROUP));
    case RN_SOFTMAX: return dim3((unsigned)s.t.NI);
    default: return dim3(0);
    }
}

int rn_launch(void *uc, hipStream_t st, const Step &s) {
    const char *name = rn_names[s.launch];
    const dim3 grid = rn_grid(s);
    switch (s.launch) {
    case RN_MFMA: HLMI_LAUNCH(uc, name, st, (rn_conv_mfma<TILE / 32, TILE / 32>), grid, dim3(TILE * TILE / 16), 0, s.c); return 0;
    case RN_MFMA_WIDE: HLMI_LAUNCH(uc, name, st, (rn_conv_mfma<TILE / 32, WIDE / 32>), grid, dim3(TILE * WIDE / 16), 0, s.c); return 0;
    case RN_GENERAL: HLMI_LAUNCH(uc, name, st, rn_conv_general, grid, dim3(256), 0, s.c); return 0;
    case RN_MAXPOOL: HLMI_LAUNCH(uc, name, st, rn_maxpool, grid, dim3(256), 0, s.p); return 0;
    case RN_AVGPOOL: HLMI_LAUNCH(uc, name, st, rn_avgpool, grid, dim3(256), 0, s.p); return 0;
    case RN_FC:   // one image: the one-chain instance resnet50 has always run
        if (s.t.NI == 1) HLMI_LAUNCH(uc, name, st, rn_fc<1>, dim3(grid.x), dim3(64), 0, s.t);
        else HLMI_LAUNCH(uc, name, st, rn_fc<FC_GROUP>, grid, dim3(64), 0, s.t);
        return 0;
    case RN_SOFTMAX: HLMI_LAUNCH(uc, name, st, rn_softmax, grid, dim3(1024), 0, s.t); return 0;
    default: return 0;
    }
}

int rn50_run(void *uc, hipStream_t st, const std::vector<Step> &plan) {
    for (const Step &s : plan)
        if (int r = rn_launch(uc, st, s)) return r;
    return 0;
}

// compute_shape (:245-251): truncating
int out_extent(int in, int k, int stride, int pad) { return (pad * 2 + in - k + 1 + stride - 1) / stride; }

// ---- the fixed network.  Convolution c of the 53 is argument 1 + 53 G + c of group G (gamma, beta, mu, sig, weights): conv1, br1_0 .. 3,
// br2a_0 .. 15, br2b_0 .. 15, br2c_0 .. 15.
struct Layer {
    int ci, co, k, stride, pad, w, h;   // w, h: the input's
};
constexpr int BR1 = 1, BR2A = 5, BR2B = 21, BR2C = 37;
struct Net {
    Layer conv[NCONV];
    Net() {
        conv[0] = {3, 64, 7, 2, 3, 224, 224};
        const int mid[4] = {64, 128, 256, 512}, blocks[4] = {3, 4, 6, 3}, strides[4] = {1, 2, 2, 2};
        int cin = 64, size = 56, b = 0;   // behind pool1
        for (int s = 0; s < 4; s++)
            for (int i = 0; i < blocks[s]; i++, b++) {
                const int st = i == 0 ? strides[s] : 1, osize = out_extent(size, 1, st, 0);
                if (i == 0) conv[BR1 + s] = {cin, 4 * mid[s], 1, st, 0, size, size};
                conv[BR2A + b] = {cin, mid[s], 1, 1, 0, size, size};
                conv[BR2B + b] = {mid[s], mid[s], 3, st, 1, size, size};
                conv[BR2C + b] = {mid[s], 4 * mid[s], 1, 1, 0, osize, osize};
                cin = 4 * mid[s], size = osize;
            }
    }
};
const Net net;
inline int br1_of(int block) { return block == 0 ? 0 : block == 3 ? 1 : block == 7 ? 2 : block == 13 ? 3 : -1; }

CGeom conv_geom(const Layer &l, int nimg, const float *in, const float *const *par, const float *res, float *out, int mode) {
    CGeom g = {};
    g.in = in, g.gamma = par[0], g.beta = par[1], g.mu = par[2], g.sig = par[3], g.w = par[4], g.res = res, g.out = out;
    g.CI = l.ci, g.W = l.w, g.H = l.h, g.CO = l.co, g.KW = g.KH = l.k, g.S = l.stride, g.P = l.pad, g.mode = mode;
    g.OW = out_extent(l.w, l.k, l.stride, l.pad), g.OH = out_extent(l.h, l.k, l.stride, l.pad);
    g.isx = l.ci, g.isy = l.ci * l.w;
    g.osx = g.rsx = l.co, g.osy = g.rsy = l.co * g.OW;
    g.NI = nimg, g.isn = l.ci * l.w * l.h, g.osn = g.rsn = l.co * g.OW * g.OH;   // the workspace: [c, x, y, n], n outermost and dense
    return g;
}

// floats of workspace a run of the plan over `nimg` images needs: the slots, the pooled vectors, the logits and their exponentials
size_t rn50_workspace(int nimg) { return ((size_t)NSLOTS * SLOT + 2048 + 2 * CLASSES) * (size_t)nimg; }

// The launch list of one run over `nimg` images (resnet50: one; resnet50_batch: a chunk).  p[i]: argument i with its device address at
// its element (0, 0, ...); in0: the first image, `isn` floats between images; out0: the first column of the output, `osn` floats between
// columns; ws: rn50_workspace(nimg) floats.
std::vector<Step> rn50_plan(halide_buffer_t *const *p, float *ws, bool general_only, int nimg, const float *in0, int isn, float *out0, int osn) {
    std::vector<Step> plan;
    float *slot[NSLOTS];
    for (int i = 0; i < NSLOTS; i++) slot[i] = ws + (size_t)i * SLOT * nimg;
    float *pool = ws + (size_t)NSLOTS * SLOT * nimg, *fc = pool + (size_t)2048 * nimg, *e = fc + (size_t)CLASSES * nimg;
    auto conv = [&](int c, const float *in, const float *res, float *out, int mode) {
        const float *par[5];
        for (int G = 0; G < 5; G++) par[G] = dev_ptr<float>(p[1 + NCONV * G + c]);
        Step s = {};
        s.c = conv_geom(net.conv[c], nimg, in, par, res, out, mode);
        if (c == 0) s.c.isx = p[0]->dim[1].stride, s.c.isy = p[0]->dim[2].stride, s.c.isn = isn;   // the caller's own strides feed conv1
        const halide_buffer_t *w = p[1 + NCONV * 4 + c];
        s.c.wkx = w->dim[1].stride, s.c.wky = w->dim[2].stride, s.c.wci = w->dim[3].stride;
        s.launch = conv_plan(s.c, general_only);
        plan.push_back(s);
    };
    // the stem: conv1 + norm + scale + relu -> slot 1, pool1 -> slot 0
    conv(0, in0, nullptr, slot[1], SCALED_RELU);
    {
        Step s = {};
        s.launch = RN_MAXPOOL;
        s.p = {slot[1], slot[0], 64, 112, 112, 3, 2, 1, 56, 56, 64, 64 * 112, 64, 64 * 56, nimg, 64 * 112 * 112, 64 * 56 * 56};
        plan.push_back(s);
    }
    // 16 blocks: x = the block's input, y = its output, slots 2 .. 4 = br1, br2a, br2b
    float *x = slot[0], *y = slot[1];
    for (int b = 0; b < 16; b++) {
        const float *shortcut = x;
        if (br1_of(b) >= 0) conv(BR1 + br1_of(b), x, nullptr, slot[2], SCALED), shortcut = slot[2];
        conv(BR2A + b, x, nullptr, slot[3], SCALED_RELU);
        conv(BR2B + b, slot[3], nullptr, slot[4], SCALED_RELU);
        conv(BR2C + b, slot[4], shortcut, y, RESIDUAL_RELU);
        std::swap(x, y);
    }
    Step s = {};
    s.launch = RN_AVGPOOL;
    s.p = {x, pool, 2048, 7, 7, 7, 1, 0, 1, 1, 2048, 2048 * 7, 2048, 2048, nimg, 2048 * 49, 2048};
    plan.push_back(s);
    const halide_buffer_t *fw = p[NARGS - 3], *out = p[NARGS - 1];
    s = {};
    s.t = {pool, dev_ptr<float>(fw), dev_ptr<float>(p[NARGS - 2]), fc, e, out0, 2048, CLASSES, fw->dim[1].stride, out->dim[0].min, out->dim[0].extent,
           nimg, 2048, CLASSES, osn};
    s.launch = RN_FC;
    plan.push_back(s);
    s.launch = RN_SOFTMAX;
    plan.push_back(s);
    return plan;
}

// ---------------------------------------------------------------------------------------------------------------- the argument table
// the names come from the list the declaration itself is written with (HLMI_RN50_INPUTS of hlmi_pipelines.h)
#define RN50_NAME(n) #n,
#define RN50_VALUE(n) n,

const char *const rn_arg_names[NARGS] = {HLMI_RN50_INPUTS(RN50_NAME) "final_output"};
// resnet50_batch differs in two buffers: input has the image dimension behind (c, x, y), final_output behind the classes
inline int rn_arg_dims(int i, bool batch) {
    return i == 0 ? 3 + batch : i <= 4 * NCONV ? 1 : i <= 5 * NCONV ? 4 : i == NARGS - 3 ? 2 : i == NARGS - 1 ? 1 + batch : 1;
}

std::vector<Arg> rn_arg_lines(bool batch) {
    std::vector<Arg> v;
    for (int i = 0; i < NARGS; i++)
        v.push_back(i == NARGS - 1 ? out_buf(rn_arg_names[i], T_F32, rn_arg_dims(i, batch)) : in_buf(rn_arg_names[i], T_F32, rn_arg_dims(i, batch)));
    return v;
}
const std::vector<Arg> rn_lines = rn_arg_lines(false), rn_batch_lines = rn_arg_lines(true);
const ArgTable rn_table("resnet50", rn_lines.data(), rn_lines.size());
const ArgTable rn_batch_table("resnet50_batch", rn_batch_lines.data(), rn_batch_lines.size());

// the fixed box of input i (every min is 0): extents, rn_arg_dims(i) of them
void rn_box(int i, int ext[4]) {
    if (i == 0) ext[0] = 3, ext[1] = 224, ext[2] = 224, ext[3] = 1;   // (the batch's fourth: the entry sets its range)
    else if (i <= 4 * NCONV) ext[0] = net.conv[(i - 1) % NCONV].co;
    else if (i <= 5 * NCONV) {
        const Layer &l = net.conv[i - 1 - 4 * NCONV];
        ext[0] = l.co, ext[1] = l.k, ext[2] = l.k, ext[3] = l.ci;
    } else if (i == NARGS - 3) ext[0] = CLASSES, ext[1] = 2048;
    else ext[0] = CLASSES;
}

// every element of the buffer is within 2^31 - 1 elements of its first: the kernels index with ints.  With `images_dim` >= 0 that
// dimension counts `images` elements: resnet50_batch addresses one chunk of images at a time, from a pointer of the chunk's own.
bool span_fits(const halide_buffer_t *b, int images_dim = -1, int images = 0) {
    int64_t span = 0;
    for (int d = 0; d < b->dimensions; d++)
        span += (int64_t)std::max((d == images_dim ? std::min(images, b->dim[d].extent) : b->dim[d].extent) - 1, 0) * std::abs((int64_t)b->dim[d].stride);
    return span < INT32_MAX;
}

// HLMI_RN50_BATCH_CHUNK, read once per call: the images per run of the plan, 1 .. MAX_CHUNK, BATCH_CHUNK where it is unset
int batch_chunk(void *uc, int *chunk) {
    *chunk = env_int("HLMI_RN50_BATCH_CHUNK").value_or(BATCH_CHUNK);
    if (*chunk < 1 || *chunk > MAX_CHUNK)
        return report(uc, halide_error_code_constraint_violated, "Constraint violated: HLMI_RN50_BATCH_CHUNK (%d) must be 1 .. %d", *chunk, MAX_CHUNK);
    return 0;
}

// resnet50 and, with `batch`, resnet50_batch: one protocol.  The batch adds one range, the images [bmin, bmin + bext): dimension 1 of
// final_output where that is known, else dimension 3 of input where that is known, else [0, 1).
int rn50_entry(halide_buffer_t *const *p, bool general_only, bool batch) {
    void *uc = nullptr;
    const ArgTable &table = batch ? rn_batch_table : rn_table;
    BufArg args[NARGS];
    for (int i = 0; i < NARGS; i++) {
        const Arg &a = table.spec[i];
        args[i] = {a.name, p[i], a.type, a.dims, i == NARGS - 1};
    }
    int r = check_not_null(uc, args, NARGS);
    if (r) return r;
    if ((r = check_type_and_dims(uc, args, NARGS))) return r;
    // the output may be any box; a class outside [0, 1000) is a read of fc1000_bias and fc1000_weights outside theirs, as in the reference
    halide_buffer_t *out = p[NARGS - 1];
    const bool out_known = buffer_known(out), in_known = batch && buffer_known(p[0]);
    const int omin = out_known ? out->dim[0].min : 0, oext = out_known ? out->dim[0].extent : CLASSES;
    const int cmin = oext > 0 ? std::min(0, omin) : 0, cmax = oext > 0 ? std::max(CLASSES, omin + oext) : CLASSES;
    const int bmin = !batch ? 0 : out_known ? out->dim[1].min : in_known ? p[0]->dim[3].min : 0;
    const int bext = !batch ? 1 : out_known ? out->dim[1].extent : in_known ? p[0]->dim[3].extent : 1;
    if (any_bounds_query(args, NARGS)) {
        for (int i = 0; i < NARGS - 1; i++) {
            int ext[4];
            rn_box(i, ext);
            int mins[4] = {0, 0, 0, 0};
            if (i >= NARGS - 3) mins[0] = cmin, ext[0] = cmax - cmin;
            if (i == 0) mins[3] = bmin, ext[3] = bext;
            answer_query(p[i], mins, ext);
        }
        const int om[2] = {0, bmin}, oe[2] = {CLASSES, bext};
        if (!out_known) answer_query(out, om, oe);
        return 0;
    }
    if ((r = check_shapes(uc, args, NARGS))) return r;
    for (int i = 0; i < NARGS - 1; i++) {
        int ext[4];
        rn_box(i, ext);
        for (int d = 0; d < args[i].dims; d++) {
            const bool classes = i >= NARGS - 3 && d == 0, images = i == 0 && d == 3;
            check_covers(uc, args[i], d, classes ? cmin : images ? bmin : 0, classes ? cmax - cmin : images ? bext : ext[d]);
        }
    }
    if ((r = checks_done(uc))) return r;
    int chunk = 1;
    if (batch && (r = batch_chunk(uc, &chunk))) return r;
    for (int i = 0; i < NARGS; i++)
        if (!span_fits(p[i], !batch ? -1 : i == 0 ? 3 : i == NARGS - 1 ? 1 : -1, chunk))
            return report(uc, halide_error_code_buffer_extents_too_large, "%s spans more than 2^31 - 1 elements", args[i].name);
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, NARGS))) return r;
    void *ws = nullptr;
    if ((r = get_workspace(uc, ctx, rn50_workspace(std::max(1, std::min(chunk, bext))) * sizeof(float), &ws))) return r;
    // the kernels address an input from its element (0, 0, ...): fold the mins of a larger buffer into the pointers
    halide_buffer_t view[NARGS];
    halide_buffer_t *vp[NARGS];
    for (int i = 0; i < NARGS; i++) {
        view[i] = *p[i], vp[i] = &view[i];
        if (i == NARGS - 1) continue;
        int64_t off = 0;
        for (int d = 0; d < p[i]->dimensions; d++) off -= (int64_t)p[i]->dim[d].min * p[i]->dim[d].stride;
        view[i].device = p[i]->device + (uint64_t)(off * (int64_t)sizeof(float));
    }
    // ceil(bext / chunk) runs of the plan, in order on the call's stream under the one call lock: a run reuses the workspace of the one before
    const int isn = batch ? p[0]->dim[3].stride : 0, osn = batch ? out->dim[1].stride : 0;
    for (int first = 0; first < bext; first += chunk) {
        const float *in0 = dev_ptr<float>(vp[0]) + (int64_t)(bmin + first) * isn;
        float *out0 = dev_ptr<float>(out) + (int64_t)first * osn;
        if ((r = rn50_run(uc, ctx.stream, rn50_plan(vp, (float *)ws, general_only, std::min(chunk, bext - first), in0, isn, out0, osn)))) return r;
    }
    mark_output_written(out);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- the hooks' shared checks
// null, type and dimensions, then one buffer's extents against what the others imply (-8), then the device
struct Want {
    const char *name;
    halide_buffer_t *buf;
    int dims;
    int ext[4];
};
int hook_prologue(void *uc, const Want *w, int n, int n_out, BufArg *args, DeviceCtx *ctx) {
    for (int i = 0; i < n; i++) args[i] = {w[i].name, w[i].buf, T_F32, w[i].dims, i >= n - n_out};
    int r = check_not_null(uc, args, n);
    if (r) return r;
    if ((r = check_type_and_dims(uc, args, n))) return r;
    if (any_bounds_query(args, n)) return report(uc, halide_error_code_constraint_violated, "Constraint violated: the resnet50 hooks answer no bounds query");
    if ((r = check_shapes(uc, args, n))) return r;
    char what[48], expect[16];
    for (int i = 0; i < n; i++)
        for (int d = 0; d < w[i].dims; d++) {
            snprintf(what, sizeof what, "%s.min.%d", w[i].name, d);
            check_equal(uc, what, w[i].buf->dim[d].min, "0", 0);
            snprintf(what, sizeof what, "%s.extent.%d", w[i].name, d);
            snprintf(expect, sizeof expect, "%d", w[i].ext[d]);
            check_equal(uc, what, w[i].buf->dim[d].extent, expect, w[i].ext[d]);
        }
    if ((r = checks_done(uc))) return r;
    for (int i = 0; i < n; i++)
        if (!span_fits(w[i].buf)) return report(uc, halide_error_code_buffer_extents_too_large, "%s spans more than 2^31 - 1 elements", w[i].name);
    return to_device(uc, ctx, args, n);
}

// ---- the three hooks, each serving its unbatched form (`batch` false: one image, buffers without the image dimension) and its batched one
// variant: 0 = conv_plan's choice, 1 = the general kernel, 2, 3, ... = each MFMA tile instance in turn; anything else is refused
int layer_hook(halide_buffer_t *input, halide_buffer_t *weights, halide_buffer_t *gamma, halide_buffer_t *beta, halide_buffer_t *mu, halide_buffer_t *sig,
               halide_buffer_t *residual, int stride, int pad, int mode, int variant, halide_buffer_t *output, bool batch) {
    void *uc = nullptr;
    const RnLaunch forced[2] = {RN_MFMA, RN_MFMA_WIDE};
    if (stride < 1 || pad < 0 || mode < RAW || mode > RESIDUAL_RELU || variant < 0 || variant > 3)
        return report(uc, halide_error_code_constraint_violated, "Constraint violated: resnet50 layer hook: stride %d, pad %d, mode %d, variant %d", stride, pad,
                      mode, variant);
    if (variant >= 2 && !dev::CANON_FMA)   // an MFMA step is fused by construction: a missing kernel is an error, not another kernel
        return report(uc, halide_error_code_constraint_violated, "Constraint violated: resnet50 layer hook: variant %d, an MFMA tile, in a HLMI_CANON_FMA=0 build",
                      variant);
    if (!input || !weights) return report(uc, halide_error_code_buffer_argument_is_null, "Buffer argument %s is nullptr", input ? "weights" : "input");
    const int ad = batch ? 4 : 3;   // dimensions of an activation
    if (input->dimensions != ad || weights->dimensions != 4)
        return report(uc, halide_error_code_bad_dimensions, "input is %d-D and weights is 4-D", ad);
    const int CI = input->dim[0].extent, W = input->dim[1].extent, H = input->dim[2].extent, NI = batch ? input->dim[3].extent : 1;
    const int CO = weights->dim[0].extent, KW = weights->dim[1].extent, KH = weights->dim[2].extent;
    const int OW = out_extent(W, KW, stride, pad), OH = out_extent(H, KH, stride, pad);
    if (CI < 1 || CO < 1 || KW < 1 || KH < 1 || OW < 1 || OH < 1 || NI < 1)
        return report(uc, halide_error_code_constraint_violated, "Constraint violated: resnet50 layer hook: an empty layer");
    const bool with_res = mode == RESIDUAL_RELU;
    const Want w[8] = {{"input", input, ad, {CI, W, H, NI}}, {"weights", weights, 4, {CO, KW, KH, CI}}, {"gamma", gamma, 1, {CO}}, {"beta", beta, 1, {CO}},
                       {"mu", mu, 1, {CO}}, {"sig", sig, 1, {CO}}, {"residual", residual, ad, {CO, OW, OH, NI}}, {"output", output, ad, {CO, OW, OH, NI}}};
    BufArg args[8];
    DeviceCtx ctx;
    Want list[8];   // the residual is read, and looked at, in its own mode only
    int n = 0;
    for (int i = 0; i < 8; i++)
        if (i != 6 || with_res) list[n++] = w[i];
    if (int r = hook_prologue(uc, list, n, 1, args, &ctx)) return r;
    CGeom g = {};
    g.in = dev_ptr<float>(input), g.w = dev_ptr<float>(weights), g.gamma = dev_ptr<float>(gamma), g.beta = dev_ptr<float>(beta), g.mu = dev_ptr<float>(mu);
    g.sig = dev_ptr<float>(sig), g.res = with_res ? dev_ptr<float>(residual) : nullptr, g.out = dev_ptr<float>(output);
    g.CI = CI, g.W = W, g.H = H, g.CO = CO, g.KW = KW, g.KH = KH, g.S = stride, g.P = pad, g.OW = OW, g.OH = OH, g.mode = mode;
    g.isx = input->dim[1].stride, g.isy = input->dim[2].stride;
    g.wkx = weights->dim[1].stride, g.wky = weights->dim[2].stride, g.wci = weights->dim[3].stride;
    g.osx = output->dim[1].stride, g.osy = output->dim[2].stride;
    if (with_res) g.rsx = residual->dim[1].stride, g.rsy = residual->dim[2].stride;
    g.NI = NI;
    if (batch) g.isn = input->dim[3].stride, g.osn = output->dim[3].stride, g.rsn = with_res ? residual->dim[3].stride : 0;
    Step s = {};
    s.c = g, s.launch = variant >= 2 ? forced[variant - 2] : conv_plan(g, variant == 1);
    if (int r = rn_launch(uc, ctx.stream, s)) return r;
    mark_output_written(output);
    return 0;
}

int maxpool_hook(halide_buffer_t *input, int k, int stride, int pad, halide_buffer_t *output, bool batch) {
    void *uc = nullptr;
    if (k < 1 || stride < 1 || pad < 0) return report(uc, halide_error_code_constraint_violated, "Constraint violated: resnet50 max pool hook: k %d, stride %d, pad %d", k, stride, pad);
    if (!input) return report(uc, halide_error_code_buffer_argument_is_null, "Buffer argument input is nullptr");
    const int ad = batch ? 4 : 3;
    if (input->dimensions != ad) return report(uc, halide_error_code_bad_dimensions, "input is %d-D", ad);
    const int Cn = input->dim[0].extent, W = input->dim[1].extent, H = input->dim[2].extent, NI = batch ? input->dim[3].extent : 1;
    const int OW = out_extent(W, k, stride, pad), OH = out_extent(H, k, stride, pad);
    if (Cn < 1 || OW < 1 || OH < 1 || NI < 1) return report(uc, halide_error_code_constraint_violated, "Constraint violated: resnet50 max pool hook: an empty layer");
    const Want w[2] = {{"input", input, ad, {Cn, W, H, NI}}, {"output", output, ad, {Cn, OW, OH, NI}}};
    BufArg args[2];
    DeviceCtx ctx;
    if (int r = hook_prologue(uc, w, 2, 1, args, &ctx)) return r;
    Step s = {};
    s.launch = RN_MAXPOOL;
    s.p = {dev_ptr<float>(input), dev_ptr<float>(output), Cn, W, H, k, stride, pad, OW, OH, input->dim[1].stride, input->dim[2].stride,
           output->dim[1].stride, output->dim[2].stride, NI, batch ? input->dim[3].stride : 0, batch ? output->dim[3].stride : 0};
    if (int r = rn_launch(uc, ctx.stream, s)) return r;
    mark_output_written(output);
    return 0;
}

int tail_hook(halide_buffer_t *input, halide_buffer_t *fc_weights, halide_buffer_t *fc_bias, halide_buffer_t *output, bool batch) {
    void *uc = nullptr;
    if (!input || !fc_bias) return report(uc, halide_error_code_buffer_argument_is_null, "Buffer argument %s is nullptr", input ? "fc_bias" : "input");
    const int ad = batch ? 4 : 3;
    if (input->dimensions != ad || fc_bias->dimensions != 1) return report(uc, halide_error_code_bad_dimensions, "input is %d-D and fc_bias is 1-D", ad);
    const int Cn = input->dim[0].extent, W = input->dim[1].extent, H = input->dim[2].extent, N = fc_bias->dim[0].extent, NI = batch ? input->dim[3].extent : 1;
    if (Cn < 1 || W < 1 || H < 1 || N < 1 || NI < 1) return report(uc, halide_error_code_constraint_violated, "Constraint violated: resnet50 tail hook: an empty layer");
    const Want w[4] = {{"input", input, ad, {Cn, W, H, NI}}, {"fc_weights", fc_weights, 2, {N, Cn}}, {"fc_bias", fc_bias, 1, {N}}, {"output", output, ad - 2, {N, NI}}};
    BufArg args[4];
    DeviceCtx ctx;
    if (int r = hook_prologue(uc, w, 4, 1, args, &ctx)) return r;
    void *ws = nullptr;
    if (int r = get_workspace(uc, ctx, ((size_t)Cn + 2 * (size_t)N) * NI * sizeof(float), &ws)) return r;
    float *pool = (float *)ws, *fc = pool + (size_t)Cn * NI, *e = fc + (size_t)N * NI;
    Step s = {};
    s.launch = RN_AVGPOOL;
    s.p = {dev_ptr<float>(input), pool, Cn, W, H, W, 1, 0, 1, 1, input->dim[1].stride, input->dim[2].stride, Cn, Cn, NI, batch ? input->dim[3].stride : 0, Cn};
    if (int r = rn_launch(uc, ctx.stream, s)) return r;
    s = {};
    s.t = {pool, dev_ptr<float>(fc_weights), dev_ptr<float>(fc_bias), fc, e, dev_ptr<float>(output), Cn, N, fc_weights->dim[1].stride, 0, N,
           NI, Cn, N, batch ? output->dim[1].stride : 0};
    s.launch = RN_FC;
    if (int r = rn_launch(uc, ctx.stream, s)) return r;
    s.launch = RN_SOFTMAX;
    if (int r = rn_launch(uc, ctx.stream, s)) return r;
    mark_output_written(output);
    return 0;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------- exported
extern "C" int resnet50(HLMI_RN50_INPUTS(HLMI_RN50_PARAM) halide_buffer_t *final_output) {
    halide_buffer_t *const p[NARGS] = {HLMI_RN50_INPUTS(RN50_VALUE) final_output};
    return rn50_entry(p, false, false);
}
HLMI_ENTRY(resnet50, rn_table.md)

// A library extension (the reference has no such generator): input [3, 224, 224, N] -> final_output [1000, N], column n bit for bit what
// resnet50 writes for image n.
extern "C" int resnet50_batch(HLMI_RN50_INPUTS(HLMI_RN50_PARAM) halide_buffer_t *final_output) {
    halide_buffer_t *const p[NARGS] = {HLMI_RN50_INPUTS(RN50_VALUE) final_output};
    return rn50_entry(p, false, true);
}
HLMI_ENTRY(resnet50_batch, rn_batch_table.md)

// The same calls, in argv form, with every convolution on the one-thread-per-output kernel.
extern "C" int hlmi_resnet50_general(void **argv) { return rn50_entry((halide_buffer_t *const *)argv, true, false); }
extern "C" int hlmi_resnet50_batch_general(void **argv) { return rn50_entry((halide_buffer_t *const *)argv, true, true); }

// One convolution layer of any shape through conv_plan() and the network's kernels.
extern "C" int hlmi_debug_resnet50_layer(halide_buffer_t *input, halide_buffer_t *weights, halide_buffer_t *gamma, halide_buffer_t *beta, halide_buffer_t *mu,
                                         halide_buffer_t *sig, halide_buffer_t *residual, int32_t stride, int32_t pad, int32_t mode, int32_t general_only,
                                         halide_buffer_t *output) {
    return layer_hook(input, weights, gamma, beta, mu, sig, residual, stride, pad, mode, general_only != 0, output, false);
}
// The same over N images: input [CI, W, H, N], residual and output [CO, OW, OH, N]; variant as layer_hook() has it.
extern "C" int hlmi_debug_resnet50_layer_batch(halide_buffer_t *input, halide_buffer_t *weights, halide_buffer_t *gamma, halide_buffer_t *beta,
                                               halide_buffer_t *mu, halide_buffer_t *sig, halide_buffer_t *residual, int32_t stride, int32_t pad, int32_t mode,
                                               int32_t variant, halide_buffer_t *output) {
    return layer_hook(input, weights, gamma, beta, mu, sig, residual, stride, pad, mode, variant, output, true);
}

// The max pool at any size: input [C, W, H] -> output [C, OW, OH], k x k window; _batch: [C, W, H, N] -> [C, OW, OH, N].
extern "C" int hlmi_debug_resnet50_maxpool(halide_buffer_t *input, int32_t k, int32_t stride, int32_t pad, halide_buffer_t *output) {
    return maxpool_hook(input, k, stride, pad, output, false);
}
extern "C" int hlmi_debug_resnet50_maxpool_batch(halide_buffer_t *input, int32_t k, int32_t stride, int32_t pad, halide_buffer_t *output) {
    return maxpool_hook(input, k, stride, pad, output, true);
}

// The tail at any size: input [C, W, H] -> mean over W x H -> fc with weights [N, C] and bias [N] -> softmax -> output [N]; _batch: input
// [C, W, H, images] -> output [N, images].
extern "C" int hlmi_debug_resnet50_tail(halide_buffer_t *input, halide_buffer_t *fc_weights, halide_buffer_t *fc_bias, halide_buffer_t *output) {
    return tail_hook(input, fc_weights, fc_bias, output, false);
}
extern "C" int hlmi_debug_resnet50_tail_batch(halide_buffer_t *input, halide_buffer_t *fc_weights, halide_buffer_t *fc_bias, halide_buffer_t *output) {
    return tail_hook(input, fc_weights, fc_bias, output, true);
}

// The plan of the first run of a batch of n_images >= 1 images, min(n_images, *chunk) of them, without a device: steps[57][5] = launch (an index into names: 0 resnet50_conv_mfma,
// 1 resnet50_conv_general, 2 resnet50_maxpool, 3 resnet50_avgpool, 4 resnet50_fc, 5 resnet50_softmax, 6 resnet50_conv_mfma_wide), grid x,
// grid y, and the co and pixel edges of the tile (0 where the launch has none); *chunk: the images per run in force
// (HLMI_RN50_BATCH_CHUNK, -8 where that is out of range).
extern "C" int hlmi_debug_resnet50_batch_plan(int32_t n_images, int32_t general_only, int32_t *chunk, int32_t *steps) {
    void *uc = nullptr;
    if (n_images < 1 || !chunk || !steps)
        return report(uc, halide_error_code_constraint_violated, "Constraint violated: resnet50 batch plan hook: %d images", n_images);
    int c = 0;
    if (int r = batch_chunk(uc, &c)) return r;
    *chunk = c;
    n_images = std::min(n_images, c);
    // dense buffers of the fixed boxes at address 0: the plan reads strides, and its pointers are never followed
    std::vector<halide_buffer_t> bufs(NARGS);
    std::vector<halide_dimension_t> dims((size_t)NARGS * 4);
    halide_buffer_t *p[NARGS];
    for (int i = 0; i < NARGS; i++) {
        int ext[4] = {CLASSES, n_images, 1, 1};
        if (i < NARGS - 1) rn_box(i, ext);
        if (i == 0) ext[3] = n_images;
        bufs[i] = halide_buffer_t{};
        bufs[i].dimensions = rn_arg_dims(i, true), bufs[i].dim = &dims[(size_t)i * 4];
        int stride = 1;
        for (int d = 0; d < 4; d++) dims[(size_t)i * 4 + d] = {0, ext[d], stride, 0}, stride *= ext[d];
        p[i] = &bufs[i];
    }
    const std::vector<Step> plan = rn50_plan(p, nullptr, general_only != 0, n_images, nullptr, p[0]->dim[3].stride, nullptr, CLASSES);
    for (size_t i = 0; i < plan.size(); i++) {
        const dim3 grid = rn_grid(plan[i]);
        const int32_t line[5] = {(int32_t)plan[i].launch, (int32_t)grid.x, (int32_t)grid.y, tile_co(plan[i].launch), tile_px(plan[i].launch)};
        std::copy_n(line, 5, steps + 5 * i);
    }
    return (int)plan.size();
}
