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
// coalesce) and resnet50_softmax (one workgroup; the 1000-step sum is one serial chain by contract).
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
constexpr int CLASSES = 1000;
constexpr int NARGS = 269, NCONV = 53;
constexpr int SLOT = 64 * 112 * 112;   // floats in a workspace slot: the largest activation (conv1's output; 256 x 56 x 56 is as large)
constexpr int NSLOTS = 5;

enum Mode { RAW = 0, SCALED = 1, SCALED_RELU = 2, RESIDUAL_RELU = 3 };

// One convolution: activations (c, x, y) and weights (co, kx, ky, ci), dimension 0 innermost with stride 1; the other strides in elements
struct CGeom {
    const float *in, *w, *gamma, *beta, *mu, *sig, *res;
    float *out;
    int CI, W, H, CO, KW, KH, S, P, OW, OH, mode;
    int isx, isy, wkx, wky, wci, osx, osy, rsx, rsy;
};
struct PGeom {   // a pool: max (k x k, stride, pad) or, with avg, the mean over the whole w x h image
    const float *in;
    float *out;
    int C, W, H, K, S, P, OW, OH, isx, isy, osx, osy;
};
struct TGeom {   // fc and softmax
    const float *pool, *w, *bias;
    float *fc, *e, *out;
    int C, N, ws, omin, oext;   // C inputs, N classes, ws = stride of w's dimension 1; classes [omin, omin + oext) are stored
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
    const int co0 = blockIdx.x * TC, p0 = blockIdx.y * TP, npix = g.OW * g.OH, K = g.KH * g.KW * g.CI;
    const int nchunk = (K + KC - 1) / KC;

    if (tid < TP) {   // a pixel past the end repeats the last one: loaded, computed, never stored
        const int p = min(p0 + tid, npix - 1), j = p / g.OW, i = p - j * g.OW;
        sPx[tid] = i * g.S, sPy[tid] = j * g.S;
        sPa[tid] = i * g.S * g.isx + j * g.S * g.isy;
        sPo[tid] = i * g.osx + j * g.osy;
        sPr[tid] = i * g.rsx + j * g.rsy;
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
    if (idx >= (long)g.CO * g.OW * g.OH) return;
    const int co = (int)(idx % g.CO), p = (int)(idx / g.CO), j = p / g.OW, i = p - j * g.OW;
    float acc = 0.0f;
    for (int ky = 0; ky < g.KH; ky++)
        for (int kx = 0; kx < g.KW; kx++) {
            const int x = g.S * i + kx - g.P, y = g.S * j + ky - g.P;
            const bool inside = (unsigned)x < (unsigned)g.W && (unsigned)y < (unsigned)g.H;
            const float *ip = g.in + (inside ? x * g.isx + y * g.isy : 0);
            const float *wp = g.w + kx * g.wkx + ky * g.wky + co;
            for (int ci = 0; ci < g.CI; ci++) acc = dev::mad(wp[(long)ci * g.wci], inside ? ip[ci] : 0.0f, acc);
        }
    g.out[i * g.osx + j * g.osy + co] = rn_finish(g, rn_chan(g, co), acc, i * g.rsx + j * g.rsy + co);
}

__global__ __launch_bounds__(256) void rn_maxpool(PGeom g) {
    const long idx = blockIdx.x * 256L + threadIdx.x;
    if (idx >= (long)g.C * g.OW * g.OH) return;
    const int c = (int)(idx % g.C), p = (int)(idx / g.C), j = p / g.OW, i = p - j * g.OW;
    float acc = -__builtin_inff();
    for (int ry = 0; ry < g.K; ry++)
        for (int rx = 0; rx < g.K; rx++) {
            const int x = g.S * i + rx - g.P, y = g.S * j + ry - g.P;
            const float v = ((unsigned)x < (unsigned)g.W && (unsigned)y < (unsigned)g.H) ? g.in[x * g.isx + y * g.isy + c] : 0.0f;
            acc = v > acc ? v : acc;
        }
    g.out[i * g.osx + j * g.osy + c] = acc;
}

__global__ __launch_bounds__(256) void rn_avgpool(PGeom g) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= g.C) return;
    const float n = 1.0f / (float)(g.W * g.H);
    float acc = 0.0f;
    for (int y = 0; y < g.H; y++)
        for (int x = 0; x < g.W; x++) acc = dev::mad(n, g.in[x * g.isx + y * g.isy + c], acc);
    g.out[c] = acc;
}

__global__ __launch_bounds__(64) void rn_fc(TGeom g) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= g.N) return;
    float acc = g.bias[c];
    const float *w = g.w + c;
#pragma unroll 8
    for (int k = 0; k < g.C; k++) acc = dev::mad(w[(long)k * g.ws], g.pool[k], acc);
    g.fc[c] = acc;
}

__global__ __launch_bounds__(1024) void rn_softmax(TGeom g) {
    __shared__ float S;
    for (int c = threadIdx.x; c < g.N; c += 1024) g.e[c] = dev::halide_exp(g.fc[c]);
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.0f;
        for (int c = 0; c < g.N; c++) s = s + g.e[c];
        S = s;
    }
    __syncthreads();
    for (int c = g.omin + (int)threadIdx.x; c < g.omin + g.oext; c += 1024) g.out[c - g.omin] = g.e[c] / S;
}

// ---------------------------------------------------------------------------------------------------------------- plan
enum RnLaunch { RN_MFMA, RN_GENERAL, RN_MAXPOOL, RN_AVGPOOL, RN_FC, RN_SOFTMAX };
const char *const rn_names[6] = {"resnet50_conv_mfma", "resnet50_conv_general", "resnet50_maxpool", "resnet50_avgpool", "resnet50_fc", "resnet50_softmax"};

// THE predicate.  The general kernel takes the whole HLMI_CANON_FMA=0 build, every call that asks for it by name, and the layers where
// it measured faster than the tile loop: at most SHORT_K steps and at most TILE output channels.  The MFMA kernel takes the rest.
RnLaunch conv_plan(const CGeom &g, bool general_only) {
    if (general_only || !dev::CANON_FMA) return RN_GENERAL;
    return (g.KH * g.KW * g.CI <= SHORT_K && g.CO <= TILE) ? RN_GENERAL : RN_MFMA;
}

struct Step {
    RnLaunch launch;
    CGeom c;
    PGeom p;
    TGeom t;
};

int rn_launch(void *uc, hipStream_t st, const Step &s) {
    const char *name = rn_names[s.launch];
    auto blocks = [](long n, int per) { return dim3((unsigned)((n + per - 1) / per)); };
    switch (s.launch) {
    case RN_MFMA: {
        const dim3 grid((unsigned)((s.c.CO + TILE - 1) / TILE), (unsigned)((s.c.OW * s.c.OH + TILE - 1) / TILE));
        HLMI_LAUNCH(uc, name, st, (rn_conv_mfma<TILE / 32, TILE / 32>), grid, dim3(TILE * TILE / 16), 0, s.c);
        return 0;
    }
    case RN_GENERAL: HLMI_LAUNCH(uc, name, st, rn_conv_general, blocks((long)s.c.CO * s.c.OW * s.c.OH, 256), dim3(256), 0, s.c); return 0;
    case RN_MAXPOOL: HLMI_LAUNCH(uc, name, st, rn_maxpool, blocks((long)s.p.C * s.p.OW * s.p.OH, 256), dim3(256), 0, s.p); return 0;
    case RN_AVGPOOL: HLMI_LAUNCH(uc, name, st, rn_avgpool, blocks(s.p.C, 256), dim3(256), 0, s.p); return 0;
    case RN_FC: HLMI_LAUNCH(uc, name, st, rn_fc, blocks(s.t.N, 64), dim3(64), 0, s.t); return 0;
    case RN_SOFTMAX: HLMI_LAUNCH(uc, name, st, rn_softmax, dim3(1), dim3(1024), 0, s.t); return 0;
    }
    return 0;
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

CGeom conv_geom(const Layer &l, const float *in, const float *const *par, const float *res, float *out, int mode) {
    CGeom g = {};
    g.in = in, g.gamma = par[0], g.beta = par[1], g.mu = par[2], g.sig = par[3], g.w = par[4], g.res = res, g.out = out;
    g.CI = l.ci, g.W = l.w, g.H = l.h, g.CO = l.co, g.KW = g.KH = l.k, g.S = l.stride, g.P = l.pad, g.mode = mode;
    g.OW = out_extent(l.w, l.k, l.stride, l.pad), g.OH = out_extent(l.h, l.k, l.stride, l.pad);
    g.isx = l.ci, g.isy = l.ci * l.w;
    g.osx = g.rsx = l.co, g.osy = g.rsy = l.co * g.OW;
    return g;
}

// The launch list of one call.  dev[i]: device address of argument i (its strides: see set_weight_strides); ws: the workspace.
std::vector<Step> rn50_plan(halide_buffer_t *const *p, float *ws, bool general_only) {
    std::vector<Step> plan;
    float *slot[NSLOTS];
    for (int i = 0; i < NSLOTS; i++) slot[i] = ws + (size_t)i * SLOT;
    float *pool = ws + (size_t)NSLOTS * SLOT, *fc = pool + 2048, *e = fc + CLASSES;
    auto conv = [&](int c, const float *in, int isx, int isy, const float *res, float *out, int mode) {
        const float *par[5];
        for (int G = 0; G < 5; G++) par[G] = dev_ptr<float>(p[1 + NCONV * G + c]);
        Step s = {};
        s.c = conv_geom(net.conv[c], in, par, res, out, mode);
        if (isx) s.c.isx = isx, s.c.isy = isy;
        const halide_buffer_t *w = p[1 + NCONV * 4 + c];
        s.c.wkx = w->dim[1].stride, s.c.wky = w->dim[2].stride, s.c.wci = w->dim[3].stride;
        s.launch = conv_plan(s.c, general_only);
        plan.push_back(s);
    };
    // the stem: conv1 + norm + scale + relu -> slot 1, pool1 -> slot 0
    conv(0, dev_ptr<float>(p[0]), p[0]->dim[1].stride, p[0]->dim[2].stride, nullptr, slot[1], SCALED_RELU);
    {
        Step s = {};
        s.launch = RN_MAXPOOL;
        s.p = {slot[1], slot[0], 64, 112, 112, 3, 2, 1, 56, 56, 64, 64 * 112, 64, 64 * 56};
        plan.push_back(s);
    }
    // 16 blocks: x = the block's input, y = its output, slots 2 .. 4 = br1, br2a, br2b
    float *x = slot[0], *y = slot[1];
    for (int b = 0; b < 16; b++) {
        const float *shortcut = x;
        if (br1_of(b) >= 0) conv(BR1 + br1_of(b), x, 0, 0, nullptr, slot[2], SCALED), shortcut = slot[2];
        conv(BR2A + b, x, 0, 0, nullptr, slot[3], SCALED_RELU);
        conv(BR2B + b, slot[3], 0, 0, nullptr, slot[4], SCALED_RELU);
        conv(BR2C + b, slot[4], 0, 0, shortcut, y, RESIDUAL_RELU);
        std::swap(x, y);
    }
    Step s = {};
    s.launch = RN_AVGPOOL;
    s.p = {x, pool, 2048, 7, 7, 7, 1, 0, 1, 1, 2048, 2048 * 7, 2048, 2048};
    plan.push_back(s);
    const halide_buffer_t *fw = p[NARGS - 3], *out = p[NARGS - 1];
    s = {};
    s.t = {pool, dev_ptr<float>(fw), dev_ptr<float>(p[NARGS - 2]), fc, e, dev_ptr<float>(out), 2048, CLASSES, fw->dim[1].stride, out->dim[0].min, out->dim[0].extent};
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
inline int rn_arg_dims(int i) { return i == 0 ? 3 : i <= 4 * NCONV ? 1 : i <= 5 * NCONV ? 4 : i == NARGS - 3 ? 2 : 1; }

std::vector<Arg> rn_arg_lines() {
    std::vector<Arg> v;
    for (int i = 0; i < NARGS; i++) v.push_back(i == NARGS - 1 ? out_buf(rn_arg_names[i], T_F32, 1) : in_buf(rn_arg_names[i], T_F32, rn_arg_dims(i)));
    return v;
}
const std::vector<Arg> rn_lines = rn_arg_lines();
const ArgTable rn_table("resnet50", rn_lines.data(), rn_lines.size());

// the fixed box of input i (every min is 0): extents, rn_arg_dims(i) of them
void rn_box(int i, int ext[4]) {
    if (i == 0) ext[0] = 3, ext[1] = 224, ext[2] = 224;
    else if (i <= 4 * NCONV) ext[0] = net.conv[(i - 1) % NCONV].co;
    else if (i <= 5 * NCONV) {
        const Layer &l = net.conv[i - 1 - 4 * NCONV];
        ext[0] = l.co, ext[1] = l.k, ext[2] = l.k, ext[3] = l.ci;
    } else if (i == NARGS - 3) ext[0] = CLASSES, ext[1] = 2048;
    else ext[0] = CLASSES;
}

// every element of the buffer is within 2^31 - 1 elements of its first: the kernels index with ints
bool span_fits(const halide_buffer_t *b) {
    int64_t span = 0;
    for (int d = 0; d < b->dimensions; d++) span += (int64_t)std::max(b->dim[d].extent - 1, 0) * std::abs((int64_t)b->dim[d].stride);
    return span < INT32_MAX;
}

int rn50_entry(halide_buffer_t *const *p, bool general_only) {
    void *uc = nullptr;
    BufArg args[NARGS];
    for (int i = 0; i < NARGS; i++) {
        const Arg &a = rn_table.spec[i];
        args[i] = {a.name, p[i], a.type, a.dims, i == NARGS - 1};
    }
    int r = check_not_null(uc, args, NARGS);
    if (r) return r;
    if ((r = check_type_and_dims(uc, args, NARGS))) return r;
    // the output may be any box; a class outside [0, 1000) is a read of fc1000_bias and fc1000_weights outside theirs, as in the reference
    halide_buffer_t *out = p[NARGS - 1];
    const bool out_known = buffer_known(out);
    const int omin = out_known ? out->dim[0].min : 0, oext = out_known ? out->dim[0].extent : CLASSES;
    const int cmin = oext > 0 ? std::min(0, omin) : 0, cmax = oext > 0 ? std::max(CLASSES, omin + oext) : CLASSES;
    if (any_bounds_query(args, NARGS)) {
        const int zero[4] = {0, 0, 0, 0};
        for (int i = 0; i < NARGS - 1; i++) {
            int ext[4];
            rn_box(i, ext);
            int mins[4] = {0, 0, 0, 0};
            if (i >= NARGS - 3) mins[0] = cmin, ext[0] = cmax - cmin;
            answer_query(p[i], mins, ext);
        }
        const int oe[1] = {CLASSES};
        if (!out_known) answer_query(out, zero, oe);
        return 0;
    }
    if ((r = check_shapes(uc, args, NARGS))) return r;
    for (int i = 0; i < NARGS - 1; i++) {
        int ext[4];
        rn_box(i, ext);
        for (int d = 0; d < args[i].dims; d++) {
            const bool classes = i >= NARGS - 3 && d == 0;
            check_covers(uc, args[i], d, classes ? cmin : 0, classes ? cmax - cmin : ext[d]);
        }
    }
    if ((r = checks_done(uc))) return r;
    for (int i = 0; i < NARGS; i++)
        if (!span_fits(p[i])) return report(uc, halide_error_code_buffer_extents_too_large, "%s spans more than 2^31 - 1 elements", args[i].name);
    DeviceCtx ctx;
    if ((r = to_device(uc, &ctx, args, NARGS))) return r;
    void *ws = nullptr;
    if ((r = get_workspace(uc, ctx, ((size_t)NSLOTS * SLOT + 2048 + 2 * CLASSES) * sizeof(float), &ws))) return r;
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
    if ((r = rn50_run(uc, ctx.stream, rn50_plan(vp, (float *)ws, general_only)))) return r;
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

}  // namespace

// ---------------------------------------------------------------------------------------------------------------- exported
extern "C" int resnet50(HLMI_RN50_INPUTS(HLMI_RN50_PARAM) halide_buffer_t *final_output) {
    halide_buffer_t *const p[NARGS] = {HLMI_RN50_INPUTS(RN50_VALUE) final_output};
    return rn50_entry(p, false);
}
HLMI_ENTRY(resnet50, rn_table.md)

// The same call, in argv form, with every convolution on the one-thread-per-output kernel.
extern "C" int hlmi_resnet50_general(void **argv) { return rn50_entry((halide_buffer_t *const *)argv, true); }

// One convolution layer of any shape through conv_plan() and the network's kernels.
extern "C" int hlmi_debug_resnet50_layer(halide_buffer_t *input, halide_buffer_t *weights, halide_buffer_t *gamma, halide_buffer_t *beta, halide_buffer_t *mu,
                                         halide_buffer_t *sig, halide_buffer_t *residual, int32_t stride, int32_t pad, int32_t mode, int32_t general_only,
                                         halide_buffer_t *output) {
    void *uc = nullptr;
    if (stride < 1 || pad < 0 || mode < RAW || mode > RESIDUAL_RELU)
        return report(uc, halide_error_code_constraint_violated, "Constraint violated: resnet50 layer hook: stride %d, pad %d, mode %d", stride, pad, mode);
    if (!input || !weights) return report(uc, halide_error_code_buffer_argument_is_null, "Buffer argument %s is nullptr", input ? "weights" : "input");
    if (input->dimensions != 3 || weights->dimensions != 4) return report(uc, halide_error_code_bad_dimensions, "input is 3-D and weights is 4-D");
    const int CI = input->dim[0].extent, W = input->dim[1].extent, H = input->dim[2].extent;
    const int CO = weights->dim[0].extent, KW = weights->dim[1].extent, KH = weights->dim[2].extent;
    const int OW = out_extent(W, KW, stride, pad), OH = out_extent(H, KH, stride, pad);
    if (CI < 1 || CO < 1 || KW < 1 || KH < 1 || OW < 1 || OH < 1)
        return report(uc, halide_error_code_constraint_violated, "Constraint violated: resnet50 layer hook: an empty layer");
    const bool with_res = mode == RESIDUAL_RELU;
    const Want w[8] = {{"input", input, 3, {CI, W, H}}, {"weights", weights, 4, {CO, KW, KH, CI}}, {"gamma", gamma, 1, {CO}}, {"beta", beta, 1, {CO}},
                       {"mu", mu, 1, {CO}}, {"sig", sig, 1, {CO}}, {"residual", residual, 3, {CO, OW, OH}}, {"output", output, 3, {CO, OW, OH}}};
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
    Step s = {};
    s.c = g, s.launch = conv_plan(g, general_only != 0);
    if (int r = rn_launch(uc, ctx.stream, s)) return r;
    mark_output_written(output);
    return 0;
}

// The max pool at any size: input [C, W, H] -> output [C, OW, OH], k x k window.
extern "C" int hlmi_debug_resnet50_maxpool(halide_buffer_t *input, int32_t k, int32_t stride, int32_t pad, halide_buffer_t *output) {
    void *uc = nullptr;
    if (k < 1 || stride < 1 || pad < 0) return report(uc, halide_error_code_constraint_violated, "Constraint violated: resnet50 max pool hook: k %d, stride %d, pad %d", k, stride, pad);
    if (!input) return report(uc, halide_error_code_buffer_argument_is_null, "Buffer argument input is nullptr");
    if (input->dimensions != 3) return report(uc, halide_error_code_bad_dimensions, "input is 3-D");
    const int Cn = input->dim[0].extent, W = input->dim[1].extent, H = input->dim[2].extent, OW = out_extent(W, k, stride, pad), OH = out_extent(H, k, stride, pad);
    if (Cn < 1 || OW < 1 || OH < 1) return report(uc, halide_error_code_constraint_violated, "Constraint violated: resnet50 max pool hook: an empty layer");
    const Want w[2] = {{"input", input, 3, {Cn, W, H}}, {"output", output, 3, {Cn, OW, OH}}};
    BufArg args[2];
    DeviceCtx ctx;
    if (int r = hook_prologue(uc, w, 2, 1, args, &ctx)) return r;
    Step s = {};
    s.launch = RN_MAXPOOL;
    s.p = {dev_ptr<float>(input), dev_ptr<float>(output), Cn, W, H, k, stride, pad, OW, OH, input->dim[1].stride, input->dim[2].stride,
           output->dim[1].stride, output->dim[2].stride};
    if (int r = rn_launch(uc, ctx.stream, s)) return r;
    mark_output_written(output);
    return 0;
}

// The tail at any size: input [C, W, H] -> mean over W x H -> fc with weights [N, C] and bias [N] -> softmax -> output [N].
extern "C" int hlmi_debug_resnet50_tail(halide_buffer_t *input, halide_buffer_t *fc_weights, halide_buffer_t *fc_bias, halide_buffer_t *output) {
    void *uc = nullptr;
    if (!input || !fc_bias) return report(uc, halide_error_code_buffer_argument_is_null, "Buffer argument %s is nullptr", input ? "fc_bias" : "input");
    if (input->dimensions != 3 || fc_bias->dimensions != 1) return report(uc, halide_error_code_bad_dimensions, "input is 3-D and fc_bias is 1-D");
    const int Cn = input->dim[0].extent, W = input->dim[1].extent, H = input->dim[2].extent, N = fc_bias->dim[0].extent;
    if (Cn < 1 || W < 1 || H < 1 || N < 1) return report(uc, halide_error_code_constraint_violated, "Constraint violated: resnet50 tail hook: an empty layer");
    const Want w[4] = {{"input", input, 3, {Cn, W, H}}, {"fc_weights", fc_weights, 2, {N, Cn}}, {"fc_bias", fc_bias, 1, {N}}, {"output", output, 1, {N}}};
    BufArg args[4];
    DeviceCtx ctx;
    if (int r = hook_prologue(uc, w, 4, 1, args, &ctx)) return r;
    void *ws = nullptr;
    if (int r = get_workspace(uc, ctx, ((size_t)Cn + 2 * (size_t)N) * sizeof(float), &ws)) return r;
    float *pool = (float *)ws, *fc = pool + Cn, *e = fc + N;
    Step s = {};
    s.launch = RN_AVGPOOL;
    s.p = {dev_ptr<float>(input), pool, Cn, W, H, W, 1, 0, 1, 1, input->dim[1].stride, input->dim[2].stride, Cn, Cn};
    if (int r = rn_launch(uc, ctx.stream, s)) return r;
    s = {};
    s.t = {pool, dev_ptr<float>(fc_weights), dev_ptr<float>(fc_bias), fc, e, dev_ptr<float>(output), Cn, N, fc_weights->dim[1].stride, 0, N};
    s.launch = RN_FC;
    if (int r = rn_launch(uc, ctx.stream, s)) return r;
    s.launch = RN_SOFTMAX;
    if (int r = rn_launch(uc, ctx.stream, s)) return r;
    mark_output_written(output);
    return 0;
}
