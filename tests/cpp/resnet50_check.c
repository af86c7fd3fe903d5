/* resnet50_check.c — plain-C checker of apps/resnet_50 (Resnet50Generator.cpp:117-218, :236-379): TEST INFRASTRUCTURE ONLY.
 *
 * Restated from the generator, layer by layer, in both canonical float forms (o_mad of oracle/oracle_common.h: fused, or multiply then
 * add; the switch is check_canon.c's):
 *   conv       conv(c, i, j) += weights(c, r.y, r.z, r.x) * padded(r.x, s i + r.y - p, s j + r.z - p), RDom r(ci, kx, ky) with r.x fastest:
 *              one chain per output from +0, a tap outside the image a step with the value +0
 *   norm       (v - mu(c)) / sqrt(sig(c) + 1e-5f);   scale: mad(t, gamma(c), beta(c));   relu: v > 0 ? v : 0;   sum: shortcut + scaled
 *   max pool   from -inf, r.x fastest: acc = v > acc ? v : acc over the +0-padded input
 *   avg pool   from +0, acc = mad(n, v, acc), n = 1.0f / (float)(w h);   fc: from bias(c), acc = mad(w(c, k), pool(k), acc)
 *   softmax    e(c) = halide_exp(fc(c)), S = e(0) + e(1) + ... from +0, out(c) = e(c) / S
 * Dimension 0 is innermost: an activation (c, x, y) is a[c + x sx + y sy], a weight (co, kx, ky, ci) is w[co + kx s1 + ky s2 + ci s3];
 * strides in elements.  Built with -ffp-contract=off: the only fused operation is the fmaf of o_mad.  The loops run pixel, k, co so
 * that a compiler may do several co at once (the chains of neighbouring co are independent and contiguous in the weights); every
 * output still sees its own k = 0, 1, 2, ... in that order, which is all the contract says.  Rows of pixels go to OpenMP threads. */
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include "oracle_common.h"

enum { RAW = 0, SCALED = 1, SCALED_RELU = 2, RESIDUAL_RELU = 3 };

/* compute_shape (:245-251) */
int rn_out_extent(int in, int k, int stride, int pad) { return (pad * 2 + in - k + 1 + stride - 1) / stride; }

void rn_conv(const float *in, long isx, long isy, const float *w, long wkx, long wky, long wci, const float *gamma, const float *beta,
             const float *mu, const float *sig, const float *res, long rsx, long rsy, float *out, long osx, long osy, int CI, int W, int H, int CO,
             int KW, int KH, int S, int P, int mode) {
    const int OW = rn_out_extent(W, KW, S, P), OH = rn_out_extent(H, KH, S, P), fma = o_canon_fma;
    float *sd = (float *)malloc(sizeof(float) * (size_t)CO);
    for (int c = 0; c < CO; c++) sd[c] = mode == RAW ? 1.0f : sqrtf(sig[c] + 1e-5f);
#pragma omp parallel for schedule(dynamic)
    for (int j = 0; j < OH; j++) {
        float *acc = (float *)malloc(sizeof(float) * (size_t)CO);
        for (int i = 0; i < OW; i++) {
            for (int c = 0; c < CO; c++) acc[c] = 0.0f;
            for (int ky = 0; ky < KH; ky++)
                for (int kx = 0; kx < KW; kx++) {
                    const int x = S * i + kx - P, y = S * j + ky - P, inside = x >= 0 && x < W && y >= 0 && y < H;
                    const float *ip = inside ? in + x * isx + y * isy : NULL;
                    for (int ci = 0; ci < CI; ci++) {
                        const float v = inside ? ip[ci] : 0.0f;
                        const float *wr = w + kx * wkx + ky * wky + ci * wci;
                        if (fma)
                            for (int c = 0; c < CO; c++) acc[c] = fmaf(wr[c], v, acc[c]);
                        else
                            for (int c = 0; c < CO; c++) acc[c] = wr[c] * v + acc[c];
                    }
                }
            float *o = out + i * osx + j * osy;
            for (int c = 0; c < CO; c++) {
                float v = acc[c];
                if (mode != RAW) {
                    v = o_mad((v - mu[c]) / sd[c], gamma[c], beta[c]);
                    if (mode == RESIDUAL_RELU) v = res[i * rsx + j * rsy + c] + v;
                    if (mode >= SCALED_RELU) v = v > 0.0f ? v : 0.0f;
                }
                o[c] = v;
            }
        }
        free(acc);
    }
    free(sd);
}

void rn_maxpool(const float *in, long isx, long isy, float *out, long osx, long osy, int C, int W, int H, int K, int S, int P) {
    const int OW = rn_out_extent(W, K, S, P), OH = rn_out_extent(H, K, S, P);
    for (int j = 0; j < OH; j++)
        for (int i = 0; i < OW; i++)
            for (int c = 0; c < C; c++) {
                float acc = -INFINITY;
                for (int ry = 0; ry < K; ry++)
                    for (int rx = 0; rx < K; rx++) {
                        const int x = S * i + rx - P, y = S * j + ry - P;
                        const float v = (x >= 0 && x < W && y >= 0 && y < H) ? in[x * isx + y * isy + c] : 0.0f;
                        acc = v > acc ? v : acc;
                    }
                out[i * osx + j * osy + c] = acc;
            }
}

/* pool[C], fc[N], e[N] and out[N] are all written: the tests look at every stage */
void rn_tail(const float *in, long isx, long isy, int C, int W, int H, const float *fw, long fws, const float *fb, int N, float *pool, float *fc,
             float *e, float *out) {
    const float n = 1.0f / (float)(W * H);
    for (int c = 0; c < C; c++) {
        float acc = 0.0f;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) acc = o_mad(n, in[x * isx + y * isy + c], acc);
        pool[c] = acc;
    }
    for (int c = 0; c < N; c++) fc[c] = fb[c];
    for (int k = 0; k < C; k++)
        for (int c = 0; c < N; c++) fc[c] = o_mad(fw[k * fws + c], pool[k], fc[c]);
    float s = 0.0f;
    for (int c = 0; c < N; c++) {
        e[c] = o_halide_exp(fc[c]);
        s = s + e[c];
    }
    for (int c = 0; c < N; c++) out[c] = e[c] / s;
}

/* The whole network on dense buffers.  par[G * 53 + c]: group G (gamma, beta, mu, sig, weights) of convolution c in the order conv1,
 * br1 0 .. 3, br2a 0 .. 15, br2b 0 .. 15, br2c 0 .. 15 — the arguments 1 .. 265 of the entry point as they come.  fc[1000] and out[1000]. */
enum { NCONV = 53, BR1 = 1, BR2A = 5, BR2B = 21, BR2C = 37, SLOT = 64 * 112 * 112 };

static void conv_dense(const float *in, const float *const *par, int c, const float *res, float *out, int CI, int W, int CO, int K, int S, int P, int mode) {
    const int OW = rn_out_extent(W, K, S, P);
    rn_conv(in, CI, (long)CI * W, par[4 * NCONV + c], CO, (long)CO * K, (long)CO * K * K, par[c], par[NCONV + c], par[2 * NCONV + c], par[3 * NCONV + c], res, CO,
            (long)CO * OW, out, CO, (long)CO * OW, CI, W, W, CO, K, K, S, P, mode);
}

void rn_network(const float *input, const float *const *par, const float *fw, const float *fb, float *pooled, float *fc, float *out) {
    float *slot[5], *e = (float *)malloc(sizeof(float) * 1000);
    for (int i = 0; i < 5; i++) slot[i] = (float *)malloc(sizeof(float) * SLOT);
    conv_dense(input, par, 0, NULL, slot[1], 3, 224, 64, 7, 2, 3, SCALED_RELU);
    rn_maxpool(slot[1], 64, 64 * 112, slot[0], 64, 64 * 56, 64, 112, 112, 3, 2, 1);
    static const int mid[4] = {64, 128, 256, 512}, blocks[4] = {3, 4, 6, 3}, strides[4] = {1, 2, 2, 2};
    float *x = slot[0], *y = slot[1];
    int cin = 64, size = 56, b = 0;
    for (int s = 0; s < 4; s++)
        for (int i = 0; i < blocks[s]; i++, b++) {
            const int st = i == 0 ? strides[s] : 1, osize = rn_out_extent(size, 1, st, 0);
            const float *shortcut = x;
            if (i == 0) {
                conv_dense(x, par, BR1 + s, NULL, slot[2], cin, size, 4 * mid[s], 1, st, 0, SCALED);
                shortcut = slot[2];
            }
            conv_dense(x, par, BR2A + b, NULL, slot[3], cin, size, mid[s], 1, 1, 0, SCALED_RELU);
            conv_dense(slot[3], par, BR2B + b, NULL, slot[4], mid[s], size, mid[s], 3, st, 1, SCALED_RELU);
            conv_dense(slot[4], par, BR2C + b, shortcut, y, mid[s], osize, 4 * mid[s], 1, 1, 0, RESIDUAL_RELU);
            float *t = x;
            x = y, y = t;
            cin = 4 * mid[s], size = osize;
        }
    rn_tail(x, 2048, 2048 * 7, 2048, 7, 7, fw, 1000, fb, 1000, pooled, fc, e, out);
    for (int i = 0; i < 5; i++) free(slot[i]);
    free(e);
}
