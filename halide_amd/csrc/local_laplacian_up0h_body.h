// The body of ll_up0h and ll_up0r (local_laplacian.hip), included into both kernels: the text between the braces of
//     template<class MP, bool EM1, int CH> __global__ void ll_up0h(Up0HArgs ph, Geometry gm)     with ROWS1 = false
//     template<class MP>                   __global__ void ll_up0r(Up0HArgs ph, Geometry gm)     with EM1 = ROWS1 = true, CH = 2
// MP: the MemPolicy (local_laplacian.hip, above ld_frame4) — the flavours of the input and outLPyramid[0] loads and the output stores of
// the row loop, of the outLPyramid[1] loads (EM1) and of phase 0's level-2 / 3 loads.  The three-plane phase 1 (EM1 off) stays plain.
// It is text and not a function the two kernels call because ll_up0h must compile to the instructions it had before ll_up0r
// existed (the stream that owns the device runs it): as an inlined function the compiler commutes operands and schedules otherwise.
    static_assert(EM1 || !ROWS1, "ROWS1 adds the stored outLPyramid[1] plane");
    const Up0Args &p = ph.u;
    LL_RESIDENCY(1);
    extern __shared__ float s_out1[];
    // tiles in row-major order, a contiguous run of them per XCD (blocks are dealt round-robin over the 8 XCDs): a tile's
    // 130 x (RU + 2) coarse window overlaps its neighbours' by two columns / rows, and its 130-float rows start one float before a
    // 512-byte boundary — 6 lines for 4 of payload, the outer two shared with the neighbour tile: same L2 now (131.5 -> 118.1 MB
    // fetched per 4K frame)
    int bx, by;
    {
        const int b = (int)blockIdx.y * (int)gridDim.x + (int)blockIdx.x, nb8 = (int)(gridDim.x * gridDim.y) >> 3;
        const int lb = b < (nb8 << 3) ? (b & 7) * nb8 + (b >> 3) : b;
        by = lb / (int)gridDim.x, bx = lb - by * (int)gridDim.x;
    }
    const int X0 = p.ox0 + bx * 256;                       // even
    const int Yw0 = p.oy0 + by * (2 * p.RU);
    const int Yw1 = min(Yw0 + 2 * p.RU, p.oy0 + p.oh) - 1;
    const int cx0 = (X0 >> 1) - 1, cy0 = dev::fdiv2(Yw0 - 1);
    const int th = dev::fdiv2(Yw1 + 1) - cy0 + 1;
    float *const s_out2 = s_out1 + (ROWS1 ? 0 : U0_TS * (p.RU + 2));
    const int cx1 = min(cx0 + U0_TW - 1, p.rx1_1);                               // last level-1 column of the tile
    const int c2x0 = dev::fdiv2(cx0 - 1), c2y0 = dev::fdiv2(cy0 - 1);             // level-2 window the level-1 tile's upsampling reads
    // The two tile phases below are each a handful of values per thread, and a value takes two DEPENDENT memory round trips
    // (inGPyramid -> which planes -> their bilinear taps).  As per-element loops they ran those trips element after element — and
    // every workgroup of the launch (one round of resident workgroups) sat in that prologue at the same time, the memory system idle.
    // Round 5: CH elements per thread at a time, all first loads, then all gathers, then the arithmetic (outl_value's and up_at's
    // operations in their order): two trips per chunk.  Worth ~1 % of the frame: the resident workgroups of a CU already interleave
    // their prologues.  Every load is `uniform base + 32-bit byte offset` (the workspace offsets of this path are < 4 GB): as
    // 64-bit element indices the address arithmetic was 60 % of the 148 VALU instructions a tile value cost, and the tile values
    // 45 % of the launch's instructions.
    // The four taps of an upsampled value are f(yb, xb), f(yb, xb + 1) and the same pair one row on (fdiv2(v + 1) = fdiv2(v - 1) + 1):
    // two unaligned 8-byte loads from two byte offsets.  Rows are numbered from the tile's first one, so every row x stride product
    // is (small) x (stride < 2^24, the host checks) = one full-rate v_mul_u32_u24 on top of a scalar base; e / tile width is a
    // multiplication by ceil(2^22 / width), exact while e x width < 2^22 (130 x 302 rows x 130 at the largest tile LDS can hold).
    struct Taps32 {
        uint32_t b, a;             // byte offsets of f(yb, xb) and f(yb + 1, xb) inside a plane
    };
    auto mul24 = [](uint32_t a, uint32_t b) { return (uint32_t)__umul24(a, b); };
    auto tap_bytes = [&](uint32_t row0, int y0, int lox, int ws, int X, int Y) {   // row0 = (y0 - loy) * ws (uniform), y0 <= fdiv2(Y - 1)
        Taps32 t;
        t.b = (row0 + mul24((uint32_t)(dev::fdiv2(Y - 1) - y0), (uint32_t)ws) + (uint32_t)(dev::fdiv2(X - 1) - lox)) << 2;
        t.a = t.b + ((uint32_t)ws << 2);
        return t;
    };
    auto taps_at = [](const float *base, uint32_t plane_bytes, const Taps32 &t) {
        const F2U lo = ld_su<F2U>(base, plane_bytes + t.b), hi = ld_su<F2U>(base, plane_bytes + t.a);
        UpTaps r;
        r.bb = lo.x, r.ba = lo.y, r.ab = hi.x, r.aa = hi.y;
        return r;
    };
    const uint32_t ps1b = (uint32_t)p.ps1 * 4u, ps2b = (uint32_t)p.ps2 * 4u, ps3b = (uint32_t)ph.ps3 * 4u;
    if (ph.fuse2) {
        const int n2x = dev::fdiv2(cx1 + 1) - c2x0 + 1, n2y = dev::fdiv2(cy0 + th) - c2y0 + 1, n2 = n2x * n2y;
        const uint32_t m2 = (4194304u + (uint32_t)n2x - 1u) / (uint32_t)n2x;
        const int c3y0 = dev::fdiv2(c2y0 - 1);
        const uint32_t row2 = (uint32_t)((c2y0 - p.loy2) * p.ws2), row3 = (uint32_t)((c3y0 - ph.loy3) * ph.ws3);
        auto taps23 = [](const float *base, uint32_t plane_bytes, const Taps32 &t) {   // taps_at with the policy's flavour
            const F2U lo = ld_su<F2U, MP::l23_ld>(base, plane_bytes + t.b), hi = ld_su<F2U, MP::l23_ld>(base, plane_bytes + t.a);
            UpTaps r;
            r.bb = lo.x, r.ba = lo.y, r.ab = hi.x, r.aa = hi.y;
            return r;
        };
        for (int e0 = threadIdx.x; e0 < n2; e0 += 256 * CH) {
            int X2[CH], Y2[CH];
            uint32_t ti[CH];
            bool ok[CH];
            uint32_t ob[CH];
            Taps32 t3[CH];
            float inG[CH], lf[CH], ga[CH], gb[CH];
            UpTaps o3[CH], t0[CH], t1[CH];
#pragma unroll
            for (int i = 0; i < CH; i++) {
                const int e = e0 + 256 * i;
                const uint32_t ec = (uint32_t)min(e, n2 - 1), ty = mul24(ec, m2) >> 22, tx = ec - mul24(ty, (uint32_t)n2x);
                ok[i] = e < n2, ti[i] = mul24(ty, U0H_T2) + tx;
                X2[i] = c2x0 + (int)tx, Y2[i] = c2y0 + (int)ty;
                ob[i] = (row2 + mul24(ty, (uint32_t)p.ws2) + (uint32_t)(X2[i] - p.lox2)) << 2;
                inG[i] = ld_su<float, MP::l23_ld>(p.g2, (uint32_t)gm.K * ps2b + ob[i]);
                t3[i] = tap_bytes(row3, c3y0, ph.lox3, ph.ws3, X2[i], Y2[i]);
                o3[i] = taps23(ph.out3, 0u, t3[i]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < CH; i++) {
                const float level = inG[i] * gm.Km1;
                const int li = dev::clampi((int)level, 0, gm.K - 2);
                lf[i] = level - (float)li;
                ga[i] = ld_su<float, MP::l23_ld>(p.g2, (uint32_t)li * ps2b + ob[i]), gb[i] = ld_su<float, MP::l23_ld>(p.g2, (uint32_t)(li + 1) * ps2b + ob[i]);
                t0[i] = taps23(ph.g3, (uint32_t)li * ps3b, t3[i]);
                t1[i] = taps23(ph.g3, (uint32_t)(li + 1) * ps3b, t3[i]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < CH; i++) {
                // outGPyramid[2] = upsample(outGPyramid[3]) + outLPyramid[2]   (:76-79), exactly as ll_up computes it
                const float l0 = ga[i] - up_from(t0[i], X2[i], Y2[i]), l1 = gb[i] - up_from(t1[i], X2[i], Y2[i]);
                const float outL = dev::mad2(1.0f - lf[i], l0, lf[i], l1);
                if (ok[i]) s_out2[ti[i]] = up_from(o3[i], X2[i], Y2[i]) + outL;
            }
        }
        __syncthreads();
    }
    if constexpr (!ROWS1) {
        const int n1 = U0_TW * th;
        constexpr uint32_t M1 = (4194304u + U0_TW - 1) / U0_TW;
        const uint32_t row1 = (uint32_t)((cy0 - p.loy1) * p.ws1), row2 = (uint32_t)((c2y0 - p.loy2) * p.ws2);
        if constexpr (EM1) {
            for (int e0 = threadIdx.x; e0 < n1; e0 += 256 * CH) {
                // outGPyramid[1] = upsample(outGPyramid[2]) + outLPyramid[1]   (:76-79): the stored value and up_at on the LDS tile
                int cx[CH], cy[CH];
                uint32_t ti[CH];
                bool ok[CH];
                float outL[CH];
#pragma unroll
                for (int i = 0; i < CH; i++) {
                    const int e = e0 + 256 * i;
                    const uint32_t ec = (uint32_t)min(e, n1 - 1), ty = mul24(ec, M1) >> 22, tx = ec - mul24(ty, U0_TW);
                    ok[i] = e < n1 && cx0 + (int)tx <= p.rx1_1, ti[i] = mul24(ty, U0_TS) + tx;
                    cx[i] = min(cx0 + (int)tx, p.rx1_1), cy[i] = cy0 + (int)ty;
                    outL[i] = ld_su<float, MP::l1_ld>(p.g1, (row1 + mul24(ty, (uint32_t)p.ws1) + (uint32_t)(cx[i] - p.lox1)) << 2);
                }
#pragma unroll
                for (int i = 0; i < CH; i++) {
                    const float *q = s_out2 + mul24((uint32_t)(dev::fdiv2(cy[i] - 1) - c2y0), U0H_T2) + (uint32_t)(dev::fdiv2(cx[i] - 1) - c2x0);
                    UpTaps t;
                    t.bb = q[0], t.ba = q[1], t.ab = q[U0H_T2], t.aa = q[U0H_T2 + 1];
                    if (ok[i]) s_out1[ti[i]] = up_from(t, cx[i], cy[i]) + outL[i];
                }
            }
        } else {
            for (int e0 = threadIdx.x; e0 < n1; e0 += 256 * CH) {
                int cx[CH], cy[CH];
                uint32_t ti[CH];
                bool ok[CH];
                Taps32 t2[CH];
                float inG[CH], lf[CH], ga[CH], gb[CH];
                UpTaps o2[CH], t0[CH], t1[CH];
#pragma unroll
                for (int i = 0; i < CH; i++) {
                    const int e = e0 + 256 * i;
                    const uint32_t ec = (uint32_t)min(e, n1 - 1), ty = mul24(ec, M1) >> 22, tx = ec - mul24(ty, U0_TW);
                    ok[i] = e < n1 && cx0 + (int)tx <= p.rx1_1, ti[i] = mul24(ty, U0_TS) + tx;
                    cx[i] = min(cx0 + (int)tx, p.rx1_1), cy[i] = cy0 + (int)ty;      // columns right of R_1 are not tile values: their threads re-read its last one
                    const uint32_t ob = (row1 + mul24(ty, (uint32_t)p.ws1) + (uint32_t)(cx[i] - p.lox1)) << 2;
                    // level 1 as ll_down01e stored it: plane 0 / 1 = gPyramid[1](., ., li / li + 1) of the pixel's own li, plane K = inGPyramid[1]
                    inG[i] = ld_su<float>(p.g1, (uint32_t)gm.K * ps1b + ob), ga[i] = ld_su<float>(p.g1, ob), gb[i] = ld_su<float>(p.g1, ps1b + ob);
                    t2[i] = tap_bytes(row2, c2y0, p.lox2, p.ws2, cx[i], cy[i]);
                    if (!ph.fuse2) o2[i] = taps_at(p.out2, 0u, t2[i]);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < CH; i++) {
                    const float level = inG[i] * gm.Km1;
                    const int li = dev::clampi((int)level, 0, gm.K - 2);
                    lf[i] = level - (float)li;
                    t0[i] = taps_at(p.g2, (uint32_t)li * ps2b, t2[i]);
                    t1[i] = taps_at(p.g2, (uint32_t)(li + 1) * ps2b, t2[i]);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < CH; i++) {
                    // outGPyramid[1] = upsample(outGPyramid[2]) + outLPyramid[1]   (:76-79), exactly as ll_up computes it
                    const float l0 = ga[i] - up_from(t0[i], cx[i], cy[i]), l1 = gb[i] - up_from(t1[i], cx[i], cy[i]);
                    const float outL = dev::mad2(1.0f - lf[i], l0, lf[i], l1);
                    float up2;
                    if (ph.fuse2) {   // up_at on the LDS tile: the same taps, weights and lerps
                        const float *q = s_out2 + mul24((uint32_t)(dev::fdiv2(cy[i] - 1) - c2y0), U0H_T2) + (uint32_t)(dev::fdiv2(cx[i] - 1) - c2x0);
                        UpTaps t;
                        t.bb = q[0], t.ba = q[1], t.ab = q[U0H_T2], t.aa = q[U0H_T2 + 1];
                        up2 = up_from(t, cx[i], cy[i]);
                    } else {
                        up2 = up_from(o2[i], cx[i], cy[i]);
                    }
                    if (ok[i]) s_out1[ti[i]] = up2 + outL;
                }
            }
        }
    }
    if constexpr (!ROWS1) __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int x = bx * 256 + (wave & 1) * 128 + 2 * lane;  // output storage column of the lane's pair
    const int y0 = by * (2 * p.RU) + (wave >> 1) * p.RU;
    // ROWS1: a lane right of the image stays to serve its left neighbour — it reads the last pair's frame values and stores nothing
    if (y0 >= p.oh || (ROWS1 ? x - 2 * lane : x) >= p.ow) return;
    const bool live = x < p.ow;                                           // ROWS1 only: the others have left
    const int y1 = min(y0 + p.RU, p.oh);
    const int X = p.ox0 + (ROWS1 ? min(x, p.ow - 2) : x);                 // even
    uint32_t inb = (uint32_t)(X - gm.ix0) * 2u, outb = (uint32_t)x * 2u, l0b = (uint32_t)(X - gm.ix0) * 4u;
    // fma canon: the contracted product is the one with `zero` (dev::mad2) — f[c] * 3/4 for even X, f[c+1] * 1/4 for odd X
    auto hl0 = [](float rm, float r0) {   // lerp(f[c], f[c-1], 1/4): X even
        return dev::CANON_FMA ? __builtin_fmaf(r0, 0.75f, rm * 0.25f) : __builtin_fmaf(rm, 0.25f, r0 * 0.75f);
    };
    auto hl1 = [](float r0, float rp) { return __builtin_fmaf(rp, 0.25f, r0 * 0.75f); };  // lerp(f[c+1], f[c], 3/4): X odd
    auto vl = [](float uq, float ut, float wq, float wt) {   // as in ll_up0f
        return dev::CANON_FMA ? __builtin_fmaf(uq, wq, ut * wt) : __builtin_fmaf(uq, 0.25f, ut * 0.75f);
    };
    struct Frame {
        ushort2 c0, c1, c2;
        float2 l0;
    };
    // The lane's byte offsets are loop invariants: hoisted out of the row loop as 64-bit values they cost a v_lshl_add_u64 per load
    // and store (7 per row); redefined in place per use (an empty asm) they stay 32-bit and every access is `row base in SGPRs +
    // VGPR offset`.
    auto fresh = [](uint32_t &v) {
        asm volatile("" : "+v"(v));
        return v;
    };
    auto load_frame = [&](int y, Frame &f) {
        const int yc = min(y, y1 - 1);
        const uint16_t *irow = p.in + (long)(p.oy0 + yc - gm.iy0) * p.in_sy;
        const uint32_t ib = fresh(inb);
        f.c0 = ld_frame2<MP::in_up>(irow + p.gco[0], ib), f.c1 = ld_frame2<MP::in_up>(irow + p.gco[1], ib), f.c2 = ld_frame2<MP::in_up>(irow + p.gco[2], ib);
        if constexpr (MP::l0_ld == MF_SC1) {
            const f2 v = ld_flavour<MF_SC1, f2>(ph.outl0 + (size_t)yc * ph.l0_ws, ROWS1 ? 2u * fresh(inb) : fresh(l0b));
            f.l0 = make_float2(v.x, v.y);
        } else {
            const f2 *const lp = reinterpret_cast<const f2 *>(reinterpret_cast<const char *>(ph.outl0 + (size_t)yc * ph.l0_ws) + (ROWS1 ? 2u * fresh(inb) : fresh(l0b)));   // ROWS1: one loop register less
            const f2 v = MP::l0_ld == MF_NT ? __builtin_nontemporal_load(lp) : *lp;
            f.l0 = make_float2(v.x, v.y);
        }
    };
    if constexpr (!ROWS1) {
        auto finish = [&](int y, const Frame &f) {
            const int Y = p.oy0 + min(y, y1 - 1);
            const int ya = dev::fdiv2(Y + 1), yb = dev::fdiv2(Y - 1);
            const bool yodd = dev::fmod2(Y) != 0;  // wave-uniform
            // q: the coarse row whose weight is 1/4; fma canon: q = row ya (`zero`), t = row yb (`one`) with weights wq, wt (see ll_up0f)
            const int yq = (dev::CANON_FMA || yodd) ? ya : yb, yt = (dev::CANON_FMA || yodd) ? yb : ya;
            const float wq = yodd ? 0.25f : 0.75f, wt = yodd ? 0.75f : 0.25f;
            const float *oa = s_out1 + (yq - cy0) * U0_TS + (wave & 1) * 64 + lane;
            const float *ob = s_out1 + (yt - cy0) * U0_TS + (wave & 1) * 64 + lane;
            const float ax = oa[0], ay = oa[1], az = oa[2], bx = ob[0], by = ob[1], bz = ob[2];
            const float uo[2] = {vl(hl0(ax, ay), hl0(bx, by), wq, wt), vl(hl1(ay, az), hl1(by, bz), wq, wt)};
            const float outL[2] = {f.l0.x, f.l0.y};
            const uint16_t ch[3][2] = {{f.c0.x, f.c0.y}, {f.c1.x, f.c1.y}, {f.c2.x, f.c2.y}};
            uint16_t res[3][2];
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const float gray = gray_from(ch[0][i], ch[1][i], ch[2][i]);
                const float og = (uo[i] + outL[i]) + 0.01f;
                const float gr = gray + 0.01f;
                const float n[3] = {(float)ch[0][i] * og, (float)ch[1][i] * og, (float)ch[2][i] * og};
                float q[3];
                div3_by(n, gr, q);
#pragma unroll
                for (int c = 0; c < 3; c++) res[c][i] = (uint16_t)__builtin_amdgcn_fmed3f(q[c], 0.0f, 65535.0f);  // q is never NaN
            }
            if (y < y1) {
                uint16_t *orow = p.out + (long)y * p.out_sy;
#pragma unroll
                for (int c = 0; c < 3; c++) st_frame2<MP::out_st>(reinterpret_cast<char *>(orow + (long)c * p.out_sc) + fresh(outb), res[c][0], res[c][1]);
            }
        };
        Frame f[U0H_PF];
#pragma unroll
        for (int i = 0; i < U0H_PF; i++) load_frame(y0 + i, f[i]);
        for (int y = y0; y < y1; y += U0H_PF) {
#pragma unroll
            for (int i = 0; i < U0H_PF; i++) {
                const Frame cur = f[i];
                load_frame(y + U0H_PF + i, f[i]);
                finish(y + i, cur);
            }
        }
    } else {
        // finish (above) from `uo` on: the pair's two values of upsample(outGPyramid[1]) + outLPyramid[0], recolour, u16 store —
        // a second copy, since the instances of ll_up0h keep the parent's instructions only with `finish` as it stands
        auto recolour = [&](int y, const Frame &f, const float (&uo)[2]) {
            const float outL[2] = {f.l0.x, f.l0.y};
            const uint16_t ch[3][2] = {{f.c0.x, f.c0.y}, {f.c1.x, f.c1.y}, {f.c2.x, f.c2.y}};
            uint16_t res[3][2];
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const float gray = gray_from(ch[0][i], ch[1][i], ch[2][i]);
                const float og = (uo[i] + outL[i]) + 0.01f;
                const float gr = gray + 0.01f;
                const float n[3] = {(float)ch[0][i] * og, (float)ch[1][i] * og, (float)ch[2][i] * og};
                float q[3];
                div3_by(n, gr, q);
#pragma unroll
                for (int c = 0; c < 3; c++) res[c][i] = (uint16_t)__builtin_amdgcn_fmed3f(q[c], 0.0f, 65535.0f);  // q is never NaN
            }
            if (y < y1 && live) {
                uint16_t *orow = p.out + (long)y * p.out_sy;
#pragma unroll
                for (int c = 0; c < 3; c++) st_frame2<MP::out_st>(reinterpret_cast<char *>(orow + (long)c * p.out_sc) + fresh(outb), res[c][0], res[c][1]);
            }
        };
        // Output rows Y = 2m - 1 and 2m lerp coarse rows m - 1 and m: a wave meets a new coarse row at every odd Y.  It keeps the
        // horizontal lerps (h0: the pair's even column, h1: its odd one) of the last two coarse rows, `lo` = row fdiv2(Y - 1) and
        // `hi` = row fdiv2(Y + 1).  The stored value of row m travels with the frame row that meets it, U0H_PF rows ahead.
        const int c0 = (X0 >> 1) + (wave & 1) * 64;                               // lane 0's coarse column (X0 is even)
        const int cc = min(c0 + lane, p.rx1_1);                                   // the lane's, with the column clamp of phase 1
        const int m0 = dev::fdiv2(p.oy0 + y0 - 1), mlast = dev::fdiv2(p.oy0 + y1);   // the coarse rows the wave's rows read: <= RU / 2 + 2
        uint32_t c1b = (uint32_t)(cc - p.lox1) * 4u, ln = (uint32_t)lane;
        const float *const qc = s_out2 + (dev::fdiv2(cc - 1) - c2x0);
        auto g1_at = [&](const float *q, float outL, int cx, int m) {             // outGPyramid[1](cx, m), as phase 1 forms it
            UpTaps t;
            t.bb = q[0], t.ba = q[1], t.ab = q[U0H_T2], t.aa = q[U0H_T2 + 1];
            return up_from(t, cx, m) + outL;
        };
        // No lane holds the columns beside lanes 0 and 63, c0 - 1 and c0 + 64: the wave forms them for all its coarse rows first — a
        // value per lane, into 2 x (RU / 2 + 2) floats of its own behind the level-2 tile ([row][side]), so no workgroup barrier —
        // and lanes 0 and 63 read one back per coarse row.
        float *const s_edge = s_out2 + U0H_T2 * (p.RU / 2 + 4) + wave * (2 * (p.RU / 2 + 2));
        {
            const uint32_t row1 = (uint32_t)((m0 - p.loy1) * p.ws1);
            for (int e = lane; e < 2 * (mlast - m0 + 1); e += 64) {
                const int m = m0 + (e >> 1), cx = (e & 1) ? min(c0 + 64, p.rx1_1) : c0 - 1;
                const float outL = ld_su<float, MP::l1_ld>(p.g1, (row1 + mul24((uint32_t)(e >> 1), (uint32_t)p.ws1) + (uint32_t)(cx - p.lox1)) << 2);
                s_edge[e] = g1_at(s_out2 + mul24((uint32_t)(dev::fdiv2(m - 1) - c2y0), U0H_T2) + (dev::fdiv2(cx - 1) - c2x0), outL, cx, m);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        auto load_row1 = [&](int m, float &l) {
            l = ld_su<float, MP::l1_ld>(p.g1 + (long)(min(m, mlast) - p.loy1) * p.ws1, fresh(c1b));   // row base wave-uniform
        };
        auto coarse_row = [&](int m, float l, float (&h)[2]) {
            const int mc = min(m, mlast);
            const float g = g1_at(qc + mul24((uint32_t)(dev::fdiv2(mc - 1) - c2y0), U0H_T2), l, cc, mc);
            // the lane number is redefined in place so that what derives from it stays out of the loop's registers
            const uint32_t lu = fresh(ln);
            const float e = s_edge[2 * (mc - m0) + (int)(lu >> 5)];               // lane 0: side 0, lane 63: side 1
            // a wave shift that keeps `old` where there is no source lane: e in lane 0 (lane 63), the neighbour's g elsewhere
            const float gm1 = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, e), __builtin_bit_cast(int, g), 0x138, 0xf, 0xf, false));
            const float gp1 = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, e), __builtin_bit_cast(int, g), 0x130, 0xf, 0xf, false));
            h[0] = hl0(gm1, g), h[1] = hl1(g, gp1);
            __builtin_amdgcn_sched_barrier(0);
        };
        auto rows = [&](auto P) {                                                 // P: the wave's first row Y is odd
            constexpr bool ODD = decltype(P)::value;
            const int Yf = p.oy0 + y0;
            float lo[2] = {0.0f, 0.0f}, hi[2];
            Frame f[U0H_PF];
            float r1[U0H_PF / 2], ra, rb = 0.0f;
            load_row1(dev::fdiv2(Yf - 1), ra);
            if (!ODD) load_row1(dev::fdiv2(Yf + 1), rb);
#pragma unroll
            for (int i = 0; i < U0H_PF; i++) {
                load_frame(y0 + i, f[i]);
                if (ODD != ((i & 1) != 0)) load_row1(dev::fdiv2(Yf + i + 1), r1[i >> 1]);
            }
            coarse_row(dev::fdiv2(Yf - 1), ra, hi);
            if (!ODD) {
                lo[0] = hi[0], lo[1] = hi[1];
                coarse_row(dev::fdiv2(Yf + 1), rb, hi);
            }
            for (int y = y0; y < y1; y += U0H_PF) {
#pragma unroll
                for (int i = 0; i < U0H_PF; i++) {
                    const bool yodd = ODD != ((i & 1) != 0);   // constant once unrolled
                    if (yodd) {
                        lo[0] = hi[0], lo[1] = hi[1];
                        coarse_row(dev::fdiv2(p.oy0 + y + i + 1), r1[i >> 1], hi);
                    }
                    // q: the coarse row whose weight is 1/4 (finish, above): row ya = `hi` for odd Y and in the fma canon
                    const bool qhi = dev::CANON_FMA || yodd;
                    const float wq = yodd ? 0.25f : 0.75f, wt = yodd ? 0.75f : 0.25f;
                    const float uo[2] = {vl(qhi ? hi[0] : lo[0], qhi ? lo[0] : hi[0], wq, wt), vl(qhi ? hi[1] : lo[1], qhi ? lo[1] : hi[1], wq, wt)};
                    recolour(y + i, f[i], uo);
                    __builtin_amdgcn_sched_barrier(0);
                    load_frame(y + U0H_PF + i, f[i]);
                    if (yodd) load_row1(dev::fdiv2(p.oy0 + y + U0H_PF + i + 1), r1[i >> 1]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        };
        if (dev::fmod2(p.oy0 + y0) != 0) rows(std::true_type{});
        else rows(std::false_type{});
    }
