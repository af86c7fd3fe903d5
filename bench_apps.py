#!/usr/bin/env python3
"""bench_apps.py — the other rows of SURVEY.md §8(a) at their BASELINE.json configs, one JSON line per pipeline.

bench.py measures the headline metric (local_laplacian 4K); this script times the remaining entry points of
libhlmi.so the same way — inputs resident in HBM, calls through the C ABI, `benchmark()`-style best-of-samples of
`iters` back-to-back calls + device sync (tools/halide_benchmark.h:165-241 of the reference) — and prices each
against the roofline that bounds it: HBM bytes for the stencil pipelines, fp32 VALU for
nl_means, bf16 / f32 matrix-core flops for conv_layer.

    python bench_apps.py [--only name,name] [--samples 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md
VALU_F32_PEAK_TF = 157.3       # packed-FMA vector peak
MFMA_BF16_PEAK_TF = 2500.0     # dense
MFMA_F32_PEAK_TF = 157.3
MFMA_I8_PEAK_TOPS = 5000.0     # dense: twice the bf16 rate (MI355X_MICROARCH.md, the I8 row of the MFMA table)
VALU_F64_PEAK_TF = 78.6        # the vendor's published f64 vector figure; scripts/ubench/valu_f64.hip measures the issue rate behind it


def cpu_time(fn, budget_s=4.0, max_reps=8):
    """Bounded timing of one oracle call on the host cores (cpu_baseline leg only): one warm call, then repetitions until
    `budget_s` is spent.  Returns (seconds per call, calls timed)."""
    fn()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t0
        if dt > budget_s or n >= max_reps:
            return dt / n, n


def run(only=(), samples=5, sink=None, cpu=False, batched=True):
    """Times the pipelines named in `only` (all when empty) and hands one dict per pipeline to `sink` (default: print as a
    JSON line).  cpu=True adds a bounded `cpu_baseline` (the C oracle, OpenMP, kind "port") beside the BASELINE.json
    configs (bilateral_grid, nl_means, conv_layer_bf16) — bench.py's `other_configs` leg."""
    import numpy as np
    import halide_amd as hl
    if hl.device_count() < 1:   # (no torch here: its first import on a fresh box can take minutes)
        raise SystemExit("bench_apps.py needs a gfx950 device (no CPU fallback)")
    rng = np.random.default_rng(0)
    only = set(only)
    if sink is None:
        sink = lambda d: print(json.dumps(d), flush=True)

    class _A:
        pass
    args = _A()
    args.samples = samples

    def cpu_base(fn, units, unit, what):
        if not cpu:
            return {}
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import oracle_lib  # cpu_baseline leg only: the checker timed as the host-CPU reference point
        oracle_lib.set_canon(hl.canon_fma())
        sec, n = cpu_time(lambda: fn(oracle_lib))
        return {"cpu_baseline": {"value": round(units / sec / 1e6, 3), "unit": unit, "cores": os.cpu_count() or 1, "kind": "port",
                                 "ms_per_call": round(sec * 1e3, 2), "sample": f"{n} calls of {what} (C oracle, OpenMP, all host threads)"}}

    last_clock = [None]

    def timed(call, sync_buf, iters):
        call()
        sync_buf.device_sync()
        best = 1e30
        for _ in range(args.samples):
            t0 = time.perf_counter()
            for _ in range(iters):
                call()
            sync_buf.device_sync()
            best = min(best, (time.perf_counter() - t0) / iters)
        # shader clock / package power under this call pattern (0.25 s of it, untimed): per-call figures of short pipelines move with
        # the box's clock state (bench.ClockSampler)
        import bench
        with bench.ClockSampler(0) as cs:
            t_end = time.perf_counter() + 0.25
            while time.perf_counter() < t_end:
                for _ in range(iters):
                    call()
                sync_buf.device_sync()
        last_clock[0] = cs.summary()
        return best

    def timed_batched(make_call, nframes=8, rounds=6):
        """Throughput mode: `nframes` independent frames (own inputs and outputs) enqueued back to back without host
        synchronisation — on one stream, and spread over 2 / 4 frame-queue streams (halide_hip_partition_stream, as bench.py
        runs the headline pipeline); returns (seconds per frame, scheduling) of the fastest.  The single-call figure is a
        latency: two or three short dependent launches cannot fill 256 CUs, several frames side by side can."""
        if not batched:   # profiler runs (rocprofv3 over this script): one call at a time only
            return None
        calls = [make_call(i) for i in range(nframes)]
        hip = hl.hip_runtime()
        best, how = 1e30, None
        for nparts in (1, 2, 4):
            streams = [None] if nparts == 1 else [hl.partition_stream(p, nparts) for p in range(nparts)]
            if nparts > 1 and not all(streams):
                continue

            def one_round():
                for i, c in enumerate(calls):
                    hl.set_stream(streams[i % nparts])
                    c()
                hl.set_stream(None)
            one_round()
            hip.hipDeviceSynchronize()
            for _ in range(args.samples):
                t0 = time.perf_counter()
                for _ in range(rounds):
                    one_round()
                hip.hipDeviceSynchronize()
                dt = (time.perf_counter() - t0) / (rounds * nframes)
                if dt < best:
                    best, how = dt, ("1 stream, back to back" if nparts == 1 else f"{nparts} frame-queue streams")
        return best, how

    def batched_fields(tb, unit_work, peak, what):
        if tb is None:
            return {}
        t, how = tb
        return {"batched": {"ms_per_frame": round(t * 1e3, 4), "frames_in_flight": 8, "streams": how,
                            "roofline_frac": round(unit_work / t / peak, 4), "bound": what}}

    def kernels(call, sync_buf):
        hl.kernel_timing_reset()
        hl.kernel_timing(True)
        for _ in range(3):
            call()
        sync_buf.device_sync()
        hl.kernel_timing(False)
        rep = hl.kernel_timing_report()
        hl.kernel_timing_reset()
        return {k["name"]: round(k["total_ms"] / 3, 5) for k in rep}

    def emit(name, workload, t, mpx, bound, achieved, peak, unit, extra):
        sink({"pipeline": name, "workload": workload, "ms_per_call": round(t * 1e3, 4),
              "value": round(mpx / t / 1e6, 1), "unit": "Mpx/s",
              "roofline": {"bound": bound, "achieved": round(achieved, 1), "peak": peak, "unit": unit,
                           "frac": round(achieved / peak, 4)}, "clock_state": last_clock[0], **extra})

    # ---- the practical HBM ceiling: copy / read / write kernels over 1 GiB buffers (4x the MALL)
    copy_gbs = [None]   # this run's device copy rate, for the blocks that state their rate as a fraction of it
    if not only or "membench" in only:
        m = hl.membench(1 << 30, 10)
        copy_gbs[0] = m["copy_gbs"]
        sink({"pipeline": "membench", "workload": "grid-stride float4 kernels over 1 GiB buffers, HIP events over 10 launches",
              "copy_gbs": round(m["copy_gbs"], 1), "read_gbs": round(m["read_gbs"], 1),
              "write_gbs": round(m["write_gbs"], 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
              "copy_frac_of_peak": round(m["copy_gbs"] / HBM_PEAK_GBS, 4)})

    # ---- the headline pipeline on the other inputs SURVEY.md §8(d) lists for configs[2] (bench.py uses the smooth synthetic
    #      frame): uniform full-range noise — the worst case for the data-dependent plane gathers of the up pass — and
    #      7680x4320; one stream, one frame at a time
    if not only or "local_laplacian" in only:
        for tag, (W, H), kind in (("uniform noise 3840x2160", (3840, 2160), "uniform"), ("smooth 7680x4320", (7680, 4320), "smooth"),
                                  ("uniform noise 7680x4320", (7680, 4320), "uniform")):
            if kind == "uniform":
                img = rng.integers(0, 65536, (3, H, W), dtype=np.uint16)
            else:
                yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
                base = (np.sin(xx / 311.0) + np.cos(yy / 173.0) + np.sin((xx + yy) / 97.0) + 3.3) / 6.6
                img = np.clip(np.stack([base * 65535.0, np.roll(base, 64, 1) * 52000.0, base[::-1] * 46000.0]) +
                              rng.normal(0.0, 900.0, (3, H, W)).astype(np.float32), 0, 65535).astype(np.uint16)
            a, o = hl.Buffer(img), hl.Buffer(np.zeros_like(img))
            call = lambda: hl.local_laplacian(a, 8, 1.0 / 7.0, 1.0, o)
            t = timed(call, o, 20)
            emit("local_laplacian", f"apps/local_laplacian J=8 levels=8, u16 RGB, {tag}, 1 stream", t, W * H, "hbm",
                 12.0 * W * H / t / 1e9, HBM_PEAK_GBS, "GB/s", {"alg_bytes": 12 * W * H})

    # ---- configs[0]: blur 3x3, u16 1536x2560 (input 1538x2562)
    if not only or "blur" in only:
        W, H = 1536, 2560
        a = hl.Buffer(rng.integers(0, 65536, (H + 2, W + 2), dtype=np.uint16))
        o = hl.Buffer(np.zeros((H, W), np.uint16))
        call = lambda: hl.halide_blur(a, o)
        t = timed(call, o, 50)
        emit("halide_blur", "apps/blur 3x3 box, u16 1536x2560", t, W * H, "hbm", 4.0 * W * H / t / 1e9, HBM_PEAK_GBS, "GB/s",
             {"alg_bytes": 4 * W * H, "kernels_ms": kernels(call, o)})

    # ---- configs[1]: bilateral_grid f32 1920x1080, r_sigma 0.1
    if not only or "bilateral_grid" in only:
        W, H = 1920, 1080
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        img = (0.5 + 0.25 * np.sin(xx / 97.0) * np.cos(yy / 61.0) + 0.2 * (xx > W / 2) + rng.normal(0, 0.03, (H, W))).clip(0, 1)
        a, o = hl.Buffer(img.astype(np.float32)), hl.Buffer(np.zeros((H, W), np.float32))
        call = lambda: hl.bilateral_grid(a, 0.1, o)
        t = timed(call, o, 50)
        img32 = img.astype(np.float32)

        def mk_bg(i):
            ai, oi = hl.Buffer(np.roll(img32, 17 * i, 1).copy()), hl.Buffer(np.zeros((H, W), np.float32))
            return lambda: hl.bilateral_grid(ai, 0.1, oi)
        tb = timed_batched(mk_bg)
        emit("bilateral_grid", "apps/bilateral_grid f32 1920x1080 s_sigma=8 r_sigma=0.1", t, W * H, "hbm",
             8.0 * W * H / t / 1e9, HBM_PEAK_GBS, "GB/s",
             {"alg_bytes": 8 * W * H, "kernels_ms": kernels(call, o), **batched_fields(tb, 8.0 * W * H / 1e9, HBM_PEAK_GBS, "hbm"),
              **cpu_base(lambda ol: ol.bilateral_grid(img32, 0.1), W * H, "Mpx/s", "1920x1080 f32")})

    # ---- stencil_chain u16 1536x2560, 32 stages
    if not only or "stencil_chain" in only:
        W, H = 1536, 2560
        a = hl.Buffer(rng.integers(0, 65536, (H, W), dtype=np.uint16))
        o = hl.Buffer(np.zeros((H, W), np.uint16))
        call = lambda: hl.stencil_chain(a, o)
        t = timed(call, o, 20)
        # Priced on the operations the kernel EXECUTES: the separable 5 + 5 form is 10 u16 multiply-adds per pixel and stage
        # (the reference's 25-tap form would be 2.5x more), over the 128 x 128 register window of a tile whose 8 fused stages
        # leave 96 x 96 outputs (1.78x halo recomputation; the LDS-window kernel, HLMI_SC_LDS=1: 128 x 96 -> 96 x 64, 2.0x) = 569
        # executed multiply-adds per output pixel; bound: the packed 16-bit integer VALU rate (v_pk_mad_u16: 2 MACs per lane
        # and clock = the packed-f32 figure).  Next to it the figure on the ALGORITHMIC count (32 stages x 25 taps = 1600 MACs
        # per pixel) and the fraction of the HBM roofline SURVEY.md §8(d) assigns the pipeline (4 B/px: read + write once).
        halo = (128.0 * 128.0) / (96.0 * 96.0)
        ops_exec = 2.0 * 32 * 10 * halo * W * H
        ops_alg = 2.0 * 1600 * W * H
        sc_src = rng.integers(0, 65536, (H, W), dtype=np.uint16)

        def mk_sc(i):
            ai, oi = hl.Buffer(np.roll(sc_src, 13 * i, 1).copy()), hl.Buffer(np.zeros((H, W), np.uint16))
            return lambda: hl.stencil_chain(ai, oi)
        tb = timed_batched(mk_sc, rounds=3)
        emit("stencil_chain", "apps/stencil_chain 32 stages 5x5, u16 1536x2560", t, W * H, "valu", ops_exec / t / 1e12,
             VALU_F32_PEAK_TF, "TOP/s (u16, packed, executed)",
             {"executed_ops": ops_exec, "halo_recompute": halo, "alg_ops": ops_alg,
              "alg_ops_frac": round(ops_alg / t / 1e12 / VALU_F32_PEAK_TF, 4), "alg_bytes": 4 * W * H,
              "hbm_gbs": 4.0 * W * H / t / 1e9, "hbm_frac": round(4.0 * W * H / t / 1e9 / HBM_PEAK_GBS, 4),
              "kernels_ms": kernels(call, o), **batched_fields(tb, ops_exec / 1e12, VALU_F32_PEAK_TF, "valu")})

    # ---- camera_pipe 2592x1968 raw -> 2560x1920x3 u8
    if not only or "camera_pipe" in only:
        IW, IH, OW, OH = 2592, 1968, 2560, 1920
        raw = hl.Buffer(rng.integers(0, 1024, (IH, IW), dtype=np.uint16))
        m3 = hl.Buffer(np.array([[1.6697, -0.2693, -0.4004, -42.4346], [-0.3576, 1.0615, 1.5949, -37.1158],
                                 [-0.2175, -1.8751, 6.9640, -26.6970]], np.float32))
        m7 = hl.Buffer(np.array([[2.2997, -0.4478, 0.1706, -39.0923], [-0.3826, 1.5906, -0.2080, -25.4311],
                                 [-0.0888, -0.7344, 2.2832, -20.0826]], np.float32))
        o = hl.Buffer(np.zeros((3, OH, OW), np.uint8))
        call = lambda: hl.camera_pipe(raw, m3, m7, 3700.0, 2.0, 50.0, 1.0, 25, 1023, o)
        t = timed(call, o, 50)
        cp_src = rng.integers(0, 1024, (IH, IW), dtype=np.uint16)

        def mk_cp(i):
            ri, oi = hl.Buffer(np.roll(cp_src, 2 * i, 1).copy()), hl.Buffer(np.zeros((3, OH, OW), np.uint8))
            return lambda: hl.camera_pipe(ri, m3, m7, 3700.0, 2.0, 50.0, 1.0, 25, 1023, oi)
        tb = timed_batched(mk_cp)
        # the same call on a raw frame with spatial structure (a smooth scene under the Bayer mosaic + sensor noise): the tone-curve
        # look-ups of neighbouring pixels then mostly share LDS words, where the uniform-noise frame above (what RunGen's benchmark
        # fills its inputs with) makes every one of them a bank conflict lottery
        yy, xx = np.mgrid[0:IH, 0:IW].astype(np.float32)
        scene = (np.sin(xx / 173.0) + np.cos(yy / 97.0) + np.sin((xx + yy) / 311.0) + 3.2) / 6.4
        gain = np.where((yy % 2 == 0) & (xx % 2 == 1), 0.6, np.where((yy % 2 == 1) & (xx % 2 == 0), 0.5, 1.0))   # R and B sites darker than G
        raw_scene = hl.Buffer(np.clip(scene * gain * 900.0 + 40.0 + rng.normal(0.0, 6.0, (IH, IW)), 0, 1023).astype(np.uint16))
        t_scene = timed(lambda: hl.camera_pipe(raw_scene, m3, m7, 3700.0, 2.0, 50.0, 1.0, 25, 1023, o), o, 50)
        emit("camera_pipe", "apps/camera_pipe u16 2592x1968 -> u8 2560x1920x3", t, OW * OH, "hbm", 5.0 * OW * OH / t / 1e9,
             HBM_PEAK_GBS, "GB/s", {"alg_bytes": 5 * OW * OH, "kernels_ms": kernels(call, o), "input": "uniform 10-bit noise",
                                   "ms_per_call_scene_input": round(t_scene * 1e3, 4),
                                   **batched_fields(tb, 5.0 * OW * OH / 1e9, HBM_PEAK_GBS, "hbm")})

    # ---- configs[3]: nl_means 7x7 / 7x7, f32 1920x1080x3 (one frame per call; frames of a batch are independent)
    if not only or "nl_means" in only:
        W, H = 1920, 1080
        nlm_in = rng.random((3, H, W), dtype=np.float32)
        a = hl.Buffer(nlm_in)
        o = hl.Buffer(np.zeros((3, H, W), np.float32))
        call = lambda: hl.nl_means(a, 7, 7, 0.12, o)
        t = timed(call, o, 10)
        flops = 2200.0 * W * H       # ~49 offsets x ~45 flops per pixel

        def mk_nlm(i):
            ai, oi = hl.Buffer(np.roll(nlm_in, 13 * i, 2).copy()), hl.Buffer(np.zeros((3, H, W), np.float32))
            return lambda: hl.nl_means(ai, 7, 7, 0.12, oi)
        tb = timed_batched(mk_nlm, rounds=2)
        emit("nl_means", "apps/nl_means patch 7 search 7 sigma 0.12, f32 1920x1080x3", t, W * H, "valu",
             flops / t / 1e12, VALU_F32_PEAK_TF, "TFLOP/s",
             {"alg_flops": flops, "alg_bytes": 24 * W * H, "kernels_ms": kernels(call, o),
              **batched_fields(tb, flops / 1e12, VALU_F32_PEAK_TF, "valu"),
              **cpu_base(lambda ol: ol.nl_means(nlm_in, 7, 7, 0.12), W * H, "Mpx/s", "1920x1080x3 f32, patch 7 search 7")})

    # ---- unsharp f32 1536x2560x3 (generator estimates)
    if not only or "unsharp" in only:
        W, H = 1536, 2560
        a = hl.Buffer((rng.random((3, H, W), dtype=np.float32) * 0.9 + 0.05).astype(np.float32))
        o = hl.Buffer(np.zeros((3, H, W), np.float32))
        call = lambda: hl.unsharp(a, o)
        t = timed(call, o, 50)
        emit("unsharp", "apps/unsharp sigma=1.5, f32 1536x2560x3", t, W * H, "hbm", 24.0 * W * H / t / 1e9, HBM_PEAK_GBS, "GB/s",
             {"alg_bytes": 24 * W * H, "kernels_ms": kernels(call, o)})

    # ---- max_filter f32 1536x2560x3 (generator estimates).  LDS bound.  `lds_bytes` is the ALGORITHMIC sample count, not the bytes the
    # LDS moves: every output folds 55 footprint rows x 2 four-byte samples (440 B) and the four doubling slices of a 64x64 tile's 120
    # staged rows are written once each (15 chunks x 4 x 1024 words x 4 B / 4096 outputs = 60 B).  With 16 output rows per lane a lane's
    # outputs share sample reads (about 70 LDS read instructions per output row of eight, max_filter.hip), so the instructions issued
    # move fewer bytes than this figure: `frac` is the algorithmic sample rate against the ds_read_b32 rate of 128 B/clk/CU
    # (MI355X_MICROARCH.md, LDS table), an upper bound on the LDS utilisation, and is labelled that way.
    if not only or "max_filter" in only:
        W, H = 1536, 2560
        a = hl.Buffer(rng.random((3, H, W), dtype=np.float32))
        o = hl.Buffer(np.zeros((3, H, W), np.float32))
        call = lambda: hl.max_filter(a, o)
        t = timed(call, o, 20)
        lds_bytes = (440.0 + 60.0) * 3 * W * H
        emit("max_filter", "apps/max_filter radius 26, f32 1536x2560x3", t, W * H, "lds", lds_bytes / t / 1e9, 256 * 128 * 2.4, "GB/s",
             {"alg_bytes": 24 * W * H, "hbm_gbs": 24.0 * W * H / t / 1e9, "lds_bytes": lds_bytes,
              "lds_bytes_are": "algorithmic samples (440 B read + 60 B written per output), not LDS instructions issued: shared reads make the real traffic smaller",
              "kernels_ms": kernels(call, o)})

    # ---- hist u8 1536x2560x3 (generator estimates)
    if not only or "hist" in only:
        W, H = 1536, 2560
        a = hl.Buffer(rng.integers(0, 256, (3, H, W), dtype=np.uint8))
        o = hl.Buffer(np.zeros((3, H, W), np.uint8))
        call = lambda: hl.hist(a, o)
        t = timed(call, o, 50)
        emit("hist", "apps/hist histogram equalisation, u8 1536x2560x3", t, W * H, "hbm", 9.0 * W * H / t / 1e9, HBM_PEAK_GBS, "GB/s",
             {"alg_bytes": 9 * W * H, "kernels_ms": kernels(call, o)})

    # ---- harris f32 1536x2560x3 -> 1530x2554 (generator estimates)
    if not only or "harris" in only:
        W, H = 1536, 2560
        a = hl.Buffer(rng.random((3, H, W), dtype=np.float32))
        o = hl.Buffer(np.zeros((H - 6, W - 6), np.float32)).set_min(3, 3)
        call = lambda: hl.harris(a, o)
        t = timed(call, o, 50)
        emit("harris", "apps/harris corner response, f32 1536x2560x3 -> 1530x2554", t, (W - 6) * (H - 6), "hbm", 16.0 * W * H / t / 1e9,
             HBM_PEAK_GBS, "GB/s", {"alg_bytes": 16 * W * H, "kernels_ms": kernels(call, o)})

    # ---- interpolate f32 1536x2560x4 -> x3 (generator estimates)
    if not only or "interpolate" in only:
        W, H = 1536, 2560
        img = rng.random((4, H, W), dtype=np.float32)
        img[3][rng.random((H, W)) < 0.4] = 0.0
        a = hl.Buffer(img)
        o = hl.Buffer(np.zeros((3, H, W), np.float32))
        call = lambda: hl.interpolate(a, o)
        t = timed(call, o, 20)
        emit("interpolate", "apps/interpolate 10-level pull-push, f32 1536x2560x4 -> x3", t, W * H, "hbm", 28.0 * W * H / t / 1e9,
             HBM_PEAK_GBS, "GB/s", {"alg_bytes": 28 * W * H, "kernels_ms": kernels(call, o)})

    # ---- iir_blur f32 1536x2560x3, alpha 0.1 (the shape the generator pins)
    if not only or "iir_blur" in only:
        W, H = 1536, 2560
        a = hl.Buffer(rng.random((3, H, W), dtype=np.float32))
        o = hl.Buffer(np.zeros((3, H, W), np.float32))
        call = lambda: hl.iir_blur(a, 0.1, o)
        t = timed(call, o, 10)
        emit("iir_blur", "apps/iir_blur alpha=0.1, f32 1536x2560x3", t, W * H, "hbm", 24.0 * W * H / t / 1e9, HBM_PEAK_GBS, "GB/s",
             {"alg_bytes": 24 * W * H, "kernels_ms": kernels(call, o),
              "note": "bound by the sequential recurrence: 2 (W + H) dependent multiply-add steps per scan line"})

    # ---- resize: the reference's two configurations (apps/resize/Makefile:53-79: 0.5 down on the full image, 4.0 up on the image reduced
    #      by 0.125) at this project's usual size, every kernel and type, and 3840x2160 u8 cubic x 0.5.  Roofline: compulsory HBM bytes
    #      (input read once + output written once).  Each line also times the same call on the general two-launch path
    #      (hlmi_resize_general): the fused path must not be slower.  `--only resize` selects all of them, a variant's name that one.
    if not only or any(n.startswith("resize") for n in only):
        shapes = {"1536x2560 x0.5": (1536, 2560, 0.5), "192x320 x4": (192, 320, 4.0), "3840x2160 x0.5": (3840, 2160, 0.5)}
        cases = [(k, t, tag) for tag in ("1536x2560 x0.5", "192x320 x4") for k in hl.RESIZE_KERNELS for t in ("uint8", "uint16", "float32")]
        cases.append(("cubic", "uint8", "3840x2160 x0.5"))
        for kernel, tname, tag in cases:
            W, H, scale = shapes[tag]
            name = f"resize_{kernel}_{tname}_{'up' if scale > 1 else 'down'}"
            if only and "resize" not in only and name not in only:
                continue
            dt = np.dtype(tname)
            img = rng.random((3, H, W), dtype=np.float32) if tname == "float32" else rng.integers(0, np.iinfo(dt).max + 1, (3, H, W)).astype(dt)
            ow, oh = int(np.float32(W) * np.float32(scale)), int(np.float32(H) * np.float32(scale))
            a, o = hl.Buffer(img), hl.Buffer(np.zeros((3, oh, ow), dt))
            call = lambda: hl.resize(a, scale, o, kernel)
            general = lambda: hl.debug_resize_general(name, a, scale, o)
            iters = 50
            t = timed(call, o, iters)
            clock = last_clock[0]
            tg = timed(general, o, iters)
            last_clock[0] = clock
            nbytes = dt.itemsize * 3 * (W * H + ow * oh)
            emit(name, f"apps/resize {kernel} {tname} {tag}, 3 channels", t, ow * oh, "hbm", nbytes / t / 1e9, HBM_PEAK_GBS, "GB/s",
                 {"alg_bytes": nbytes, "kernels_ms": kernels(call, o), "general_path": {"ms_per_call": round(tg * 1e3, 4), "kernels_ms": kernels(general, o)},
                  "fused_not_slower": bool(t <= tg)})

    # ---- gaussian_blur: the reference's own invocation (apps/gaussian_blur/Makefile: sigma 10 on the app image) at this project's usual
    #      size, f32 1536x2560: the direct blur at trunc 3, 4, 5 and three resampled variants at trunc 5.  Bounds: direct, 2 (2 R + 1) fused
    #      operations per pixel at the f32 vector peak (its 16 B/px of HBM traffic with the f32 intermediate is reported beside it); the
    #      variants, the compulsory 8 B/px.  Each line also times the same call with its blur passes on the general path
    #      (hlmi_gaussian_blur_general).  `--only gaussian_blur` selects all of them, an entry point's name that one.
    if not only or any(n.startswith("gaussian_blur") for n in only):
        W, H, sigma = 1536, 2560, 10.0
        img = rng.random((H, W), dtype=np.float32)
        a, o = hl.Buffer(img), hl.Buffer(hl.aligned_array((H, W)))
        cases = [("gaussian_blur_direct", t) for t in (3, 4, 5)] + [(hl.gaussian_blur_variant(*v), 5) for v in ((3, 2, 8), (2, 1, 2), (4, 3, 16))]
        for name, trunc in cases:
            if only and "gaussian_blur" not in only and name not in only:
                continue
            fn = hl._fn[name]
            call = lambda: hl._check(fn(a.ptr, sigma, trunc, o.ptr))
            general = lambda: hl.debug_gaussian_blur_general(name, a, sigma, trunc, o)
            iters = 50
            t = timed(call, o, iters)
            clock = last_clock[0]
            tg = timed(general, o, iters)
            last_clock[0] = clock
            extra = {"kernels_ms": kernels(call, o), "general_path": {"ms_per_call": round(tg * 1e3, 4), "kernels_ms": kernels(general, o)},
                     "tiled_over_general": round(t / tg, 4)}
            if name == "gaussian_blur_direct":
                radius = int(np.ceil(np.float32(trunc) * np.float32(sigma)))
                flops = 2.0 * 2 * (2 * radius + 1) * W * H
                emit(name, f"apps/gaussian_blur direct sigma={sigma:g} trunc={trunc} (radius {radius}), f32 1536x2560", t, W * H, "valu",
                     flops / t / 1e12, VALU_F32_PEAK_TF, "TFLOP/s",
                     {"alg_flops": flops, "alg_bytes": 16 * W * H, "hbm_gbs": round(16.0 * W * H / t / 1e9, 1),
                      "hbm_frac": round(16.0 * W * H / t / 1e9 / HBM_PEAK_GBS, 4), **extra})
            else:
                emit(name, f"apps/gaussian_blur {name[14:]} sigma={sigma:g} trunc={trunc}, f32 1536x2560", t, W * H, "hbm",
                     8.0 * W * H / t / 1e9, HBM_PEAK_GBS, "GB/s", {"alg_bytes": 8 * W * H, **extra})

    # ---- linear_blur / simple_blur: f32 1536x2560x4, the generator's estimate (apps/linear_blur/linear_blur_generator.cpp:20-21).  Roofline:
    #      the compulsory 8 B per value.  Each line also times the same call as the unfused composition (hlmi_linear_blur_general: three
    #      launches and three times the bytes for linear_blur, one launch with nine global taps for simple_blur): the one-launch path must
    #      not be slower.  linear_blur is bound by VALU issue, not by bytes: its line adds the VALU instructions lb_fused issues per output
    #      value, counted in its disassembly (scripts/asm_hist.sh halide_amd/csrc/linear_blur.hip lb_fusedILb1; per workgroup of 4 waves
    #      and 2048 outputs: 4 x 23 set-up + 34 staged rows x 55 + 2 edge columns x 80 + 4 x (76 + 7 x 65) output rows = 4246 wave
    #      instructions for 32 wave-rows of outputs), and the time that count takes at 2 cycles per wave64 instruction on each of
    #      256 x 4 SIMDs at 2.4 GHz.  The count is STATIC: taken once from the code object that hipcc 7.2.26015 (AMD clang 22.0.0git, roc-7.2.0)
    #      makes of linear_blur.hip as it stood when this block was added (688 VALU instructions in lb_fused<true>, 21 VGPRs); the line
    #      names that source in `valu_count_source`.  Count again after a change to the kernel or the compiler.
    if not only or "linear_blur" in only or "simple_blur" in only:
        W, H, NC = 1536, 2560, 4
        LB_TILE, LB_FUSED_VALU_PER_WORKGROUP = (64, 32), 4246   # linear_blur.hip: TW x TH, and the count above
        a, o = hl.Buffer(rng.random((NC, H, W), dtype=np.float32)), hl.Buffer(np.zeros((NC, H, W), np.float32))
        a.copy_to_device()
        for name in ("linear_blur", "simple_blur"):
            if only and name not in only:
                continue
            call = (lambda: hl.linear_blur(a, o)) if name == "linear_blur" else (lambda: hl.simple_blur(a, W, H, o))
            general = lambda: hl.debug_linear_blur_general(name, a, W, H, o)
            iters = 50
            t = timed(call, o, iters)
            clock = last_clock[0]
            tg = timed(general, o, iters)
            last_clock[0] = clock
            nbytes = 8 * W * H * NC
            extra = {"alg_bytes": nbytes, "kernels_ms": kernels(call, o), "general_path": {"ms_per_call": round(tg * 1e3, 4), "kernels_ms": kernels(general, o)},
                     "fused_not_slower": bool(t <= tg)}
            if name == "linear_blur":
                valu = LB_FUSED_VALU_PER_WORKGROUP / (LB_TILE[0] * LB_TILE[1] / 64.0)
                issue_s = W * H * NC / 64.0 * valu * 2.0 / (256 * 4 * 2.4e9)
                extra.update({"valu_per_output": round(valu, 1), "valu_issue_bound_ms": round(issue_s * 1e3, 4), "valu_issue_frac": round(issue_s / t, 4),
                              "conversions_per_output": round((LB_TILE[0] + 2) * (LB_TILE[1] + 2) / float(LB_TILE[0] * LB_TILE[1]), 4),
                              "valu_count_source": "static count in the disassembly of lb_fused<true>, hipcc 7.2.26015, 64 x 32 tile; not re-derived by this run"})
            emit(name, f"apps/linear_blur {name}, f32 {W}x{H}x{NC}", t, W * H, "hbm", nbytes / t / 1e9, HBM_PEAK_GBS, "GB/s", extra)

    # ---- wavelet: haar_x, inverse_haar_x, daubechies_x, inverse_daubechies_x on f32 1536x2560, the size of apps/images/gray.png that the
    #      reference's test feeds apps/wavelet/wavelet.cpp, and on 7680x4320, whose bytes do not fit the on-die caches.  The transform is
    #      (W / 2, H, 2), as the driver allocates it.  Roofline: the compulsory 8 B per sample, which is what a device copy moves, so the
    #      yardstick is membench's copy rate of the same run.  Each line also times the same call with one thread per output and
    #      per-tap clamped scalar loads (hlmi_wavelet_general): the default path must not be slower.
    if not only or "wavelet" in only or only & {"haar_x", "inverse_haar_x", "daubechies_x", "inverse_daubechies_x"}:
        for W, H in ((1536, 2560), (7680, 4320)):
            img, tr = hl.Buffer(rng.random((H, W), dtype=np.float32)), hl.Buffer(rng.random((2, H, W // 2), dtype=np.float32))
            img_out, tr_out = hl.Buffer(np.zeros((H, W), np.float32)), hl.Buffer(np.zeros((2, H, W // 2), np.float32))
            img.copy_to_device()
            tr.copy_to_device()
            for name in ("haar_x", "inverse_haar_x", "daubechies_x", "inverse_daubechies_x"):
                if only and "wavelet" not in only and name not in only:
                    continue
                a, o = (tr, img_out) if name.startswith("inverse_") else (img, tr_out)
                fn = getattr(hl, name)
                call = lambda: fn(a, o)
                general = lambda: hl.debug_wavelet_general(name, a, o)
                iters = 50 if W == 1536 else 20
                t = timed(call, o, iters)
                clock = last_clock[0]
                tg = timed(general, o, iters)
                last_clock[0] = clock
                nbytes = 8 * W * H
                emit(name, f"apps/wavelet {name}, f32 {W}x{H}", t, W * H, "hbm", nbytes / t / 1e9, HBM_PEAK_GBS, "GB/s",
                     {"alg_bytes": nbytes, "kernels_ms": kernels(call, o), "general_path": {"ms_per_call": round(tg * 1e3, 4), "kernels_ms": kernels(general, o)},
                      "fused_not_slower": bool(t <= tg)})

    # ---- reaction_diffusion: the app's own 1024x1024x3 state (apps/HelloWasm/app/core.cpp) and 4096x4096x3, whose 201 MB do not fit the
    #      on-die caches: one update, render, update + render, and hlmi_reaction_diffusion_run of 16 steps under each steps-per-launch
    #      instance (HLMI_RD_STEPS_PER_LAUNCH = 1, 2, 4) and under the hook (one thread per output, one launch per step).  Compulsory
    #      traffic: 24 B/px per update, 16 B/px per render; the yardstick is membench's copy rate of the same run.
    if not only or "reaction_diffusion" in only:
        for W, H in ((1024, 1024), (4096, 4096)):
            s, n = hl.Buffer(rng.random((3, H, W), dtype=np.float32)), hl.Buffer(np.zeros((3, H, W), np.float32))
            pix = hl.Buffer(np.zeros((H, W), np.uint32))
            s.copy_to_device()
            mouse = (W // 2, H // 2)
            iters = 50 if W == 1024 else 10

            def line(name, what, call, general, out, nbytes, extra=None):
                t = timed(call, out, iters)
                clock = last_clock[0]
                tg = timed(general, out, iters)
                last_clock[0] = clock
                emit(name, f"apps/HelloWasm {what}, f32 {W}x{H}x3", t, W * H, "hbm", nbytes / t / 1e9, HBM_PEAK_GBS, "GB/s",
                     {"alg_bytes": nbytes, "kernels_ms": kernels(call, out), "general_path": {"ms_per_call": round(tg * 1e3, 4), "kernels_ms": kernels(general, out)},
                      "fused_not_slower": bool(t <= tg), **(extra or {})})

            line("reaction_diffusion_update", "reaction_diffusion_update", lambda: hl.reaction_diffusion_update(s, *mouse, 7, n),
                 lambda: hl.debug_reaction_diffusion_general("reaction_diffusion_update", s, *mouse, 7, out=n), n, 24 * W * H)
            line("reaction_diffusion_render", "reaction_diffusion_render", lambda: hl.reaction_diffusion_render(s, pix),
                 lambda: hl.debug_reaction_diffusion_general("reaction_diffusion_render", s, render=pix), pix, 16 * W * H)
            line("reaction_diffusion_update_render", "reaction_diffusion_update + reaction_diffusion_render, two calls against run of one step",
                 lambda: hl.reaction_diffusion_run(s, *mouse, 7, 1, n, pix),
                 lambda: (hl.reaction_diffusion_update(s, *mouse, 7, n), hl.reaction_diffusion_render(n, pix)), pix, 28 * W * H)
            before = os.environ.get("HLMI_RD_STEPS_PER_LAUNCH")
            try:
                for S in ("plan", 1, 2, 4):
                    if S == "plan":
                        os.environ.pop("HLMI_RD_STEPS_PER_LAUNCH", None)
                    else:
                        os.environ["HLMI_RD_STEPS_PER_LAUNCH"] = str(S)
                    for with_render in (False, True):
                        r = pix if with_render else None
                        line(f"reaction_diffusion_run16_{S}{'_render' if with_render else ''}",
                             f"hlmi_reaction_diffusion_run, 16 steps, steps per launch {S}{', rendered' if with_render else ''}",
                             lambda: hl.reaction_diffusion_run(s, *mouse, 7, 16, n, r),
                             lambda: hl.debug_reaction_diffusion_general("run", s, *mouse, 7, 16, n, r), n, (16 * 24 + (4 if with_render else 0)) * W * H,
                             {"steps": 16, "steps_per_launch": S})
            finally:
                if before is None:
                    os.environ.pop("HLMI_RD_STEPS_PER_LAUNCH", None)
                else:
                    os.environ["HLMI_RD_STEPS_PER_LAUNCH"] = before

    # ---- compositing: six u8 RGBA layers and five op codes at 1536x2560 (the generator's estimate and the size of the image the
    #      reference's test feeds apps/compositing/process.cpp) and at 7680x4320, with the driver's blobs and op codes {4, 3, 2, 1, 0}
    #      (process.cpp:33-51) over a noise input.  Compulsory traffic: 24 B/px read, 4 B/px written; the yardstick is membench's copy
    #      rate of the same run over those 28 B/px (`of_copy_rate`, absent when membench is not part of the run).  Whether bytes or
    #      integer VALU issue bounds it is what the line is there to show.  It also times the same call with one thread per pixel and
    #      byte loads (hlmi_compositing_general): the default path must not be slower.
    if not only or "compositing" in only:
        for W, H in ((1536, 2560), (7680, 4320)):
            xs, ys = np.arange(W)[None, :], np.arange(H)[:, None]
            layers = [hl.Buffer(rng.integers(0, 256, (4, H, W), dtype=np.uint8))]
            for i in range(5):
                cx, cy = int(np.cos(i * 2 * np.pi / 5) * 300 + W // 2), int(np.sin(i * 2 * np.pi / 5) * 300 + H // 2)
                blob = np.empty((4, H, W), np.uint8)
                g = ((255 // 3) * i) & 255   # stored into a uint8 by the driver: 340 wraps to 84
                blob[0], blob[1], blob[2] = 255, g, 255 - g
                blob[3] = np.minimum(255, np.minimum(np.maximum(0, 500 - np.abs(xs - cx)), np.maximum(0, 500 - np.abs(ys - cy))))
                layers.append(hl.Buffer(blob))
            ops, o = hl.Buffer(np.array([4, 3, 2, 1, 0], np.int32)), hl.Buffer(np.zeros((4, H, W), np.uint8))
            for b in layers + [ops]:
                b.copy_to_device()
            call = lambda: hl.compositing(layers, ops, o)
            general = lambda: hl.debug_compositing_general(layers, ops, o)
            iters = 50 if W == 1536 else 10
            t = timed(call, o, iters)
            clock = last_clock[0]
            tg = timed(general, o, iters)
            last_clock[0] = clock
            nbytes = 28 * W * H
            extra = {"alg_bytes": nbytes, "kernels_ms": kernels(call, o),
                     "general_path": {"ms_per_call": round(tg * 1e3, 4), "kernels_ms": kernels(general, o)}, "fused_not_slower": bool(t <= tg)}
            if copy_gbs[0]:
                extra["of_copy_rate"] = round(nbytes / t / 1e9 / copy_gbs[0], 4)
            emit("compositing", f"apps/compositing, six u8 RGBA layers {W}x{H}, ops 4 3 2 1 0", t, W * H, "hbm", nbytes / t / 1e9, HBM_PEAK_GBS, "GB/s", extra)

    # ---- hexagon_benchmarks: the six u8 stencils at 1024x1024 (the size apps/hexagon_benchmarks/process.cpp runs them at) and at
    #      7680x4320, noise under the driver's mask (process.h).  Compulsory traffic: 1 B/px read, 1 B/px written; the yardstick is
    #      membench's copy rate of the same run over those 2 B/px (`of_copy_rate`, absent when membench is not part of the run),
    #      which at such a rate is some 3 Tpx/s: whether bytes or packed 16-bit VALU issue bounds a filter is what the lines are there
    #      to show.  Each also times the same call with one thread per pixel and clamped byte taps (hlmi_hexagon_benchmarks_general):
    #      the default path must not be slower.
    if not only or "hexagon_benchmarks" in only:
        for W, H in ((1024, 1024), (7680, 4320)):
            a, o = hl.Buffer(rng.integers(0, 256, (H, W), dtype=np.uint8)), hl.Buffer(np.zeros((H, W), np.uint8))
            mask = hl.Buffer(np.array([[1, -4, 7], [2, -5, 8], [3, -6, 9]], np.int8))
            a.copy_to_device()
            for name in hl.HEXAGON_BENCHMARKS:
                m = mask if name.startswith("conv3x3") else None
                call = (lambda f=getattr(hl, name), m=m: f(a, m, o)) if m is not None else (lambda f=getattr(hl, name): f(a, o))
                general = lambda name=name, m=m: hl.debug_hexagon_benchmarks_general(name, a, m, o)
                iters = 200 if W == 1024 else 20
                t = timed(call, o, iters)
                clock = last_clock[0]
                tg = timed(general, o, iters)
                last_clock[0] = clock
                nbytes = 2 * W * H
                k, kg = kernels(call, o), kernels(general, o)
                extra = {"alg_bytes": nbytes, "kernels_ms": k, "gpx_per_s": round(W * H / t / 1e9, 2),
                         "general_path": {"ms_per_call": round(tg * 1e3, 4), "kernels_ms": kg}, "fused_not_slower": bool(t <= tg),
                         "kernel_not_slower": bool(sum(k.values()) <= sum(kg.values()))}
                if copy_gbs[0]:
                    extra["of_copy_rate"] = round(nbytes / t / 1e9 / copy_gbs[0], 4)
                    extra["kernel_of_copy_rate"] = round(nbytes / (sum(k.values()) * 1e-3) / 1e9 / copy_gbs[0], 4)
                emit(name, f"apps/hexagon_benchmarks {name}, u8 {W}x{H}, noise" + (", the driver's mask" if m is not None else ""), t, W * H, "hbm",
                     nbytes / t / 1e9, HBM_PEAK_GBS, "GB/s", extra)

    # ---- mat_mul: the f32 product at 1024^2 (the size apps/cuda_mat_mul builds and its runner times beside cuBLAS) and, in the same
    #      line under "size_4096", at 4096^2.  2 n^3 flops against the f32 matrix-core peak.  Beside each: the same call with one
    #      thread per output (hlmi_mat_mul_general), which the default path must beat or the plan may not choose it, and torch.mm on
    #      the same operands in the same run, the runner's vendor-BLAS column: recorded, not thresholded.  torch.mm is not bound to the
    #      chain order, so its bits may differ from mat_mul's.
    if not only or "mat_mul" in only:
        import torch   # this block only: the runner's BLAS column
        fields = {}
        for n in (1024, 4096):
            A, B = (rng.random((n, n), dtype=np.float32) * 2 - 1 for _ in range(2))
            a, b, o = hl.Buffer(A), hl.Buffer(B), hl.Buffer(np.zeros((n, n), np.float32))
            a.copy_to_device(), b.copy_to_device()
            call = (lambda: hl.mat_mul(a, b, o)) if n == 1024 else (lambda n=n: hl.mat_mul_sized(n, a, b, o))
            general = lambda n=n: hl.debug_mat_mul_general(n, a, b, o)
            iters = 200 if n == 1024 else 10
            t = timed(call, o, iters)
            clock = last_clock[0]
            tg = timed(general, o, max(2, iters // 10))
            ta, tb_ = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
            tm = 1e30
            torch.mm(tb_, ta)
            torch.cuda.synchronize()
            for _ in range(args.samples):
                t0 = time.perf_counter()
                for _ in range(iters):
                    torch.mm(tb_, ta)   # B @ A, as mat_mul
                torch.cuda.synchronize()
                tm = min(tm, (time.perf_counter() - t0) / iters)
            del ta, tb_
            last_clock[0] = clock
            flops = 2.0 * n ** 3
            k, kg = kernels(call, o), kernels(general, o)
            fields[n] = {"ms_per_call": round(t * 1e3, 4), "tflops": round(flops / t / 1e12, 2), "mfma_frac": round(flops / t / 1e12 / MFMA_F32_PEAK_TF, 4),
                         "alg_flops": flops, "alg_bytes": 12.0 * n * n, "kernels_ms": k,
                         "general_path": {"ms_per_call": round(tg * 1e3, 4), "kernels_ms": kg}, "fast_path_faster": bool(t < tg),
                         "kernel_faster": bool(sum(k.values()) < sum(kg.values())),
                         "torch_mm_ms": round(tm * 1e3, 4), "torch_mm_tflops": round(flops / tm / 1e12, 2),
                         "torch_mm_note": "torch.mm(B, A) on the same f32 operands; not bound to the chain order, its bits may differ"}
            if n == 1024:
                t1024 = t
        extra = {k_: v for k_, v in fields[1024].items() if k_ not in ("ms_per_call",)}
        extra["size_4096"] = fields[4096]
        emit("mat_mul", "apps/cuda_mat_mul, f32 1024x1024 = B @ A as a k-ordered fmaf chain, noise in [-1, 1)", t1024, 1024 * 1024, "mfma",
             2.0 * 1024 ** 3 / t1024 / 1e12, MFMA_F32_PEAK_TF, "TFLOP/s", extra)

    # ---- hannk_conv / hannk_depthwise: the quantised convolution pair of apps/hannk's op library on MobileNet-v1 224 shapes, each at batch
    #      1 and batch 32, device-resident operands, the filter tiled once outside the timed calls.  conv: 2 * outputs * k integer ops
    #      against the dense i8 matrix-core peak; depthwise: input + output bytes against membench's copy rate of the same run.  Beside
    #      each: the same call with one thread per output (hlmi_hannk_general), which the default path must beat wherever the plan
    #      chooses it, and torch.nn.functional.conv2d in f16 on the same shape in the same run: recorded, not thresholded, and not
    #      comparable bit for bit (another arithmetic).
    def hannk_layer(kind, ci, co, k, stride, size, batch):
        import torch
        pad = k // 2
        x = rng.integers(0, 256, (batch, size, size, ci), dtype=np.uint8)
        out_size = hl.hannk_conv_out_extent(size, k, stride, 1, pad)
        bias = hl.Buffer(rng.integers(-4096, 4096, co).astype(np.int32))
        az, fz = 128, 131
        if kind == "conv":
            inp = hl.Buffer(hl.hannk_pad_input(x, az, hl.HANNK_VECTOR_REDUCTION, (pad, pad)))
            filt = hl.hannk_tile_filter(rng.integers(0, 256, (co, k, k, ci), dtype=np.uint8), fz)
            entry, extra_args = "conv_u8_u8_u8", []
            fn = hl.conv_u8_u8_u8
        else:
            inp = hl.Buffer(hl.hannk_pad_input(x, az, hl.HANNK_DEPTHWISE_VECTOR, (pad, pad)))
            filt = hl.Buffer(rng.integers(0, 256, (k, k, co), dtype=np.uint8))
            entry, extra_args = "depthwise_conv_uint8", [0]
            fn = hl.depthwise_conv_uint8
        o = hl.Buffer(np.zeros((batch, out_size, out_size, co), np.uint8))
        for b_ in (inp, filt, bias):
            b_.copy_to_device()
        q = (1518500250, 9 if kind == "conv" else 5, 128, 0, 255)
        call = lambda: fn(inp, az, filt, fz, bias, (stride, stride), (1, 1), *q, o)
        general = lambda: hl.debug_hannk_general(entry, inp, az, filt, fz, bias, stride, stride, 1, 1, *extra_args, *q, o)
        outputs = batch * out_size * out_size * co
        iters = 200 if outputs * (ci if kind == "conv" else 1) * k * k < 1 << 30 else 50
        t = timed(call, o, iters)
        clock = last_clock[0]
        tg = timed(general, o, max(2, iters // 10))
        # the same shape in f16 through torch (MIOpen / hipBLASLt), channels_last
        tx = torch.from_numpy(x).cuda().permute(0, 3, 1, 2).half().contiguous(memory_format=torch.channels_last)
        tw = torch.randn((co, 1 if kind == "depthwise" else ci, k, k), dtype=torch.float16, device="cuda").contiguous(memory_format=torch.channels_last)
        groups = co if kind == "depthwise" else 1
        tconv = lambda: torch.nn.functional.conv2d(tx, tw, None, stride, pad, 1, groups)
        tconv()
        torch.cuda.synchronize()
        tt = 1e30
        for _ in range(args.samples):
            t0 = time.perf_counter()
            for _ in range(iters):
                tconv()
            torch.cuda.synchronize()
            tt = min(tt, (time.perf_counter() - t0) / iters)
        del tx, tw
        last_clock[0] = clock
        plan = hl.debug_hannk_conv_plan(batch * out_size * out_size, co, k * k * -(-ci // 4)) if kind == "conv" else None
        k_, kg = kernels(call, o), kernels(general, o)
        d = {"shape": f"{k}x{k} s{stride} {ci}->{co} at {size}^2, batch {batch}", "ms_per_call": round(t * 1e3, 4), "kernels_ms": k_,
             "general_path": {"ms_per_call": round(tg * 1e3, 4), "kernels_ms": kg}, "fast_path_faster": bool(t < tg),
             "kernel_faster": bool(sum(k_.values()) < sum(kg.values())), "torch_f16_conv2d_ms": round(tt * 1e3, 4), "clock_state": clock}
        if kind == "conv":
            ops = 2.0 * outputs * ci * k * k
            d.update({"alg_ops": ops, "tops": round(ops / t / 1e12, 3), "i8_peak_frac": round(ops / t / 1e12 / MFMA_I8_PEAK_TOPS, 5), "plan": plan,
                      "torch_f16_tflops": round(ops / tt / 1e12, 3)})
        else:
            nbytes = float(x.size + outputs)
            d.update({"alg_bytes": nbytes, "gbs": round(nbytes / t / 1e9, 1)})
            if copy_gbs[0]:
                d["of_copy_rate"] = round(nbytes / t / 1e9 / copy_gbs[0], 4)
        return d, t

    if not only or "hannk_conv" in only:
        layers = [hannk_layer("conv", ci, co, k, s, size, batch) for (ci, co, k, s, size) in ((3, 32, 3, 2, 224), (512, 512, 1, 1, 14), (1024, 1024, 1, 1, 7))
                  for batch in (1, 32)]
        d0, t0_ = layers[3]   # pointwise 512 -> 512 at 14^2, batch 32
        emit("hannk_conv", "apps/hannk conv_u8_u8_u8, MobileNet-v1 224 layers (u8 operands, i32 accumulate on the i8 MFMA); headline: " + d0["shape"],
             t0_, 32 * 14 * 14, "mfma_i8", d0["tops"], MFMA_I8_PEAK_TOPS, "TOP/s",
             {"layers": [d for d, _ in layers], "torch_note": "torch.nn.functional.conv2d in f16, channels_last, same shape and run; another arithmetic"})
    if not only or "hannk_depthwise" in only:
        layers = [hannk_layer("depthwise", 512, 512, 3, 1, 14, batch) for batch in (1, 32)]
        d0, t0_ = layers[1]
        emit("hannk_depthwise", "apps/hannk depthwise_conv_uint8, MobileNet-v1 224: " + d0["shape"], t0_, 32 * 14 * 14, "hbm", d0["gbs"], HBM_PEAK_GBS, "GB/s",
             {"layers": [d for d, _ in layers], "torch_note": "torch.nn.functional.conv2d in f16 with groups = channels, same shape and run"})

    # ---- hannk_pool / hannk_softmax / hannk_add: the memory- and latency-bound ops of apps/hannk's op library on the shapes a MobileNet
    #      runs them at, each at batch 1 and 32, device-resident operands.  Input + output bytes against membench's copy rate of the same
    #      run (`of_copy_rate`, absent when membench is not part of the run); beside each the same call with one thread per output
    #      (hlmi_hannk_general): wherever the default path is not faster, the plan's predicate is wrong.
    def hannk_nn_line(shape, entry, fn_args, out, nbytes):
        """fn_args: the entry point's C arguments in order (device-resident Buffers), out among them"""
        call = lambda: hl._check(hl._fn[entry](*[a.ptr if isinstance(a, hl.Buffer) else a for a in fn_args]))
        general = lambda: hl.debug_hannk_general(entry, *fn_args)
        t = timed(call, out, 200)
        clock = last_clock[0]
        tg = timed(general, out, 20)
        last_clock[0] = clock
        k_, kg = kernels(call, out), kernels(general, out)
        d = {"shape": shape, "entry": entry, "ms_per_call": round(t * 1e3, 4), "kernels_ms": k_, "general_path": {"ms_per_call": round(tg * 1e3, 4), "kernels_ms": kg},
             "fast_path_faster": bool(t < tg), "kernel_faster": bool(sum(k_.values()) < sum(kg.values())), "alg_bytes": float(nbytes),
             "gbs": round(nbytes / t / 1e9, 2), "kernel_gbs": round(nbytes / (sum(k_.values()) / 1e3) / 1e9, 2), "clock_state": clock}
        if copy_gbs[0]:
            d["of_copy_rate"] = round(nbytes / t / 1e9 / copy_gbs[0], 5)
            d["kernel_of_copy_rate"] = round(d["kernel_gbs"] / copy_gbs[0], 5)
        return d, t

    def dev(a, mins=None):
        b_ = hl.Buffer(a, mins=mins)
        b_.copy_to_device()
        return b_

    if not only or "hannk_pool" in only:
        lines = []
        for batch in (1, 32):
            x = dev(rng.integers(0, 256, (batch, 7, 7, 1024), dtype=np.uint8))
            o = hl.Buffer(np.zeros((batch, 1, 1, 1024), np.uint8))
            lines.append(hannk_nn_line(f"average 7x7 over 7^2 x 1024, batch {batch}", "average_pool_uint8", [x, 1, 1, 7, 7, 0, 255, o], o, x.array.size + o.array.size))
            o2 = hl.Buffer(np.zeros((batch, 1, 1, 1024), np.uint8))
            lines.append(hannk_nn_line(f"mean over 7 x 7 x 1024, batch {batch}", "mean_uint8", [x, 0, 1, 0, 7, 0, 7, 0, 1, o2], o2, x.array.size + o2.array.size))
            y = dev(rng.integers(0, 256, (batch, 112, 112, 64), dtype=np.uint8), mins=(0, 1, 1, 0))   # "same" padding: translated by 1
            o3 = hl.Buffer(np.zeros((batch, 56, 56, 64), np.uint8))
            lines.append(hannk_nn_line(f"max 3x3 s2 over 112^2 x 64, batch {batch}", "max_pool_uint8", [y, 2, 2, 3, 3, 0, 255, o3], o3, y.array.size + o3.array.size))
        d0, t0_ = lines[5]   # the max pool at batch 32
        emit("hannk_pool", "apps/hannk average_pool_uint8, mean_uint8 and max_pool_uint8; headline: " + d0["shape"], t0_, 32 * 56 * 56, "hbm", d0["gbs"],
             HBM_PEAK_GBS, "GB/s", {"layers": [d for d, _ in lines]})
    if not only or "hannk_softmax" in only:
        lines = []
        for batch in (1, 32):
            x = dev(rng.integers(0, 256, (batch, 1001), dtype=np.uint8))
            o = hl.Buffer(np.zeros((batch, 1001), np.uint8))
            lines.append(hannk_nn_line(f"softmax on {batch} rows of 1001", "softmax_uint8", [x, 23637, 9, 0, 16384, 6, o], o, 2 * x.array.size))
        d0, t0_ = lines[1]
        emit("hannk_softmax", "apps/hannk softmax_uint8 (input scale 1/16, output scale 1/256); headline: " + d0["shape"], t0_, 32 * 1001, "hbm", d0["gbs"],
             HBM_PEAK_GBS, "GB/s", {"layers": [d for d, _ in lines]})
    if not only or "hannk_add" in only:
        lines = []
        for batch in (1, 32):
            a_, b_ = dev(rng.integers(0, 256, (batch * 56 * 56, 24), dtype=np.uint8)), dev(rng.integers(0, 256, (batch * 56 * 56, 24), dtype=np.uint8))
            o = hl.Buffer(np.zeros((batch * 56 * 56, 24), np.uint8))
            lines.append(hannk_nn_line(f"add on 56^2 x 24, batch {batch}", "add_uint8_uint8", [a_, 120, 640, b_, 7, 384, 100, 0, 255, o], o, 3 * o.array.size))
        d0, t0_ = lines[1]
        emit("hannk_add", "apps/hannk add_uint8_uint8, MobileNet-v2's residual add; headline: " + d0["shape"], t0_, 32 * 56 * 56, "hbm", d0["gbs"], HBM_PEAK_GBS,
             "GB/s", {"layers": [d for d, _ in lines]})

    # ---- fft: apps/fft's c2c, r2c and c2r at 16^2 (the size the reference builds; launch-bound), 256^2, 1024^2 and 4096^2, device buffers,
    #      gain 1.  The two line passes move each complex array twice in and twice out: "moved_bytes" is that, its rate stands beside
    #      membench's copy rate of the same run ("copy_frac"); "launch_bound": moving those bytes at that rate would take under a tenth
    #      of the call's time.  Beside each: the same call with one thread per line
    #      (hlmi_fft2d_general), which every launch the plan chooses must beat, and torch.fft.fft2 / rfft2 / irfft2 on the same data in
    #      the same run: recorded, not thresholded (rocFFT is bound to no operation order, its bits differ).
    if not only or "fft" in only:
        import torch   # this block only: the vendor column
        for n in (16, 256, 1024, 4096):
            for kind in ("c2c_forward", "r2c", "c2r"):
                ishape = {"r2c": (n, n, 1), "c2r": (n // 2 + 1, n, 2)}.get(kind, (n, n, 2))
                oshape = {"r2c": (n // 2 + 1, n, 2), "c2r": (n, n, 1)}.get(kind, (n, n, 2))
                x = (rng.random(ishape, dtype=np.float32) * 2 - 1).astype(np.float32)
                a, o = hl.fft_buffer(x), hl.fft_buffer(np.zeros(oshape, np.float32))
                a.copy_to_device()
                call = lambda kind=kind, n=n: hl.fft2d(kind, a, o, 1.0, sizes=(n, n))
                general = lambda kind=kind, n=n: hl.debug_fft2d_general(kind, a, o, 1.0, sizes=(n, n))
                iters = 200 if n <= 256 else 50 if n == 1024 else 5
                t = timed(call, o, iters)
                clock = last_clock[0]
                tg = timed(general, o, max(1, iters // (10 if n <= 1024 else 5)))
                tx = torch.from_numpy(x).cuda()
                if kind == "c2c_forward":
                    z = torch.view_as_complex(tx)
                    vendor, vname = (lambda: torch.fft.fft2(z)), "torch.fft.fft2"
                elif kind == "r2c":
                    r = tx[..., 0].T.contiguous()   # rfft2 halves its last dimension: hand it dimension 1 there
                    vendor, vname = (lambda: torch.fft.rfft2(r)), "torch.fft.rfft2"
                else:
                    z = torch.view_as_complex(tx).T.contiguous()
                    vendor, vname = (lambda n=n: torch.fft.irfft2(z, s=(n, n))), "torch.fft.irfft2"
                vendor()
                torch.cuda.synchronize()
                tv = 1e30
                for _ in range(args.samples):
                    t0 = time.perf_counter()
                    for _ in range(iters):
                        vendor()
                    torch.cuda.synchronize()
                    tv = min(tv, (time.perf_counter() - t0) / iters)
                del tx
                last_clock[0] = clock
                k, kg = kernels(call, o), kernels(general, o)
                a_cols = kind == "r2c" and n >= 16   # pass A of the zipped r2c runs down columns, every other pass A along rows
                pass_a = sum(v for name, v in k.items() if name.startswith("fft_cols") == a_cols)
                pass_b = sum(v for name, v in k.items() if name.startswith("fft_cols") != a_cols)
                if len(k) == 1:   # the whole transform in one launch: it stands against both launches of the general path
                    faster = bool(sum(k.values()) < sum(kg.values()))
                else:
                    faster = bool(pass_a < kg["fft_general_a"] and pass_b < kg["fft_general_b"])
                moved = 2.0 * 4.0 * (np.prod(ishape) + np.prod(oshape)) if kind == "c2c_forward" else 4.0 * (np.prod(ishape) + np.prod(oshape)) + 2.0 * 8.0 * n * n / 2
                extra = {"moved_bytes": float(moved), "kernels_ms": k, "general_path": {"ms_per_call": round(tg * 1e3, 4), "kernels_ms": kg},
                         "fast_path_faster": bool(t < tg), "every_launch_faster": faster,
                         "launch_bound": bool(moved / 1e9 / (copy_gbs[0] or HBM_PEAK_GBS) < 0.1 * t), "vendor": vname, "vendor_ms": round(tv * 1e3, 4),
                         "vendor_note": "rocFFT through torch on the same data; bound to no operation order, its bits differ"}
                if copy_gbs[0]:
                    extra["copy_frac"] = round(moved / t / 1e9 / copy_gbs[0], 4)
                emit(f"fft_{kind}_{n}", f"apps/fft {kind}, f32 {n}x{n}, gain 1, noise in [-1, 1)", t, n * n, "hbm", moved / t / 1e9, HBM_PEAK_GBS, "GB/s", extra)

    # ---- linear_algebra: apps/linear_algebra's f32 BLAS subset.  "sgemm": the four variants at 768^3 and 1024^3, notrans at 4096^3 and
    #      one rectangular notrans case, each beside its one-thread-per-output path (which the plan's choice must beat) and beside
    #      hl.mat_mul_sized / torch.addmm on the same operands in the same run (recorded, not thresholded; neither is bound to the
    #      contract's order).  "linear_algebra": sgemv (both) at 768, 4096 and 8192 and the vector routines and sger at 2^20 and 2^24
    #      (sger: 1024^2 and 4096^2), time and fraction of the HBM roofline on moved bytes, beside the general path; for sdot, sasum and
    #      sgemv_notrans the contract's chain length is in the line ("chain_steps"): time / steps is the latency per dependent step.
    if not only or "sgemm" in only or "linear_algebra" in only:
        import torch
        F = np.float32
        mk = lambda *s: (rng.random(s, dtype=F) * 2 - 1).astype(F)

        def dev(m):
            b = hl.Buffer(m)
            b.copy_to_device()
            return b

    if not only or "sgemm" in only:
        cases = [(ta, tb, n, n, n) for n in (768, 1024) for ta in (0, 1) for tb in (0, 1)] + [(0, 0, 4096, 4096, 4096), (0, 0, 4096, 512, 1024)]
        for ta, tb, M, N, K in cases:
            name = hl.sgemm_name(ta, tb)
            A, B, Cm = dev(mk(K, M)), dev(mk(N, K)), dev(mk(N, M))
            o = hl.Buffer(np.zeros((N, M), F))
            big = M * N * K >= 2 ** 34
            iters = 10 if big else 100
            t = timed(lambda: hl.sgemm(ta, tb, 0.75, A, B, -1.5, Cm, o), o, iters)
            clock = last_clock[0]
            tg = timed(lambda: hl.debug_sgemm_general(ta, tb, 0.75, A, B, -1.5, Cm, o), o, max(2, iters // 10))
            extra = {"general_ms_per_call": round(tg * 1e3, 4), "default_over_general": round(t / tg, 4), "canon_fma": hl.canon_fma()}
            if M == N == K and not ta and not tb:
                tm = timed(lambda: hl.mat_mul_sized(M, A, B, o), o, iters)
                extra["mat_mul_ms_per_call"] = round(tm * 1e3, 4)
                extra["c_read_ms_at_copy_rate"] = round(4.0 * M * N / ((copy_gbs[0] or HBM_PEAK_GBS) * 1e9) * 1e3, 4)
            tA, tB, tC = (torch.from_numpy(x.array).cuda() for x in (A, B, Cm))
            opA, opB = (tA if ta else tA.T), (tB if tb else tB.T)   # (M, K) and (K, N) in torch's terms
            torch.addmm(tC.T, opA, opB, beta=-1.5, alpha=0.75)
            torch.cuda.synchronize()
            tt = 1e30
            for _ in range(args.samples):
                t0 = time.perf_counter()
                for _ in range(iters):
                    torch.addmm(tC.T, opA, opB, beta=-1.5, alpha=0.75)
                torch.cuda.synchronize()
                tt = min(tt, (time.perf_counter() - t0) / iters)
            del tA, tB, tC, opA, opB
            extra["torch_addmm_ms_per_call"] = round(tt * 1e3, 4)
            last_clock[0] = clock
            emit(f"sgemm_{name[13:]}_{M}x{N}x{K}", f"apps/linear_algebra {name}, M {M} N {N} K {K}, noise in [-1, 1), a 0.75 b -1.5", t, M * N, "mfma",
                 2.0 * M * N * K / t / 1e12, MFMA_F32_PEAK_TF, "TFLOP/s", extra)
            for x in (A, B, Cm, o):
                x.device_free()

    if not only or "linear_algebra" in only:
        def line(label, what, call, general, sync, nbytes, outputs, iters, more=None):
            t = timed(call, sync, iters)
            clock = last_clock[0]
            tg = timed(general, sync, max(1, iters // 10))
            last_clock[0] = clock
            extra = {"general_ms_per_call": round(tg * 1e3, 4), "default_over_general": round(t / tg, 4), "moved_bytes": nbytes, **(more or {})}
            if "chain_steps" in extra:
                extra["ns_per_chain_step"] = round(t * 1e9 / extra["chain_steps"], 3)
            emit(label, what, t, outputs, "hbm", nbytes / t / 1e9, HBM_PEAK_GBS, "GB/s", extra)

        G = hl.debug_linear_algebra_general
        for n in (768, 4096, 8192):
            A, x, y, o = dev(mk(n, n)), dev(mk(n)), dev(mk(n)), hl.Buffer(np.zeros(n, F))
            nbytes = 4.0 * (n * n + 3 * n)
            line(f"sgemv_notrans_{n}", f"apps/linear_algebra halide_sgemv_notrans, {n}x{n}", lambda: hl.sgemv(False, 0.75, A, x, -1.5, y, o),
                 lambda: G("halide_sgemv_notrans", 0.75, A, x, -1.5, y, o), o, nbytes, n, 50, {"chain_steps": n})
            line(f"sgemv_trans_{n}", f"apps/linear_algebra halide_sgemv_trans, {n}x{n}", lambda: hl.sgemv(True, 0.75, A, x, -1.5, y, o),
                 lambda: G("halide_sgemv_trans", 0.75, A, x, -1.5, y, o), o, nbytes, n, 50, {"chain_steps": n // 8 + 8})
            for b_ in (A, x, y, o):
                b_.device_free()
        for lg in (20, 24):
            n = 1 << lg
            x, y, o, s = dev(mk(n)), dev(mk(n)), hl.Buffer(np.zeros(n, F)), hl.Buffer(np.zeros((), F))
            line(f"scopy_2^{lg}", f"apps/linear_algebra halide_scopy_impl, n 2^{lg}", lambda: hl.scopy(x, o), lambda: G("halide_scopy_impl", 0.0, x, None, o), o, 8.0 * n, n, 50)
            line(f"sscal_2^{lg}", f"apps/linear_algebra halide_sscal_impl, n 2^{lg}", lambda: hl.sscal(0.75, x, o), lambda: G("halide_sscal_impl", 0.75, x, None, o), o,
                 8.0 * n, n, 50)
            line(f"saxpy_2^{lg}", f"apps/linear_algebra halide_saxpy_impl, n 2^{lg}", lambda: hl.saxpy(0.75, x, y, o), lambda: G("halide_saxpy_impl", 0.75, x, y, o), o,
                 12.0 * n, n, 50)
            slow = 2 if lg == 24 else 10
            line(f"sdot_2^{lg}", f"apps/linear_algebra halide_sdot, n 2^{lg}: one wave, 8 chains", lambda: hl.sdot(x, y, s), lambda: G("halide_sdot", x, y, s), s, 8.0 * n, 1,
                 slow, {"chain_steps": n // 8})
            line(f"sasum_2^{lg}", f"apps/linear_algebra halide_sasum, n 2^{lg}: one wave, 8 chains", lambda: hl.sasum(x, s), lambda: G("halide_sasum", x, s), s, 4.0 * n, 1,
                 slow, {"chain_steps": n // 8})
            m = 1 << (lg // 2)
            xm, ym, R = dev(mk(m)), dev(mk(m)), dev(mk(m, m))
            line(f"sger_{m}x{m}", f"apps/linear_algebra halide_sger_impl, {m}x{m} in place", lambda: hl.sger(2.0 ** -20, xm, ym, R),
                 lambda: G("halide_sger_impl", 2.0 ** -20, xm, ym, R), R, 8.0 * m * m + 8.0 * m, m * m, 50)
            for b_ in (x, y, o, s, xm, ym, R):
                b_.device_free()

    # ---- linear_algebra, the f64 half: the blocks above at T = double.  "dgemm": the same shapes, each beside its one-thread-per-output
    #      path (which the plan's choice must beat) and beside torch.addmm in float64 on the same operands (recorded, not thresholded:
    #      it is not bound to the contract's order).  "linear_algebra_f64": dgemv (both), the vector routines and dger at the f32
    #      block's element counts; for ddot, dasum and dgemv_notrans the contract's chain length is in the line ("chain_steps", V = 4).
    if not only or "dgemm" in only or "linear_algebra_f64" in only:
        import torch
        D = np.float64
        mkd = lambda *s: rng.random(s) * 2 - 1

        def devd(m):
            b = hl.Buffer(m)
            b.copy_to_device()
            return b

    if not only or "dgemm" in only:
        cases = [(ta, tb, n, n, n) for n in (768, 1024) for ta in (0, 1) for tb in (0, 1)] + [(0, 0, 4096, 4096, 4096), (0, 0, 4096, 512, 1024)]
        for ta, tb, M, N, K in cases:
            name = hl.dgemm_name(ta, tb)
            A, B, Cm = devd(mkd(K, M)), devd(mkd(N, K)), devd(mkd(N, M))
            o = hl.Buffer(np.zeros((N, M), D))
            iters = 5 if M * N * K >= 2 ** 34 else 50
            t = timed(lambda: hl.dgemm(ta, tb, 0.75, A, B, -1.5, Cm, o), o, iters)
            clock = last_clock[0]
            tg = timed(lambda: hl.debug_linear_algebra_general_f64(name, 0.75, A, B, -1.5, Cm, o), o, max(2, iters // 10))
            extra = {"general_ms_per_call": round(tg * 1e3, 4), "default_over_general": round(t / tg, 4), "canon_fma": hl.canon_fma()}
            tA, tB, tC = (torch.from_numpy(x.array).cuda() for x in (A, B, Cm))
            opA, opB = (tA if ta else tA.T), (tB if tb else tB.T)   # (M, K) and (K, N) in torch's terms
            torch.addmm(tC.T, opA, opB, beta=-1.5, alpha=0.75)
            torch.cuda.synchronize()
            tt = 1e30
            for _ in range(args.samples):
                t0 = time.perf_counter()
                for _ in range(iters):
                    torch.addmm(tC.T, opA, opB, beta=-1.5, alpha=0.75)
                torch.cuda.synchronize()
                tt = min(tt, (time.perf_counter() - t0) / iters)
            del tA, tB, tC, opA, opB
            extra["torch_addmm_f64_ms_per_call"] = round(tt * 1e3, 4)
            last_clock[0] = clock
            emit(f"dgemm_{name[13:]}_{M}x{N}x{K}", f"apps/linear_algebra {name}, M {M} N {N} K {K}, noise in [-1, 1), a 0.75 b -1.5", t, M * N, "valu_f64",
                 2.0 * M * N * K / t / 1e12, VALU_F64_PEAK_TF, "TFLOP/s", extra)
            for x in (A, B, Cm, o):
                x.device_free()

    if not only or "linear_algebra_f64" in only:
        def line64(label, what, call, general, sync, nbytes, outputs, iters, more=None):
            t = timed(call, sync, iters)
            clock = last_clock[0]
            tg = timed(general, sync, max(1, iters // 10))
            last_clock[0] = clock
            extra = {"general_ms_per_call": round(tg * 1e3, 4), "default_over_general": round(t / tg, 4), "moved_bytes": nbytes, **(more or {})}
            if "chain_steps" in extra:
                extra["ns_per_chain_step"] = round(t * 1e9 / extra["chain_steps"], 3)
            if copy_gbs[0]:
                extra["copy_frac"] = round(nbytes / t / 1e9 / copy_gbs[0], 4)
            emit(label, what, t, outputs, "hbm", nbytes / t / 1e9, HBM_PEAK_GBS, "GB/s", extra)

        G64 = hl.debug_linear_algebra_general_f64
        for n in (768, 4096, 8192):
            A, x, y, o = devd(mkd(n, n)), devd(mkd(n)), devd(mkd(n)), hl.Buffer(np.zeros(n, D))
            nbytes = 8.0 * (n * n + 3 * n)
            line64(f"dgemv_notrans_{n}", f"apps/linear_algebra halide_dgemv_notrans, {n}x{n}", lambda: hl.dgemv(False, 0.75, A, x, -1.5, y, o),
                   lambda: G64("halide_dgemv_notrans", 0.75, A, x, -1.5, y, o), o, nbytes, n, 50, {"chain_steps": n})
            line64(f"dgemv_trans_{n}", f"apps/linear_algebra halide_dgemv_trans, {n}x{n}", lambda: hl.dgemv(True, 0.75, A, x, -1.5, y, o),
                   lambda: G64("halide_dgemv_trans", 0.75, A, x, -1.5, y, o), o, nbytes, n, 50, {"chain_steps": n // 4 + 4})
            for b_ in (A, x, y, o):
                b_.device_free()
        for lg in (20, 24):
            n = 1 << lg
            x, y, o, s = devd(mkd(n)), devd(mkd(n)), hl.Buffer(np.zeros(n, D)), hl.Buffer(np.zeros((), D))
            line64(f"dcopy_2^{lg}", f"apps/linear_algebra halide_dcopy_impl, n 2^{lg}", lambda: hl.dcopy(x, o), lambda: G64("halide_dcopy_impl", 0.0, x, None, o), o, 16.0 * n, n, 50)
            line64(f"dscal_2^{lg}", f"apps/linear_algebra halide_dscal_impl, n 2^{lg}", lambda: hl.dscal(0.75, x, o), lambda: G64("halide_dscal_impl", 0.75, x, None, o), o,
                   16.0 * n, n, 50)
            line64(f"daxpy_2^{lg}", f"apps/linear_algebra halide_daxpy_impl, n 2^{lg}", lambda: hl.daxpy(0.75, x, y, o), lambda: G64("halide_daxpy_impl", 0.75, x, y, o), o,
                   24.0 * n, n, 50)
            slow = 2 if lg == 24 else 10
            line64(f"ddot_2^{lg}", f"apps/linear_algebra halide_ddot, n 2^{lg}: one wave, 4 chains", lambda: hl.ddot(x, y, s), lambda: G64("halide_ddot", x, y, s), s, 16.0 * n, 1,
                   slow, {"chain_steps": n // 4})
            line64(f"dasum_2^{lg}", f"apps/linear_algebra halide_dasum, n 2^{lg}: one wave, 4 chains", lambda: hl.dasum(x, s), lambda: G64("halide_dasum", x, s), s, 8.0 * n, 1,
                   slow, {"chain_steps": n // 4})
            m = 1 << (lg // 2)
            xm, ym, R = devd(mkd(m)), devd(mkd(m)), devd(mkd(m, m))
            line64(f"dger_{m}x{m}", f"apps/linear_algebra halide_dger_impl, {m}x{m} in place", lambda: hl.dger(2.0 ** -20, xm, ym, R),
                   lambda: G64("halide_dger_impl", 2.0 ** -20, xm, ym, R), R, 16.0 * m * m + 16.0 * m, m * m, 50)
            for b_ in (x, y, o, s, xm, ym, R):
                b_.device_free()

    # ---- lens_blur u8 stereo pair 768x1280(the size of apps/images/rgb.png the reference's Makefile feeds process.cpp), 32 slices, 32 samples
    if not only or "lens_blur" in only:
        W, H = 768, 1280
        left = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
        right = np.roll(left, 7, 2)
        a, b = hl.Buffer(left), hl.Buffer(right)
        o = hl.Buffer(np.zeros((3, H, W), np.float32))
        call = lambda: hl.lens_blur(a, b, 32, 13, 0.5, 32, o)
        t = timed(call, o, 5)
        # traffic of the decomposition the library runs: level 0 of the push pyramid (33 planes: 32 costs + the one confidence
        # plane the generator's 32 copies collapse to) is never stored; levels >= 1 of the push pyramid are written once and
        # read twice (the next level, the pull level), the pull levels written once and read once: 5 accesses of 33 * 4 B
        # per level-1 element, 4/3 of that for the coarser levels, + the depth record / radius / output planes at level 0.
        # (The staged front end, HLMI_LB_UNFUSED=1, adds 3 * 132 B per pixel.)
        bytes_px = (5.0 / 4.0) * (4.0 / 3.0) * 33 * 4 + 6 + 4 * 4 + 12
        emit("lens_blur", "apps/lens_blur 32 slices, 32 aperture samples, u8 768x1280x3 stereo pair -> f32", t, W * H, "hbm",
             bytes_px * W * H / t / 1e9, HBM_PEAK_GBS, "GB/s", {"alg_bytes": bytes_px * W * H, "kernels_ms": kernels(call, o),
                                                              "note": "instruction-bound (cost stack ~800, depth ~1750, samples ~2400 VALU instructions per pixel); "
                                                                      "level 0 of the push pyramid is never stored"})

    # ---- bgu at the generator's estimates (bgu_generator.cpp:674-687): 192x320 low-res pair, 1536x2560 full-res image
    if not only or "bgu" in only:
        W, H = 1536, 2560
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        hi = np.stack([(np.sin(xx / (91.0 + 7 * c)) + np.cos(yy / (133.0 - 9 * c))) * 0.22 + 0.5 for c in range(3)]).astype(np.float32)
        hi += rng.random((3, H, W), dtype=np.float32) * 0.06
        lo = hi.reshape(3, H // 8, 8, W // 8, 8).mean(axis=(2, 4)).astype(np.float32)
        val = (lo * lo * (3 - 2 * lo)).astype(np.float32)
        bl, bv, bh = hl.Buffer(lo), hl.Buffer(val), hl.Buffer(hi)
        o = hl.Buffer(np.zeros((3, H, W), np.float32))
        call = lambda: hl.bgu(1.0 / 8.0, 16, bl, bv, bh, o)
        t = timed(call, o, 20)
        emit("bgu", "apps/bgu r_sigma=1/8 s_sigma=16, f32 192x320x3 pair -> 1536x2560x3", t, W * H, "hbm", 24.0 * W * H / t / 1e9,
             HBM_PEAK_GBS, "GB/s", {"alg_bytes": 24 * W * H, "kernels_ms": kernels(call, o)})

    # ---- depthwise_separable_conv at the driver's shape (MobileNet-v2 layer 2, process.cpp:13)
    if not only or "depthwise_separable_conv" in only:
        N, Hh, Ww, CI, CO = 4, 112, 112, 32, 16
        bufs = [hl.Buffer(rng.uniform(-1, 1, sh).astype(np.float32)) for sh in ((N, Hh, Ww, CI), (3, 3, CI, 1), (CI, CO), (CO,))]
        o = hl.Buffer(np.zeros((N, Hh, Ww, CO), np.float32))
        call = lambda: hl.depthwise_separable_conv(*bufs, o)
        t = timed(call, o, 50)
        nbytes = 4.0 * N * Hh * Ww * (CI + CO)
        emit("depthwise_separable_conv", "apps/depthwise_separable_conv N=4 CI=32 CO=16 CM=1 112x112 3x3", t, N * Hh * Ww, "hbm",
             nbytes / t / 1e9, HBM_PEAK_GBS, "GB/s", {"alg_bytes": nbytes, "alg_flops": 2.0 * N * Hh * Ww * (CI * 9 + CI * CO),
                                                      "kernels_ms": kernels(call, o)})

    # ---- configs[4]: conv_layer N=16 CI=CO=128 56x56 k=3 — bf16 matrix cores and the exact f32 path
    for name, fn, peak in (("conv_layer_bf16", "conv_layer_bf16", MFMA_BF16_PEAK_TF), ("conv_layer", "conv_layer", MFMA_F32_PEAK_TF)):
        if only and name not in only:
            continue
        N, Hh, Ww, CI, CO = 16, 56, 56, 128, 128
        c_in = rng.uniform(-1, 1, (N, Hh + 2, Ww + 2, CI)).astype(np.float32)
        c_f = rng.uniform(-1, 1, (CI, 3, 3, CO)).astype(np.float32)
        c_b = rng.uniform(-1, 1, CO).astype(np.float32)
        inp, filt, bias = hl.Buffer(c_in), hl.Buffer(c_f), hl.Buffer(c_b)
        o = hl.Buffer(np.zeros((N, Hh, Ww, CO), np.float32))
        f = getattr(hl, fn)
        call = lambda: f(inp, filt, bias, o)
        t = timed(call, o, 50)
        flops = 2.0 * N * Hh * Ww * CI * CO * 9

        def mk_conv(i):
            ii, oi = hl.Buffer(np.roll(c_in, i, 1).copy()), hl.Buffer(np.zeros((N, Hh, Ww, CO), np.float32))
            return lambda: f(ii, filt, bias, oi)
        tb = timed_batched(mk_conv)
        cold = None
        if "bf16" in name:
            # the bf16 re-ordering of the filter is cached across calls with the same filter buffer (a layer's weights do not change
            # between inferences): the figure above is the cached case; this one re-orders the filter inside every timed call
            os.environ["HLMI_CONV_NO_FILTER_CACHE"] = "1"
            cold = timed(call, o, 50)
            del os.environ["HLMI_CONV_NO_FILTER_CACHE"]
        io_bytes = 4 * (N * (Hh + 2) * (Ww + 2) * CI + N * Hh * Ww * CO)   # the reference's f32 input and output, each moved once
        orc = (lambda ol: ol.conv_layer_bf16(c_in, c_f, c_b)) if "bf16" in name else (lambda ol: ol.conv_layer(c_in, c_f, c_b))
        emit(name, f"apps/conv_layer N=16 CI=CO=128 56x56 k=3 ({'bf16 operands, f32 accumulate' if 'bf16' in name else 'exact f32'})",
             t, N * Hh * Ww, "mfma", flops / t / 1e12, peak, "TFLOP/s",
             {"alg_flops": flops, "alg_bytes": io_bytes, "kernels_ms": kernels(call, o),
              **batched_fields(tb, flops / 1e12, peak, "mfma"),
              **({"filter_cached": True, "ms_per_call_filter_uncached": round(cold * 1e3, 4)} if cold is not None else {}),
              # the second bound: with f32 I/O the call cannot beat its bytes — reported beside the matrix-core fraction
              "hbm_bound": {"alg_bytes": io_bytes, "achieved_gbs": round(io_bytes / t / 1e9, 1), "peak": HBM_PEAK_GBS,
                            "frac": round(io_bytes / t / 1e9 / HBM_PEAK_GBS, 4)},
              **(cpu_base(orc, flops / 1e6, "TFLOP/s", "N=16 56x56 128->128 k=3") if "bf16" in name else {})})


def nl_means_batch32(samples=3):
    """BASELINE.json configs[3] at N = 1: the batch of 32 nl_means frames (7x7 search / 7x7 patch, f32 1920x1080x3, seeds 0..31 as
    SURVEY.md §8d names them) resident on one GPU — what every rank of bench_batch.py does with its share, without the exchange
    step — enqueued back to back over four frame-queue streams, ONE sync at the end; min over `samples` batches."""
    import numpy as np
    import halide_amd as hl
    W, H, B = 1920, 1080, 32
    frames = [np.random.default_rng(seed).random((3, H, W), dtype=np.float32) for seed in range(B)]
    ins = [hl.Buffer(f) for f in frames]
    outs = [hl.Buffer(np.zeros((3, H, W), np.float32)) for _ in range(B)]
    hip = hl.hip_runtime()
    results = {}
    for nparts in (1, 4):
        streams = [None] if nparts == 1 else [hl.partition_stream(p, nparts) for p in range(nparts)]
        if nparts > 1 and not all(streams):
            continue

        def batch():
            for i, (a, o) in enumerate(zip(ins, outs)):
                hl.set_stream(streams[i % nparts])
                hl.nl_means(a, 7, 7, 0.12, o)
            hl.set_stream(None)
            hip.hipDeviceSynchronize()
        batch()      # uploads the inputs, allocates the outputs
        best = 1e30
        for _ in range(samples):
            t0 = time.perf_counter()
            batch()
            best = min(best, time.perf_counter() - t0)
        results["1 stream" if nparts == 1 else f"{nparts} frame-queue streams"] = best
    for b in ins + outs:
        b.device_free()
    how, t = min(results.items(), key=lambda kv: kv[1])
    flops = 2200.0 * W * H * B
    return {"pipeline": "nl_means_batch32", "workload": "BASELINE configs[3] at N=1: 32 frames of apps/nl_means patch 7 search 7 sigma 0.12, "
            "f32 1920x1080x3, resident on one GPU (bench_batch.py shards the same batch over N GPUs with RCCL send/recv)",
            "ms_per_batch": round(t * 1e3, 3), "ms_per_frame": round(t * 1e3 / B, 4), "value": round(B * W * H / t / 1e6, 1), "unit": "Mpx/s",
            "streams": how, "ms_per_batch_by_scheduling": {k: round(v * 1e3, 3) for k, v in results.items()},
            "roofline": {"bound": "valu", "achieved": round(flops / t / 1e12, 2), "peak": VALU_F32_PEAK_TF, "unit": "TFLOP/s",
                         "frac": round(flops / t / 1e12 / VALU_F32_PEAK_TF, 4)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--cpu-baseline", action="store_true", help="time the C oracle beside the BASELINE.json configs")
    ap.add_argument("--no-batched", action="store_true", help="skip the frames-in-flight leg (profiler runs)")
    a = ap.parse_args()
    names = [n for n in a.only.split(",") if n]
    if "nl_means_batch32" in names:      # configs[3] as a batch (not one of run()'s per-call pipelines)
        print(json.dumps(nl_means_batch32(a.samples)), flush=True)
        names.remove("nl_means_batch32")
        if not names:
            return
    run(names, a.samples, None, a.cpu_baseline, not a.no_batched)


if __name__ == "__main__":
    main()
