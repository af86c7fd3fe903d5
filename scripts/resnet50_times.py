#!/usr/bin/env python3
"""Times of hl.resnet50 on device-resident buffers (torch-free unless --torch is given), in the style of scripts/kernel_times.py.

Reports, for the default path and for the general path (hl.debug_resnet50_general):
  ms per call + sync, ms per call back to back, and the per-kernel totals of one call (HIP events around every launch);
per layer class (the distinct convolution shapes of the network, each through the layer hook, both paths): ms per launch, the share of
the dense f32 matrix peak, and which path the standing rule would pick.  With --torch: a plain torch.nn.functional f32 forward of the
same network on the same device (MIOpen / hipBLASLt, not bit-exact), the outside yardstick.

With --batch N[,N...]: hl.resnet50_batch (a library extension, N images per call) at each N, default and general path: ms per call back to
back, ms per image, TFLOP/s, and with --torch the same torch forward at that batch size.  With --tile-ab N: every layer class over N
images through the batched layer hook on each MFMA tile instance (64 x 64, 64 x 128) and on the plan's choice, alternating, which is
the measurement conv_plan()'s batch rule rests on.  --no-classes skips the single-image layer classes.

    python scripts/resnet50_times.py [--reps 20] [--torch] [--json out.json] [--batch 1,2,4] [--tile-ab 32] [--no-classes]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import halide_amd as hl  # noqa: E402

PEAK_F32_MATRIX_TFLOPS = 157.3   # MI355X dense f32 matrix peak (vendor figure)
f32 = np.float32


def out_extent(size, k, stride, pad):
    return (pad * 2 + size - k + 1 + stride - 1) // stride


def convs():
    """(class name, ci, co, k, stride, pad, input size) of the 53 convolutions in argument order"""
    br1, a, b, c = [], [], [], []
    cin, size = 64, 56
    for s, (mid, blocks, stride) in enumerate(((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2))):
        for i in range(blocks):
            st = stride if i == 0 else 1
            osize = out_extent(size, 1, st, 0)
            if i == 0:
                br1.append((cin, 4 * mid, 1, st, 0, size))
            a.append((cin, mid, 1, 1, 0, size))
            b.append((mid, mid, 3, st, 1, size))
            c.append((mid, 4 * mid, 1, 1, 0, osize))
            cin, size = 4 * mid, osize
    return [(3, 64, 7, 2, 3, 224)] + br1 + a + b + c


def flops(ci, co, k, stride, pad, size):
    return 2.0 * ci * k * k * co * out_extent(size, k, stride, pad) ** 2


def random_params(rng):
    shapes = convs()
    vec = lambda lo, hi: [(rng.random(s[1]) * (hi - lo) + lo).astype(f32) for s in shapes]
    gamma = vec(0.5, 1.5)
    for i in range(37, 53):
        gamma[i] = (gamma[i] * f32(0.25)).astype(f32)
    beta = [(0.1 * rng.standard_normal(s[1])).astype(f32) for s in shapes]
    mu = [(0.1 * rng.standard_normal(s[1])).astype(f32) for s in shapes]
    sig = vec(0.5, 1.5)
    w = [(rng.standard_normal((ci, k, k, co)) * np.sqrt(2.0 / (k * k * ci))).astype(f32) for ci, co, k, _, _, _ in shapes]
    fcw = (rng.standard_normal((2048, 1000)) * np.sqrt(4.0 / 2048)).astype(f32)
    fcb = (0.1 * rng.standard_normal(1000)).astype(f32)
    return gamma + beta + mu + sig + w + [fcw, fcb]


def timed(fn, out, reps):
    """(ms per call + sync, ms per call back to back)"""
    fn(), out.device_sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn(), out.device_sync()
    each = (time.perf_counter() - t0) / reps * 1e3
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    out.device_sync()
    return each, (time.perf_counter() - t0) / reps * 1e3


def kernel_report(fn, out):
    hl.kernel_timing(True)
    hl.kernel_timing_reset()
    try:
        fn(), out.device_sync()
        return hl.kernel_timing_report()
    finally:
        hl.kernel_timing(False)
        hl.kernel_timing_reset()


def layer_classes(reps):
    rng = np.random.default_rng(1)
    seen, rows = {}, []
    for shape in convs():
        seen[shape] = seen.get(shape, 0) + 1
    for (ci, co, k, stride, pad, size), count in seen.items():
        osz = out_extent(size, k, stride, pad)
        bufs = [hl.Buffer(rng.random((size, size, ci), dtype=f32)), hl.Buffer((rng.standard_normal((ci, k, k, co)) * 0.05).astype(f32))]
        bufs += [hl.Buffer((rng.random(co) + 0.5).astype(f32)) for _ in range(4)]
        res, out = hl.Buffer(rng.random((osz, osz, co), dtype=f32)), hl.Buffer(np.zeros((osz, osz, co), f32))
        row = dict(ci=ci, co=co, k=k, stride=stride, size=size, out=osz, layers=count, gflop=flops(ci, co, k, stride, pad, size) / 1e9)
        for general in (False, True):
            call = lambda: hl.debug_resnet50_layer(*bufs, res, stride, pad, 3, out, general_only=general)
            call(), out.device_sync()
            hl.kernel_timing(True)
            hl.kernel_timing_reset()
            for _ in range(reps):
                call()
            out.device_sync()
            rep = hl.kernel_timing_report()
            hl.kernel_timing(False)
            hl.kernel_timing_reset()
            assert len(rep) == 1, rep
            row["general_ms" if general else "default_ms"] = rep[0]["avg_ms"]
            if not general:
                row["kernel"] = rep[0]["name"]
        row["tflops"] = row["gflop"] / row["default_ms"]
        # (a class the plan already sends to the general kernel is the same launch timed twice)
        row["default_slower"] = row["kernel"] != "resnet50_conv_general" and row["default_ms"] > row["general_ms"]
        rows.append(row)
        for b in bufs + [res, out]:
            b.device_free()
    return rows


def fill_reps(fn, out, seconds=0.3):
    """calls that fill `seconds` back to back, from one timed call"""
    fn(), out.device_sync()
    t0 = time.perf_counter()
    fn(), out.device_sync()
    return max(3, int(seconds / max(time.perf_counter() - t0, 1e-6)))


def batch_times(params, par, sizes, total_gflop, with_torch):
    """hl.resnet50_batch at each size, default and general path, device-resident, warm, back to back"""
    rng = np.random.default_rng(2)
    rows = []
    for n in sizes:
        images = rng.random((n, 224, 224, 3), dtype=f32)
        inp, out = hl.Buffer(images), hl.Buffer(np.zeros((n, 1000), f32))
        row = dict(n=n, chunk=hl.debug_resnet50_batch_plan(n)["chunk"])
        for name, fn in (("default", lambda: hl.resnet50_batch(inp, par, out)), ("general", lambda: hl.debug_resnet50_batch_general(inp, par, out))):
            reps = fill_reps(fn, out)
            runs = [timed(fn, out, reps)[1] for _ in range(3)]   # three windows: their spread is the noise of this figure
            ms = min(runs)
            device = sum(e["total_ms"] for e in kernel_report(fn, out))   # HIP events around every launch of one call
            row[name] = dict(ms_call=ms, ms_image=ms / n, tflops=total_gflop * n / ms, window_ms=runs, reps=reps, device_ms=device)
        if with_torch:
            row["torch_ms_image"] = torch_forward_ms(params, images, 10)[1] / n
        rows.append(row)
        inp.device_free(), out.device_free()
        d, g = row["default"], row["general"]
        print(f"batch {n:3d} (chunk {row['chunk']:2d})  default {d['ms_call']:9.3f} ms = {d['ms_image']:7.3f} ms per image {d['tflops']:6.2f} TFLOP/s "
              f"(windows {' '.join(f'{w:.3f}' for w in d['window_ms'])}; device events {d['device_ms']:.3f} ms)   general {g['ms_image']:7.3f} ms per image {g['tflops']:6.2f} TFLOP/s"
              + (f"   torch {row['torch_ms_image']:7.3f} ms per image" if with_torch else ""), flush=True)
    return rows


def tile_ab(n, reps, rounds=3):
    """every layer class over n images on each MFMA tile instance and on the plan's choice, alternating inside each round"""
    rng = np.random.default_rng(1)
    seen, rows = {}, []
    for shape in convs():
        seen[shape] = seen.get(shape, 0) + 1
    for (ci, co, k, stride, pad, size), count in seen.items():
        osz = out_extent(size, k, stride, pad)
        bufs = [hl.Buffer(rng.random((n, size, size, ci), dtype=f32)), hl.Buffer((rng.standard_normal((ci, k, k, co)) * 0.05).astype(f32))]
        bufs += [hl.Buffer((rng.random(co) + 0.5).astype(f32)) for _ in range(4)]
        res, out = hl.Buffer(rng.random((n, osz, osz, co), dtype=f32)), hl.Buffer(np.zeros((n, osz, osz, co), f32))
        row = dict(ci=ci, co=co, k=k, stride=stride, size=size, out=osz, layers=count, gflop=n * flops(ci, co, k, stride, pad, size) / 1e9)
        best = {}
        for _ in range(rounds):
            for variant in ("mfma_64x64", "mfma_64x128", "plan"):
                call = lambda: hl.debug_resnet50_layer_batch(*bufs, res, stride, pad, 3, out, variant=variant)
                call(), out.device_sync()
                hl.kernel_timing(True)
                hl.kernel_timing_reset()
                for _ in range(reps):
                    call()
                out.device_sync()
                rep = hl.kernel_timing_report()
                hl.kernel_timing(False)
                hl.kernel_timing_reset()
                assert len(rep) == 1, rep
                best.setdefault(variant, []).append(rep[0]["avg_ms"])
                if variant == "plan":
                    row["kernel"] = rep[0]["name"]
        row["ms"] = {v: min(t) for v, t in best.items()}
        row["all_ms"] = best
        rows.append(row)
        for b in bufs + [res, out]:
            b.device_free()
        m = row["ms"]
        print(f"{ci:5d} {co:5d}  {k} {stride} {size:3d} {osz:3d}  x{count:2d} {row['gflop']:8.3f} GFLOP  64x64 {m['mfma_64x64']:8.4f} ms  64x128 {m['mfma_64x128']:8.4f} ms "
              f"({m['mfma_64x128'] / m['mfma_64x64']:5.2f} x)  plan {m['plan']:8.4f} ms {row['kernel']:24s} {row['gflop'] / m['plan']:7.2f} TFLOP/s", flush=True)
    return rows


def torch_forward_ms(params, image, reps):
    import torch
    import torch.nn.functional as F
    shapes = convs()
    dev = torch.device("cuda")
    t = [torch.from_numpy(p).to(dev) for p in params]
    w = [t[4 * 53 + i].permute(3, 0, 1, 2).contiguous() for i in range(53)]   # (ci, kh, kw, co) -> (co, ci, kh, kw)
    batch = image if image.ndim == 4 else image[None]   # (N, 224, 224, 3) -> (N, 3, 224, 224)
    x0 = torch.from_numpy(np.ascontiguousarray(batch.transpose(0, 3, 1, 2))).to(dev)

    def layer(x, i, relu=True, res=None):
        _, _, k, stride, pad, _ = shapes[i]
        y = F.batch_norm(F.conv2d(x, w[i], stride=stride, padding=pad), t[2 * 53 + i], t[3 * 53 + i], t[i], t[53 + i], False, 0.0, 1e-5)
        if res is not None:
            y = y + res
        return F.relu(y) if relu else y

    def forward():
        x = F.max_pool2d(layer(x0, 0), 3, 2, 1)
        b = 0
        for s, blocks in enumerate((3, 4, 6, 3)):
            for i in range(blocks):
                short = layer(x, 1 + s, relu=False) if i == 0 else x
                x = layer(layer(layer(x, 5 + b), 21 + b), 37 + b, res=short)
                b += 1
        return torch.softmax(x.mean(dim=(2, 3)) @ t[-2] + t[-1], 1)

    with torch.no_grad():
        for _ in range(3):
            forward()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            forward()
            torch.cuda.synchronize()
        each = (time.perf_counter() - t0) / reps * 1e3
        t0 = time.perf_counter()
        for _ in range(reps):
            forward()
        torch.cuda.synchronize()
        return each, (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch", action="store_true")
    ap.add_argument("--json")
    ap.add_argument("--batch", help="batch sizes of hl.resnet50_batch, comma-separated")
    ap.add_argument("--tile-ab", type=int, help="images of the per-class A/B of the MFMA tile instances")
    ap.add_argument("--no-classes", action="store_true", help="skip the single-image layer classes")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    params = random_params(rng)
    image = rng.random((224, 224, 3), dtype=f32)
    inp, par, out = hl.Buffer(image.copy()), [hl.Buffer(p.copy()) for p in params], hl.Buffer(np.zeros(1000, f32))
    total_gflop = sum(flops(*s) for s in convs()) / 1e9 + 2 * 2048 * 1000 / 1e9
    result = dict(canon_fma=hl.canon_fma(), gflop=total_gflop, peak_tflops=PEAK_F32_MATRIX_TFLOPS)
    for name, fn in (("default", lambda: hl.resnet50(inp, par, out)), ("general", lambda: hl.debug_resnet50_general(inp, par, out))):
        each, b2b = timed(fn, out, a.reps)
        rep = kernel_report(fn, out)
        result[name] = dict(ms_call_sync=each, ms_back_to_back=b2b, tflops=total_gflop / b2b, kernels=rep, device_ms=sum(e["total_ms"] for e in rep))
        print(f"{name:8s} {each:8.3f} ms per call + sync   {b2b:8.3f} ms back to back   {total_gflop / b2b:6.2f} TFLOP/s "
              f"({100 * total_gflop / b2b / PEAK_F32_MATRIX_TFLOPS:.1f} % of the f32 matrix peak)   device time {result[name]['device_ms']:.3f} ms")
        for e in rep:
            print(f"    {e['name']:24s} x {e['calls']:2d}  {e['total_ms']:8.3f} ms  ({e['avg_ms'] * 1e3:8.1f} us each)")
    if not a.no_classes:
        rows = layer_classes(a.reps)
        result["classes"] = rows
        print("layer classes (ms per launch, residual + ReLU epilogue):")
        print("   ci    co  k s  in out  layers   GFLOP  kernel                  default   general  TFLOP/s  default slower?")
        for r in sorted(rows, key=lambda r: -r["gflop"] * r["layers"]):
            print(f"{r['ci']:5d} {r['co']:5d}  {r['k']} {r['stride']} {r['size']:3d} {r['out']:3d}  {r['layers']:6d} {r['gflop']:7.3f}  {r['kernel']:22s} {r['default_ms']:8.4f} "
                  f"{r['general_ms']:8.4f} {r['tflops']:8.2f}  {'YES' if r['default_slower'] else 'no'}")
    if a.batch:
        result["batch"] = batch_times(params, par, [int(n) for n in a.batch.split(",")], total_gflop, a.torch)
    if a.tile_ab:
        print(f"layer classes over {a.tile_ab} images, each MFMA tile instance and the plan's choice (ms per launch, best of 3 alternating rounds):")
        result["tile_ab"] = dict(images=a.tile_ab, classes=tile_ab(a.tile_ab, a.reps))
    if a.torch:
        each, b2b = torch_forward_ms(params, image, a.reps)
        result["torch"] = dict(ms_call_sync=each, ms_back_to_back=b2b)
        print(f"torch.nn.functional f32 forward: {each:.3f} ms per call + sync, {b2b:.3f} ms back to back")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
