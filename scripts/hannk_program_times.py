#!/usr/bin/env python3
"""Times of hannk's elementwise programs, copy, fill, upsample_channels and the shallow depthwise variant on device-resident buffers, in
the style of scripts/resnet50_times.py: every path of an op back to back in one process, HIP events around every launch.

Per shape: us per launch of the default path, of the general kernel (hl.debug_hannk_general) and, for the elementwise programs, of each
plan HLMI_HANNK_EW_PLAN can force (the byte table, the interpreter kernel with its slots in LDS, in registers); for the shallow depthwise
variant of depthwise_conv_uint8 on the layout with 16 channels per pixel that it replaces; the algorithmic bytes per second of the default
path as a share of the device-to-device copy rate measured in the same run.

    python scripts/hannk_program_times.py [--reps 50] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import halide_amd as hl  # noqa: E402

PLANS = {"table": 1, "interp_lds": 2, "interp_reg": 3}


def device_copy_rate(nbytes=256 << 20, reps=10):
    """GB/s (read + write) of hipMemcpy device to device"""
    hip = hl.hip_runtime()
    a, b = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(a), C.c_size_t(nbytes)) == 0 and hip.hipMalloc(C.byref(b), C.c_size_t(nbytes)) == 0
    assert hip.hipMemset(a, 1, C.c_size_t(nbytes)) == 0 and hip.hipMemcpy(b, a, C.c_size_t(nbytes), 3) == 0
    assert hip.hipDeviceSynchronize() == 0
    t0 = time.perf_counter()
    for _ in range(reps):
        assert hip.hipMemcpyAsync(b, a, C.c_size_t(nbytes), 3, None) == 0
    assert hip.hipDeviceSynchronize() == 0
    dt = time.perf_counter() - t0
    hip.hipFree(a), hip.hipFree(b)
    return 2.0 * nbytes * reps / dt / 1e9


def per_launch_us(call, sync, reps):
    call(), sync()
    hl.kernel_timing(True)
    hl.kernel_timing_reset()
    try:
        for _ in range(reps):
            call()
        sync()
        rep = hl.kernel_timing_report()
    finally:
        hl.kernel_timing(False)
        hl.kernel_timing_reset()
    assert len(rep) == 1, rep
    return rep[0]["name"], rep[0]["avg_ms"] * 1e3


def resident(a):
    return hl.Buffer(np.ascontiguousarray(a)).copy_to_device()


def cases():
    rng = np.random.default_rng(0)
    u8 = lambda *shape: rng.integers(0, 256, shape, dtype=np.uint8)
    out = []
    for name, program in (("logistic", hl.hannk_logistic_program(1 / 16, 128)), ("tanh", hl.hannk_tanh_program(1 / 32, 128))):
        sweep = [(f"1x{n}", (1, n)) for n in (16384, 65536, 262144, 1048576)] if name == "logistic" else []   # where the table starts to pay
        for what, shape in [("32x56x56x24", (32 * 56 * 56, 24)), ("1x1001", (1, 1001))] + sweep:
            x, o, p = resident(u8(*shape)), resident(np.zeros(shape, np.uint8)), hl.Buffer(program)
            out.append(dict(op=f"{name} {what}", entry="elementwise_5xuint8_1xuint8", args=[x, x, x, x, x, p, o], out=o, bytes=2.0 * x.array.size, plans=True))
    for shape in ((32, 2048), (128, 2048), (512, 2048), (2048, 2048)):   # one LSTM layer of 2048 units at batch 32, then larger outputs: where two elements per lane would have to pay
        s = [resident(rng.integers(-32768, 32768, shape).astype(np.int16)) for _ in range(5)]
        o0, o1 = resident(np.zeros(shape, np.uint8)), resident(np.zeros(shape, np.int16))
        out.append(dict(op=f"lstm {shape[0]}x{shape[1]}", entry="elementwise_5xint16_1xuint8int16", args=s + [hl.Buffer(hl.hannk_lstm_program()), o0, o1],
                        out=o1, bytes=13.0 * shape[0] * shape[1], plans=True))
    x, o = resident(u8(32, 224, 224, 3)), resident(np.zeros((32, 224, 224, 4), np.uint8))
    out.append(dict(op="copy 3->4 32x224x224", entry="copy_uint8_uint8", args=[x, 0, o], out=o, bytes=7.0 * 32 * 224 * 224))
    x, o = resident(u8(32, 56, 56, 8)), resident(np.zeros((32, 56, 56, 8), np.uint8))
    out.append(dict(op="copy equal 32x56x56x8", entry="copy_uint8_uint8", args=[x, 0, o], out=o, bytes=2.0 * x.array.size))
    out.append(dict(op="fill 32x56x56x8", entry="fill_uint8", args=[7, o], out=o, bytes=1.0 * o.array.size))
    o64 = resident(np.zeros((32, 56, 56, 64), np.uint8))
    out.append(dict(op="upsample x8 32x56x56x8", entry="upsample_channels_uint8", args=[x, 8, o64], out=o64, bytes=1.0 * x.array.size + o64.array.size))
    for d in (3, 4):   # the stem's 3 channels as they lie, and 4 (a divisor of 16, whose taps the dword kernel can take)
        img, filt, bias = u8(32, 224, 1, 224 * d), u8(3, 3, d), rng.integers(-1000, 1000, d).astype(np.int32)
        padded = np.zeros((32, 224, 224, 16), np.uint8)
        padded[..., :d] = img.reshape(32, 224, 224, d)
        f16, b16 = np.zeros((3, 3, 16), np.uint8), np.zeros(16, np.int32)
        f16[..., :d], b16[:d] = filt, bias
        o, o16 = resident(np.zeros((32, 222, 1, 222 * d), np.uint8)), resident(np.zeros((32, 222, 222, 16), np.uint8))
        tail = [1 << 30, 8, 3, 0, 255]
        out.append(dict(op=f"shallow 3x3 32x224x224x{d}", entry="depthwise_conv_shallow_uint8",
                        args=[resident(img), 5, resident(filt), 120, resident(bias), 1, 1, 1, 1, d] + tail + [o], out=o, bytes=1.0 * img.size + o.array.size,
                        other=("depthwise_conv_uint8", [resident(padded), 5, resident(f16), 120, resident(b16), 1, 1, 1, 1, 0] + tail + [o16], o16)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--json")
    a = ap.parse_args()
    for s in ("HLMI_HANNK_EW_PLAN", "HLMI_HANNK_MOVE_VECTOR"):
        os.environ.pop(s, None)
    rate = device_copy_rate()
    print(f"device-to-device copy: {rate:.0f} GB/s (read + write)")
    rows = []
    print(f"{'op':26s} {'default kernel':20s} {'default':>9s} {'general':>9s} {'table':>9s} {'interp lds':>11s} {'interp reg':>11s} {'padded dw':>9s} {'GB/s':>7s} {'of copy':>8s}  default slower?")
    for c in cases():
        direct = lambda: hl._check(hl._fn[c["entry"]](*[v.ptr if isinstance(v, hl.Buffer) else v for v in c["args"]]))
        general = lambda: hl.debug_hannk_general(c["entry"], *c["args"])
        sync = c["out"].device_sync
        row = dict(op=c["op"], bytes=c["bytes"])
        row["kernel"], row["default_us"] = per_launch_us(direct, sync, a.reps)
        _, row["general_us"] = per_launch_us(general, sync, a.reps)
        for plan, v in PLANS.items():
            if c.get("plans"):
                os.environ["HLMI_HANNK_EW_PLAN"] = str(v)
                name, us = per_launch_us(direct, sync, a.reps)
                os.environ.pop("HLMI_HANNK_EW_PLAN")
                # (a plan the program does not allow falls back to the general kernel: the table of a five-input program)
                row[plan + "_us"] = us if (plan == "table") == (name == "hannk_prog_table") else None
        if c.get("other"):   # the shallow variant: depthwise_conv_uint8 on the padded layout
            name, args, out = c["other"]
            _, row["padded_us"] = per_launch_us(lambda: hl._check(hl._fn[name](*[v.ptr if isinstance(v, hl.Buffer) else v for v in args])), out.device_sync, a.reps)
        row["gbs"] = c["bytes"] / row["default_us"] / 1e3
        row["of_copy"] = row["gbs"] / rate
        row["default_slower"] = row["kernel"] not in ("hannk_prog_general", "hannk_move_general", "hannk_dw_general") and row["default_us"] > row["general_us"]
        rows.append(row)
        f = lambda v: f"{v:9.2f}" if v is not None else "        -"
        print(f"{row['op']:26s} {row['kernel']:20s} {f(row['default_us'])} {f(row['general_us'])} {f(row.get('table_us'))} {f(row.get('interp_lds_us')):>11s} "
              f"{f(row.get('interp_reg_us')):>11s} {f(row.get('padded_us'))} {row['gbs']:7.0f} {100 * row['of_copy']:7.1f}%  {'YES' if row['default_slower'] else 'no'}")
    if a.json:
        with open(a.json, "w") as fjson:
            json.dump(dict(copy_gbs=rate, rows=rows), fjson, indent=1)


if __name__ == "__main__":
    main()
