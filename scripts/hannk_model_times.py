"""Times hannk's data movement without torch: hlmi_hannk_copy_from by the plan's choice against the one-thread-per-element
kernel (hlmi_hannk_general) and against the device copy rate measured in the same run (the rows copy of 256 MB), on the shapes 5.15 quotes; then
the 21 MobileNet-v1-0.25 one-op files as one HannkModel run back to back against the same ops through the hl.hannk_* wrappers.  One JSON line per
case; `--out FILE` also writes them to a file.  Kernel times are medians of `--reps` timed launches read from the library's own events
(hlmi_kernel_timing_*), after `--warmup` untimed ones; the model's are by host clock around one whole pass."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import halide_amd as hl  # noqa: E402


def device_array(a):
    hip = hl.hip_runtime()
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(max(a.nbytes, 16))) == 0
    assert hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
    return p


def view(p, like):
    return hl.Buffer.wrap_device(p.value, like.dtype, like.shape[::-1], [s // like.itemsize for s in like.strides][::-1])


def kernel_us(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    hl.kernel_timing(True)
    ms, name = [], None
    for _ in range(reps):       # one report per launch: the report holds totals, the median needs each time
        hl.kernel_timing_reset()
        fn()
        report = hl.kernel_timing_report()
        name = report[0]["name"]
        ms.append(report[0]["total_ms"])
    hl.kernel_timing(False)
    hl.kernel_timing_reset()
    return name, 1e3 * sorted(ms)[len(ms) // 2]


def device_copy_rate(warmup, reps, nbytes=256 << 20):
    """GB/s (read + written) of the library's rows copy over two dense 256 MB buffers, by the same events: the device copy rate of this run"""
    like = np.zeros(1, np.uint8)
    hip = hl.hip_runtime()
    a, b = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(a), C.c_size_t(nbytes)) == 0 and hip.hipMalloc(C.byref(b), C.c_size_t(nbytes)) == 0
    s = hl.Buffer.wrap_device(a.value, like.dtype, [nbytes]); d = hl.Buffer.wrap_device(b.value, like.dtype, [nbytes])
    name, us = kernel_us(lambda: hl.hannk_copy_from(s, d), warmup, reps)
    s.device_detach(), d.device_detach()
    hip.hipFree(a), hip.hipFree(b)
    return {"case": "device_copy_rate_256MB", "kernel": name, "us": round(us, 2), "GBps": round(2 * nbytes / us / 1e3, 1)}


def mobilenet_graph():
    """the 21 one-op files of MobileNet-v1-0.25 as ONE graph: 000 .. 014 chained output to input, the other six beside them with inputs of their own"""
    from halide_amd import tflite_reader as tfl
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "hannk", "mobilenet_v1_0.25_128_quant")
    files = sorted(os.path.join(root, f) for f in os.listdir(root) if f.endswith(".tflite"))
    tensors, ops, inputs, outputs, prev = [], [], [], [], None
    for k, path in enumerate(files):
        g = tfl.read(path)
        base = len(tensors)
        tensors += g.tensors
        op = g.ops[0]
        ins = [i + base for i in op.inputs]
        if k <= 14 and prev is not None:
            ins[0] = prev
        else:
            inputs.append(ins[0])
        out = op.outputs[0] + base
        if k >= 14:
            outputs.append(out)
        prev = out
        ops.append(tfl.Op(op.kind, ins, [out], dict(op.attrs)))
    return tfl.Graph(tensors, ops, inputs, outputs), files


def wrappers_pass(graph, xs):
    """the same 21 ops through today's hl.hannk_* wrappers: numpy in, numpy out, padded on the host, one op at a time (SAME padding is given
    to the wrappers as the symmetric padding of the same output size: the work is the same, the taps are shifted)"""
    val, it = {}, iter(xs)
    for i in graph.inputs:
        val[i] = next(it)
    f32 = np.float32
    for op in graph.ops:
        t = graph.tensors
        x, o = val[op.inputs[0]], t[op.outputs[0]]
        a = op.attrs
        if op.kind in ("CONV_2D", "DEPTHWISE_CONV_2D"):
            f, bias = t[op.inputs[1]], t[op.inputs[2]]
            m, e = hl.hannk_int_float(f32(t[op.inputs[0]].scale[0]) * f32(f.scale[0]) / f32(o.scale[0]), 32)
            fh, fw = f.data.shape[1:3]
            pad = ((o.shape[1] - 1) * a["stride"][0] + fw - x.shape[2] + 1) // 2, ((o.shape[2] - 1) * a["stride"][1] + fh - x.shape[1] + 1) // 2
            pad = (max(pad[0], 0), max(pad[1], 0))
            if op.kind == "CONV_2D":
                y = hl.hannk_conv2d(x, f.data, bias.data, t[op.inputs[0]].zero[0], f.zero[0], a["stride"], a["dilation"], pad, m, -e, o.zero[0], 0, 255)
            else:
                y = hl.hannk_depthwise_conv2d(x, f.data[0], bias.data, t[op.inputs[0]].zero[0], f.zero[0], a["stride"], a["dilation"], pad, m, -e, o.zero[0], 0, 255)
            y = y[:, :o.shape[2], :o.shape[1]]
        elif op.kind == "AVERAGE_POOL_2D":
            y = hl.hannk_pool2d("average", x, a["filter"], a["stride"], a["padding"])
        elif op.kind == "RESHAPE":
            y = x.reshape(tuple(reversed(o.shape)))
        elif op.kind == "SOFTMAX":
            y = hl.hannk_softmax(x, t[op.inputs[0]].scale[0], a["beta"], o.scale[0], o.zero[0])
        else:
            raise NotImplementedError(op.kind)
        val[op.outputs[0]] = y
    return [val[i] for i in graph.outputs]


def host_us(fn, warmup, reps):
    hip = hl.hip_runtime()
    times = []
    for i in range(warmup + reps):
        hip.hipDeviceSynchronize()
        t0 = time.perf_counter()
        fn()
        hip.hipDeviceSynchronize()
        if i >= warmup:
            times.append(1e6 * (time.perf_counter() - t0))
    return sorted(times)[len(times) // 2]


def mobilenet_times(warmup, reps):
    from halide_amd.hannk_model import HannkModel
    graph, files = mobilenet_graph()
    model = HannkModel(graph).prepare()
    r = np.random.RandomState(0)
    xs = [r.randint(0, 256, tuple(reversed(graph.tensors[i].shape))).astype(np.uint8) for i in graph.inputs]
    model.run_host(*xs)
    return {"case": "mobilenet_v1_0.25_128_21_files", "ops": len(graph.ops), "launches_per_run": len(model.plan),
            "model_launch_resident_us": round(host_us(model.launch, warmup, reps), 1),
            "model_run_host_us": round(host_us(lambda: model.run_host(*xs), warmup, reps), 1),
            "wrappers_us": round(host_us(lambda: wrappers_pass(graph, xs), warmup, max(reps // 3, 3)), 1),
            "method": "host clock around one pass, device idle before and after, median"}


def cases():
    t = np.zeros((16, 28, 384), np.uint8)          # the TRANSPOSE fixture: (16, 28, 384) -> (28, 16, 384)
    yield "transpose_fixture_384x28x16_u8", t, np.zeros((28, 16, 384), np.uint8).transpose(1, 0, 2)
    x = np.zeros((1, 224, 224, 3), np.uint8)       # space-to-depth 224^2 x 3 -> 112^2 x 12
    yield ("space_to_depth_224x224x3_b2_u8", x.reshape(1, 112, 2, 112, 2, 3),
           np.zeros((1, 112, 112, 12), np.uint8).reshape(1, 112, 112, 2, 2, 3).transpose(0, 1, 3, 2, 4, 5))
    for n in (1024, 4096):
        for dtype in (np.uint8, np.uint16, np.float32):
            yield f"transpose_{n}x{n}_{np.dtype(dtype).itemsize}B", np.zeros((n, n), dtype), np.zeros((n, n), dtype).T
    yield "rows_1024x1024_u8_padded", np.zeros((1024, 1040), np.uint8)[:, :1024], np.zeros((1024, 1024), np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out")
    args = ap.parse_args()
    lines = [device_copy_rate(args.warmup, args.reps)]
    print(json.dumps(lines[-1]), flush=True)
    for name, src_like, dst_like in cases():
        base = src_like if src_like.base is None else src_like.base
        while base.base is not None:
            base = base.base
        dbase = dst_like if dst_like.base is None else dst_like.base
        while dbase.base is not None:
            dbase = dbase.base
        ps, pd = device_array(np.ascontiguousarray(base)), device_array(np.ascontiguousarray(dbase))
        s, d = view(ps, src_like), view(pd, dst_like)
        plan = hl.debug_hannk_move_plan(s, d)
        kernel, us = kernel_us(lambda: hl.hannk_copy_from(s, d), args.warmup, args.reps)
        _, general_us = kernel_us(lambda: hl.hannk_copy_from(s, d, True), args.warmup, args.reps)
        nbytes = src_like.size * src_like.itemsize
        lines.append({"case": name, "plan": plan["kernel"], "rank": plan["rank"], "kernel": kernel, "us": round(us, 2), "general_us": round(general_us, 2),
                      "speedup_vs_general": round(general_us / us, 2), "bytes_moved": 2 * nbytes, "GBps": round(2 * nbytes / us / 1e3, 1)})
        print(json.dumps(lines[-1]), flush=True)
        s.device_detach(), d.device_detach()
        hl.hip_runtime().hipFree(ps), hl.hip_runtime().hipFree(pd)
    lines.append(mobilenet_times(args.warmup, args.reps))
    print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
