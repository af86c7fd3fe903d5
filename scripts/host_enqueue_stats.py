"""scripts/host_enqueue_probe.py's two loops, with the enqueue time of EVERY repetition kept: min / median / max of 15 per mode."""
import os, sys, threading, time, statistics
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import halide_amd as hl
import bench
hip = hl.hip_runtime()
nframes, nq, passes = 8, 4, 16
fr = [bench.synth_frame(i) for i in range(nframes)]
ins = [hl.Buffer(f) for f in fr]
outs = [hl.Buffer(np.zeros_like(f)) for f in fr]
queues = [hl.partition_stream(p, nq) for p in range(nq)]
def one_thread():
    t0 = time.perf_counter()
    for _ in range(passes):
        for i, (a, o) in enumerate(zip(ins, outs)):
            hl.set_stream(queues[i % nq]); hl.local_laplacian(a, 8, 1 / 7, 1.0, o)
    t1 = time.perf_counter(); hl.set_stream(None); hip.hipDeviceSynchronize()
    return t1 - t0
def per_queue_threads():
    def work(q):
        hl.set_stream(queues[q])
        for _ in range(passes):
            for i in range(q, nframes, nq):
                hl.local_laplacian(ins[i], 8, 1 / 7, 1.0, outs[i])
        hl.set_stream(None)
    t0 = time.perf_counter()
    th = [threading.Thread(target=work, args=(q,)) for q in range(nq)]
    for t in th: t.start()
    for t in th: t.join()
    t1 = time.perf_counter(); hip.hipDeviceSynchronize()
    return t1 - t0
n = passes * nframes
for name, fn in (("one host thread", one_thread), ("a host thread per queue", per_queue_threads)):
    fn()
    v = sorted(fn() / n * 1e6 for _ in range(15))
    print(f"{name}: enqueue us per frame over 15 repetitions: min {v[0]:.1f} median {statistics.median(v):.1f} max {v[-1]:.1f}", flush=True)
