"""Per-launch durations of 4K local_laplacian frames IN THE MIX — the headline loop's pattern: 8 noise frames round-robin on the four
frame queues, so that every launch runs beside the other frames' kernels — next to the same launches ALONE on one frame queue
(scripts/kernel_times_part.py's figure: what a launch costs when it has the device to itself).

    [HLMI_LIB=halide_amd/lib/libhlmi<variant>.so] python scripts/kernel_times_mix.py [blocks [passes]]

The durations are the library's own HIP events (hl.kernel_timing), recorded on the launch's stream before and after the launch.
The report gives a mean per launch name, so the script measures in `blocks` blocks of `passes` x 8 frames: mean = over all launches,
median = of the blocks' means.  The events themselves cost a little on every queue: compare builds with each other, not these
figures with bench.py's."""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import halide_amd as hl
import bench

blocks = int(sys.argv[1]) if len(sys.argv) > 1 else 9
passes = int(sys.argv[2]) if len(sys.argv) > 2 else 5
nframes, nq = 8, 4
hip = hl.hip_runtime()
frames = [bench.synth_frame(i) for i in range(nframes)]
ins = [hl.Buffer(f) for f in frames]
outs = [hl.Buffer(np.zeros_like(f)) for f in frames]
queues = [hl.partition_stream(p, nq) for p in range(nq)]


def loop(n, nqueues):
    for _ in range(n):
        for i, (a, o) in enumerate(zip(ins, outs)):
            hl.set_stream(queues[i % nqueues])
            hl.local_laplacian(a, 8, 1 / 7, 1.0, o)
    hl.set_stream(None)
    hip.hipDeviceSynchronize()


def measure(nqueues):
    """{launch name: [mean duration in us of each block]}"""
    loop(3, nqueues)
    per_block = {}
    for _ in range(blocks):
        hl.kernel_timing_reset()
        hl.kernel_timing(True)
        loop(passes, nqueues)
        hl.kernel_timing(False)
        for k in hl.kernel_timing_report():
            per_block.setdefault(k["name"], []).append(k["avg_ms"] * 1e3)
    hl.kernel_timing_reset()
    return per_block


mix, alone = measure(nq), measure(1)
print(f"{hl.LIB_PATH}: {blocks} blocks of {passes} x {nframes} frames; HLMI_LL_CHAIN_FIT={os.environ.get('HLMI_LL_CHAIN_FIT', '(default)')}")
print(f"{'launch':20s} {'mix mean':>9s} {'mix median':>11s} {'alone mean':>11s} {'alone median':>13s}   mix / alone   (us)")
tot = [0.0, 0.0]
for name in mix:
    m, a = mix[name], alone.get(name, [float('nan')])
    mm, am = statistics.median(m), statistics.median(a)
    print(f"{name:20s} {statistics.fmean(m):9.1f} {mm:11.1f} {statistics.fmean(a):11.1f} {am:13.1f} {mm / am:10.2f}")
    tot[0] += mm
    tot[1] += am
print(f"{'sum of medians':20s} {'':9s} {tot[0]:11.1f} {'':11s} {tot[1]:13.1f}")
chain = [n for n in mix if n.startswith(("ll_down_strip2", "ll_down_multi", "ll_up_multi"))]
print("chain (" + " + ".join(chain) + f"): {sum(statistics.median(mix[n]) for n in chain):.1f} us in the mix, "
      f"{sum(statistics.median(alone[n]) for n in chain):.1f} us alone")
