"""bench.py's measurement helpers: the clock / power sampler must degrade to None fields where the amdgpu hwmon files are absent (this
container), hlmi_kernel_timing_only must select exactly one launch of a chain and restore normal operation afterwards, and a
plain run must print the headline line alone while --full adds the other legs."""
import time

import numpy as np
import pytest


def test_clock_sampler_without_hwmon_files_reports_none():
    import bench
    with bench.ClockSampler(0) as cs:
        time.sleep(0.05)
    s = cs.summary()
    assert set(s) == {"sclk_mhz_median", "sclk_mhz_min", "sclk_mhz_max", "power_w_median", "power_w_max", "samples"}
    assert s["samples"] >= 1
    if cs.freq is None:
        assert s["sclk_mhz_median"] is None and s["sclk_mhz_min"] is None
    if cs.power is None:
        assert s["power_w_median"] is None


def test_headline_input_is_the_protocol_input():
    import bench
    assert bench.HEADLINE_KIND == "noise"
    f = bench.synth_frame(3, 64, 48, kind=bench.HEADLINE_KIND)
    assert f.dtype == np.uint16 and f.shape == (3, 48, 64)
    assert np.array_equal(f, bench.synth_frame(3, 64, 48, kind="noise"))          # seeded
    assert f.min() < 2000 and f.max() > 63000                                     # full range


@pytest.mark.gpu
def test_kernel_timing_only_selects_one_launch_and_restores(hl, oracle):
    rng = np.random.default_rng(5)
    inp = rng.integers(0, 65536, (3, 256, 512), dtype=np.uint16)
    a, o = hl.Buffer(inp), hl.Buffer(np.zeros_like(inp))
    hl.local_laplacian(a, 8, 1.0 / 7.0, 1.0, o)
    want = o.numpy().copy()
    hl.kernel_timing_reset()
    hl.kernel_timing(True)
    hl.local_laplacian(a, 8, 1.0 / 7.0, 1.0, o)
    o.device_sync()
    names = [k["name"] for k in hl.kernel_timing_report()]
    assert "ll_down01" in names and len(names) >= 3
    hl.kernel_timing_reset()
    hl.kernel_timing_only("ll_down01")
    try:
        for _ in range(3):
            hl.local_laplacian(a, 8, 1.0 / 7.0, 1.0, o)
        o.device_sync()
        rep = hl.kernel_timing_report()
        assert [k["name"] for k in rep] == ["ll_down01"] and rep[0]["calls"] == 3
    finally:
        hl.kernel_timing_only(None)
        hl.kernel_timing(False)
        hl.kernel_timing_reset()
    hl.local_laplacian(a, 8, 1.0 / 7.0, 1.0, o)       # normal operation again: the complete chain, the right answer
    assert np.array_equal(o.numpy(), want)
    assert np.array_equal(want, oracle.local_laplacian(inp, 8, 1.0 / 7.0, 1.0))


HEADLINE_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype"}
FULL_ONLY_KEYS = {"roofline", "ms_per_call_one_stream", "value_smooth", "value_natural_tiled", "cpu_baseline"}


def _bench(*argv):
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "HLMI_BENCH_STUB")}
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", *argv], env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone(tmp_path):
    """A plain run times, dumps and prints the headline line; the legs of --full do not run."""
    d = _bench("--steps", "1", "--warmup", "0", "--passes", "1", "--dump-outputs", str(tmp_path))
    assert HEADLINE_KEYS <= set(d) and not (FULL_ONLY_KEYS & set(d))
    assert d["steps"] == 1 and d["warmup"] == 0 and d["value"] > 0 and d["ms_per_step"] > 0
    assert "variants" not in d["config"] and "other_configs" not in d["config"]
    assert sorted(p.name for p in tmp_path.iterdir()) == [f"local_laplacian_frame{i:03d}.npy" for i in range(8)]


@pytest.mark.gpu
def test_full_run_adds_the_other_legs():
    d = _bench("--steps", "1", "--warmup", "0", "--passes", "1", "--full", "--no-cpu-baseline", "--no-other-configs",
               "--no-variants", "--no-ceiling")
    assert HEADLINE_KEYS <= set(d)
    assert d["roofline"]["kernel"] and d["roofline"]["kernel_avg_ms"] > 0
    assert set(d["ms_per_call_one_stream"]) == {"noise", "smooth", "natural"}
    assert "cpu_baseline" not in d and d["config"]["variants"] is None and d["config"]["other_configs"] is None
