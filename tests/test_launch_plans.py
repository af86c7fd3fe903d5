"""The chain shape of the multi-launch host paths of lens_blur and interpolate: which launches one call makes, in which order and
how often, by the names the kernel timing reports (the names bench_apps.py and hlmi_kernel_timing_only select launches by).

Both entry points decide their chain in a plan (lb_plan() / ip_plan(), csrc/lens_blur.hip and csrc/interpolate.hip) before
anything is enqueued.  tests/golden/launch_plans.json holds the chain of every case below, recorded from the library as it was
before the plans existed; run this module as a script (`python tests/test_launch_plans.py`, on a GPU) to record it again from the
library under HLMI_LIB / halide_amd/lib.  Grids and LDS sizes are not pinned here.
"""
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_plans.json")

LB_SHAPES = [(200, 130, 32, 13, 0.5, 32), (130, 17, 64, 32, 0.25, 16), (37, 23, 5, 2, 0.7, 7), (1, 1, 1, 1, 0.0, 1)]
LB_LARGE = (1100, 960, 3, 1, 1.0, 2)   # levels above the one-launch tail: lb_down:2, lb_down:3, lb_tail:4, lb_pull_multi:1
LB_SWITCHES = [("HLMI_LB_UNFUSED", "1"), ("HLMI_LB_NO_A32", "1"), ("HLMI_LB_WCY_LAUNCH", "1"), ("HLMI_LB_ROWS2", "0"), ("HLMI_LB_NDY", "3")]
# (pipeline, arguments, {switch: value})
CASES = ([("lens_blur", s, {}) for s in LB_SHAPES] + [("lens_blur", LB_SHAPES[0], {k: v}) for k, v in LB_SWITCHES] +
         [("lens_blur", LB_LARGE, env) for env in ({}, {"HLMI_LB_UNFUSED": "1"})] +
         [("interpolate", (640, 480), env) for env in ({}, {"HLMI_IP_UNFUSED": "1"}, {"HLMI_IP_TAIL_FROM": "3"}, {"HLMI_IP_TAIL_FROM": "99"})] +
         [("interpolate", (13, 9), {})])


def case_id(case):
    name, shape, env = case
    return "-".join([name, "x".join(str(v) for v in shape)] + [f"{k}={v}" for k, v in env.items()])


def _call(hl, name, shape):
    rng = np.random.default_rng(7)
    if name == "lens_blur":
        w, h, slices, focus, scale, samples = shape
        left, right = (hl.Buffer(rng.integers(0, 256, (3, h, w), dtype=np.uint8)) for _ in range(2))
        hl.lens_blur(left, right, slices, focus, scale, samples, hl.Buffer(np.zeros((3, h, w), np.float32)))
    else:
        w, h = shape
        hl.interpolate(hl.Buffer(rng.random((4, h, w), dtype=np.float32)), hl.Buffer(np.zeros((3, h, w), np.float32)))


def chain(hl, case):
    """[[launch name, calls], ...] of one call, in the order of each name's first launch."""
    name, shape, env = case
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)            # the library reads its switches at every call
    hl.kernel_timing(True)
    hl.kernel_timing_reset()
    try:
        _call(hl, name, shape)
        return [[k["name"], k["calls"]] for k in hl.kernel_timing_report()]
    finally:
        hl.kernel_timing(False)
        hl.kernel_timing_reset()
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(case_id(c) for c in CASES) and len(CASES) == 16


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_chain_is_the_recorded_one(hl, golden, case):
    assert chain(hl, case) == golden[case_id(case)]


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    import halide_amd
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(case_id(c))}: {json.dumps(chain(halide_amd, c))}" for c in CASES) + "\n}\n")   # a case per line
    print(f"wrote {GOLDEN}: {len(CASES)} cases from {halide_amd.LIB_PATH}")
