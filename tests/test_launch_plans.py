"""The chain shape of the multi-launch host paths of lens_blur, interpolate, bilateral_grid, bgu, camera_pipe and conv_layer_bf16:
which launches one call makes, in which order and how often, by the names the kernel timing reports (the names bench_apps.py and
hlmi_kernel_timing_only select launches by).

Each entry point decides its chain in a plan (lb_plan(), ip_plan(), bg_plan(), bgu_plan(), cp_plan(), conv_bf16_plan() in csrc/)
before anything is enqueued.  tests/golden/launch_plans.json holds the chain of every case below, recorded from the library as it
was before the plans existed; run this module as a script (`python tests/test_launch_plans.py`, on a GPU) to record it again from
the library under HLMI_LIB / halide_amd/lib.  Grids and LDS sizes are not pinned here.
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

# bilateral_grid (bg_plan): (ow, oh, ox, oy, iw, ih, r_sigma) — a 200 x 130 image, and a 37 x 23 output at (5, 3) inside a 64 x 40
# input.  r_sigma picks ZD = int(1 / r_sigma + 0.5) + 2 against the two constants of the plan:
#   0.1    ZD = 12       hist = Par12 (bg_histogram_blurz_par<12>), fused blur + slice with ZP = 12
#   0.077  ZD = 15       12 < ZD <= FZ (16): hist = Par16, ZP = 16
#   0.0625 ZD = 18 > FZ  hist = Serial (bg_histogram_blurz), then bg_blurx, bg_blury, bg_slice
# HLMI_BG_ONE_LAUNCH=1 sets one_launch (bg_fused alone) at ZD <= FZ; HLMI_BG_NO_A32=1 clears a32; a 201-wide input (row stride
# 201, not a multiple of 4) and an input whose min.0 is 2 clear vec.  (vec and a32 pick arguments and instantiations, not names.)
BG_A, BG_B = (200, 130, 0, 0, 200, 130), (37, 23, 5, 3, 64, 40)
BG_CASES = ([("bilateral_grid", s + (r,), {}) for s in (BG_A, BG_B) for r in (0.1, 0.077, 0.0625)] +
            [("bilateral_grid", BG_A + (r,), {"HLMI_BG_ONE_LAUNCH": "1"}) for r in (0.1, 0.077)] +
            [("bilateral_grid", BG_B + (0.1,), {"HLMI_BG_ONE_LAUNCH": "1"}), ("bilateral_grid", BG_A + (0.1,), {"HLMI_BG_NO_A32": "1"}),
             ("bilateral_grid", (200, 130, 0, 0, 201, 130, 0.1), {}), ("bilateral_grid", (37, 23, 5, 3, 62, 40, 0.1, 2), {})])

# bgu (bgu_plan): (ow, oh, s_sigma, r_sigma), the low-res pair one eighth of the output.  The slice kernel's LDS request is
# lds = 4 * nlc * nz * 12 * 4 bytes with nlc = (TW - 1) // big + 3, big = s_sigma * 8 and nz = int(1 / r_sigma) + 2:
#   1/8   lds <= 48 KB           bgu_slice, the LDS window stays
#   1/16  48 KB < lds <= 64 KB   bgu_slice, the window is raised
#   1/32  lds > 64 KB            bgu_slice_direct
BGU_TW, BGU_S = 256, 2
BGU_R = (1 / 8, 1 / 16, 1 / 32)
BGU_CASES = [("bgu", (64, 48, BGU_S, r), {}) for r in BGU_R]


def bgu_slice_lds(s_sigma, r_sigma, factor=8):
    return 4 * ((BGU_TW - 1) // (s_sigma * factor) + 3) * (int(1 / r_sigma) + 2) * 12 * 4


# camera_pipe (cp_plan): (W, H, input min.0, calls).  The input's row stride is even in every case; min.0 = 1 puts the first element
# the kernels read 2 bytes off a 4-byte boundary.  The output is dense.
#   64 x 40, min.0 = 0   one_launch: cp_fused
#   63 x 40, min.0 = 0   odd W: demosaic_vec (cp_demosaic<true>), cp_sharpen
#   64 x 40, min.0 = 1   !demosaic_vec (cp_demosaic<false>), sharpen4 (W % 4 == 0, dense output): cp_sharpen4
#   62 x 40, min.0 = 1   !demosaic_vec, !sharpen4: cp_sharpen
#   two calls, cache on  fresh matrix buffers miss once: cp_setup once (cp_stage_setup), the frame launches twice
CP_OFF = {"HLMI_CP_NO_SETUP_CACHE": "1"}
CP_CASES = ([("camera_pipe", s, CP_OFF) for s in ((64, 40, 0, 1), (63, 40, 0, 1), (64, 40, 1, 1), (62, 40, 1, 1))] +
            [("camera_pipe", s, {}) for s in ((64, 40, 0, 2), (63, 40, 0, 2))])

# conv_layer_bf16 (conv_bf16_plan): (N, H, W, CI, CO, calls).  Every main kernel reports as conv3x3_bf16_mfma: the chain separates
# the filter pre-pass (conv_stage_filter) from the main launch (conv_stage_main).
#   W = 8    layout 2 (conv3x3_bf16_p)
#   W = 126  layout 0 (W > 125: the fallback, conv3x3_bf16_mfma)
#   two calls with one resident filter: conv_filter_bf16 once
# Layout 1 (conv3x3_bf16_lin) has no case: the argument checks admit only CO % 128 == 0 and CI % 64 == 0, and the two window limits
# (AR <= 384 for lin, ARp <= 512 for p) both mean W <= 125, so every call that is `lin` is also `p`.
CONV_CASES = [("conv_layer_bf16", s, {}) for s in ((1, 2, 8, 64, 128, 1), (1, 1, 126, 64, 128, 1), (1, 2, 8, 64, 128, 2))]

# (pipeline, arguments, {switch: value})
CASES = ([("lens_blur", s, {}) for s in LB_SHAPES] + [("lens_blur", LB_SHAPES[0], {k: v}) for k, v in LB_SWITCHES] +
         [("lens_blur", LB_LARGE, env) for env in ({}, {"HLMI_LB_UNFUSED": "1"})] +
         [("interpolate", (640, 480), env) for env in ({}, {"HLMI_IP_UNFUSED": "1"}, {"HLMI_IP_TAIL_FROM": "3"}, {"HLMI_IP_TAIL_FROM": "99"})] +
         [("interpolate", (13, 9), {})] + BG_CASES + BGU_CASES + CP_CASES + CONV_CASES)


def case_id(case):
    name, shape, env = case
    return "-".join([name, "x".join(str(v) for v in shape)] + [f"{k}={v}" for k, v in env.items()])


def _call(hl, name, shape):
    rng = np.random.default_rng(7)
    if name == "lens_blur":
        w, h, slices, focus, scale, samples = shape
        left, right = (hl.Buffer(rng.integers(0, 256, (3, h, w), dtype=np.uint8)) for _ in range(2))
        hl.lens_blur(left, right, slices, focus, scale, samples, hl.Buffer(np.zeros((3, h, w), np.float32)))
    elif name == "bilateral_grid":
        ow, oh, ox, oy, iw, ih, r_sigma = shape[:7]
        inp = hl.Buffer(rng.random((ih, iw), dtype=np.float32)).set_min(*shape[7:])
        hl.bilateral_grid(inp, r_sigma, hl.Buffer(np.zeros((oh, ow), np.float32)).set_min(ox, oy))
    elif name == "bgu":
        ow, oh, s_sigma, r_sigma = shape
        lo, val = (hl.Buffer(rng.random((3, oh // 8, ow // 8), dtype=np.float32)) for _ in range(2))
        hl.bgu(r_sigma, s_sigma, lo, val, hl.Buffer(rng.random((3, oh, ow), dtype=np.float32)), hl.Buffer(np.zeros((3, oh, ow), np.float32)))
    elif name == "camera_pipe":
        w, h, xmin, calls = shape
        raw = hl.Buffer(rng.integers(0, 1024, (h + 18, (w + 23) & ~1), dtype=np.uint16)).set_min(xmin)
        m3, m7 = (hl.Buffer(rng.random((3, 4), dtype=np.float32)) for _ in range(2))   # fresh buffers: the first call misses the cache
        for _ in range(calls):
            hl.camera_pipe(raw, m3, m7, 3700.0, 2.0, 50.0, 1.0, 25, 1023, hl.Buffer(np.zeros((3, h, w), np.uint8)))
    elif name == "conv_layer_bf16":
        n, h, w, ci, co, calls = shape
        inp, bias = hl.Buffer(rng.random((n, h + 2, w + 2, ci), dtype=np.float32)), hl.Buffer(rng.random(co, dtype=np.float32))
        filt = hl.Buffer(rng.random((ci, 3, 3, co), dtype=np.float32))                 # a fresh buffer likewise
        for _ in range(calls):
            hl.conv_layer_bf16(inp, filt, bias, hl.Buffer(np.zeros((n, h, w, co), np.float32)))
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
    assert sorted(golden) == sorted(case_id(c) for c in CASES) and len(CASES) == 40


def test_bgu_cases_reach_the_three_lds_ranges():
    lds = [bgu_slice_lds(BGU_S, r) for r in BGU_R]
    assert lds[0] <= 48 * 1024 < lds[1] <= 64 * 1024 < lds[2]


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
