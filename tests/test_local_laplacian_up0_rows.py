"""local_laplacian with HLMI_LL_UP1_ROWS=1 (on top of HLMI_LL_EMIT1=1): ll_up0r, the form of ll_up0h that keeps no level-1 tile in
LDS.  A wave forms outGPyramid[1] of a coarse row in its row loop, when its output rows reach it: a lane makes its own coarse column
(the stored outLPyramid[1] value + up_from on four taps of the level-2 tile) and takes the columns beside it from the lanes beside
it by wave shifts; lanes 0 and 63 read their outer column from values the wave formed for all its coarse rows beforehand.  Where the
value is formed changes, no operation does: the u16 image and outGPyramid[3 .. 1] must equal the oracle's bit for bit, on the
device's own stream and on a frame queue.

The shapes are the smallest at which this kernel can go wrong: the lane 63 / lane 0 hand-over inside a workgroup (width > 128) and
across workgroups (> 256), a last wave whose lanes right of the image serve a live left neighbour, the coarse column clamp at the
level's right edge, every parity of the level-1 / level-2 origins in x and of the first output row in y, waves with an odd row
count, with one row and with none.

Which cases run ll_up0r: the one-plane path needs the re-cut dataflow, i.e. an input width divisible by 4 and an even origin x (ll_plan:
vec_in, fast).  Width 250 and origin x = 1, 3 therefore run the general chain whatever the switch says; they stay because a switch that
is set must never break them.  Every other case names the launch it expects: the library reports ll_up0r's launches as "ll_up0r" and
ll_up0h's as "ll_up0" (hl.kernel_timing_report), and `_check_rows` asserts which of the two ran."""
import numpy as np
import pytest

from test_local_laplacian import _rand_image
from test_local_laplacian_outl1 import ALPHA, _check, _run


def _check_rows(hl, oracle, inp, origin=(0, 0), beta=1.0, ran=True):
    """_check, and the level-0 launch was ll_up0r's (ran=True), was not (False), or either (None)"""
    hl.kernel_timing_reset()
    hl.kernel_timing(True)
    try:
        _check(hl, oracle, inp, origin, beta)
        names = {k["name"] for k in hl.kernel_timing_report()}
    finally:
        hl.kernel_timing(False)
        hl.kernel_timing_reset()
    if ran is not None:
        assert ("ll_up0r" in names) == ran and ("ll_up0" in names) == (not ran), sorted(names)


@pytest.fixture
def rows1(monkeypatch, on_stream):
    monkeypatch.setenv("HLMI_LL_EMIT1", "1")
    monkeypatch.setenv("HLMI_LL_UP1_ROWS", "1")
    return on_stream


@pytest.mark.gpu
@pytest.mark.parametrize("w", [120, 128, 132, 248, 250, 252, 256, 260, 520])
def test_wave_and_tile_seams_in_x(hl, oracle, rows1, w):
    """120: one wave, its last four lanes right of the image; 132 / 260: a last wave of two live lanes; 248 / 252: a last wave with
    60 / 62 live lanes, lanes 60 / 62 serving their left neighbour; 256 / 520: full waves, the hand-over across workgroups.  250 is not
    divisible by 4: the general chain."""
    _check_rows(hl, oracle, _rand_image(w, 37, seed=w, kind="uniform" if w & 4 else "smooth"), ran=w % 4 == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("oy", [4, 5, -7])
@pytest.mark.parametrize("ox", [0, 1, 2, 3])
def test_parities_of_the_level_origins(hl, oracle, rows1, ox, oy):
    """x: the per-lane column parity of up_from at levels 1 and 2; y: the row parity of vl and which output row meets the first
    new coarse row.  Odd origins x run the general chain."""
    _check_rows(hl, oracle, _rand_image(260, 29, seed=10 * ox + oy + 7, kind="uniform"), (ox, oy), ran=ox % 2 == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("ru", [3, 4, 24, 32, 64])
def test_heights_around_the_rows_of_a_wave(hl, oracle, monkeypatch, rows1, ru):
    """RU - 1: one wave row, short; RU + 1: a second wave row with one row; 2 RU - 1 / 2 RU + 1: an odd count / a second workgroup
    row with one row and waves with none.  Origin y = 1 makes the first output row odd for even RU and changes the parity from
    wave row to wave row for RU = 3."""
    monkeypatch.setenv("HLMI_LL_RU", str(ru))
    for h in (ru - 1, ru + 1, 2 * ru - 1, 2 * ru + 1):
        _check_rows(hl, oracle, _rand_image(132, h, seed=ru + h, kind="uniform"), (0, h & 1))


@pytest.mark.gpu
def test_smallest_boxes(hl, oracle, rows1):
    _check_rows(hl, oracle, _rand_image(8, 1, seed=12, kind="uniform"), ran=None)
    _check_rows(hl, oracle, _rand_image(64, 48, seed=11, kind="uniform"))


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [0, 1])
def test_non_temporal_frames(hl, oracle, monkeypatch, rows1, nt):
    monkeypatch.setenv("HLMI_LL_NT", str(nt))
    _check_rows(hl, oracle, _rand_image(260, 50, seed=nt, kind="uniform"), (-2, 7))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["uniform", "smooth"])
def test_beta_other_than_one(hl, oracle, rows1, kind):
    _check_rows(hl, oracle, _rand_image(300, 70, seed=5, kind=kind), (0, 0), beta=0.7)


@pytest.mark.gpu
def test_different_frames_back_to_back_through_one_workspace(hl, oracle, rows1):
    for seed, kind in [(1, "uniform"), (2, "smooth"), (3, "uniform")]:
        inp = _rand_image(520, 100, seed=seed, kind=kind)
        got, want = _run(hl, inp, (0, 0)).numpy(), oracle.local_laplacian(inp, 8, ALPHA, 1.0)
        assert np.array_equal(got, want), seed


@pytest.mark.gpu
def test_switch_off_gives_the_same_image(hl, oracle, monkeypatch, rows1):
    inp = _rand_image(520, 131, seed=21, kind="uniform")
    hl.kernel_timing_reset()
    hl.kernel_timing(True)
    try:
        on = _run(hl, inp, (0, 0)).numpy()
        names_on = {k["name"] for k in hl.kernel_timing_report()}
        hl.kernel_timing_reset()
        monkeypatch.setenv("HLMI_LL_UP1_ROWS", "0")
        off = _run(hl, inp, (0, 0)).numpy()
        names_off = {k["name"] for k in hl.kernel_timing_report()}
    finally:
        hl.kernel_timing(False)
        hl.kernel_timing_reset()
    assert "ll_up0r" in names_on and "ll_up0" not in names_on, sorted(names_on)
    assert "ll_up0" in names_off and "ll_up0r" not in names_off, sorted(names_off)
    assert on.tobytes() == off.tobytes()
    assert np.array_equal(on, oracle.local_laplacian(inp, 8, ALPHA, 1.0))
