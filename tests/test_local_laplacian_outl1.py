"""local_laplacian with HLMI_LL_EMIT1=1: ll_down01e stores level 1 as ONE plane, outLPyramid[1], and ll_up0h adds it to its
upsampled level-2 tile, instead of three level-1 planes and a collapse in ll_up0h.  Who computes outLPyramid[1] changes, no
operation does: the u16 result and every outGPyramid level the launch chain materialises must equal the oracle's bit for bit.

Every case runs on the device's own stream, where the switch alone puts the path on, and on a frame queue.  outGPyramid levels:
the default chain materialises 3 .. 1 (4 .. 7 stay inside ll_up_multi); the one-plane path needs the level-2 collapse inside
ll_up0h and with it an ll_up_multi launch, whose coarsest level is the one it stores — HLMI_LL_UPCHAIN_FROM=6 makes that levels
6 .. 1, the most this path can show (test_every_materialised_level_matches_oracle)."""
import numpy as np
import pytest

from test_local_laplacian import _rand_image

ALPHA = 1.0 / 7


def _run(hl, inp, origin, beta=1.0):
    a = hl.Buffer(inp).set_min(origin[0], origin[1], 0)
    o = hl.Buffer(np.zeros_like(inp)).set_min(origin[0], origin[1], 0)
    hl.local_laplacian(a, 8, ALPHA, beta, o)
    return o


def _check(hl, oracle, inp, origin=(0, 0), beta=1.0, top=3):
    o = _run(hl, inp, origin, beta)
    bad = []
    for level in range(top, 0, -1):
        got = hl.debug_local_laplacian_outg(level)
        want = oracle.local_laplacian_outg(inp, 8, ALPHA, beta, level, origin=origin)
        assert got.shape == want.shape
        if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
            ys, xs = np.nonzero(got.view(np.uint32) != want.view(np.uint32))
            bad.append((level, len(ys), int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max())))
    assert not bad, f"(level, #bad, xmin, xmax, ymin, ymax): {bad}"
    got, want = o.numpy(), oracle.local_laplacian(inp, 8, ALPHA, beta, origin=origin)
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} of {got.size} differ"


@pytest.fixture
def emit1(monkeypatch, on_stream):
    monkeypatch.setenv("HLMI_LL_EMIT1", "1")
    return on_stream


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,origin", [(256, 200, (0, 0)), (256, 200, (1, 0)), (256, 200, (2, 0)), (256, 200, (3, 0)), (260, 97, (3, -7))])
def test_column_parities_of_the_level_origins(hl, oracle, emit1, w, h, origin):
    """Input origin x = 0 .. 3 mod 4: every parity of the level-0 / 1 / 2 storage origins, i.e. both lane layouts of the level-2
    taps (lanes L - 1, L / L - 1, L, L + 1) and all three strip widths."""
    _check(hl, oracle, _rand_image(w, h, seed=3 * w + h + origin[0], kind="smooth" if (w + h) & 1 else "uniform"), origin)


@pytest.mark.gpu
@pytest.mark.parametrize("exch", [1, 0])
@pytest.mark.parametrize("units", [0, 48, 4096, 300])
@pytest.mark.parametrize("w,h,origin", [(512, 131, (2, 5)), (776, 250, (-4, 5))])
def test_seams_between_units_and_strips(hl, oracle, monkeypatch, emit1, w, h, origin, exch, units):
    """Rows exchanged through LDS inside a workgroup / every unit walks on to its next level-2 row itself; tall units, 2-row units
    with idle waves, several workgroups stacked, workgroups whose last wave walks its own halo; more than one strip per row."""
    monkeypatch.setenv("HLMI_LL_D01_EXCH", str(exch))
    if units:
        monkeypatch.setenv("HLMI_LL_UNITS0", str(units))
    _check(hl, oracle, _rand_image(w, h, seed=w + h + units + exch, kind="uniform"), origin)


@pytest.mark.gpu
def test_smallest_level_2_boxes(hl, oracle, emit1):
    """64 x 48: level 2 is 16 rows (rows -2 .. 13), three workgroups of at most 7, the last with idle waves.  The plan gives a
    workgroup at least 4 level-2 rows or takes the plain units; a level-2 box is never lower than 4 rows (8 x 1 below: rows
    -2 .. 1), so that fall-back is not reachable from a shape — HLMI_LL_D01_EXCH=0 above is what runs the plain units."""
    _check(hl, oracle, _rand_image(8, 1, seed=12, kind="uniform"))
    _check(hl, oracle, _rand_image(64, 48, seed=11, kind="uniform"))


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("ru", [3, 28, 32])
def test_tile_heights_and_non_temporal_frames(hl, oracle, monkeypatch, emit1, ru, nt):
    monkeypatch.setenv("HLMI_LL_RU", str(ru))
    monkeypatch.setenv("HLMI_LL_NT", str(nt))
    _check(hl, oracle, _rand_image(520, 333, seed=ru + nt, kind="uniform"), (-2, 7))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["uniform", "smooth"])
def test_beta_other_than_one(hl, oracle, emit1, kind):
    _check(hl, oracle, _rand_image(300, 204, seed=5, kind=kind), (0, 0), beta=0.7)


@pytest.mark.gpu
def test_every_materialised_level_matches_oracle(hl, oracle, monkeypatch, emit1):
    """One launch per level down to 2 and up from 6: outGPyramid[6] .. [1] are all stored."""
    monkeypatch.setenv("HLMI_LL_FUSE_FROM", "8")
    monkeypatch.setenv("HLMI_LL_UPCHAIN_FROM", "6")
    _check(hl, oracle, _rand_image(520, 332, seed=9, kind="smooth"), (1, 3), top=6)


@pytest.mark.gpu
def test_different_frames_back_to_back_through_one_workspace(hl, oracle, emit1):
    """The second frame must not read what the first left in planes 1 and K of level 1 (unwritten on this path) or in plane 0."""
    for seed, kind in [(1, "uniform"), (2, "smooth"), (3, "uniform")]:
        inp = _rand_image(520, 332, seed=seed, kind=kind)
        got, want = _run(hl, inp, (0, 0)).numpy(), oracle.local_laplacian(inp, 8, ALPHA, 1.0)
        assert np.array_equal(got, want), seed


@pytest.mark.gpu
def test_switch_off_gives_the_same_image(hl, oracle, monkeypatch, emit1):
    inp = _rand_image(1024, 131, seed=21, kind="uniform")
    on = _run(hl, inp, (0, 0)).numpy()
    monkeypatch.setenv("HLMI_LL_EMIT1", "0")
    off = _run(hl, inp, (0, 0)).numpy()
    assert np.array_equal(on, off)
    assert np.array_equal(on, oracle.local_laplacian(inp, 8, ALPHA, 1.0))
