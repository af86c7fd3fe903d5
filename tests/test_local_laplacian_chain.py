"""local_laplacian's three short launches between the two big kernels — ll_down_strip2, ll_down_multi, ll_up_multi — have a second
set of instances, HLMI_LL_CHAIN_FIT, that keep fewer loads in flight so as to fit the registers a full CU has left (at most 56 per
lane).  What is in flight changes, no operation and no operand does: the u16 result and every outGPyramid level the test hook
reaches must equal the oracle's bit for bit with the switch at 0 and at 1, with the one-plane level 1 (HLMI_LL_EMIT1) on and off,
on the device's stream and on a frame queue.

Shapes: the smallest at which level 7 is 1 to 5 pixels wide or high beyond its margin (136 x 136, 520 x 392, 1000 x 600: several
16 x 16 tiles of level 3 and 4 x 4 tiles of level 7 with a last partial one, more than one ll_down_strip2 unit per column);
input / output minima (0,0), (1,0), (0,1), (3,5): all four parity instances of ll_down_strip2.  The reference of a case is
computed once and shared by its four switch settings."""
import functools

import numpy as np
import pytest

from test_local_laplacian import _rand_image


@functools.lru_cache(maxsize=None)
def _case(w, h, origin, levels, top):
    """(input, expected u16 image, {level: expected outGPyramid[level]}); read-only"""
    import oracle_lib as oracle
    inp = _rand_image(w, h, seed=7 * w + h + 3 * origin[0] + origin[1], kind="uniform" if (w // 8) & 1 else "smooth")
    alpha = 1.0 / (levels - 1)
    want = oracle.local_laplacian(inp, levels, alpha, 1.0, origin=origin)
    outg = {lv: oracle.local_laplacian_outg(inp, levels, alpha, 1.0, lv, origin=origin) for lv in range(top, 0, -1)}
    for a in (inp, want, *outg.values()):
        a.setflags(write=False)
    return inp, want, outg


def _check(hl, monkeypatch, w, h, origin, levels=8, top=3):
    inp, want, outg = _case(w, h, origin, levels, top)
    bad = []
    for fit in (0, 1):
        for emit1 in (0, 1):
            monkeypatch.setenv("HLMI_LL_CHAIN_FIT", str(fit))
            monkeypatch.setenv("HLMI_LL_EMIT1", str(emit1))
            a = hl.Buffer(inp.copy()).set_min(origin[0], origin[1], 0)
            o = hl.Buffer(np.zeros_like(inp)).set_min(origin[0], origin[1], 0)
            hl.local_laplacian(a, levels, 1.0 / (levels - 1), 1.0, o)
            for lv, ref in outg.items():
                got = hl.debug_local_laplacian_outg(lv)
                assert got.shape == ref.shape
                n = np.count_nonzero(got.view(np.uint32) != ref.view(np.uint32))
                if n:
                    bad.append((fit, emit1, f"outGPyramid[{lv}]", n))
            n = np.count_nonzero(o.numpy() != want)
            if n:
                bad.append((fit, emit1, "output", n))
    assert not bad, f"(CHAIN_FIT, EMIT1, what, values that differ): {bad}"


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,origin", [(136, 136, (0, 0)), (136, 136, (3, 5)), (520, 392, (1, 0)), (520, 392, (0, 1)),
                                        (1000, 600, (0, 0)), (1000, 600, (3, 5))])
def test_fit_instances_match_oracle(hl, monkeypatch, on_stream, w, h, origin):
    _check(hl, monkeypatch, w, h, origin)


@pytest.mark.gpu
def test_seven_levels(hl, monkeypatch, on_stream):
    """levels = 7: seven planes per pyramid level through the chain kernels (and ll_down_strip for levels 2 to 4: the two-level
    walk is built for eight)."""
    _check(hl, monkeypatch, 520, 392, (3, 5), levels=7)


@pytest.mark.gpu
@pytest.mark.parametrize("switch,value,top", [("HLMI_LL_UPCHAIN_FROM", 4, 4), ("HLMI_LL_FUSE_FROM", 5, 5), ("HLMI_LL_UPCHAIN_FROM", 1, 1),
                                              ("HLMI_LL_FUSE_FROM", 3, 3)])
def test_other_depths_of_the_multi_level_kernels(hl, monkeypatch, on_stream, switch, value, top):
    """ll_up_multi<3> (collapse from level 4), ll_down_multi<2> / ll_up_multi<2> (levels 6 and 7 only), ll_up_multi<6> (three groups
    of levels), ll_down_multi<4>: every fit instance a switch can reach, and the levels it stores."""
    monkeypatch.setenv(switch, str(value))
    _check(hl, monkeypatch, 520, 392, (0, 1), top=top)
