"""tests/checker_lib.py itself: a Checker builds once; the resize / gaussian_blur / linear_blur checkers are one object whose one
canonical-form switch restores itself and reaches each of them; another object's switch restores itself too and moves independently.
CPU only; needs neither the product library nor a GPU."""
import numpy as np
import pytest

import checker_lib
from parity_helpers import noise


def test_the_object_is_built_once():
    first = checker_lib.lib()
    assert checker_lib.lib() is first and checker_lib.resize.lib is first and checker_lib.linear_blur.lib is first
    assert all(hasattr(first, fn) for fn in ("ck_set_canon", "rc_resize", "gc_resampled", "lc_blur"))
    assert not any(hasattr(first, fn) for fn in ("rc_set_canon", "gc_set_canon", "lc_set_canon"))


def test_canon_restores_the_form_in_force():
    before = checker_lib.get_canon()
    with checker_lib.canon(1 - before):
        assert checker_lib.get_canon() == 1 - before
        with checker_lib.canon(before):
            assert checker_lib.get_canon() == before
        assert checker_lib.get_canon() == 1 - before
    assert checker_lib.get_canon() == before
    with pytest.raises(KeyError):
        with checker_lib.canon(1 - before):
            raise KeyError("on the way out")
    assert checker_lib.get_canon() == before


def test_a_checker_builds_once_and_binds():
    import wavelet_checker
    second = checker_lib.Checker("second", ("wavelet_check.c",), wavelet_checker._bind, float_forms=True)
    first = second.lib()
    assert second.lib() is first and first is not wavelet_checker.lib() and first is not checker_lib.lib()
    assert first.wc_constant.restype is wavelet_checker.lib().wc_constant.restype and first.ck_get_canon.restype is not None
    plain = checker_lib.Checker("plain", ("compositing_check.c",), lambda L: None)
    assert plain.lib() is plain.lib() and not hasattr(plain.lib(), "ck_set_canon")


def test_canon_restores_on_a_second_object_and_the_switches_are_independent():
    import wavelet_checker as wc
    mine, theirs = checker_lib.get_canon(), wc.get_canon()
    with wc.canon(1 - theirs):
        assert wc.get_canon() == 1 - theirs and checker_lib.get_canon() == mine
        with checker_lib.canon(1 - mine):
            assert checker_lib.get_canon() == 1 - mine and wc.get_canon() == 1 - theirs
        assert checker_lib.get_canon() == mine and wc.get_canon() == 1 - theirs
    assert wc.get_canon() == theirs
    with pytest.raises(KeyError):
        with wc.canon(1 - theirs):
            raise KeyError("on the way out")
    assert wc.get_canon() == theirs and checker_lib.get_canon() == mine
    wc.set_canon(1 - theirs)
    assert checker_lib.get_canon() == mine
    wc.set_canon(theirs)


# Inputs on which the separately built checkers of the parent commit already give different bits in the two forms (measured there):
# each pipeline has a multiply that feeds an add or a subtract on them.
REACHED = {
    "rc_resize": lambda: checker_lib.resize.resize("cubic", noise((3, 40, 50), 50 * 40), 0.37, False),
    "gc_resampled": lambda: checker_lib.gaussian_blur.resampled((3, 2, 8), noise((45, 70), 70), 10.0, 5),
    "lc_blur": lambda: checker_lib.linear_blur.blur("linear_blur", noise((3, 45, 70), 3)),
}


@pytest.mark.parametrize("entry", list(REACHED))
def test_the_one_switch_reaches_every_checker(entry):
    out = {}
    for fma in (0, 1, 0, 1):
        with checker_lib.canon(fma):
            got = REACHED[entry]()
        assert np.array_equal(out.setdefault(fma, got).view(np.uint32), got.view(np.uint32)), f"form {fma} is not reproducible"
    assert out[0].shape == out[1].shape and not np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))
