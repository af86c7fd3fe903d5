"""local_laplacian's memory policy per access class (MemPolicy, csrc/local_laplacian.hip above ld_frame4): on a frame queue
ll_down01e, ll_up0r and ll_down_strip2's chain_fit instances load and store each class of data — the input, outLPyramid[0], the
output, outLPyramid[1], the level-2 / 3 planes — with the flavour the frame-queue policy gives it (plain, nt, or sc1 through a raw
buffer access); on the device's own stream everything is plain.  A flavour changes where a line lives in the caches, never a value:
the u16 image and outGPyramid[3 .. 1] must equal the oracle's bit for bit, levels = 8, alpha = 1/7.

Shapes (u16 RGB): 252 x 70 is one strip of ll_down01e and three workgroups of it vertically, with the seam rows exchanged through
LDS; 520 x 70 is three strips, with wave and tile seams of ll_up0r in x; 300 x 301 has an odd height and a last partial tile of
ll_up0r.  Origins (0, 0), (1, 5) and (2, 5): both parities of the level origins; an odd origin x runs the general chain (ll_plan: the
re-cut dataflow needs an even one), which the policy must leave alone.  Every case names the launches it expects (the library reports
ll_up0r's launches as "ll_up0r", ll_up0h's as "ll_up0").

Where variant libraries of the sweep (scripts/ll_mem_policy_sweep.py: halide_amd/lib/libhlmi_pol<hex>.so) lie next to the product
library, the 520 x 70 case runs through each of them in a process of its own; the committed default needs none of them."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA = 1.0 / 7
SHAPES = [(252, 70), (520, 70), (300, 301)]
VARIANTS = sorted(glob.glob(os.path.join(ROOT, "halide_amd", "lib", "libhlmi_pol*.so")))


def _timed_names(hl, fn):
    hl.kernel_timing_reset()
    hl.kernel_timing(True)
    try:
        r = fn()
        names = {k["name"] for k in hl.kernel_timing_report()}
    finally:
        hl.kernel_timing(False)
        hl.kernel_timing_reset()
    return r, names


def _check_launches(names, stream, recut=True):
    """frame queue: ll_down01 (ll_down01e) and ll_up0r; device stream: ll_up0 (ll_up0h); the general chain (recut=False): no ll_up0r"""
    if not recut:
        assert "ll_up0r" not in names and "ll_up0" in names, sorted(names)
    elif stream == "partition":
        assert "ll_down01" in names and "ll_up0r" in names and "ll_up0" not in names, sorted(names)
    else:
        assert "ll_down01" in names and "ll_up0" in names and "ll_up0r" not in names, sorted(names)


def _check_policy(hl, oracle, stream, inp, origin=(0, 0), beta=1.0):
    from test_local_laplacian_outl1 import _check
    _, names = _timed_names(hl, lambda: _check(hl, oracle, inp, origin, beta))
    _check_launches(names, stream, recut=origin[0] % 2 == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("beta", [1.0, 0.7])
@pytest.mark.parametrize("kind", ["uniform", "smooth"])
@pytest.mark.parametrize("w,h", SHAPES)
def test_shapes_inputs_and_beta(hl, oracle, on_stream, w, h, kind, beta):
    from test_local_laplacian import _rand_image
    _check_policy(hl, oracle, on_stream, _rand_image(w, h, seed=w + h, kind=kind), beta=beta)


@pytest.mark.gpu
@pytest.mark.parametrize("origin", [(0, 0), (1, 5), (2, 5)])
@pytest.mark.parametrize("w,h", SHAPES)
def test_parities_of_the_level_origins(hl, oracle, on_stream, w, h, origin):
    from test_local_laplacian import _rand_image
    _check_policy(hl, oracle, on_stream, _rand_image(w, h, seed=w + 7 * origin[0] + origin[1], kind="uniform"), origin)


@pytest.mark.gpu
def test_two_different_frames_back_to_back_through_one_workspace(hl, oracle, on_stream):
    """A policy that keeps lines on the die for longer must not serve the first frame's to the second: same shape, same
    workspace, same queue, no synchronisation in between beyond the stream's order."""
    from test_local_laplacian import _rand_image
    from test_local_laplacian_outl1 import _run
    frames = [_rand_image(520, 70, seed=1, kind="uniform"), _rand_image(520, 70, seed=2, kind="smooth")]
    outs = [_run(hl, f, (0, 0)) for f in frames]
    for f, o in zip(frames, outs):
        assert np.array_equal(o.numpy(), oracle.local_laplacian(f, 8, ALPHA, 1.0))
    # ... and the second frame's planes are the ones the workspace holds now
    from test_local_laplacian_outl1 import _check
    _check(hl, oracle, frames[0], (0, 0))
    _check(hl, oracle, frames[1], (0, 0))


@pytest.mark.gpu
def test_switch_off_on_a_frame_queue_gives_the_same_image(hl, oracle, monkeypatch):
    """HLMI_LL_NT=0: the device-stream policy on a frame queue — the same launches, the same image"""
    from test_local_laplacian import _rand_image
    from test_local_laplacian_outl1 import _run
    inp = _rand_image(520, 70, seed=21, kind="uniform")
    s = hl.partition_stream(1, 4)
    assert s, "the device refused a frame-queue stream"
    hl.set_stream(s)
    try:
        on, names_on = _timed_names(hl, lambda: _run(hl, inp, (0, 0)).numpy())
        monkeypatch.setenv("HLMI_LL_NT", "0")
        off, names_off = _timed_names(hl, lambda: _run(hl, inp, (0, 0)).numpy())
    finally:
        hl.set_stream(None)
    _check_launches(names_on, "partition")
    _check_launches(names_off, "partition")
    assert on.tobytes() == off.tobytes()
    assert np.array_equal(on, oracle.local_laplacian(inp, 8, ALPHA, 1.0))


@pytest.mark.gpu
@pytest.mark.skipif(not VARIANTS, reason="no libhlmi_pol<hex>.so next to libhlmi.so (scripts/ll_mem_policy_sweep.py builds them)")
@pytest.mark.parametrize("lib", VARIANTS or [None], ids=[os.path.basename(v) for v in VARIANTS] or ["none"])
def test_variant_libraries_of_the_sweep(oracle, tmp_path, lib):
    """the 520 x 70 case on a frame queue through a variant library: a process of its own (this file as a script), HLMI_LIB = the
    variant; the oracle evaluates the canonical float form the VARIANT was built for, whatever library the session loads"""
    from test_local_laplacian import _rand_image
    inp = _rand_image(520, 70, seed=590, kind="uniform")
    np.save(tmp_path / "in.npy", inp)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(tmp_path / "in.npy"), str(tmp_path / "out.npy")],
                       env=dict(os.environ, HLMI_LIB=lib), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ll_down01" in p.stdout and "ll_up0r" in p.stdout, p.stdout
    canon = int(p.stdout.split("canon_fma=")[1].split()[0])
    with oracle.canon(canon):
        want = oracle.local_laplacian(inp, 8, ALPHA, 1.0)
    assert np.array_equal(np.load(tmp_path / "out.npy"), want)


if __name__ == "__main__":   # the child of test_variant_libraries_of_the_sweep
    sys.path.insert(0, ROOT)
    import halide_amd as hl
    inp = np.load(sys.argv[1])
    s = hl.partition_stream(1, 4)
    assert s, "the device refused a frame-queue stream"
    hl.set_stream(s)
    a, o = hl.Buffer(inp), hl.Buffer(np.zeros_like(inp))
    hl.kernel_timing(True)
    hl.local_laplacian(a, 8, ALPHA, 1.0, o)
    print(hl.LIB_PATH, f"canon_fma={hl.canon_fma()}", sorted(k["name"] for k in hl.kernel_timing_report()))
    np.save(sys.argv[2], o.numpy())
    hl.set_stream(None)
