"""ctypes bindings to tests/cpp/reaction_diffusion_check.c, the plain-C checker of reaction_diffusion_init, reaction_diffusion_update
and reaction_diffusion_render — TEST INFRASTRUCTURE ONLY.

A checker_lib.Checker with float forms: a shared object of its own, with a canonical-form switch of its own, separate from every
other checker's and the oracle's.  tests/test_reaction_diffusion.py and scripts/fuzz_parity.py both come here.  Imports neither the
product nor torch."""
from __future__ import annotations

import ctypes as C

import numpy as np

from checker_lib import Checker

NAMES = ("reaction_diffusion_init", "reaction_diffusion_update", "reaction_diffusion_render")
CALLS = ("init", "row_min", "row_max", "col_min", "col_max", "noise")   # rdc_table's rows
f32 = np.float32


def _bind(L):
    I, F, P = C.c_int, C.c_float, C.c_void_p
    L.rdc_random_int.restype, L.rdc_random_int.argtypes = C.c_uint32, [P, I]
    L.rdc_random_float.restype, L.rdc_random_float.argtypes = F, [P, I]
    L.rdc_table.argtypes = [I, I]
    L.rdc_init_value.restype, L.rdc_init_value.argtypes = F, [I, I, I]
    L.rdc_edge_value.restype, L.rdc_edge_value.argtypes = F, [I, I, I, I]
    L.rdc_noise.restype, L.rdc_noise.argtypes = F, [I, I, I, I]
    L.rdc_blurry_noise.restype, L.rdc_blurry_noise.argtypes = F, [I, I, I, I]
    L.rdc_init.argtypes = [P, I, I, I, I, I, I]
    L.rdc_clobber_box.restype, L.rdc_clobber_box.argtypes = None, [I, I, I, I, P]
    L.rdc_update.argtypes = [P, I, I, I, I, I, I, I, I, P, I, I, I, I]
    L.rdc_pack.restype, L.rdc_pack.argtypes = C.c_uint32, [F, F, F]
    L.rdc_render.argtypes = [P, P, I, I]


checker = Checker("reaction_diffusion", ("reaction_diffusion_check.c",), _bind, float_forms=True)
lib, set_canon, get_canon, canon = checker.lib, checker.set_canon, checker.get_canon, checker.canon


def table():
    """{call: (id, tag)} as the checker holds it"""
    return {name: (lib().rdc_table(i, 0), lib().rdc_table(i, 1)) for i, name in enumerate(CALLS)}


def _args(e):
    return np.ascontiguousarray(np.asarray(e, np.int64).astype(np.uint32).view(np.int32))


def random_int(e):
    """random_int of one argument list (any integers, taken modulo 2^32)"""
    a = _args(e)
    return int(lib().rdc_random_int(a.ctypes.data, a.size))


def random_float(e):
    a = _args(e)
    return f32(lib().rdc_random_float(a.ctypes.data, a.size))


def edge_value(which, frame, c, v):
    """random_float(frame) * 0.2f of edge definition `which` ("row_min", ...) at channel c and coordinate v (x for rows, y for columns)"""
    return f32(lib().rdc_edge_value(CALLS.index(which), _i32(frame), c, v))


def blurry_noise(frame, x, y, c):
    return f32(lib().rdc_blurry_noise(_i32(frame), x, y, c))


def noise_value(frame, x, y, c):
    return f32(lib().rdc_noise(_i32(frame), x, y, c))


def _i32(v):
    """an int32 that wraps"""
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


def clobber_box(w, h, mouse_x, mouse_y):
    box = (C.c_int * 4)()
    lib().rdc_clobber_box(w, h, mouse_x, mouse_y, box)
    return tuple(box)


def init(shape, mins=(0, 0, 0)):
    """shape (C, H, W) at mins (x, y, c)"""
    out = np.zeros(shape, f32)
    assert lib().rdc_init(out.ctypes.data, mins[0], mins[1], mins[2], shape[2], shape[1], shape[0]) == 0
    return out


def update(state, mouse_x, mouse_y, frame, state_min=(0, 0), out_shape=None, out_min=None, stage=2, expect=0):
    """state: (3, H, W) at mins state_min = (x, y); the output (3, H', W') at out_min, default the state's own box.  stage: 0 the pure
    stage alone, 1 with the edge updates, 2 everything"""
    state = np.ascontiguousarray(state, f32)
    assert state.ndim == 3 and state.shape[0] == 3
    out_shape = state.shape if out_shape is None else out_shape
    out_min = state_min if out_min is None else out_min
    out = np.zeros(out_shape, f32)
    r = lib().rdc_update(state.ctypes.data, state_min[0], state_min[1], state.shape[2], state.shape[1], mouse_x, mouse_y, _i32(frame), stage,
                         out.ctypes.data, out_min[0], out_min[1], out_shape[2], out_shape[1])
    assert r == expect, r
    return out


def run(state, mouse_x, mouse_y, frame0, steps, state_min=(0, 0)):
    """`steps` updates of the full frame, frames frame0 .. frame0 + steps - 1 (wrapping int32)"""
    for k in range(steps):
        state = update(state, mouse_x, mouse_y, _i32(frame0 + k), state_min=state_min)
    return state


def render(state):
    """state: (3, H, W) -> (H, W) uint32"""
    state = np.ascontiguousarray(state, f32)
    out = np.zeros(state.shape[1:], np.uint32)
    assert lib().rdc_render(state.ctypes.data, out.ctypes.data, state.shape[2], state.shape[1]) == 0
    return out


def pack(s0, s1, s2):
    return int(lib().rdc_pack(float(s0), float(s1), float(s2)))
