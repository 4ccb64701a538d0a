"""The light buffer's occupied-direction bound (rt_lightbuf.h, RT_OPT_LB_REGION):
its host builder alone (rt_debug_lb_region_build, no device) on hand-made cell
sets.  The stored float cone [a, cosB] must contain, in double and with the
kernel test's rounding allowance, the cone of every cell that holds an entry;
the cell cones are recomputed here (cube-map cell corners, the lookup's 1e-5
widening of u and v, the 1e-6 the library adds to the half-angle)."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

import rt_amd
from conftest import REPO


def build(R, cells):
    """Offsets of a buffer whose `cells` hold one entry each -> [a, cosB, n]."""
    L = rt_amd.lib()
    L.rt_debug_lb_region_build.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    cnt = np.zeros(6 * R * R, np.uint32)
    cnt[np.asarray(cells, np.int64)] = 1
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    out = np.zeros(5, np.float64)
    assert L.rt_debug_lb_region_build(off.ctypes.data, R, out.ctypes.data) == 0
    return out


def face_dir(face, u, v):
    d = {0: (1.0, u, v), 1: (-1.0, u, v), 2: (v, 1.0, u), 3: (v, -1.0, u), 4: (u, v, 1.0), 5: (u, v, -1.0)}[face]
    d = np.array(d, np.float64)
    return d / np.linalg.norm(d)


def angle(a, b):
    return float(np.arctan2(np.linalg.norm(np.cross(a, b)), np.dot(a, b)))


def cell_cone(R, c):
    """(w, W): the centre direction and half-angle of cell c = (face R + j) R + i."""
    face, j, i = c // (R * R), c // R % R, c % R
    du = 1e-5
    u0, u1 = 2.0 * i / R - 1.0 - du, 2.0 * (i + 1) / R - 1.0 + du
    v0, v1 = 2.0 * j / R - 1.0 - du, 2.0 * (j + 1) / R - 1.0 + du
    w = face_dir(face, 0.5 * (u0 + u1), 0.5 * (v0 + v1))
    W = max(angle(w, face_dir(face, u, v)) for u in (u0, u1) for v in (v0, v1))
    return w, W + 1e-6


def assert_contains(R, cells, out):
    """Every cell's cone inside the stored cone: cos(angle(a, w) + W), lowered
    by the test's allowance (1 - 2e-6, 4e-6), is at least the float cosB."""
    a, cosB = out[:3], out[3]
    assert cosB == np.float32(cosB) and all(x == np.float32(x) for x in a)  # floats, as stored
    if cosB == -2.0:
        return
    assert -1.0 < cosB <= 1.0 and abs(np.linalg.norm(a) - 1.0) < 1e-6
    for c in cells:
        w, W = cell_cone(R, c)
        need = angle(a, w) + W
        assert need < 1.0
        assert np.cos(need) * (1.0 - 2e-6) - 4e-6 >= cosB, (c, need, cosB)


def cell(R, face, i, j):
    return (face * R + j) * R + i


@pytest.mark.parametrize("R", [16, 128])
def test_no_cell_never_looks(R):
    out = build(R, [])
    assert out[3] == 2.0 and out[4] == 0


@pytest.mark.parametrize("R", [16, 128, 144])
@pytest.mark.parametrize("where", ["centre", "corner", "edge"])
def test_one_cell(R, where):
    for face in range(6):
        i, j = {"centre": (R // 2, R // 2), "corner": (0, R - 1), "edge": (R - 1, R // 3)}[where]
        c = cell(R, face, i, j)
        out = build(R, [c])
        assert out[4] == 1
        assert_contains(R, [c], out)
        w, W = cell_cone(R, c)
        assert out[3] > -2.0 and angle(out[:3], w) < 1e-6  # one cell: its own cone, nearly
        assert np.arccos(out[3]) < W + 4e-3  # (the 6e-6 on the cosine is 3.5e-3 rad at angle 0)


def test_patch_across_a_cube_edge():
    """A 6 x 6 patch around the edge between faces 0 (+x) and 2 (+y)."""
    R = 128
    cells = [cell(R, 0, R - 1 - k, j) for k in range(3) for j in range(60, 66)]
    cells += [cell(R, 2, i, R - 1 - k) for k in range(3) for i in range(60, 66)]
    out = build(R, cells)
    assert out[4] == len(cells)
    assert_contains(R, cells, out)
    assert out[3] > 0.9


def test_two_opposite_faces_always_look():
    R = 16
    cells = [cell(R, 0, 8, 8), cell(R, 1, 8, 8)]
    out = build(R, cells)
    assert out[3] == -2.0 and out[4] == 2


def test_wide_sets():
    """A whole face (0.955 rad to its corners: a bound or "always look",
    either must hold) and three faces around a cube corner (beyond the 1 rad
    a bound may have)."""
    R = 16
    face = [cell(R, 4, i, j) for i in range(R) for j in range(R)]
    out = build(R, face)
    assert out[4] == R * R and out[3] < np.cos(0.955)
    assert_contains(R, face, out)
    three = [cell(R, f, i, j) for f in (0, 2, 4) for i in range(R) for j in range(R)]
    out = build(R, three)
    assert out[3] == -2.0 and out[4] == 3 * R * R


def test_all_cells_always_look():
    R = 16
    out = build(R, list(range(6 * R * R)))
    assert out[3] == -2.0 and out[4] == 6 * R * R


def test_half_a_face_is_bounded():
    """The largest sets that still get a bound: a disc of 0.7 rad around +z."""
    R = 32
    cells = [c for c in range(6 * R * R) if angle(cell_cone(R, c)[0], np.array([0.0, 0.0, 1.0])) < 0.7]
    out = build(R, cells)
    assert out[4] == len(cells) and -2.0 < out[3] < np.cos(0.7)
    assert_contains(R, cells, out)


def test_random_patches():
    rng = np.random.default_rng(5)
    R = 128
    for _ in range(20):
        face, i0, j0 = int(rng.integers(6)), int(rng.integers(R - 12)), int(rng.integers(R - 12))
        cells = [cell(R, face, i0 + int(rng.integers(12)), j0 + int(rng.integers(12))) for _ in range(25)]
        cells = sorted(set(cells))
        out = build(R, cells)
        assert out[4] == len(cells) and out[3] > 0.9
        assert_contains(R, cells, out)


def test_bad_arguments():
    L = rt_amd.lib()
    L.rt_debug_lb_region_build.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    out = np.zeros(5)
    off = np.zeros(7, np.uint32)
    assert L.rt_debug_lb_region_build(None, 1, out.ctypes.data) == -1
    assert L.rt_debug_lb_region_build(off.ctypes.data, 0, out.ctypes.data) == -1
    assert L.rt_debug_lb_region_build(off.ctypes.data, 1, None) == -1


def test_option_is_bound_and_round_trips():
    assert rt_amd.LB_OPTIONS == {"lb_region": 21}
    assert not set(rt_amd.LB_OPTIONS) & (set(rt_amd.OPTIONS) | set(rt_amd.SS_OPTIONS))
    text = open(os.path.join(REPO, "include", "rt.h")).read()
    assert "#define RT_OPT_LB_REGION 21" in text
    L = rt_amd.lib()
    h = ctypes.c_void_p()
    assert L.rt_create_cpu(1, ctypes.byref(h)) == 0
    try:
        got = ctypes.c_double()
        assert L.rt_get_option(h, 21, ctypes.byref(got)) == 0 and got.value == 1.0  # on by default
        assert L.rt_set_option(h, 21, ctypes.c_double(0)) == 0
        assert L.rt_get_option(h, 21, ctypes.byref(got)) == 0 and got.value == 0.0
    finally:
        L.rt_destroy(h)
