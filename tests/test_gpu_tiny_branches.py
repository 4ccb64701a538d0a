"""The launch-camera kernels' exact-math dispatches, the select form of the
light buffer's cube-face choice and the walks that run the triangle test for
every lane (rt_trace_tiny: sqrt_recip_w, recip_det_tiny, lb_cell_sel,
shadow_opaque_tiny's one-cell walk and dcap list).

Every case goes through test_gpu_tiny_scalar's check_frame: the general
kernels of the same library (launch_camera=0) bit for bit against the oracle,
then three renders of the launch-camera kernels (every mask mode), an RGBA8
render and a counted render whose rays, plane tests and quadric tests equal
the general kernels'.  A scene that does not select rt_trace_tiny fails.

Shapes are the smallest that reach each path:
  * scenes 1-3 at one pixel, one tile, ragged edges, more than one tile row;
  * a 64x48 frame of a ground plane with a 12-triangle box and one light,
    straight above the view centre or on one of the two horizontal diagonals
    at the box centre's height: the shadow directions (light to ground point)
    then cross the cube's face boundaries, the |x| = |z| ties on the
    diagonals included; each placement leaves lit and shadowed ground on the
    oracle;
  * a light 1e17 units away (d^2 beyond 2^100: the IEEE side of the distance
    dispatch) and the same light near;
  * a triangle with edges of 1e19 and 1.2e19 in the plane two units under
    the camera: |e1 x e2| = 1.2e38 and 1.7e38, so |det| = |D.y| |e1 x e2|
    passes 2^125 = 4.3e37 where the ray points down steeply enough (|D.y| >
    0.35 / 0.25; the frame's rays have |D.y| from 0.073 to 0.513): waves on
    the IEEE side of the reciprocal's dispatch and waves on the fast side in
    one frame.  The oracle's frame is finite and shows the triangle;
  * a row slab off the 8-row grid and a 16-row band split of 2.
"""
from __future__ import annotations

import numpy as np
import pytest

import rt_amd
from conftest import bits_equal, scene
from test_gpu_tiny_scalar import (GROUND, HEAD, KEY, TENT, check_frame, counts, far_scene, light, planes, poly,
                                  write)

pytestmark = pytest.mark.gpu

W, H = 64, 48


@pytest.fixture(scope="module")
def ctx():
    return rt_amd.Context(0)


@pytest.fixture(scope="module")
def general():
    """The same library without the launch-camera kernels."""
    return rt_amd.Context(0, launch_camera=0)


def upload(ctx, general, path, w=W, h=H):
    s = rt_amd.Scene(path, w, h, 0)
    ctx.upload(s)
    general.upload(s)
    return s


# ---- frame shapes
@pytest.mark.parametrize("wh", [(1, 1), (8, 8), (13, 7), (67, 33)])
@pytest.mark.parametrize("i", [1, 2, 3])
def test_frame_shapes(ctx, general, oracle, i, wh):
    w, h = wh
    s = upload(ctx, general, scene(i), w, h)
    check_frame(ctx, general, s, s.frame, oracle.render(scene(i), w, h, 0), i)


# ---- the cube-face choice
def box(x0, x1, y0, y1, z0, z1):
    """An axis-aligned box as 12 triangles."""
    c = [(x, y, z) for x in (x0, x1) for y in (y0, y1) for z in (z0, z1)]  # corner 4 ix + 2 iy + iz
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    out = []
    for k, (a, b, d, e) in enumerate(quads):
        out += poly(2 * k % 5, [c[a], c[b], c[d]]) + poly((2 * k + 1) % 5, [c[a], c[d], c[e]])
    return out


BOX = box(-30, 30, -45, 15, -30, 30)  # on the ground y = -45, its centre at y = -15, under the view centre
PLACEMENTS = {
    "above": (0.0, 200.0, 0.0),          # the -y face, its four edges towards the horizon
    "diagonal_xz": (200.0, -15.0, 200.0),   # d.x = d.z through the box: the -x / -z boundary
    "diagonal_x_z": (200.0, -15.0, -200.0),  # d.x = -d.z: the -x / +z boundary
}


@pytest.mark.parametrize("where", sorted(PLACEMENTS))
def test_face_choice(ctx, general, oracle, tmp_path, where):
    pos = PLACEMENTS[where]
    ground = planes(GROUND)
    path = write(tmp_path, where, HEAD + light(0, pos, 0.8) + ground + BOX)
    want = oracle.render(path, W, H, 0)
    # on the oracle: ground the light reaches without the box, and of it what
    # the box shadows (the ambient term alone) and what stays lit
    no_box = oracle.render(write(tmp_path, where + "_no_box", HEAD + light(0, pos, 0.8) + ground), W, H, 0)
    ambient = oracle.render(write(tmp_path, where + "_ambient", HEAD + ground), W, H, 0)
    reached = (no_box != ambient).any(axis=-1)
    shadowed = reached & (want == ambient).all(axis=-1)
    lit = reached & (want == no_box).all(axis=-1)
    assert shadowed.sum() >= 32 and lit.sum() >= 32, (where, shadowed.sum(), lit.sum())
    s = upload(ctx, general, path)
    check_frame(ctx, general, s, s.frame, want)


# ---- the IEEE side of the distance dispatch
@pytest.mark.parametrize("where", ["far", "near"])
def test_far_light(ctx, general, oracle, tmp_path, where):
    pos = (0.0, 1e17, 0.0) if where == "far" else (0.0, 400.0, 0.0)
    assert where == "near" or (np.isfinite(np.float32(pos[1]) * np.float32(pos[1])) and pos[1] ** 2 > 2.0 ** 100)
    path = write(tmp_path, where, far_scene(pos))
    want = oracle.render(path, W, H, 0)
    without = oracle.render(write(tmp_path, where + "_without", far_scene(pos, False)), W, H, 0)
    assert np.isfinite(want).all()
    assert (want != without).any(axis=-1).mean() > 0.25, "the light must light a good part of the frame"
    s = upload(ctx, general, path)
    check_frame(ctx, general, s, s.frame, want)


# ---- the IEEE side of the reciprocal's dispatch
CAMERA = (150.0, 60.0, 120.0)  # HEAD's origin
LIGHTS = light(0, KEY) + light(1, (100.0, 300.0, 50.0))


def giant(edge):
    """A triangle in the plane y = 58, two units under the camera, around the
    camera's foot point: e1 = (edge, 0, 0), e2 = (edge / 2, 0, 1.2 edge)."""
    cx, _, cz = CAMERA
    pts = [(cx - 0.5 * edge, 58.0, cz - 0.4 * edge), (cx + 0.5 * edge, 58.0, cz - 0.4 * edge),
           (cx, 58.0, cz + 0.8 * edge)]
    return ["Poly: giant"] + ["        point: %d %.1f %.1f %.1f" % ((j,) + p) for j, p in enumerate(pts)] + \
        ["        color: 200 90 40", "        ambient: 0.2", "        diffus: 0.8"]


@pytest.mark.parametrize("edge", [1e19, 1.2e19])
def test_giant_triangle(ctx, general, oracle, tmp_path, edge):
    cross = np.float32(edge) * np.float32(1.2 * edge)  # |e1 x e2|
    # this frame's camera rays have |D.y| from 0.073 (top row) to 0.513 (bottom row)
    assert np.isfinite(cross) and 0.45 * float(cross) > 2.0 ** 125  # |det| > 2^125 in the lower rows
    assert 0.1 * float(cross) < 2.0 ** 125                          # and inside the domain in the upper rows
    path = write(tmp_path, "giant", HEAD + LIGHTS + giant(edge) + TENT)
    want = oracle.render(path, W, H, 0)
    without = oracle.render(write(tmp_path, "no_giant", HEAD + LIGHTS + TENT), W, H, 0)
    assert np.isfinite(want).all()
    assert (want != without).any(axis=-1).sum() >= 64, "the triangle must show"
    s = upload(ctx, general, path)
    check_frame(ctx, general, s, s.frame, want)


# ---- slabs and bands
def test_row_slab_off_the_tile_grid(ctx, general, oracle):
    w, h = 67, 33
    s = upload(ctx, general, scene(2), w, h)
    full = oracle.render(scene(2), w, h, 0)
    f = s.frame.copy()
    f.row_begin, f.row_end = 3, 20
    check_frame(ctx, general, s, f, full[3:20], 2)


def test_band_split_of_two(ctx, general, oracle):
    w, h, count = 67, 50, 2
    s = upload(ctx, general, scene(2), w, h)
    full = oracle.render(scene(2), w, h, 0)
    for r in range(count):
        f = s.frame.copy()
        f.band_rows, f.band_count, f.band_index = 16, count, r
        rows = rt_amd.band_rows(h, 16, count, r)
        want = np.zeros((rows, w, 3), np.float32)
        live = np.zeros(rows, bool)
        for q in range(rows // 16):
            a = (q * count + r) * 16
            e = min(h, a + 16)
            want[q * 16: q * 16 + (e - a)] = full[a:e]
            live[q * 16: q * 16 + (e - a)] = True
        got = general.render_float(f)
        assert got.shape == want.shape and bits_equal(got[live], want[live])
        for rep in range(3):
            g = ctx.render_float(f)
            assert ctx.stats().kernel.startswith("rt_trace_tiny")
            assert bits_equal(g[live], want[live]), (r, rep)
        counted = f.copy()
        counted.flags |= rt_amd.FLAG_STATS
        general.render_float(counted)
        want_counts = counts(general)
        ctx.render_float(counted)
        assert counts(ctx) == want_counts, (counts(ctx), want_counts)
        assert np.array_equal(ctx.render(f)[live], general.render(f)[live])
