"""The launch-camera kernels' scalar-side paths (rt_trace_tiny): the prologue's
frame arithmetic, the light pass's opaque-plane section and its exits, and the
domain dispatch of the light's distance and direction.

Every case is checked against the oracle (bit for bit) and against the
general kernels of the same library (launch_camera=0), three renders per
camera so that every mask mode runs (masks computed, computed and stored,
read), plus a counted render whose counters must equal the general kernels'
wherever both count the same tests: the rays (a primary ray per pixel, a
shadow ray per gated pixel and light), and the plane and quadric tests (both
kernels run every lane of a wave in step, test each plane and quadric once per
wave for the camera rays, and take shadow_opaque_lb's tests in its order for
the shadow rays).  triangle_tests are not compared: the camera side culls
with tile masks here and with camera lists there.

Shapes are the smallest that reach each path: one pixel, one tile, ragged
edges, more than one tile row; row slabs off the 8-row tile grid (no masks);
16-row bands (the prologue's division); 0..3 opaque planes (the launch record
holds two, the third takes the loop over plane[]) with whole tiles ungated,
occluded by the first plane, only by the second / third, only by a triangle;
a light so far that d^2 leaves the fast square root's domain.
"""
from __future__ import annotations

import numpy as np
import pytest

import rt_amd
from conftest import bits_equal, rgba8, scene, ulp_diff

pytestmark = pytest.mark.gpu

PHONG_SCENES = {4}  # test_gpu_parity: ocml powf vs glibc powf, <= 8 ulp, RGBA8 within 1
PHONG_ULP = 8
SAME_COUNTS = ("primary_rays", "bounce_rays", "shadow_rays", "plane_tests", "quadric_tests")
TINY_SCENES = {1, 2, 3}  # 1 to 20 triangles, an opaque one: the launch-camera kernels (the others: general kernels)


@pytest.fixture(scope="module")
def ctx():
    return rt_amd.Context(0)


@pytest.fixture(scope="module")
def general():
    """The same library without the launch-camera kernels."""
    return rt_amd.Context(0, launch_camera=0)


def check_oracle(got, want, i=0):
    if i in PHONG_SCENES:
        assert ulp_diff(got, want) <= PHONG_ULP
        assert np.abs(rgba8(got).astype(int) - rgba8(want).astype(int)).max() <= 1
    else:
        assert bits_equal(got, want), f"max |d| {np.abs(got - want).max()} ulps {ulp_diff(got, want)}"


def counts(c):
    st = c.stats()
    return {k: getattr(st, k) for k in SAME_COUNTS}


def check_frame(ctx, general, s, frame, want, i=0, tiny=True):
    """`frame` of the uploaded scene `s`: the general kernels against the
    oracle's `want`, then three renders, an RGBA8 and a counted render of the
    launch-camera kernels against the general kernels'."""
    same = general.render_float(frame)
    check_oracle(same, want, i)
    same8 = general.render(frame)
    counted = frame.copy()
    counted.flags |= rt_amd.FLAG_STATS
    general.render_float(counted)
    want_counts = counts(general)
    assert not general.stats().kernel.startswith("rt_trace_tiny")
    for rep in range(3):
        got = ctx.render_float(frame)
        if tiny:
            assert ctx.stats().kernel.startswith("rt_trace_tiny"), ctx.stats().kernel
        assert bits_equal(got, same), rep
    assert np.array_equal(ctx.render(frame), same8)
    assert bits_equal(ctx.render_float(counted), same)
    assert counts(ctx) == want_counts, (counts(ctx), want_counts)


# ---- frame shapes
@pytest.mark.parametrize("wh", [(1, 1), (8, 8), (13, 7), (67, 33)])
@pytest.mark.parametrize("i", [1, 2, 3, 4, 5, 6])
def test_frame_shapes(ctx, general, oracle, i, wh):
    w, h = wh
    s = rt_amd.Scene(scene(i), w, h, 0)
    ctx.upload(s)
    general.upload(s)
    check_frame(ctx, general, s, s.frame, oracle.render(scene(i), w, h, 0), i, tiny=(i in TINY_SCENES))


@pytest.mark.parametrize("i", [1, 2, 3, 5, 6])
def test_row_slabs_off_the_tile_grid(ctx, general, oracle, i):
    """row_begin not a multiple of 8: the wave's rows are no tile row of the
    full frame, so its masks are off and it tests every listed triangle."""
    w, h = 67, 33
    s = rt_amd.Scene(scene(i), w, h, 0)
    full = oracle.render(scene(i), w, h, 0)
    ctx.upload(s)
    general.upload(s)
    for r0, r1 in ((3, 20), (5, 33), (17, 18)):
        f = s.frame.copy()
        f.row_begin, f.row_end = r0, r1
        check_frame(ctx, general, s, f, full[r0:r1], i, tiny=(i in TINY_SCENES))


@pytest.mark.parametrize("count", [2, 3])
def test_bands_of_16_rows(ctx, general, oracle, count):
    """16-row bands dealt to `count` ranks: a wave's first row comes from the
    prologue's division by band_rows."""
    w, h = 67, 50
    s = rt_amd.Scene(scene(2), w, h, 0)
    full = oracle.render(scene(2), w, h, 0)
    ctx.upload(s)
    general.upload(s)
    seen = np.zeros(h, bool)
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
            seen[a:e] = True
        got = general.render_float(f)
        assert got.shape == want.shape
        assert bits_equal(got[live], want[live])
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
    assert seen.all()


# ---- synthetic scenes (the reference's .dat format): opaque planes
W, H = 64, 48
HEAD = ["* scalar-path scene (tests/test_gpu_tiny_scalar.py)", "        background: 20 40 90",
        "        origin: 150.0 60.0 120.0", "        eye: 0.0 0.0 0.0", "        up:  0.0 1.0 0.0"]
GROUND, WALL_Z, WALL_X = ("0.0 1.0 0.0", "45.0"), ("0.0 0.0 1.0", "220.0"), ("1.0 0.0 0.0", "240.0")


def light(k, pos, intens=0.5):
    return [f"Lumiere: l{k}", "        position: %.3f %.3f %.3f" % pos, "        intens: %.3f" % intens]


def plane(k, p):
    lin, cst = p
    return [f"Plane: p{k}", f"        v_linear: {lin}", f"        v_const:  {cst}",
            "        color: %d %d %d" % (40 + 50 * k, 220 - 40 * k, 60 + 30 * k), "        ambient: 0.3",
            "        diffus: 0.7"]


def planes(*ps):
    return sum((plane(k, p) for k, p in enumerate(ps)), [])


def poly(k, pts):
    out = [f"Poly: t{k}"]
    for j, p in enumerate(pts):
        out.append("        point: %d %.1f %.1f %.1f" % ((j,) + p))
    return out + ["        color: %d 90 %d" % (250 - 60 * k, 40 + 90 * k), "        ambient: 0.2",
                  "        diffus: 0.8"]


TENT = poly(0, [(-40, -45, 30), (40, -45, 30), (0, 35, 0)]) + poly(1, [(-40, -45, -30), (0, 35, 0), (40, -45, -30)])
# a roof far wider than the view, between the high light and everything below
ROOF = poly(2, [(-900, 120, -900), (900, 120, -900), (0, 120, 1200)])
# a floor of two triangles where a scene has no ground plane
FLOOR = poly(3, [(-600, -45, -600), (600, -45, -600), (600, -45, 600)]) + \
    poly(4, [(-600, -45, -600), (600, -45, 600), (-600, -45, 600)])
KEY = (100.0, 90.0, 160.0)        # under the roof: lights the ground and the tent
HIGH = (0.0, 400.0, 0.0)          # above the roof: every point below it is in the roof's shadow
BELOW = (0.0, -90.0, 0.0)         # below the ground: ground pixels are not gated for it
BEHIND_Z = (0.0, 60.0, -400.0)    # behind the wall z = -220
BEHIND_X = (-400.0, 60.0, 0.0)    # behind the wall x = -240

# name: (the special light, the scene without its lights); the key light is light 0
OPAQUE = {
    "planes0_only_a_triangle": (HIGH, FLOOR + TENT + ROOF),
    "planes1_ungated": (BELOW, planes(GROUND) + TENT),
    "planes1_only_a_triangle": (HIGH, planes(GROUND) + TENT + ROOF),
    "planes2_first_plane": (BEHIND_Z, planes(WALL_Z, GROUND) + TENT),
    "planes2_only_second_plane": (BEHIND_Z, planes(GROUND, WALL_Z) + TENT),
    "planes2_ungated": (BELOW, planes(GROUND, WALL_Z) + TENT),
    "planes3_only_third_plane": (BEHIND_X, planes(GROUND, WALL_Z, WALL_X) + TENT),
    "planes3_first_plane": (BEHIND_Z, planes(WALL_Z, GROUND, WALL_X) + TENT),
    "planes3_only_a_triangle": (HIGH, planes(GROUND, WALL_Z, WALL_X) + TENT + ROOF),
}


def write(tmp_path, name, lines):
    path = tmp_path / f"{name}.dat"
    path.write_text("\n".join(lines) + "\n")
    return str(path)


@pytest.mark.parametrize("name", sorted(OPAQUE))
def test_opaque_plane_sections(ctx, general, oracle, tmp_path, name):
    special, body = OPAQUE[name]
    path = write(tmp_path, name, HEAD + light(0, KEY) + light(1, special, 0.6) + body)
    want = oracle.render(path, W, H, 0)
    # the special light reaches no pixel of the ground: where the ground (or
    # the floor) shows, the frame is the key light's alone.  (The tent's
    # faces may see it.)  Checked on the oracle, on the CPU.
    alone = oracle.render(write(tmp_path, name + "_key", HEAD + light(0, KEY) + body), W, H, 0)
    dark = (want == alone).all(axis=-1)
    tiles = dark.reshape(H // 8, 8, W // 8, 8).all(axis=(1, 3))
    assert tiles.sum() >= 8, f"{name}: only {tiles.sum()} whole tiles without the special light"
    s = rt_amd.Scene(path, W, H, 0)
    ctx.upload(s)
    general.upload(s)
    check_frame(ctx, general, s, s.frame, want)


# ---- a light beyond the fast square root's domain
def far_scene(pos, with_far=True):
    return HEAD + light(0, KEY) + (light(1, pos, 0.6) if with_far else []) + planes(GROUND) + TENT


@pytest.mark.parametrize("where", ["far", "near"])
def test_far_light(ctx, general, oracle, tmp_path, where):
    """A light 1e17 units up: d^2 = 1e34 is finite but beyond 2^100, so every
    wave takes the IEEE side of the distance / direction dispatch; the same
    light at 400 units takes the fast side."""
    pos = (0.0, 1e17, 0.0) if where == "far" else (0.0, 400.0, 0.0)
    assert np.isfinite(np.float32(pos[1]) * np.float32(pos[1])) and (where == "near" or pos[1] ** 2 > 2.0 ** 100)
    path = write(tmp_path, where, far_scene(pos))
    want = oracle.render(path, W, H, 0)
    without = oracle.render(write(tmp_path, where + "_without", far_scene(pos, False)), W, H, 0)
    assert np.isfinite(want).all()
    assert (want != without).any(axis=-1).mean() > 0.25, "the light must light a good part of the frame"
    s = rt_amd.Scene(path, W, H, 0)
    ctx.upload(s)
    general.upload(s)
    check_frame(ctx, general, s, s.frame, want)
