"""The launch-camera kernels' occupied-direction test (RT_OPT_LB_REGION,
rt_lightbuf.h): a shadow ray whose direction from the light lies outside the
cone around the light buffer's cells that hold entries skips its cell lookup.

* option on against option off (the second set of light records, "always
  look"): float RGB, RGBA8 and rt_stats bit for bit — scene1..9, ragged and
  whole tiles, the three mask modes of a camera, sync and async frames, a row
  slab and 16-row bands;
* the bound itself: rt_debug_lb_region counts, one device thread per cell,
  the cells with entries whose cone is not inside the stored float cone —
  none, for the reference scenes and for generated tiny scenes (lights near a
  triangle, inside the triangles' hull, a scene without an opaque triangle),
  which also render like the oracle with the option on and off;
* the bound is not vacuous: scene2's far lights get a narrow cone, a light
  inside the cube gets "always look"."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import rt_amd
from conftest import bits_equal, scene
from fuzz_scenes import fuzz_dat

pytestmark = pytest.mark.gpu

COUNTS = ("primary_rays", "bounce_rays", "shadow_rays", "shadow_tests_skipped", "stack_depth", "light_batch",
          "triangle_tests", "plane_tests", "quadric_tests", "bounce_triangle_tests", "bvh_nodes_visited", "kernel")


@pytest.fixture(scope="module")
def on():
    c = rt_amd.Context(0)
    assert c.get_option("lb_region") == 1.0  # the default
    return c


@pytest.fixture(scope="module")
def off():
    return rt_amd.Context(0, lb_region=0)


def region(ctx, n_lights):
    """rt_debug_lb_region: (rc, [n_lights, 6] = a.xyz, cosB, cells with entries, violations)."""
    L = rt_amd.lib()
    L.rt_debug_lb_region.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    out = np.full(6 * max(n_lights, 1), np.nan)
    rc = L.rt_debug_lb_region(ctx._h, out.ctypes.data, out.size)
    return rc, out.reshape(-1, 6)[:n_lights]


def counts(ctx):
    st = ctx.stats()
    return {k: getattr(st, k) for k in COUNTS}


def frames_of(ctx, frame):
    """A camera's first three frames (tile masks computed, computed and stored,
    read), a counted frame and an RGBA8 frame: images, tallies, kernel labels."""
    imgs, labels = [], []
    for _ in range(3):
        imgs.append(ctx.render_float(frame))
        labels.append(ctx.stats().kernel)
    counted = frame.copy()
    counted.flags |= rt_amd.FLAG_STATS
    imgs.append(ctx.render_float(counted))
    tally = counts(ctx)
    imgs.append(ctx.render(counted))
    return imgs, tally, counts(ctx), labels


def assert_same_frames(a, b):
    ia, ta, ta8, la = a
    ib, tb, tb8, lb = b
    assert la == lb
    assert ta == tb and ta8 == tb8, (ta, tb)
    for x, y in zip(ia[:4], ib[:4]):
        assert bits_equal(x, y)
    assert np.array_equal(ia[4], ib[4])


def check_bound(ctx, n_lights, tiny):
    """violations == 0 for every light; RT_E_STATE exactly where the scene has
    no launch-camera light records.  Returns the rows (or None)."""
    rc, rows = region(ctx, n_lights)
    if not tiny:
        assert rc == -4, rc
        return None
    assert rc == 0, ctx._err()
    for a0, a1, a2, cosb, cells, viol in rows:
        assert viol == 0, rows
        assert (cells == 0) == (cosb == 2.0), rows
        assert cosb in (-2.0, 2.0) or (0.54 <= cosb <= 1.0 and abs(a0 * a0 + a1 * a1 + a2 * a2 - 1.0) < 1e-6), rows
    return rows


SIZES = [(i, 64, 40) for i in range(1, 10)] + [(i, 200, 120) for i in range(1, 10)] + [(2, 480, 270)]


@pytest.mark.parametrize("i,w,h", SIZES)
def test_option_off_renders_the_same(on, off, i, w, h):
    s = rt_amd.Scene(scene(i), w, h, 0)
    on.upload(s)
    off.upload(s)
    a, b = frames_of(on, s.frame), frames_of(off, s.frame)
    assert_same_frames(a, b)
    tiny = a[3][-1].startswith("rt_trace_tiny")
    if i == 2:
        assert tiny and a[3] == ["rt_trace_tiny<0,1,101>", "rt_trace_tiny<0,1,229>", "rt_trace_tiny<0,1,37>"], a[3]
    check_bound(on, s.flat.n_lights, tiny)
    check_bound(off, s.flat.n_lights, tiny)  # (the bound is built either way; the option picks the record set)


@pytest.mark.parametrize("i", [2, 7, 9])
def test_option_off_renders_the_same_with_bounces(on, off, i):
    """Bounce frames take other kernels: the option changes nothing there either."""
    s = rt_amd.Scene(scene(i), 64, 40, 3)
    on.upload(s)
    off.upload(s)
    assert_same_frames(frames_of(on, s.frame), frames_of(off, s.frame))


def test_async_slab_and_bands(on, off):
    """Scene2 at 200 x 120: four async frames on a stream (every mask mode), a
    row slab off the tile grid and one on it, 16-row bands of 3."""
    torch = pytest.importorskip("torch")
    w, h = 200, 120
    s = rt_amd.Scene(scene(2), w, h, 0)
    on.upload(s)
    off.upload(s)
    full = on.render_float(s.frame)
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    out8 = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    got = {}
    for name, c in (("on", on), ("off", off)):
        labels = []
        for _ in range(4):
            out.zero_()
            c.render_async(s.frame, out8.data_ptr(), out.data_ptr(), stream)
            labels.append(c.stats().kernel)
            torch.cuda.synchronize()
            assert bits_equal(out.cpu().numpy(), full), (name, labels)
        got[name] = (labels, out8.cpu().numpy())
    assert got["on"][0] == got["off"][0] and got["on"][0][-1] == "rt_trace_tiny<0,1,37>", got["on"][0]
    assert np.array_equal(got["on"][1], got["off"][1])
    for r0, r1 in ((37, 91), (40, 80)):
        f = s.frame.copy()
        f.row_begin, f.row_end = r0, r1
        f.flags |= rt_amd.FLAG_STATS
        for rep in range(3):
            a, ta = on.render_float(f), counts(on)
            b, tb = off.render_float(f), counts(off)
            assert bits_equal(a, b) and bits_equal(a, full[r0:r1]) and ta == tb, (r0, r1, rep)
    for r in range(3):
        f = s.frame.copy()
        f.band_rows, f.band_count, f.band_index = 16, 3, r
        f.flags |= rt_amd.FLAG_STATS
        for rep in range(3):
            a, ta = on.render_float(f), counts(on)
            b, tb = off.render_float(f), counts(off)
            assert bits_equal(a, b) and ta == tb, (r, rep)
        for q in range(a.shape[0] // 16):
            r0 = (q * 3 + r) * 16
            r1 = min(h, r0 + 16)
            assert bits_equal(a[q * 16: q * 16 + (r1 - r0)], full[r0:r1])


# ---- generated tiny scenes (tests/fuzz_scenes.py), their lights replaced
def blocks_of(text):
    """The scene text as its header lines and its objects' blocks."""
    head, blocks = [], []
    for line in text.rstrip("\n").split("\n"):
        if line[:1] not in (" ", "\t", "*", ""):
            blocks.append([line])
        elif blocks:
            blocks[-1].append(line)
        else:
            head.append(line)
    return head, blocks


def tiny_scene(seed):
    """fuzz_dat(seed) with 1-20 triangles (some get a second scene's, untransformed
    ones) and 1-4 lights by the kind seed % 4: 0 the generator's (at least
    one), 1 each light within half a triangle radius of a triangle, 2 each
    light inside the convex hull of the triangles' corners, 3 the generator's
    with every triangle translucent on seeds 3 and 23 (no opaque triangle)."""
    rng = np.random.default_rng(1000 + seed)
    kind = seed % 4
    head, blocks = blocks_of(fuzz_dat(seed))
    strip = kind in (1, 2)  # the corners in the text are then the corners in the scene
    polys = [b for b in blocks if b[0].startswith("Poly:")]
    if seed % 5 == 4:
        extra = [b for b in blocks_of(fuzz_dat(500 + seed))[1] if b[0].startswith("Poly:")][: 20 - len(polys)]
        for k, b in enumerate(extra):
            b[0] = f"Poly: u{k}"
        polys += extra
    lights = [b for b in blocks if b[0].startswith("Lumiere:")]
    others = [b for b in blocks if not b[0].startswith(("Poly:", "Lumiere:"))]
    if strip:
        polys = [[l for l in b if l.split()[0] not in ("rotate:", "translate:", "scale:")] for b in polys]
    tri = np.array([[[float(x) for x in l.split()[2:5]] for l in b if l.split()[0] == "point:"] for b in polys])
    assert tri.shape == (len(polys), 3, 3) and 1 <= len(polys) <= 20
    n_lights = int(rng.integers(1, 5))
    pos = []
    if kind == 1:
        for _ in range(n_lights):
            t = tri[int(rng.integers(len(tri)))]
            c = t.mean(0)
            d = rng.normal(size=3)
            pos.append(c + d / np.linalg.norm(d) * rng.uniform(0.05, 0.5) * np.linalg.norm(t - c, axis=1).max())
    elif kind == 2:
        corners = tri.reshape(-1, 3)
        pos = [rng.dirichlet(np.ones(len(corners))) @ corners for _ in range(n_lights)]
    if pos:
        lights = [[f"Lumiere: l{k}", "        position: %.3f %.3f %.3f" % tuple(p),
                   "        intens: %.3f" % rng.uniform(0.2, 0.9)] for k, p in enumerate(pos)]
    elif not lights:
        lights = [["Lumiere: l0", "        position: 40.000 150.000 -60.000", "        intens: 0.700"]]
    no_opaque = seed in (3, 23)
    if no_opaque:
        for b in polys:
            b[:] = [l for l in b if l.split()[0] not in ("reflect:", "refract:", "color:")]
            b += ["        color: 200 120 60", "        refract: 0.500 1.300"]
    text = "\n".join(head + sum(lights + others + polys, [])) + "\n"
    assert max(len(l) for l in text.split("\n")) <= 78
    return text, kind, len(lights), no_opaque


SEEDS = list(range(36))


def test_generated_scenes_cover_the_cases():
    kinds = [tiny_scene(seed)[1:] for seed in SEEDS]
    assert len(kinds) >= 30
    for k in range(4):
        assert sum(1 for kind, _, _ in kinds if kind == k) >= 8
    assert sum(1 for _, _, no_opaque in kinds if no_opaque) == 2
    assert {n for _, n, _ in kinds} == {1, 2, 3, 4}


@pytest.mark.parametrize("seed", SEEDS)
def test_generated_tiny_scene(on, off, oracle, tmp_path, seed):
    text, kind, n_lights, no_opaque = tiny_scene(seed)
    path = tmp_path / f"tiny{seed}.dat"
    path.write_text(text)
    w, h = 48, 36
    s = rt_amd.Scene(str(path), w, h, 0)
    assert s.flat.n_lights == n_lights
    want = oracle.render(str(path), w, h, 0)
    on.upload(s)
    off.upload(s)
    a, b = frames_of(on, s.frame), frames_of(off, s.frame)
    assert_same_frames(a, b)
    for img in a[0][:4]:
        assert bits_equal(img, want), f"max |d| {np.abs(img - want).max()}"
    tiny = a[3][-1].startswith("rt_trace_tiny")
    assert tiny == (not no_opaque), a[3]  # (no opaque triangle: no light buffer, the general kernels)
    check_bound(on, n_lights, tiny)


def test_hull_lights_reach_always_look(on, tmp_path):
    """Lights inside the hull of the triangles' corners: where every corner
    belongs to an opaque triangle the cells with entries lie in no half-space,
    so no cone under 1 rad holds them — some of these lights must report
    cosB = -2 (translucent triangles, which make no entries, may leave others
    a cone), and none a violation."""
    always = total = 0
    for seed in [s for s in SEEDS if s % 4 == 2]:
        text, _, n_lights, _ = tiny_scene(seed)
        path = tmp_path / f"hull{seed}.dat"
        path.write_text(text)
        on.upload(rt_amd.Scene(str(path), 48, 36, 0))
        rows = check_bound(on, n_lights, True)
        always += int((rows[:, 3] == -2.0).sum())
        total += len(rows)
    assert total >= 9 and always >= 1, (always, total)


# ---- the bound is not vacuous
def test_scene2_far_lights_get_a_narrow_cone(on):
    s = rt_amd.Scene(scene(2), 64, 40, 0)
    on.upload(s)
    rows = check_bound(on, 3, True)
    for j in (0, 2):  # 600 units from a cube of 60 x 40 x 20
        assert rows[j][3] > 0.9, rows
        assert rows[j][4] > 0
        to_cube = np.array([50.0, 0.0, -25.0]) - np.array([100.0, 400.0, 360.0 if j == 0 else -300.0])
        assert np.dot(rows[j][:3], to_cube / np.linalg.norm(to_cube)) > 0.99, rows
    assert rows[1][3] == -2.0 or -2.0 < rows[1][3] <= 1.0, rows  # 35 units from the cube: either is handled


def test_light_inside_the_cube_always_looks(on, off, oracle, tmp_path):
    text = open(scene(2)).read()
    assert text.count("position: 30.0 0.0 20.0") == 1
    path = tmp_path / "inside.dat"
    path.write_text(text.replace("position: 30.0 0.0 20.0", "position: 50.0 0.0 -25.0"))
    w, h = 96, 64
    s = rt_amd.Scene(str(path), w, h, 0)
    want = oracle.render(str(path), w, h, 0)
    on.upload(s)
    off.upload(s)
    a, b = frames_of(on, s.frame), frames_of(off, s.frame)
    assert_same_frames(a, b)
    for img in a[0][:4]:
        assert bits_equal(img, want)
    rows = check_bound(on, 3, True)
    assert rows[1][3] == -2.0 and rows[1][4] > 0, rows
    assert rows[0][3] > 0.9 and rows[2][3] > 0.9, rows
