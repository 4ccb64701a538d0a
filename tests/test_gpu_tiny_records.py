"""The launch-camera kernels' packed records (rt_trace_tiny: one launch
record by value, 64-byte light records, the planes' camera-ray constants
computed on the host): every frame must keep its float32 bits.

Checkers: the golden images and the oracle (bit-exact; scene4's Phong
highlights within the powf allowance of test_gpu_parity), and the general
kernels of the same library (RT_OPT_LAUNCH_CAMERA 0 / RT_OPT_LIGHT_BUFFER 0),
which share the device's powf, bit for bit.  Shapes: frames of one pixel, one
tile, ragged edges and more than one tile row; every mask mode of a camera
(computed, stored, read twice); scenes at and around the record's plane
capacity (kTinyPlanes = 2)."""
from __future__ import annotations

import numpy as np
import pytest

import rt_amd
from conftest import bits_equal, rgba8, scene, ulp_diff

pytestmark = pytest.mark.gpu

PHONG_SCENES = {4}  # test_gpu_parity: ocml powf vs glibc powf, <= 8 ulp, RGBA8 within 1
PHONG_ULP = 8
K_TINY_PLANES = 2  # rt_cull.h kTinyPlanes


@pytest.fixture(scope="module")
def ctx():
    return rt_amd.Context(0)


@pytest.fixture(scope="module")
def general():
    """The same library without the launch-camera kernels."""
    return rt_amd.Context(0, launch_camera=0)


def check(got, want, i=0):
    if i in PHONG_SCENES:
        assert ulp_diff(got, want) <= PHONG_ULP
        assert np.abs(rgba8(got).astype(int) - rgba8(want).astype(int)).max() <= 1
    else:
        assert bits_equal(got, want), f"max |d| {np.abs(got - want).max()} ulps {ulp_diff(got, want)}"


def three_renders(ctx, frame):
    """A camera's first frames on the context's stream: masks computed,
    computed and stored, read."""
    out = [ctx.render_float(frame) for _ in range(3)]
    labels = ctx.stats().kernel
    return out, labels


@pytest.mark.parametrize("wh", [(1, 1), (8, 8), (13, 7), (67, 33), (640, 17)])
@pytest.mark.parametrize("i", [1, 2, 3, 4, 5, 6])
def test_ragged_frames(ctx, general, oracle, i, wh):
    w, h = wh
    s = rt_amd.Scene(scene(i), w, h, 0)
    want = oracle.render(scene(i), w, h, 0)
    ctx.upload(s)
    general.upload(s)
    same = general.render_float(s.frame)
    check(same, want, i)
    got, label = three_renders(ctx, s.frame)
    if i == 2:  # (a scene without triangles, such as scene4, takes the general kernels)
        assert label == "rt_trace_tiny<0,1,37>", label
    for g in got:
        assert bits_equal(g, same)


@pytest.mark.parametrize("i", [1, 2, 3, 4, 5, 6])
def test_scene_images_depth0(ctx, golden_images, i):
    s = rt_amd.Scene(scene(i), 64, 48, 0)
    ctx.upload(s)
    for g in three_renders(ctx, s.frame)[0]:
        check(g, golden_images[f"scene{i}_64x48_d0"], i)


def test_same_camera_four_times_then_moved_then_back(oracle, tmp_path):
    """One context, one stream: the mask-computing kernel, the mask-storing
    one, twice the mask-reading one; a moved camera; the first one again."""
    torch = pytest.importorskip("torch")
    w, h = 160, 120
    s = rt_amd.Scene(scene(2), w, h, 0)
    want = oracle.render(scene(2), w, h, 0)
    moved = s.frame.copy()
    moved.cam_pos[0] += 7.5
    moved.cam_pos[2] -= 3.25
    ref = rt_amd.Context(0, launch_camera=0, camera_buffer=0)
    ref.upload(s)
    want_moved = ref.render_float(moved)
    assert bits_equal(ref.render_float(s.frame), want)
    c = rt_amd.Context(0)
    c.upload(s)
    out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    labels = []
    for f, wnt in [(s.frame, want)] * 4 + [(moved, want_moved), (s.frame, want), (s.frame, want)]:
        c.render_async(f, 0, out.data_ptr(), stream)
        labels.append(c.stats().kernel)
        torch.cuda.synchronize()
        assert bits_equal(out.cpu().numpy(), wnt), labels
    assert labels[:4] == ["rt_trace_tiny<0,1,101>", "rt_trace_tiny<0,1,229>", "rt_trace_tiny<0,1,37>",
                          "rt_trace_tiny<0,1,37>"], labels
    assert labels[4] == "rt_trace_tiny<0,1,101>", labels


# ---- synthetic scenes (the reference's .dat format), against the oracle
HEAD = ["* launch-record scene (tests/test_gpu_tiny_records.py)", "        background: 20 40 90",
        "        origin: 150.0 60.0 120.0", "        eye: 0.0 0.0 0.0", "        up:  0.0 1.0 0.0"]
PLANES = [  # [v_linear, v_const]: the ground y = -45, then walls
    ("0.0 1.0 0.0", "45.0"), ("0.0 0.0 1.0", "220.0"), ("1.0 0.0 0.0", "240.0"), ("0.0 -1.0 0.0", "400.0")]


def light(k, pos, intens=0.5):
    return [f"Lumiere: l{k}", "        position: %.3f %.3f %.3f" % pos, "        intens: %.3f" % intens]


def plane(k, translucent=False):
    lin, cst = PLANES[k]
    out = [f"Plane: p{k}", f"        v_linear: {lin}", f"        v_const:  {cst}",
           "        color: %d %d %d" % (40 + 50 * k, 220 - 40 * k, 60 + 30 * k), "        ambient: 0.3",
           "        diffus: 0.7"]
    if translucent:
        out.append("        refract: 0.6 1.3")
    return out


def tris():
    """Three opaque triangles above the ground: a tent and a roof (shadows on
    the planes and on each other)."""
    pts = [[(-40, -45, 30), (40, -45, 30), (0, 35, 0)], [(-40, -45, -30), (0, 35, 0), (40, -45, -30)],
           [(-70, 50, -60), (70, 50, -60), (0, 60, 70)]]
    out = []
    for k, t in enumerate(pts):
        out.append(f"Poly: t{k}")
        for j, p in enumerate(t):
            out.append("        point: %d %.1f %.1f %.1f" % ((j,) + p))
        out += ["        color: %d 90 %d" % (250 - 60 * k, 40 + 90 * k), "        ambient: 0.2", "        diffus: 0.8"]
    return out


SPHERE = ["Quad: ball", "        v_quad: 1.0 1.0 1.0", "        v_linear: -120.0 40.0 60.0", "        v_const: 3925.0",
          "        color: 240 240 30", "        ambient: 0.3", "        diffus: 0.7"]  # a sphere that dips into the ground
THREE_LIGHTS = light(0, (100.0, 400.0, 360.0)) + light(1, (30.0, 80.0, 20.0), 0.6) + light(2, (100.0, 400.0, -300.0))
EIGHT_LIGHTS = sum((light(k, (160.0 * np.cos(k), 120.0 + 30.0 * k, 160.0 * np.sin(k)), 0.15) for k in range(8)), [])

SYNTH = {
    "no_planes": HEAD + THREE_LIGHTS + tris(),
    "planes_at_capacity": HEAD + THREE_LIGHTS + sum((plane(k) for k in range(K_TINY_PLANES)), []) + tris(),
    "planes_one_over": HEAD + THREE_LIGHTS + sum((plane(k) for k in range(K_TINY_PLANES + 1)), []) + tris(),
    "planes_two_over": HEAD + THREE_LIGHTS + sum((plane(k) for k in range(K_TINY_PLANES + 2)), []) + tris(),
    # a translucent plane first in the file: plane[] lists the opaque ground before it
    "translucent_plane_first": HEAD + THREE_LIGHTS + plane(3, translucent=True) + plane(0) + tris(),
    "translucent_planes_over": (HEAD + THREE_LIGHTS + plane(3, translucent=True) + plane(0) + plane(1) +
                                plane(2, translucent=True) + tris()),
    "quadric": HEAD + THREE_LIGHTS + plane(0) + tris() + SPHERE,
    "one_light": HEAD + light(0, (100.0, 400.0, 360.0)) + plane(0) + tris(),
    "eight_lights": HEAD + EIGHT_LIGHTS + plane(0) + plane(1) + tris() + SPHERE,
    # a light exactly in the ground plane (n . L == 0 there) and one below it
    "light_in_plane": HEAD + light(0, (30.0, -45.0, 20.0), 0.6) + light(1, (100.0, 400.0, 360.0)) +
    light(2, (0.0, -90.0, 0.0), 0.4) + plane(0) + tris(),
}


@pytest.mark.parametrize("name", sorted(SYNTH))
@pytest.mark.parametrize("wh", [(96, 64), (21, 11)])
def test_synthetic_scene_matches_oracle(ctx, oracle, tmp_path, name, wh):
    w, h = wh
    path = tmp_path / f"{name}.dat"
    path.write_text("\n".join(SYNTH[name]) + "\n")
    s = rt_amd.Scene(str(path), w, h, 0)
    want = oracle.render(str(path), w, h, 0)
    ctx.upload(s)
    got, label = three_renders(ctx, s.frame)
    assert label.startswith("rt_trace_tiny"), label
    for g in got:
        check(g, want)


def test_camera_inside_the_box(ctx, oracle, tmp_path):
    """scene2's camera moved into its cube: every tile's mask keeps faces all
    around, and the plane lies behind them."""
    text = open(scene(2)).read()
    text = text.replace("origin: 150.0 40.0 75.0", "origin: 50.0 0.0 -25.0").replace("eye: 50.0 0.0 -25.0",
                                                                                     "eye: 50.0 -5.0 -100.0")
    assert "origin: 50.0 0.0 -25.0" in text and "eye: 50.0 -5.0 -100.0" in text
    path = tmp_path / "inside.dat"
    path.write_text(text)
    s = rt_amd.Scene(str(path), 96, 64, 0)
    want = oracle.render(str(path), 96, 64, 0)
    ctx.upload(s)
    got, label = three_renders(ctx, s.frame)
    assert label.startswith("rt_trace_tiny"), label
    for g in got:
        check(g, want)


def test_slabs_and_bands_reassemble(ctx):
    """Scene2 at 200 x 150 as 3 row slabs (off the 8-row tile grid: no masks)
    and as 16-row bands of 3: the whole frame, bit for bit."""
    w, h = 200, 150
    s = rt_amd.Scene(scene(2), w, h, 0)
    ctx.upload(s)
    full = ctx.render_float(s.frame)
    for rep in range(3):
        parts = []
        for r in range(3):
            f = s.frame.copy()
            f.row_begin, f.row_end = r * h // 3, (r + 1) * h // 3
            parts.append(ctx.render_float(f))
        assert bits_equal(np.concatenate(parts, 0), full), rep
    got = np.full_like(full, np.nan)
    for r in range(3):
        f = s.frame.copy()
        f.band_rows, f.band_count, f.band_index = 16, 3, r
        for rep in range(3):
            part = ctx.render_float(f)
        assert part.shape[0] == rt_amd.band_rows(h, 16, 3, r)
        for q in range(part.shape[0] // 16):
            a = (q * 3 + r) * 16
            e = min(h, a + 16)
            got[a:e] = part[q * 16: q * 16 + (e - a)]
    assert bits_equal(got, full)


@pytest.mark.parametrize("i", [1, 2, 3, 5])
@pytest.mark.parametrize("opt", ["light_buffer", "launch_camera"])
def test_options_off_render_the_same(ctx, i, opt):
    """RT_OPT_LIGHT_BUFFER 0 and RT_OPT_LAUNCH_CAMERA 0 take the general
    kernels: the default frame, bit for bit."""
    s = rt_amd.Scene(scene(i), 96, 64, 0)
    ctx.upload(s)
    want = ctx.render_float(s.frame)
    off = rt_amd.Context(0, **{opt: 0})
    off.upload(s)
    got = off.render_float(s.frame)
    assert not off.stats().kernel.startswith("rt_trace_tiny")
    assert bits_equal(got, want)
