"""The tile word's light classes (rt_cull.h: bits 20 and up beside the tile
mask, rt_shade.h shade_local_tiny): a camera's second frame on a stream stores,
per tile and light, whether its opaque shadow pass ended with no gated lane
occluded (1, lit), with every lane occluded (2, dark) or otherwise (0); the
camera's later frames skip the passes of class 1 and 2.

Every case renders one camera four times in a row on one stream — masks
computed (<0,1,101>), computed and stored with the classes (<0,1,229>), read
twice (<0,1,37>) — as float RGB and again, after a fresh upload, as RGBA8:
every frame bit for bit the oracle's and the general kernels' (launch_camera=0),
and a counted render's ray, plane-test and quadric-test counts the general
kernels'.  The host picks the mask mode by the camera alone, so a slab off the
8-row grid carries the same labels; its waves have no tile, store no word and
read none.  A frame whose pixels are so wide that the tile cone is capped has
no masks at all: <0,1,37> four times.

Scenes (frames: one tile, two tiles, ragged edges, more than one tile row):
  a   a ground plane and a 12-triangle box; a light high above, one at the
      box centre's height beside it, one below the ground (no lane gated)
  b   the same with 7 and with 13 lights: lights 6 and up have no class
  c   an opaque sphere as the only occluder (the quadric loop's result)
  d   a translucent roof between the high light and everything: a ground tile
      it alone covers is lit (class 1) and takes its colour from the filter
  e   scenes 1-3 of tests/golden/scenes
and through rt_debug_tiny_words the stored words themselves: at 67 x 33 the
class of every whole tile that shows only ground is what the oracle says of
its 64 pixels (rendered with that light alone: all reached, none, some), each
kind present for the first two lights; class 1 on every shaded tile for the
light below the ground; no class on a tile that shows only background; bits
0-19 the masks the parent commit's kernels store (golden/tiny_words.json,
scene a).

Staleness: another camera in between, the scene uploaded again with a light
moved, two streams interleaved, a sequence's four internal streams.
"""
from __future__ import annotations

import ctypes
import json
import math
import os

import numpy as np
import pytest

import rt_amd
from conftest import GOLDEN, bits_equal, rgba8, scene
from hard_frames import Frames
from test_gpu_tiny_scalar import GROUND, HEAD, SAME_COUNTS, light, planes, poly, write

pytestmark = pytest.mark.gpu

LABELS = ["rt_trace_tiny<0,1,%d>" % k for k in (101, 229, 37, 37)]
NO_MASKS = ["rt_trace_tiny<0,1,37>"] * 4
SIZES = [(8, 8), (16, 8), (13, 7), (67, 33)]
W, H = 67, 33  # the words' frame: 8 x 4 whole tiles and a ragged edge
BACKGROUND = np.array([20, 40, 90], np.float32) / np.float32(255)


def box(x0, x1, y0, y1, z0, z1):
    """An axis-aligned box as 12 triangles."""
    c = [(x, y, z) for x in (x0, x1) for y in (y0, y1) for z in (z0, z1)]  # corner 4 ix + 2 iy + iz
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    out = []
    for k, (a, b, d, e) in enumerate(quads):
        out += poly(2 * k % 5, [c[a], c[b], c[d]]) + poly((2 * k + 1) % 5, [c[a], c[d], c[e]])
    return out


# The placements were searched on the oracle (a ring of azimuths at three
# radii and heights) for whole ground tiles of all three kinds at 67 x 33.
BOX = box(-30, 30, -45, 15, -30, 30)  # on the ground y = -45, under the view centre
HIGH = (130.0, 120.0, -75.0)      # high above: the box's shadow falls to the far left of the view
BESIDE = (160.0, -15.0, 0.0)      # at the box centre's height: a shadow that widens across the ground
BESIDE_MOVED = (50.0, -15.0, 86.6)
BELOW = (0.0, -90.0, 0.0)         # below the ground and the box: no surface faces it
THREE = [(HIGH, 0.5), (BESIDE, 0.4), (BELOW, 0.6)]
MORE = [((300.0 - 70.0 * k, 80.0 + 25.0 * k, -200.0 + 55.0 * k), 0.1) for k in range(10)]
# x^2 + (y + 15)^2 + z^2 = 30^2
SPHERE = ["Quad: ball", "        v_quad: 1.000000 1.000000 1.000000", "        v_linear: 0.000 30.000 0.000",
          "        v_const: -675.000", "        color: 230 60 60", "        ambient: 0.2", "        diffus: 0.8"]
# the launch-camera kernels want a triangle: one under the ground, seen by
# no camera ray and crossed by no shadow ray of the lights above it
HIDDEN = poly(1, [(-5, -70, -5), (5, -70, -5), (0, -70, 5)])
# above the camera (y = 60) and far wider than the view, under the high light
ROOF = ["Poly: glass", "        point: 0 -900.0 70.0 -900.0", "        point: 1 900.0 70.0 -900.0",
        "        point: 2 0.0 70.0 1200.0", "        color: 240 200 60", "        ambient: 0.2", "        diffus: 0.5",
        "        refract: 0.600 1.300"]

# name: (lights, the scene after the ground plane)
SCENES = {
    "a_box": (THREE, BOX),
    "a_box_light1_moved": ([THREE[0], (BESIDE_MOVED, 0.4), THREE[2]], BOX),
    "b_lights7": (THREE + MORE[:4], BOX),
    "b_lights13": (THREE + MORE, BOX),
    "c_sphere": (THREE[:2], SPHERE + HIDDEN),
    "d_glass": (THREE[:2], ROOF + BOX),
}
CASES = ["a_box", "b_lights7", "b_lights13", "c_sphere", "d_glass"]


def text(name, only=None, rest=True):
    """The scene's lines; only: that light alone (None: all, -1: none); rest: with what stands on the ground."""
    ls, body = SCENES[name]
    ls = ls if only is None else ([] if only < 0 else [ls[only]])
    return HEAD + sum((light(k, pos, intens) for k, (pos, intens) in enumerate(ls)), []) + planes(GROUND) + \
        (body if rest else [])


# ---- the oracle's view of the tiles
def whole_tiles(a, w, h):
    """(h, w) booleans -> per whole 8 x 8 tile of the frame: all, any of its pixels."""
    ty, tx = h // 8, w // 8
    t = a[: ty * 8, : tx * 8].reshape(ty, 8, tx, 8)
    return t.all(axis=(1, 3)), t.any(axis=(1, 3))


def oracle_kinds(oracle, tmp_path, name, w, h):
    """Per light, per whole tile of the frame that shows nothing but ground:
    1 the light reaches all 64 pixels, 2 none, 0 some; -1 another tile.  The
    ground faces every light above it, so all 64 lanes are gated there and
    `reached` is `not occluded by an opaque surface` (a translucent one
    filters the light and leaves some)."""
    ambient = oracle.render(write(tmp_path, name + "_ambient", text(name, -1)), w, h, 0)
    bare = oracle.render(write(tmp_path, name + "_bare", text(name, -1, False)), w, h, 0)
    ground = (ambient == bare).all(axis=-1) & (ambient != BACKGROUND).any(axis=-1)
    ground_tile = whole_tiles(ground, w, h)[0]
    kinds = []
    for li in range(len(SCENES[name][0])):
        alone = oracle.render(write(tmp_path, f"{name}_alone{li}", text(name, li)), w, h, 0)
        every, some = whole_tiles((alone != ambient).any(axis=-1), w, h)
        kinds.append(np.where(ground_tile, np.where(every, 1, np.where(some, 0, 2)), -1))
    return kinds


def shaded_tiles(oracle, tmp_path, name, w, h):
    """Per tile of the frame (ragged ones too): a pixel of it shows a surface."""
    ambient = oracle.render(write(tmp_path, name + "_ambient", text(name, -1)), w, h, 0)
    ty, tx = (h + 7) // 8, (w + 7) // 8
    pad = np.zeros((ty * 8, tx * 8), bool)
    pad[:h, :w] = (ambient != BACKGROUND).any(axis=-1)
    return pad.reshape(ty, 8, tx, 8).any(axis=(1, 3))


# ---- the device side
@pytest.fixture(scope="module")
def ctx():
    return rt_amd.Context(0)


@pytest.fixture(scope="module")
def general():
    """The same library without the launch-camera kernels."""
    return rt_amd.Context(0, launch_camera=0)


def masked(f):
    """rt_camhost.h tile_wbound: the tile masks (and so the stored words) hold
    while four pixels' distance on the film stays under one radian."""
    px, py = 2.0 * f.half_w * f.inv_w, 2.0 * f.half_h * f.inv_h
    return math.sqrt(16.0 * px * px + 16.0 * py * py) * 1.001 < 1.0


def counts(c):
    st = c.stats()
    return {k: getattr(st, k) for k in SAME_COUNTS}


def words(c, w, h, stream=0):
    """The tile words stored for `stream` (0: the synchronous renders'), as (tile rows, tile columns)."""
    L = rt_amd.lib()
    L.rt_debug_tiny_words.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    L.rt_debug_tiny_words.restype = ctypes.c_int
    ty, tx = (h + 7) // 8, (w + 7) // 8
    out = np.zeros(ty * tx, np.uint32)
    rc = L.rt_debug_tiny_words(c._h, stream or None, out.ctypes.data, out.size)
    if rc != 0:
        raise rt_amd.RtError("rt_debug_tiny_words", rc)
    return out.reshape(ty, tx)


def classes(wd, li):
    return (wd >> np.uint32(20 + 2 * li)) & np.uint32(3)


def four_times(ctx, general, s, frame, want, live=None):
    """`frame` of the scene `s` four times in a row as float RGB, then as
    RGBA8 after a fresh upload, then counted; want: the oracle's rows (live:
    those of them the frame writes)."""
    live = slice(None) if live is None else live
    labels = LABELS if masked(frame) else NO_MASKS
    general.upload(s)
    same = general.render_float(frame)
    assert same.shape == want.shape and bits_equal(same[live], want[live])
    same8 = general.render(frame)
    assert np.array_equal(same8[live], rgba8(want)[live])
    counted = frame.copy()
    counted.flags |= rt_amd.FLAG_STATS
    general.render_float(counted)
    want_counts = counts(general)
    for render, ref in ((ctx.render_float, same), (ctx.render, same8)):
        ctx.upload(s)
        seen = []
        for rep in range(4):
            got = render(frame)
            seen.append(ctx.stats().kernel)
            assert got.dtype == ref.dtype and got.shape == ref.shape
            assert np.array_equal(got[live].view(np.uint8), ref[live].view(np.uint8)), (rep, seen)
        assert seen == labels, seen
    assert bits_equal(ctx.render_float(counted)[live], same[live])
    assert counts(ctx) == want_counts, (counts(ctx), want_counts)
    assert bits_equal(ctx.render_float(frame)[live], same[live])  # the classes again, after the counted render


# ---- scenes and frame shapes
@pytest.mark.parametrize("wh", SIZES)
@pytest.mark.parametrize("name", CASES)
def test_synthetic_scenes(ctx, general, oracle, tmp_path, name, wh):
    w, h = wh
    path = write(tmp_path, name, text(name))
    s = rt_amd.Scene(path, w, h, 0)
    four_times(ctx, general, s, s.frame, oracle.render(path, w, h, 0))


@pytest.mark.parametrize("wh", SIZES)
@pytest.mark.parametrize("i", [1, 2, 3])
def test_golden_scenes(ctx, general, oracle, i, wh):
    w, h = wh
    s = rt_amd.Scene(scene(i), w, h, 0)
    four_times(ctx, general, s, s.frame, oracle.render(scene(i), w, h, 0))


@pytest.mark.parametrize("name", ["a_box", "d_glass"])
def test_row_slab_off_the_tile_grid(ctx, general, oracle, tmp_path, name):
    """No wave's rows are a tile row of the full frame: no word stored or read."""
    path = write(tmp_path, name, text(name))
    s = rt_amd.Scene(path, W, H, 0)
    full = oracle.render(path, W, H, 0)
    f = s.frame.copy()
    f.row_begin, f.row_end = 3, 20
    four_times(ctx, general, s, f, full[3:20])


@pytest.mark.parametrize("name", ["a_box", "c_sphere"])
def test_band_split_of_two(ctx, general, oracle, tmp_path, name):
    w, h, count = 67, 50, 2
    path = write(tmp_path, name, text(name))
    s = rt_amd.Scene(path, w, h, 0)
    full = oracle.render(path, w, h, 0)
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
        four_times(ctx, general, s, f, want, live)


# ---- the stored words
@pytest.mark.parametrize("name", CASES)
def test_stored_classes(ctx, oracle, tmp_path, name):
    path = write(tmp_path, name, text(name))
    s = rt_amd.Scene(path, W, H, 0)
    kinds = oracle_kinds(oracle, tmp_path, name, W, H)
    shaded = shaded_tiles(oracle, tmp_path, name, W, H)
    ls = SCENES[name][0]
    # on the oracle, before anything runs on the device: for each of the
    # first two lights a whole ground tile of each kind
    for li in (0, 1):
        for kind in (0, 1, 2):
            assert (kinds[li] == kind).any(), (name, "light", li, "no tile of kind", kind)
    ctx.upload(s)
    for rep in range(3):
        ctx.render_float(s.frame)
        assert ctx.stats().kernel == LABELS[rep]
        if rep == 0:
            with pytest.raises(rt_amd.RtError):  # a camera's first frame stores nothing
                words(ctx, W, H)
        elif rep == 1:
            wd = words(ctx, W, H)
    assert np.array_equal(words(ctx, W, H), wd), "a reading frame writes no word"
    for li, (pos, _) in enumerate(ls[:6]):
        c = classes(wd, li)
        assert ((c == 0) | shaded).all(), "a tile that was not shaded has no class"
        assert (c != 3).all()
        if pos[1] < -45.0:  # below the ground: no lane is gated anywhere
            assert np.array_equal(c, np.where(shaded, 1, 0)), (name, li, c)
        else:
            k = kinds[li]
            got = c[: H // 8, : W // 8]
            assert np.array_equal(got[k >= 0], k[k >= 0]), (name, li, got, k)
    # lights 6 and up have no bits (there are none to have); a scene of fewer lights leaves the rest zero
    if len(ls) < 6:
        assert (wd >> np.uint32(20 + 2 * len(ls)) == 0).all()
    if name == "a_box":
        with open(os.path.join(GOLDEN, "tiny_words.json")) as f:
            parent = np.array(json.load(f)["a_box_67x33"], np.uint32).reshape(wd.shape)
        assert (parent >> np.uint32(20) == 0).all()
        assert np.array_equal(wd & np.uint32(0xFFFFF), parent)


def test_glass_tiles_are_lit_and_coloured(ctx, oracle, tmp_path):
    """Scene d: a whole ground tile the high light reaches only through the
    roof is of class 1, and on the oracle that light's part of it is not the
    part it has without the roof (the filter's colour)."""
    kinds = oracle_kinds(oracle, tmp_path, "d_glass", W, H)[0]
    assert (kinds == 1).any()
    alone = oracle.render(write(tmp_path, "with_roof", text("d_glass", 0)), W, H, 0)
    SCENES["d_no_roof"] = (SCENES["d_glass"][0], BOX)
    clear = oracle.render(write(tmp_path, "no_roof", text("d_no_roof", 0)), W, H, 0)
    del SCENES["d_no_roof"]
    ty, tx = np.argwhere(kinds == 1)[0]
    assert (alone[8 * ty: 8 * ty + 8, 8 * tx: 8 * tx + 8] != clear[8 * ty: 8 * ty + 8, 8 * tx: 8 * tx + 8]).any(axis=-1).all()
    s = rt_amd.Scene(write(tmp_path, "d_glass", text("d_glass")), W, H, 0)
    ctx.upload(s)
    ctx.render_float(s.frame)
    ctx.render_float(s.frame)
    assert classes(words(ctx, W, H), 0)[ty, tx] == 1


# ---- staleness
def test_another_camera_in_between(oracle, tmp_path):
    path = write(tmp_path, "a_box", text("a_box"))
    s = rt_amd.Scene(path, W, H, 0)
    a = s.frame
    b = s.frame.copy()
    b.cam_pos[0] -= 35.0
    b.cam_pos[2] += 20.0
    fr = Frames(oracle, tmp_path)
    want = {"a": oracle.render(path, W, H, 0), "b": fr.want(path, W, H, 0, frame=b).img}
    assert not bits_equal(want["a"], want["b"])
    c = rt_amd.Context(0)
    c.upload(s)
    seen = []
    for cam in "aaaabbbbaaaa":
        got = c.render_float(a if cam == "a" else b)
        seen.append(c.stats().kernel)
        assert bits_equal(got, want[cam]), (cam, seen)
    assert seen == LABELS * 3, seen


def test_scene_uploaded_again_with_a_light_moved(ctx, oracle, tmp_path):
    seen = []
    for name in ("a_box", "a_box_light1_moved", "a_box"):
        path = write(tmp_path, name, text(name))
        s = rt_amd.Scene(path, W, H, 0)
        want = oracle.render(path, W, H, 0)
        ctx.upload(s)
        for rep in range(4):
            assert bits_equal(ctx.render_float(s.frame), want), (name, rep)
            seen.append(ctx.stats().kernel)
        seen.append(classes(words(ctx, W, H), 1).tolist())
    assert seen[:4] == LABELS and seen[5:9] == LABELS and seen[10:14] == LABELS, seen
    assert seen[4] != seen[9] and seen[4] == seen[14], "light 1's classes follow the light"


def test_two_streams_interleaved(oracle, tmp_path):
    torch = pytest.importorskip("torch")
    path = write(tmp_path, "a_box", text("a_box"))
    s = rt_amd.Scene(path, W, H, 0)
    want = oracle.render(path, W, H, 0)
    c = rt_amd.Context(0)
    c.upload(s)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [[torch.zeros((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(4)] for _ in streams]
    seen = [[], []]
    for rep in range(4):
        for k, st in enumerate(streams):
            c.render_async(s.frame, 0, outs[k][rep].data_ptr(), st.cuda_stream)
            seen[k].append(c.stats().kernel)
    torch.cuda.synchronize()
    for k in range(2):
        assert seen[k] == LABELS, seen
        for rep in range(4):
            assert bits_equal(outs[k][rep].cpu().numpy(), want), (k, rep)
    assert np.array_equal(words(c, W, H, streams[0].cuda_stream), words(c, W, H, streams[1].cuda_stream))


def test_sequence_stores_and_reads_on_its_internal_streams(oracle, tmp_path):
    """rt_render_sequence_async keeps the words per internal stream (four of
    them, frame i on stream i % 4): 12 copies of one camera give every stream
    that camera three times — computed, stored, read —, the same call again
    reads 12 times, and 12 frames cycling through three cameras meet the
    stored camera again only where its words still hold (a stream's other
    cameras are new to it: computed).  Every frame bit for bit the oracle's,
    and so is a synchronous render afterwards.  (A sequence fills no
    rt_stats: which kernel ran is not seen here.)  Cameras: a and b of
    test_another_camera_in_between, and one moved the other way."""
    torch = pytest.importorskip("torch")
    path = write(tmp_path, "a_box", text("a_box"))
    s = rt_amd.Scene(path, W, H, 0)
    cams = [s.frame, s.frame.copy(), s.frame.copy()]
    cams[1].cam_pos[0] -= 35.0
    cams[1].cam_pos[2] += 20.0
    cams[2].cam_pos[0] += 35.0
    cams[2].cam_pos[2] += 20.0
    fr = Frames(oracle, tmp_path)
    want = [oracle.render(path, W, H, 0)] + [fr.want(path, W, H, 0, frame=f).img for f in cams[1:]]
    assert not any(bits_equal(want[i], want[j]) for i, j in ((0, 1), (0, 2), (1, 2)))
    c = rt_amd.Context(0)
    c.upload(s)
    n = 12
    ring = torch.zeros((n, H, W, 3), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for what, order in (("a", [0] * n), ("b", [0] * n), ("c", [i % 3 for i in range(n)])):
        ring.zero_()
        c.render_sequence_async([cams[k] for k in order], 0, 0, ring.data_ptr(), H * W * 12, st)
        torch.cuda.synchronize()
        got = ring.cpu().numpy()
        for i, k in enumerate(order):
            assert bits_equal(got[i], want[k]), (what, i, k)
    assert bits_equal(c.render_float(cams[0]), want[0]), "d"
