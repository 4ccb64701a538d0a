"""The tile facts (rt_cull.h tile_facts_pack): the second word a camera's second
frame on a stream stores beside each tile's word — the one surface the tile
shows and how the search found it, and per light whether its pass left the
colour bit-identical (no-op) and whether every shaded lane faces it (all
gated) — and what the camera's later frames do with it (rt_trace_tiny,
shade_local_tiny): keep the background of a tile that missed, take the known
surface's records early and test only its primitive, skip a no-op pass.

Every case is test_gpu_tiny_light_classes.four_times: one camera four times on
one stream as float RGB and, after a fresh upload, as RGBA8, labels <0,1,101>,
<0,1,229>, <0,1,37>, <0,1,37>, every frame bit for bit the oracle's and the
general kernels', a counted render with the general kernels' counts, one more
reading frame.

Scenes (the camera and the box of test_gpu_tiny_light_classes; placements
searched on the oracle; what each shows at 67 x 33 is asserted on the CPU, from
the oracle's frames and the CPU id plane of tests/aov_ref.py, before anything
runs on the device):
  walls   ground, a wall z = -220, a wall x = -240 and the box: whole tiles on
          plane slot 0, on slot 1, on a third plane (found by the full search),
          on one triangle, on a face's two triangles (same colour, two file
          indices: no surface), silhouettes; a light below the ground (no lane
          gated: no-op), tiles in the box's shadow (dark, no Phong: no-op),
          tiles every lane of which faces a light
  sky     the box alone, seven lights: tiles that miss, the silhouette against
          the background; a seventh light (no facts)
  ball    a sphere on the ground: a whole tile on a quadric, the terminator of
          the low light across a tile
  phong   the ground with ks > 0, shin > 0: dark tiles with a Phong material
  zero    the ground with a zero colour channel and a negative ambient: the
          first dark pass turns -0 into +0, whatever the storing frame decided
          must reproduce the oracle's bits
  facet   one triangle in front of everything, across the whole view: a kept
          triangle is the surface of every tile at every frame size
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import rt_amd
from aov_ref import Cam, camera_dirs, oracle_aov
from conftest import bits_equal
from hard_frames import Frames
from test_gpu_tiny_light_classes import (BACKGROUND, BELOW, BESIDE, BESIDE_MOVED, BOX, HIDDEN, HIGH, LABELS, MORE, SIZES,
                                         classes, ctx, four_times, general, words)  # noqa: F401 (fixtures)
from test_gpu_tiny_scalar import GROUND, HEAD, WALL_X, WALL_Z, light, planes, poly, write

pytestmark = pytest.mark.gpu

W, H = 67, 33
F32 = np.float32
KIND_PLANE, KIND_TRI, KIND_SEARCH, KIND_MISS = 1, 2, 3, 4
NOOP, GATED = 1, 2


def ground(color, ambient, diffus, specular=None):
    out = ["Plane: ground", "        v_linear: 0.0 1.0 0.0", "        v_const:  45.0", "        color: %d %d %d" % color,
           "        ambient: %.3f" % ambient, "        diffus: %.3f" % diffus]
    return out + (["        specular: %.3f %.3f" % specular] if specular else [])


# x^2 + (y + 5)^2 + z^2 = 40^2: on the ground, tall enough for a whole tile at 67 x 33
BALL = ["Quad: ball", "        v_quad: 1.000000 1.000000 1.000000", "        v_linear: 0.000 10.000 0.000",
        "        v_const: -1575.000", "        color: 230 60 60", "        ambient: 0.2", "        diffus: 0.8"]
# one triangle across the whole view, 60 in front of the camera and square to it
FACET = poly(2, [(-34.3, 614.7, -27.6), (-149.7, -244.2, 545.9), (499.9, -244.2, -265.7)])
LOW = (160.0, -15.0, 0.0)  # beside the ball, below its top: a terminator on it
THREE = [(HIGH, 0.5), (BESIDE, 0.4), (BELOW, 0.6)]

# name: (lights, surfaces in file order, plain: every material without Phong, colours and ambient > 0)
SCENES = {
    "walls": (THREE, planes(GROUND, WALL_Z, WALL_X) + BOX, True),
    "sky": (THREE + MORE[:4], BOX, True),
    "ball": ([(HIGH, 0.5), (LOW, 0.4), (BELOW, 0.6)], planes(GROUND) + BALL + HIDDEN, True),
    "phong": (THREE, ground((60, 200, 90), 0.3, 0.6, (0.5, 6.0)) + BOX, False),
    "zero": (THREE, ground((0, 200, 90), -0.3, 0.7) + BOX, False),
    "facet": (THREE + [((175.0, 75.0, 150.0), 0.5)], planes(GROUND) + BOX + FACET, True),  # a light on either side
    "walls_light1_moved": ([THREE[0], (BESIDE_MOVED, 0.4), THREE[2]], planes(GROUND, WALL_Z, WALL_X) + BOX, True),
    "walls_ground_changed": (THREE, ground((0, 200, 90), -0.3, 0.7) + planes(GROUND, WALL_Z, WALL_X)[6:] + BOX, False),
}
CASES = ["walls", "sky", "ball", "phong", "zero", "facet"]


def text(name, only=None):
    """The scene's lines; only: that light alone (None: all, -1: none)."""
    ls, body, _ = SCENES[name]
    ls = ls if only is None else ([] if only < 0 else [ls[only]])
    return HEAD + sum((light(k, pos, intens) for k, (pos, intens) in enumerate(ls)), []) + body


def facts(c, w, h, stream=0):
    """The tile facts stored for `stream` (0: the synchronous renders'), as (tile rows, tile columns)."""
    L = rt_amd.lib()
    L.rt_debug_tiny_facts.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    L.rt_debug_tiny_facts.restype = ctypes.c_int
    ty, tx = (h + 7) // 8, (w + 7) // 8
    out = np.zeros(ty * tx, np.uint32)
    rc = L.rt_debug_tiny_facts(c._h, stream or None, out.ctypes.data, out.size)
    if rc != 0:
        raise rt_amd.RtError("rt_debug_tiny_facts", rc)
    return out.reshape(ty, tx)


def kind_of(fx):
    return fx & np.uint32(7)


def surf_of(fx):
    return (fx >> np.uint32(20)).astype(np.int64) - 1


def light_bits(fx, li):
    return (fx >> np.uint32(8 + 2 * li)) & np.uint32(3)


# ---- what the CPU says of the tiles
def tiles(a, w, h):
    """(h, w, ...) per pixel -> (tile rows, tile columns, 64, ...): each tile's
    lanes, a lane outside the frame on its clamped pixel as in the kernel."""
    ty, tx = (h + 7) // 8, (w + 7) // 8
    pad = [(0, ty * 8 - h), (0, tx * 8 - w)] + [(0, 0)] * (a.ndim - 2)
    p = np.pad(a, pad, mode="edge")
    p = p.reshape((ty, 8, tx, 8) + a.shape[2:])
    return np.moveaxis(p, 2, 1).reshape((ty, tx, 64) + a.shape[2:])


class Expect:
    """Per tile of the W x H frame, from the oracle alone: the one surface
    (-1: all lanes miss, -2: several), its kind, and per light the lanes'
    gate (1 every shaded lane faces it, -1 none does, 0 some or undecided)
    and whether the light changes any pixel of the tile."""

    def __init__(self, oracle, tmp_path, name):
        path = write(tmp_path, name, text(name))
        surf, cam, lig = oracle.dump(path, W, H)
        aov = oracle_aov(oracle, path, W, H)
        self.ids = aov["id"]
        ids = tiles(self.ids, W, H)
        self.shaded = (ids >= 0).any(axis=2)
        first = ids[:, :, 0]
        uniform = (ids == first[:, :, None]).all(axis=2)
        self.surf = np.where(uniform, first, -2)
        names = self.names(name)
        assert len(names) == surf.shape[0]
        plane_rank = {i: sum(n.startswith("Plane:") for n in names[:i]) for i, n in enumerate(names)
                      if n.startswith("Plane:")}
        self.kind = np.zeros(self.surf.shape, np.int64)
        self.slot = np.full(self.surf.shape, -1, np.int64)
        for (y, x), s in np.ndenumerate(self.surf):
            if s == -1:
                self.kind[y, x] = KIND_MISS
            elif s >= 0 and s in plane_rank:
                self.kind[y, x] = KIND_PLANE if plane_rank[s] < 2 else KIND_SEARCH
                self.slot[y, x] = plane_rank[s] if plane_rank[s] < 2 else -1
            elif s >= 0:
                self.kind[y, x] = KIND_TRI if names[s].startswith("Poly:") else KIND_SEARCH
        # the gate, dot(light - P, N) > 0 with P = O + t D, where it is decided by a margin
        O = cam[0:3].astype(F32)
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        D = camera_dirs(Cam.from_words(cam), xs.ravel(), ys.ravel()).reshape(H, W, 3)
        P = O + aov["t"][..., None] * D
        hit = tiles(aov["id"] >= 0, W, H)
        self.gate = []
        for li in range(lig.shape[0]):
            Lr = lig[li, 0:3].astype(F32) - P
            d = (Lr * aov["n"]).sum(axis=-1)
            margin = 1e-3 * np.sqrt((Lr * Lr).sum(axis=-1))
            pos, neg = tiles(d > margin, W, H), tiles(d < -margin, W, H)
            self.gate.append(np.where((pos | ~hit).all(axis=2), 1, np.where((neg | ~hit).all(axis=2), -1, 0)))
            self.gate[-1][~self.shaded] = 0
        ambient = oracle.render(write(tmp_path, name + "_ambient", text(name, -1)), W, H, 0)
        self.changes, self.changes_value = [], []
        for li in range(lig.shape[0]):
            alone = oracle.render(write(tmp_path, f"{name}_alone{li}", text(name, li)), W, H, 0)
            self.changes.append(tiles((alone.view(np.uint32) != ambient.view(np.uint32)).any(axis=-1), W, H))
            self.changes_value.append(tiles((alone != ambient).any(axis=-1), W, H))
        assert bits_equal(ambient[aov["id"] < 0], np.broadcast_to(BACKGROUND, ambient[aov["id"] < 0].shape))

    @staticmethod
    def names(name):
        """The surfaces' header lines in file order."""
        return [ln for ln in SCENES[name][1] if ln.startswith(("Plane:", "Poly:", "Quad:"))]

    def dark(self, li):
        """Tiles light li changes no pixel of although every lane faces it."""
        return (self.gate[li] == 1) & ~self.changes[li].any(axis=2)

    def lit(self, li):
        return (self.gate[li] == 1) & self.changes_value[li].all(axis=2)


@pytest.fixture(scope="module")
def expect(oracle, tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Expect(oracle, tmp_path_factory.mktemp("expect_" + name), name)
        return made[name]

    return get


def assert_states(expect):
    """Together the scenes show every state the facts tell apart (CPU only)."""
    wl, sk, bl, ph, ze, fa = (expect(n) for n in CASES)
    whole = np.zeros(wl.surf.shape, bool)
    whole[: H // 8, : W // 8] = True
    names = Expect.names("walls")
    for slot in (0, 1):
        assert ((wl.kind == KIND_PLANE) & (wl.slot == slot) & whole).any(), ("plane slot", slot)
    third = names.index("Plane: p2")
    assert ((wl.surf == third) & (wl.kind == KIND_SEARCH) & whole).any(), "a third plane"
    assert ((wl.kind == KIND_TRI) & whole).any(), "one triangle"
    # a tile on one face of the box, across its diagonal: two file indices, one colour
    ids = tiles(wl.ids, W, H)
    first = names.index("Poly: t0")  # the box: 12 triangles, two to a face
    face = [(first + 2 * k, first + 2 * k + 1) for k in range(6)]
    split = np.zeros(whole.shape, bool)
    for a, b in face:
        split |= ((ids == a) | (ids == b)).all(axis=2) & (ids == a).any(axis=2) & (ids == b).any(axis=2)
    assert (split & whole & (wl.surf == -2)).any(), "a face's diagonal"
    assert ((wl.surf == -2) & whole & ~split).any(), "a silhouette"
    assert ((sk.kind == KIND_MISS) & whole).any(), "a tile that misses"
    assert ((sk.surf == -2) & sk.shaded & ~(tiles(sk.ids, W, H) >= 0).all(axis=2) & whole).any(), "a silhouette on the sky"
    ball = Expect.names("ball").index("Quad: ball")
    assert ((bl.surf == ball) & (bl.kind == KIND_SEARCH) & whole).any(), "a quadric"
    assert (wl.gate[2] == -1)[wl.surf == 0].all() and (wl.surf == 0).any(), "below the ground: no lane of it gated"
    assert (wl.dark(0) | wl.dark(1)).any(), "a dark tile, no Phong"
    assert (ph.dark(0) | ph.dark(1)).any(), "a dark tile, Phong"
    # the light adds nothing there and still turns the ambient's -0 into +0
    assert any(((ze.gate[li] == 1) & ~ze.changes_value[li].any(axis=2) & ze.changes[li].all(axis=2)).any()
               for li in (0, 1)), "a dark tile, signed zero"
    assert wl.lit(0).any() and wl.lit(1).any(), "all gated and lit"
    assert ((bl.gate[1] == 0) & (bl.surf == ball)).any(), "a terminator across a tile"
    assert len(SCENES["sky"][0]) == 7
    assert (fa.kind == KIND_TRI).all() and (fa.surf == len(Expect.names("facet")) - 1).all(), \
        "one triangle on every tile (so on the one or two tiles of the small frames)"
    assert any((fa.gate[li] == 1).all() and fa.lit(li).all() for li in range(4)), "and a light that reaches all of it"


@pytest.fixture(scope="module")
def states(expect):
    """Asserted once, on the CPU, before any case touches the device."""
    assert_states(expect)
    return True


# ---- scenes and frame shapes
@pytest.mark.parametrize("wh", SIZES)
@pytest.mark.parametrize("name", CASES)
def test_scenes(ctx, general, oracle, states, tmp_path, name, wh):  # noqa: F811
    w, h = wh
    path = write(tmp_path, name, text(name))
    s = rt_amd.Scene(path, w, h, 0)
    four_times(ctx, general, s, s.frame, oracle.render(path, w, h, 0))


@pytest.mark.parametrize("name", ["walls", "zero"])
def test_row_slab_off_the_tile_grid(ctx, general, oracle, states, tmp_path, name):  # noqa: F811
    path = write(tmp_path, name, text(name))
    s = rt_amd.Scene(path, W, H, 0)
    full = oracle.render(path, W, H, 0)
    f = s.frame.copy()
    f.row_begin, f.row_end = 3, 20
    four_times(ctx, general, s, f, full[3:20])


@pytest.mark.parametrize("name", ["walls", "ball"])
def test_band_split_of_two(ctx, general, oracle, states, tmp_path, name):  # noqa: F811
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


# ---- the stored facts
def stored(c, s):
    """Upload, three frames; the words and facts after the second and the third."""
    c.upload(s)
    for rep in range(3):
        c.render_float(s.frame)
        assert c.stats().kernel == LABELS[rep]
        if rep == 0:
            with pytest.raises(rt_amd.RtError):  # a camera's first frame stores nothing
                facts(c, W, H)
        elif rep == 1:
            wd, fx = words(c, W, H), facts(c, W, H)
    assert np.array_equal(words(c, W, H), wd) and np.array_equal(facts(c, W, H), fx), "a reading frame writes nothing"
    return wd, fx


@pytest.mark.parametrize("name", CASES)
def test_stored_facts(ctx, oracle, expect, states, tmp_path, name):  # noqa: F811
    e = expect(name)
    s = rt_amd.Scene(write(tmp_path, name, text(name)), W, H, 0)
    wd, fx = stored(ctx, s)
    kind, surf = kind_of(fx), surf_of(fx)
    # the surface: every tile, a ragged one by its clamped lanes
    assert np.array_equal(kind == KIND_MISS, e.kind == KIND_MISS), (kind, e.kind)
    assert np.array_equal(np.where(e.surf >= 0, e.surf, -1), surf), (surf, e.surf)
    assert np.array_equal(kind, e.kind), (kind, e.kind)
    slot = (fx >> np.uint32(3)) & np.uint32(31)
    assert np.array_equal(slot[kind == KIND_PLANE], e.slot[kind == KIND_PLANE])
    assert (slot[kind == KIND_TRI] < 20).all() and (slot[(kind != KIND_PLANE) & (kind != KIND_TRI)] == 0).all()
    # the lights
    ls, _, plain = SCENES[name]
    for li in range(min(6, len(ls))):
        b = light_bits(fx, li)
        assert (b[~e.shaded] == 0).all(), "a tile that was not shaded has no facts"
        assert ((b & GATED) != 0)[e.gate[li] == 1].all(), (name, li, "all gated")
        assert ((b & GATED) == 0)[e.gate[li] == -1].all(), (name, li, "none gated")
        assert ((b & NOOP) != 0)[e.gate[li] == -1].all(), (name, li, "no lane gated: no-op")
        assert ((b & NOOP) == 0)[e.lit(li)].all(), (name, li, "lit: not a no-op")
        assert ((b & NOOP) == 0)[e.changes[li].any(axis=2) & (e.surf != -2) & (li == 0)].all()
        if plain:
            # dark by the word's class too, a material without Phong: add_light returns at once
            dark = e.dark(li) & (classes(wd, li) == 2)
            assert ((b & NOOP) != 0)[dark].all(), (name, li, "dark: no-op")
    assert (fx >> np.uint32(8 + 2 * min(6, len(ls))) & np.uint32((1 << (12 - 2 * min(6, len(ls)))) - 1) == 0).all(), \
        "no bits past the scene's lights, none for a seventh light"


# ---- staleness
def test_another_camera_in_between(oracle, states, tmp_path):
    path = write(tmp_path, "walls", text("walls"))
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
    seen, fxs = [], {}
    for k, cam in enumerate("aaaabbbbaaaa"):
        got = c.render_float(a if cam == "a" else b)
        seen.append(c.stats().kernel)
        assert bits_equal(got, want[cam]), (cam, seen)
        if k % 4 == 3:
            fxs[k] = facts(c, W, H)
    assert seen == LABELS * 3, seen
    assert np.array_equal(fxs[3], fxs[11]) and not np.array_equal(fxs[3], fxs[7])


def test_scene_uploaded_again_with_a_light_moved_and_a_material_changed(ctx, oracle, states, tmp_path):  # noqa: F811
    seen = []
    for name in ("walls", "walls_light1_moved", "walls_ground_changed", "walls"):
        path = write(tmp_path, name, text(name))
        s = rt_amd.Scene(path, W, H, 0)
        want = oracle.render(path, W, H, 0)
        ctx.upload(s)
        with pytest.raises(rt_amd.RtError):  # an upload drops the facts
            facts(ctx, W, H)
        for rep in range(4):
            assert bits_equal(ctx.render_float(s.frame), want), (name, rep)
            assert ctx.stats().kernel == LABELS[rep]
        seen.append(facts(ctx, W, H))
    base, moved, changed, again = seen
    assert np.array_equal(base, again)
    assert not np.array_equal(light_bits(base, 1), light_bits(moved, 1)), "light 1's facts follow the light"
    assert np.array_equal(kind_of(base), kind_of(moved)) and np.array_equal(surf_of(base), surf_of(moved))
    assert not np.array_equal(base >> np.uint32(8) & np.uint32(0xFFF), changed >> np.uint32(8) & np.uint32(0xFFF)), \
        "the no-op bits follow the material"


def test_two_streams_one_camera(oracle, states, tmp_path):
    torch = pytest.importorskip("torch")
    path = write(tmp_path, "walls", text("walls"))
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
    assert np.array_equal(facts(c, W, H, streams[0].cuda_stream), facts(c, W, H, streams[1].cuda_stream))
    assert facts(c, W, H, streams[0].cuda_stream).any()
