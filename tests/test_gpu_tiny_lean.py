"""The lean tile records (rt_tile.h LeanRec): beside each tile's word and facts
a camera's second frame on a stream stores one 64-byte record that repeats
both and, on a LEAN tile — one known plane or kept triangle, a class for every
light once a no-op pass counts as class 3, no translucent surface, at most six
lights — carries the plane slot's values, the hit normal and the material.  The
camera's later frames (rt_trace_tiny<0,1,37>, not the counted one) read that
record alone and shade a lean tile from it and the launch record
(shade_lean_tiny), without a scene pointer.

Every case is test_gpu_tiny_light_classes.four_times (labels 101, 229, 37, 37,
float RGB and RGBA8 bit for bit the oracle's and the general kernels', the
counted render's counts the general kernels', one more reading frame) at the
four frame sizes, on the scenes of the two tiny-kernel test files and on:
  six      six lights, the ground and the box: every light has a class
  seven    the same with a seventh light: no tile is lean
  sky      the box alone, three lights: lean triangle tiles beside tiles that miss
  slot1    two opaque planes, the nearer one listed second: plane slot 1
  phong    a ground with ks and shin (add_light's Phong term on lean tiles)
  zeros    a ground with a zero colour channel, a wall with kd = 0
           (add_light's exact-zero shortcuts)
  inplane  a light exactly in the ground plane (the gate's dot product at 0)
  dark     nothing but a ground with a zero colour channel and a negative
           ambient under an opaque roof, the first light above the roof: on
           every tile of every frame size that pass is dark (class 2) and no
           no-op (it turns the ambient's -0 into +0), so class 2 is read
  bare1    slot1 without the box: plane slot 1 on every tile of every size
  (translucent, never lean: scene d of the classes test)
The stored records are read back at 67 x 33 (rt_debug_tiny_lean): the flag
against the rule recomputed from the words, the facts and the scene's counts,
the contents against the scene's arrays; that the frames hold a lean plane
tile, a lean triangle tile, a lean ragged tile, a tile with a mixed light and
a background tile is asserted on the CPU first.  Staleness as in the two files.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import rt_amd
import test_gpu_tiny_light_classes as tlc
import test_gpu_tiny_tile_facts as ttf
from conftest import bits_equal
from hard_frames import Frames
from test_gpu_tiny_light_classes import (BELOW, BESIDE, BESIDE_MOVED, BOX, HIGH, LABELS, MORE, SIZES, ctx, four_times,  # noqa: F401
                                         general, words)
from test_gpu_tiny_light_classes import test_sequence_stores_and_reads_on_its_internal_streams  # noqa: F401 (run here too)
from test_gpu_tiny_scalar import GROUND, WALL_Z, plane, planes, poly, write
from test_gpu_tiny_tile_facts import Expect, facts, ground, kind_of, surf_of, tiles

pytestmark = pytest.mark.gpu

W, H = 67, 33
F32 = np.float32
KIND_PLANE, KIND_TRI = 1, 2
LEAN_PLANE, LEAN_TRI = 5, 6
MAX_LIGHTS = 6

THREE = [(HIGH, 0.5), (BESIDE, 0.4), (BELOW, 0.6)]
LOWER = ("0.0 1.0 0.0", "145.0")  # a second ground 100 below the first: never seen, listed first
WALL_KD0 = plane(1, WALL_Z)[:-1] + ["        diffus: 0.0"]
IN_PLANE = (100.0, -45.0, 50.0)  # on y = -45, the ground
ABOVE = (130.0, 200.0, -75.0)    # above the roof: reaches nothing below it
# an opaque roof far wider than the view, above the camera (y = 60) and every other light
ROOF = poly(2, [(-900, 120, -900), (900, 120, -900), (0, 120, 1200)])
# the launch-camera kernels want a triangle: one between the two grounds, seen by no camera ray
BURIED = poly(1, [(-5, -70, -5), (5, -70, -5), (0, -70, 5)])

# name: (lights, surfaces in file order, plain) as test_gpu_tiny_tile_facts.SCENES, which takes them in
LEAN_SCENES = {
    "lean_six": (THREE + MORE[:3], planes(GROUND) + BOX, True),
    "lean_seven": (THREE + MORE[:4], planes(GROUND) + BOX, True),
    "lean_sky": (THREE, BOX, True),
    "lean_slot1": (THREE, planes(LOWER, GROUND) + BOX, True),
    "lean_phong": (THREE[:2], ground((200, 120, 40), 0.25, 0.6, (0.4, 9.0)) + BOX, False),
    "lean_zeros": (THREE, ground((0, 200, 90), 0.3, 0.7) + WALL_KD0 + BOX, False),
    "lean_inplane": ([(HIGH, 0.5), (IN_PLANE, 0.6)], planes(GROUND) + BOX, True),
    "lean_dark": ([(ABOVE, 0.5), (BESIDE, 0.4)], ground((0, 200, 90), -0.3, 0.7) + ROOF, False),
    "lean_bare1": (THREE, planes(LOWER, GROUND) + BURIED, True),
    "lean_six_light1_moved": ([THREE[0], (BESIDE_MOVED, 0.4)] + THREE[2:] + MORE[:3], planes(GROUND) + BOX, True),
    "lean_six_ground_changed": (THREE + MORE[:3], ground((90, 30, 200), 0.1, 0.9) + BOX, True),
}
ttf.SCENES.update(LEAN_SCENES)
N_TRANSLUCENT = {"d_glass": 1}

# (module whose text() writes it, name)
FACT_CASES = [(ttf, n) for n in ttf.CASES]
CLASS_CASES = [(tlc, n) for n in tlc.CASES]
NEW_CASES = [(ttf, n) for n in ("lean_six", "lean_seven", "lean_sky", "lean_slot1", "lean_phong", "lean_zeros", "lean_inplane",
                                 "lean_dark", "lean_bare1")]
ALL_CASES = FACT_CASES + CLASS_CASES + NEW_CASES


def case_id(c):
    return c[1]


def lean_records(c, w, h, stream=0):
    """The lean records stored for `stream` (0: the synchronous renders'), as (tile rows, tile columns, 16) dwords."""
    L = rt_amd.lib()
    L.rt_debug_tiny_lean.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    L.rt_debug_tiny_lean.restype = ctypes.c_int
    ty, tx = (h + 7) // 8, (w + 7) // 8
    out = np.zeros(ty * tx * 16, np.uint32)
    rc = L.rt_debug_tiny_lean(c._h, stream or None, out.ctypes.data, ty * tx)
    if rc != 0:
        raise rt_amd.RtError("rt_debug_tiny_lean", rc)
    return out.reshape(ty, tx, 16)


def unpack(rec):
    """rt_tile.h lean_unpack: (word, the TileRec's facts, lean flag, the 14 floats)."""
    word, fx = rec[..., 0], rec[..., 1].copy()
    k = fx & np.uint32(7)
    lean = (k == LEAN_PLANE) | (k == LEAN_TRI)
    fx[k == LEAN_PLANE] = (fx[k == LEAN_PLANE] & ~np.uint32(7)) | np.uint32(KIND_PLANE)
    fx[k == LEAN_TRI] = (fx[k == LEAN_TRI] & ~np.uint32(7)) | np.uint32(KIND_TRI)
    return word, fx, lean, rec[..., 2:].view(F32)


def rule(wd, fx, n_lights, n_translucent):
    """A tile is lean exactly when (rt_tile.h lean_tile) — from the TileRec's two words."""
    kind = kind_of(fx)
    ok = ((kind == KIND_PLANE) | (kind == KIND_TRI)) & (surf_of(fx) >= 0)
    if n_translucent != 0 or n_lights > MAX_LIGHTS:
        return np.zeros(wd.shape, bool)
    for li in range(n_lights):
        cls = (wd >> np.uint32(20 + 2 * li)) & np.uint32(3)
        noop = (fx >> np.uint32(8 + 2 * li)) & np.uint32(1)
        ok &= (cls != 0) | (noop != 0)
    return ok


# ---- every frame four times
@pytest.mark.parametrize("wh", SIZES)
@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_scenes(ctx, general, oracle, tmp_path, case, wh):  # noqa: F811
    mod, name = case
    w, h = wh
    path = write(tmp_path, name, mod.text(name))
    s = rt_amd.Scene(path, w, h, 0)
    four_times(ctx, general, s, s.frame, oracle.render(path, w, h, 0))


# ---- what the frames hold, from the oracle and the CPU id plane alone
@pytest.fixture(scope="module")
def expect(oracle, tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Expect(oracle, tmp_path_factory.mktemp("lean_expect_" + name), name)
        return made[name]

    return get


def decided(e, n_lights):
    """Per tile: every light's pass has one outcome for the tile on the oracle
    (no lane faces it, it reaches every lane, it changes no lane): such a
    plane or triangle tile must be lean."""
    ok = np.ones(e.surf.shape, bool)
    for li in range(n_lights):
        ok &= (e.gate[li] == -1) | e.lit(li) | e.dark(li)
    return ok


def mixed(e, n_lights):
    """Per tile: some light faces every lane and reaches some lanes, not all: class 0, not a no-op."""
    out = np.zeros(e.surf.shape, bool)
    for li in range(n_lights):
        ch = e.changes_value[li]
        out |= (e.gate[li] == 1) & ch.any(axis=2) & ~ch.all(axis=2)
    return out


@pytest.fixture(scope="module")
def content(expect):
    """Asserted once, on the CPU, before any case touches the device."""
    wl, sx, sk = expect("walls"), expect("lean_six"), expect("lean_sky")
    ragged = np.ones(wl.surf.shape, bool)
    ragged[: H // 8, : W // 8] = False
    sure_w, sure_s = decided(wl, 3), decided(sx, 6)
    assert ((wl.kind == KIND_PLANE) & sure_w).any() or ((sx.kind == KIND_PLANE) & sure_s).any(), "a lean plane tile"
    assert ((wl.kind == KIND_TRI) & sure_w).any(), "a lean triangle tile"
    assert (((wl.kind == KIND_PLANE) | (wl.kind == KIND_TRI)) & sure_w & ragged).any(), "a lean ragged-edge tile"
    assert ((wl.kind == KIND_PLANE) & mixed(wl, 3)).any(), "a tile with a mixed light"
    assert (sk.kind == ttf.KIND_MISS).any() and ((sk.kind == KIND_TRI) & decided(sk, 3)).any(), \
        "a background-only tile, beside lean ones"
    return True


# ---- the stored records
def stored(c, s):
    """Upload, three frames; words, facts and lean records after the second, unchanged by the third."""
    c.upload(s)
    for rep in range(3):
        c.render_float(s.frame)
        assert c.stats().kernel == LABELS[rep]
        if rep == 0:
            with pytest.raises(rt_amd.RtError):  # a camera's first frame stores nothing
                lean_records(c, W, H)
        elif rep == 1:
            wd, fx, rec = words(c, W, H), facts(c, W, H), lean_records(c, W, H)
    assert np.array_equal(lean_records(c, W, H), rec), "a reading frame writes nothing"
    return wd, fx, rec


RECORD_CASES = [(ttf, "walls"), (ttf, "sky"), (ttf, "facet"), (ttf, "phong"), (tlc, "d_glass"), (ttf, "lean_six"),
                (ttf, "lean_seven"), (ttf, "lean_sky"), (ttf, "lean_slot1"), (ttf, "lean_zeros"), (ttf, "lean_inplane"),
                (ttf, "lean_dark"), (ttf, "lean_bare1")]


@pytest.mark.parametrize("case", RECORD_CASES, ids=case_id)
def test_stored_records(ctx, oracle, expect, content, tmp_path, case):  # noqa: F811
    mod, name = case
    path = write(tmp_path, name, mod.text(name))
    s = rt_amd.Scene(path, W, H, 0)
    typ, geom, mat, lights = s.arrays()
    wd, fx, rec = stored(ctx, s)
    word, rfx, lean, val = unpack(rec)
    assert np.array_equal(word, wd) and np.array_equal(rfx, fx), "the record repeats the TileRec"
    want = rule(wd, fx, lights.shape[0], N_TRANSLUCENT.get(name, 0))
    assert np.array_equal(lean, want), (name, lean, want)
    assert not val[~lean].any(), "a tile that is not lean stores zeros"
    if name in ("sky", "lean_seven", "d_glass"):
        assert not lean.any()
    if name in ("walls", "lean_six", "lean_sky"):
        e = expect(name)
        n = lights.shape[0]
        flat = (e.kind == KIND_PLANE) | (e.kind == KIND_TRI)
        assert lean[flat & decided(e, n)].all(), "decided on the oracle: lean"
        assert not lean[mixed(e, n)].any() and not lean[e.kind == ttf.KIND_MISS].any()
    if name == "lean_dark":  # every tile: lean, light 0 of class 2 and no no-op
        assert lean.all() and ((wd >> np.uint32(20) & np.uint32(3)) == 2).all() and (fx >> np.uint32(8) & np.uint32(1) == 0).all()
    if name == "lean_bare1":
        assert lean.all() and ((fx >> np.uint32(3) & np.uint32(31)) == 1).all()
    if name == "lean_slot1":
        slot = (fx >> np.uint32(3)) & np.uint32(31)
        assert (lean & (kind_of(fx) == KIND_PLANE) & (slot == 1)).any() and not (lean & (slot == 0)).any()
    # contents: the scene's arrays for the facts' surface, bit for bit
    O = np.array(list(s.frame.cam_pos), F32)
    for (y, x), on in np.ndenumerate(lean):
        if not on:
            continue
        sf = int(surf_of(fx)[y, x])
        v = val[y, x]
        if kind_of(fx)[y, x] == KIND_PLANE:
            assert typ[sf] == 1
            nrm = geom[sf, 0:3]
            num = F32(F32(F32(nrm[0] * O[0]) + F32(nrm[1] * O[1])) + F32(nrm[2] * O[2])) + geom[sf, 3]
            assert bits_equal(v[0:3], nrm) and bits_equal(v[3:4], np.array([num], F32)), (name, y, x)
        else:
            assert typ[sf] == 0
            nrm = geom[sf, 9:12]
            assert not v[0:4].any()
        assert bits_equal(v[4:7], nrm), (name, y, x, "normal")
        assert bits_equal(v[7:14], mat[sf, 0:7]), (name, y, x, "material")


# ---- staleness and shapes
def test_another_camera_in_between(oracle, content, tmp_path):
    path = write(tmp_path, "lean_six", ttf.text("lean_six"))
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
    seen, recs = [], {}
    for k, cam in enumerate("aaaabbbbaaaa"):
        got = c.render_float(a if cam == "a" else b)
        seen.append(c.stats().kernel)
        assert bits_equal(got, want[cam]), (cam, seen)
        if k % 4 == 3:
            recs[k] = lean_records(c, W, H)
    assert seen == LABELS * 3, seen
    assert np.array_equal(recs[3], recs[11]) and not np.array_equal(recs[3], recs[7])
    assert unpack(recs[7])[2].any()


def test_scene_uploaded_again_with_a_light_moved_and_the_ground_changed(ctx, oracle, content, tmp_path):  # noqa: F811
    seen = []
    for name in ("lean_six", "lean_six_light1_moved", "lean_six_ground_changed", "lean_six"):
        path = write(tmp_path, name, ttf.text(name))
        s = rt_amd.Scene(path, W, H, 0)
        want = oracle.render(path, W, H, 0)
        ctx.upload(s)
        with pytest.raises(rt_amd.RtError):  # an upload drops the records
            lean_records(ctx, W, H)
        for rep in range(4):
            assert bits_equal(ctx.render_float(s.frame), want), (name, rep)
            assert ctx.stats().kernel == LABELS[rep]
        seen.append((lean_records(ctx, W, H), s.arrays()[2]))
    (base, _), (moved, _), (changed, cmat), (again, _) = seen
    assert np.array_equal(base, again)
    assert not np.array_equal(unpack(base)[1], unpack(moved)[1]), "the records follow the light"
    # the record must not outlive the material: every lean ground tile carries the new one
    _, fx, lean, val = unpack(changed)
    on_ground = lean & (surf_of(fx) == 0)
    assert on_ground.any() and bits_equal(val[on_ground][:, 7:14], np.broadcast_to(cmat[0, 0:7], val[on_ground][:, 7:14].shape))
    assert not bits_equal(unpack(base)[3][on_ground][:, 7:14], val[on_ground][:, 7:14])


def test_two_streams_one_camera(oracle, content, tmp_path):
    torch = pytest.importorskip("torch")
    path = write(tmp_path, "lean_six", ttf.text("lean_six"))
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
    r0, r1 = (lean_records(c, W, H, st.cuda_stream) for st in streams)
    assert np.array_equal(r0, r1) and unpack(r0)[2].any()


@pytest.mark.parametrize("name", ["lean_six", "lean_slot1"])
def test_row_slab_off_the_tile_grid(ctx, general, oracle, tmp_path, name):  # noqa: F811
    """No wave's rows are a tile row of the full frame: no record stored or read."""
    path = write(tmp_path, name, ttf.text(name))
    s = rt_amd.Scene(path, W, H, 0)
    full = oracle.render(path, W, H, 0)
    f = s.frame.copy()
    f.row_begin, f.row_end = 3, 20
    four_times(ctx, general, s, f, full[3:20])


@pytest.mark.parametrize("name", ["lean_six", "lean_zeros"])
def test_band_split_of_two(ctx, general, oracle, tmp_path, name):  # noqa: F811
    w, h, count = 67, 50, 2
    path = write(tmp_path, name, ttf.text(name))
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
