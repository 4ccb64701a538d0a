"""The wavefront bounce levels (rt_wavefront.h, wf_layout / wf_ensure / the
level loop of rt_kernels.hip) on small frames: every case asserts

* the kernel label (rt_stats.kernel starts with "wavefront", or — the
  fallbacks — does not),
* the WHOLE frame, bit for bit in float32, against the oracle (or against a
  frame the reference's own code rendered, tests/golden/wf_small.npz), and
* the queues' per-level counts (rt_debug_wf_counts: rays, parents) against the
  oracle's bounce tree by depth (oracle_level_counts) — a ray dropped or
  duplicated anywhere in the frame changes a count or a pixel.

Scenes: tests/wf_scenes.py (no `specular:`, so no powf allowance).  The frame
shapes are the segmented queues' edge cases (kWfSeg = 16 segments picked by
chunk % 16: 1, 15, 16 and 17 tiles, ragged tiles), the depths reach the level
limit (kWfMaxLevels = 8) and one past it, the meshes sit on both sides of the
BVH's minimum (64 triangles) and of the cluster threshold (1,024).

The reference harness has no setter for the energy floor: the min_energy
cases are checked against the oracle's restatement only."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

import rt_amd
import wf_scenes
from conftest import GOLDEN, bits_equal, rgba8

pytestmark = pytest.mark.gpu

W, H = 96, 64
LEVELS = 9  # rt_debug_wf_counts: levels 0 .. kWfMaxLevels


# ---- the checkers
def wf_counts(ctx):
    L = rt_amd.lib()
    L.rt_debug_wf_counts.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    out = np.zeros(3 * LEVELS, np.uint32)
    assert L.rt_debug_wf_counts(ctx._h, out.ctypes.data, out.size) == 0, ctx._err()
    return out.reshape(LEVELS, 3).astype(np.int64)  # [level] = rays, parents, stragglers


class Want:
    """The oracle's frame and its bounce tree by depth."""

    def __init__(self, img, rays, parents):
        self.img, self.rays, self.parents = img, rays, parents


class Oracle:
    """Scene files and oracle frames, each made once for the module."""

    def __init__(self, oracle, folder):
        self.o, self.dir, self.files, self.frames = oracle, folder, {}, {}
        L = oracle.L
        L.oracle_level_counts.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        L.oracle_set_camera.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_float] * 4 + \
                                       [ctypes.c_int, ctypes.c_int]

    def path(self, family, ntri, lights=2, spread=1.0):
        k = (family, ntri, lights, spread)
        if k not in self.files:
            self.files[k] = str(self.dir / f"{family}_{ntri}_{lights}_{spread}.dat")
            with open(self.files[k], "w") as f:
                f.write(wf_scenes.wf_dat(family, ntri, lights, spread=spread))
        return self.files[k]

    def want(self, path, w, h, depth, min_energy=0.01, frame=None, rows=None) -> Want:
        """frame: an rt_frame whose camera replaces the file's; rows: a slab."""
        cam = None if frame is None else (tuple(frame.cam_pos), tuple(frame.orient))
        k = (path, w, h, depth, min_energy, cam, rows)
        if k not in self.frames:
            L = self.o.L
            rc, p = self.o.load(path, w, h, depth)
            assert rc == 0
            L.oracle_set_params(p, depth, min_energy, 1.0)
            if frame is not None:
                pos, orient = np.array(frame.cam_pos[:], np.float32), np.array(frame.orient[:], np.float32)
                assert L.oracle_set_camera(p, pos.ctypes.data, orient.ctypes.data, frame.half_w, frame.half_h,
                                           frame.inv_w, frame.inv_h, w, h) == 0
            r0, r1 = rows or (0, h)
            img = np.zeros((r1 - r0, w, 3), np.float32)
            L.oracle_render_window(p, r0, r1, 0, w, img.ctypes.data, 8)
            rays, parents = np.zeros(LEVELS, np.uint64), np.zeros(LEVELS, np.uint64)
            assert L.oracle_level_counts(p, rays.ctypes.data, parents.ctypes.data, LEVELS) == 0
            L.oracle_free(p)
            self.frames[k] = Want(img, rays.astype(np.int64), parents.astype(np.int64))
        return self.frames[k]


@pytest.fixture(scope="module")
def orc(oracle, tmp_path_factory):
    return Oracle(oracle, tmp_path_factory.mktemp("wf"))


def check_counts(ctx, want: Want, what=""):
    """Levels 1 .. 8's rays and levels 0 .. 8's parents (a level the frame does
    not run reads 0, and the oracle traces nothing there)."""
    got = wf_counts(ctx)
    print(what, "rays", got[:, 0].tolist(), "parents", got[:, 1].tolist(), "stragglers", got[:, 2].tolist())
    assert got[1:, 0].tolist() == want.rays[1:].tolist(), (what, "rays per level")
    assert got[:, 1].tolist() == want.parents.tolist(), (what, "parents per level")
    return got


def check_frame(ctx, frame, want: Want, wavefront=True, what=""):
    got = ctx.render_float(frame)
    kernel = ctx.stats().kernel
    assert kernel.startswith("wavefront") == wavefront, (what, kernel)
    bad = (got.view(np.uint32) != want.img.view(np.uint32)).any(-1)
    assert got.shape == want.img.shape and not bad.any(), \
        (what, kernel, f"{int(bad.sum())} pixels differ, first (row, col) {np.argwhere(bad)[:4].tolist()}")
    if wavefront:
        return check_counts(ctx, want, what)
    return None


def render_case(orc, family, ntri, w, h, depth, lights=2, min_energy=0.01, wavefront=True, spread=1.0, **options):
    path = orc.path(family, ntri, lights, spread)
    s = rt_amd.Scene(path, w, h, depth, min_energy=min_energy)
    ctx = rt_amd.Context(0, **options)
    try:
        ctx.upload(s)
        counts = check_frame(ctx, s.frame, orc.want(path, w, h, depth, min_energy), wavefront,
                             (family, ntri, w, h, depth, options))
        return ctx.stats().kernel, counts
    finally:
        ctx.close()


# ---- frame shapes: 1, 15, 16 and 17 tiles, ragged tiles, several tile rows
SHAPES = [(1, 1), (8, 8), (13, 7), (120, 8), (128, 8), (136, 8), (67, 33), (W, H)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("family,ntri", [("split", 1600), ("chain", 96), ("mixed", 1600)])
def test_frame_shapes(orc, family, ntri, shape):
    render_case(orc, family, ntri, shape[0], shape[1], 3)


# ---- depths
@pytest.mark.parametrize("depth", [1, 2, 7, 8])
def test_chain_depths_up_to_the_level_limit(orc, depth):
    """0.7^8 > 0.01: all eight levels are reachable, and between the mesh and
    the mirror below it hundreds of rays do reach the eighth."""
    kernel, counts = render_case(orc, "chain", 1600, W, H, depth)
    assert kernel.endswith(f"+ {depth} levels"), kernel
    assert counts[depth, 0] > 100


def test_chain_depth_9_takes_the_megakernel(orc):
    """One level more than kWfMaxLevels: the BVH megakernel, the same image."""
    render_case(orc, "chain", 1600, W, H, 9, wavefront=False)
    render_case(orc, "chain", 96, W, H, 9, wavefront=False)


@pytest.mark.parametrize("depth", [1, 5])
def test_split_depths(orc, depth):
    """0.4^5 = 0.01024 > 0.01: level 5 is reachable and runs (the open mesh
    sends few rays that deep: see test_mixed_depth_6 for full deep levels)."""
    for ntri in (96, 1600):
        kernel, counts = render_case(orc, "split", ntri, W, H, depth)
        assert kernel.endswith(f"+ {depth} levels"), kernel
        assert counts[1, 0] > 0


def test_split_depth_6_has_an_empty_last_level(orc):
    """0.4^6 < 0.01: no ray of level 6 exists, whether the level is dropped
    (reachable_depth) or run over an empty queue; its counts read 0."""
    kernel, counts = render_case(orc, "split", 96, W, H, 6)
    assert kernel.endswith("+ 5 levels") or kernel.endswith("+ 6 levels"), kernel
    assert counts[1, 0] > 0 and counts[6, 0] == 0 and counts[5, 1] == 0


def test_mixed_depth_6(orc):
    """Two children per node six levels deep (k_max = 0.5, 0.5^6 > 0.01), on
    the 96-triangle mesh: rays alive at every level."""
    kernel, counts = render_case(orc, "mixed", 96, W, H, 6)
    assert kernel.endswith("+ 6 levels"), kernel
    assert (counts[1:7, 0] > 0).all()


# ---- thresholds
@pytest.mark.parametrize("ntri,wavefront", [(63, False), (64, True), (65, True)])
def test_bvh_minimum_triangles(orc, ntri, wavefront):
    """RT_BVH_MIN_TRIANGLES = 64: below it there is no BVH and no wavefront."""
    render_case(orc, "split", ntri, W, H, 3, wavefront=wavefront)


def test_cluster_threshold_picks_another_level_0_kernel(orc):
    """1,024 triangles: the small-list level-0 kernel emits the children;
    1,026: the big-list one."""
    k1024, _ = render_case(orc, "split", 1024, W, H, 3)
    k1026, _ = render_case(orc, "split", 1026, W, H, 3)
    print("level-0 kernels:", k1024, "|", k1026)
    assert k1024.split(" + ")[0] != k1026.split(" + ")[0], (k1024, k1026)
    assert k1024.split(" + ")[1] == k1026.split(" + ")[1] == "3 levels"


# ---- min_energy (against the oracle's restatement: see the module docstring)
@pytest.mark.parametrize("w,h,depth", [(W, H, 3), (32, 24, 6)])
def test_negative_min_energy_spawns_both_children(orc, w, h, depth):
    """K * energy > -1 holds for Kt = 0 too: every hit above the last level
    is a parent of two rays."""
    kernel, counts = render_case(orc, "chain", 96, w, h, depth, min_energy=-1.0)
    for L in range(depth):
        assert counts[L + 1, 0] == 2 * counts[L, 1] > 0, L


def test_min_energy_cuts_level_2(orc):
    """0.7 > 0.5 >= 0.7^2: one level, whatever the depth asked for."""
    kernel, counts = render_case(orc, "chain", 96, W, H, 3, min_energy=0.5)
    assert kernel.endswith("+ 1 levels"), kernel
    assert counts[1, 0] > 0 and counts[2, 0] == 0


# ---- materials, lights
@pytest.mark.parametrize("lights", [1, 3])
@pytest.mark.parametrize("family", ["refract_only", "mixed"])
def test_materials_and_lights(orc, family, lights):
    kernel, counts = render_case(orc, family, 1600, W, H, 4, lights=lights)
    assert counts[2 if family == "refract_only" else 4, 0] > 0


def test_scene_without_lights_is_no_wavefront(orc):
    """No light, no light buffer, no BVH kernels: the image is still right."""
    render_case(orc, "split", 1600, W, H, 3, lights=0, wavefront=False)


# ---- options: none changes a bit, or a count
OPTIONS = [{"wf_sort": v} for v in range(8)] + [{"wf_overlap": v} for v in (0, 1)] + \
          [{"camera_buffer": v} for v in (0, 1)] + [{"xcd_deal": v} for v in (0, 2, 3)]


@pytest.mark.parametrize("options", OPTIONS, ids=lambda o: "%s=%d" % next(iter(o.items())))
def test_options_change_nothing(orc, options):
    """The sorts (bits 1 and 2: the hit sorts, whose key two kernels compute
    apart — a hole or a duplicate in the sorted order changes the next level's
    count or the image), the stragglers' second stream, the camera buffer,
    the tile deal."""
    render_case(orc, "mixed", 1600, W, H, 3, **options)


# ---- entry points
@pytest.fixture(scope="module")
def split(orc):
    path = orc.path("split", 1600)
    s = rt_amd.Scene(path, W, H, 3)
    ctx = rt_amd.Context(0)
    ctx.upload(s)
    yield ctx, s, path
    ctx.close()


def _moved(frame, k):
    g = frame.copy()
    g.cam_pos[0] += 20.0 * k
    g.cam_pos[2] -= 15.0 * k
    return g


def test_rgba8(orc, split):
    ctx, s, path = split
    want = orc.want(path, W, H, 3)
    got = ctx.render(s.frame)
    assert ctx.stats().kernel.startswith("wavefront")
    assert np.array_equal(got, rgba8(want.img))
    check_counts(ctx, want)


def test_async_frames_on_two_streams(orc, split):
    """Two cameras alternating between two streams (the queues are shared:
    each frame waits for the other stream's last one), four frames."""
    import torch

    ctx, s, path = split
    cams = [s.frame, _moved(s.frame, 1)]
    wants = [orc.want(path, W, H, 3), orc.want(path, W, H, 3, frame=cams[1])]
    assert not bits_equal(wants[0].img, wants[1].img)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = [torch.empty((H, W, 4), dtype=torch.uint8, device="cuda") for _ in range(4)]
    for k in range(4):
        ctx.render_async(cams[k % 2], outs[k].data_ptr(), 0, (s1 if k % 2 == 0 else s2).cuda_stream)
        assert ctx.stats().kernel.startswith("wavefront"), (k, ctx.stats().kernel)  # (the frame's plan)
    torch.cuda.synchronize()
    for k in range(4):
        assert np.array_equal(outs[k].cpu().numpy(), rgba8(wants[k % 2].img)), k
    check_counts(ctx, wants[1])  # the last frame's


def test_sequence_async(orc, split):
    """A sequence's frames run on internal streams with per-slot camera state
    and no shared queues: the BVH megakernel, not a wavefront (so there are no
    counts to read), between wavefront frames of the same context."""
    import torch

    ctx, s, path = split
    cams = [_moved(s.frame, 1), s.frame]
    wants = [orc.want(path, W, H, 3, frame=cams[0]), orc.want(path, W, H, 3)]
    check_frame(ctx, cams[0], wants[0], what="before")
    ring = torch.empty((2, H, W, 3), dtype=torch.float32, device="cuda")
    ctx.render_sequence_async(cams, 0, 0, ring.data_ptr(), H * W * 12, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for k in range(2):
        assert bits_equal(ring[k].cpu().numpy(), wants[k].img), k
    check_frame(ctx, cams[1], wants[1], what="after")


def test_slabs_and_bands(orc, split):
    """Row slabs off the tile grid and cyclic band sets (packed rows: a queue
    layout of their own), each a wavefront frame with its own counts,
    reassembled."""
    ctx, s, path = split
    want = orc.want(path, W, H, 3)
    parts = []
    for r0, r1 in ((0, 21), (21, 45), (45, 64)):
        f = s.frame.copy()
        f.row_begin, f.row_end = r0, r1
        parts.append(ctx.render_float(f))
        assert ctx.stats().kernel.startswith("wavefront")
        check_counts(ctx, orc.want(path, W, H, 3, rows=(r0, r1)), (r0, r1))
    assert bits_equal(np.concatenate(parts, 0), want.img)
    full = np.full((H, W, 3), np.nan, np.float32)
    for r in range(3):
        f = s.frame.copy()
        f.band_rows, f.band_count, f.band_index = 16, 3, r
        part = ctx.render_float(f)
        assert ctx.stats().kernel.startswith("wavefront")
        # the band set's counts: its bands' windows added up (windows add up:
        # tests/test_wf_oracle.py)
        rays, parents = np.zeros(LEVELS, np.int64), np.zeros(LEVELS, np.int64)
        for q in range(part.shape[0] // 16):
            a = (q * 3 + r) * 16
            if a < H:
                full[a:a + 16] = part[16 * q:16 * q + 16]
                band = orc.want(path, W, H, 3, rows=(a, min(a + 16, H)))
                rays += band.rays
                parents += band.parents
        check_counts(ctx, Want(None, rays, parents), ("band set", r))
    assert bits_equal(full, want.img)


def test_smaller_frame_after_a_larger_one(orc):
    """The queues are grown, never shrunk: a small frame laid out in the big
    frame's allocation, then the big one again."""
    path = orc.path("split", 1600)
    big, small = rt_amd.Scene(path, W, H, 3), rt_amd.Scene(path, 40, 24, 3)
    ctx = rt_amd.Context(0)
    ctx.upload(big)
    try:
        check_frame(ctx, big.frame, orc.want(path, W, H, 3), what="big")
        check_frame(ctx, small.frame, orc.want(path, 40, 24, 3), what="small")
        check_frame(ctx, big.frame, orc.want(path, W, H, 3), what="big again")
    finally:
        ctx.close()


def test_aov_and_depth_0_frames_between_wavefront_frames(orc, split):
    """The camera state is shared: an AOV render and a depth-0 colour frame of
    the file's camera between two wavefront frames of another."""
    ctx, s, path = split
    moved = _moved(s.frame, 2)
    want = orc.want(path, W, H, 3, frame=moved)
    check_frame(ctx, moved, want, what="before")
    aov = ctx.render_aov(s.frame)
    assert (aov["id"] >= 0).any()
    flat = s.frame.copy()
    flat.max_bounces = 0
    got0 = ctx.render_float(flat)
    assert not ctx.stats().kernel.startswith("wavefront")
    assert bits_equal(got0, orc.want(path, W, H, 0).img)
    check_frame(ctx, moved, want, what="after")


# ---- the stragglers (kWfPending, hit2, rt_wf_straggle, the STRAG shade variant)
@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("spread", [1.0, 0.02])
def test_stragglers_run_on_the_soup(orc, spread, overlap):
    """Walks over the trace launch's budget (RT_WF_BUDGET_SMALL = 128 steps) on
    a 96 x 64 frame, finished by the straggler launch beside the shade launch
    (RT_OPT_WF_OVERLAP 1) or after it (0).  Observed on an MI355X, stragglers
    of rays at levels 1 and 2: the soup as it is (spread 1.0) 6,144 of 6,144
    and 6,144 of 6,144 — every box overlaps every other, every walk is long;
    spread 0.02 (its long triangles 0.6 and 8 units) 1,954 of 5,014 and 1,101
    of 2,881 — waves whose lanes finish both ways (kWfPending beside plain
    hits).  At spread 0.01 and below no walk goes over the budget."""
    kernel, counts = render_case(orc, "soup", 1100, W, H, 2, lights=1, spread=spread, wf_overlap=overlap)
    assert counts[1, 2] > 0 and counts[2, 2] > 0, counts[:, 2].tolist()
    assert (counts[:, 2] <= counts[:, 0]).all()


# ---- the reference's own frames (tests/golden/wf_small.npz)
@pytest.fixture(scope="module")
def wf_golden():
    with np.load(os.path.join(GOLDEN, "wf_small.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("wavefront", [1, 0])
@pytest.mark.parametrize("frame", wf_scenes.GOLDEN_FRAMES, ids=lambda f: wf_scenes.golden_key(*f))
def test_reference_frames(orc, wf_golden, frame, wavefront):
    """The wavefront levels and the BVH megakernel (RT_OPT_WAVEFRONT 0), each
    against the whole frame the reference's code rendered."""
    family, ntri, w, h, depth = frame
    path = orc.path(family, ntri)
    with open(path) as f:
        assert str(wf_golden[wf_scenes.sha_key(family, ntri)]) == wf_scenes.text_sha(f.read()), "wf_scenes.py drifted"
    s = rt_amd.Scene(path, w, h, depth)
    ctx = rt_amd.Context(0, wavefront=wavefront)
    try:
        ctx.upload(s)
        got = ctx.render_float(s.frame)
        assert ctx.stats().kernel.startswith("wavefront") == bool(wavefront), ctx.stats().kernel
        want = wf_golden[wf_scenes.golden_key(*frame)]
        bad = (got.view(np.uint32) != want.view(np.uint32)).any(-1)
        assert not bad.any(), f"{int(bad.sum())} pixels differ, first {np.argwhere(bad)[:4].tolist()}"
        if wavefront:
            check_counts(ctx, orc.want(path, w, h, depth))
    finally:
        ctx.close()
