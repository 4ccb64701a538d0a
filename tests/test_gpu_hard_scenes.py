"""The hard scenes (tests/hard_scenes.py) on the GPU: coincident surfaces with
different colours (the tie-break by file order, through every structure that
reorders triangles), the launch-camera kernels (rt_trace_tiny) on stress
geometry and on both sides of their list-size limit, odd quadrics, materials
that reflect and refract at once, and whole scenes scaled by powers of two.

Every frame is compared bit for bit in float32 with the oracle, which
tests/test_hard_scenes.py pins to the reference's own frames
(tests/golden/hard.npz) and whose conditions it checks.  Frames are 48 x 36
(even seeds) or the ragged 47 x 35 (odd seeds); contexts are made once per
module.  Every case prints the kernel labels it saw.
"""
from __future__ import annotations

import ctypes
import re

import numpy as np
import pytest

import cameras
import hard_scenes as hs
import rt_amd
from aov_ref import planes_equal
from conftest import rgba8
from hard_frames import Frames

pytestmark = pytest.mark.gpu

WF_LEVELS = 9  # rt_debug_wf_counts: levels 0 .. kWfMaxLevels
STACKS = (0, 1, 2, 3, 4, 5, 8, 12, 16, 20, 32)  # the compiled bounce-stack capacities (rt_stats.stack_depth)


@pytest.fixture(scope="module")
def hard(oracle, tmp_path_factory):
    return Frames(oracle, tmp_path_factory.mktemp("hard_gpu"))


@pytest.fixture(scope="module")
def ctxs():
    """The default context, the same library without the launch-camera
    kernels, and without the light and camera buffers."""
    out = {"default": rt_amd.Context(0), "launch_camera=0": rt_amd.Context(0, launch_camera=0),
           "no buffers": rt_amd.Context(0, light_buffer=0, camera_buffer=0)}
    yield out
    for c in out.values():
        c.close()


@pytest.fixture(scope="module")
def no_wavefront():
    c = rt_amd.Context(0, wavefront=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def no_bvh():
    c = rt_amd.Context(0, bvh=0)
    yield c
    c.close()


def is_tiny(ctx) -> bool:
    return ctx.stats().kernel.startswith("rt_trace_tiny")


def check(ctx, frame, want, what=""):
    """One float32 render of `frame` against the oracle's image; the label."""
    got = ctx.render_float(frame)
    kernel = ctx.stats().kernel
    bad = (got.view(np.uint32) != want.view(np.uint32)).any(-1)
    assert got.shape == want.shape and not bad.any(), \
        (what, kernel, f"{int(bad.sum())} pixels differ, first (row, col) {np.argwhere(bad)[:4].tolist()}")
    return kernel


def check_all(ctxs, hard, path, w, h, depth, what):
    """The frame through the three contexts, the default context's RGBA8
    against the launch_camera=0 context's; {context: label}."""
    want = hard.want(path, w, h, depth)
    assert np.isfinite(want.img).all()
    s = rt_amd.Scene(path, w, h, depth)
    labels = {}
    for name, c in ctxs.items():
        c.upload(s)
        labels[name] = check(c, s.frame, want.img, (what, name))
    rgba = ctxs["default"].render(s.frame)
    assert np.array_equal(rgba, ctxs["launch_camera=0"].render(s.frame))
    assert np.array_equal(rgba, rgba8(want.img))
    print(what, "depth", depth, labels)
    return s, labels


# ---- every family x 6 seeds
@pytest.mark.parametrize("seed", hs.SEEDS)
@pytest.mark.parametrize("family", hs.FAMILIES)
def test_families(ctxs, hard, family, seed):
    w, h = hs.size(seed)
    path = hard.path(family, seed)
    for depth in (0, hs.DEPTH[family]):
        s, labels = check_all(ctxs, hard, path, w, h, depth, (family, seed))
        assert not labels["launch_camera=0"].startswith("rt_trace_tiny")
        if seed in (0, 3):  # a slab that starts off the 8-row tile grid
            f = s.frame.copy()
            f.row_begin, f.row_end = 3, h
            for name, c in ctxs.items():
                check(c, f, hard.want(path, w, h, depth).img[3:], (family, "rows 3..h", name))


def test_infinite_hits(ctxs, hard):
    """quadrics/axis: B == 0 on the middle row, hits at t = +inf, a finite frame."""
    path = hard.path("quadrics/axis", 0)
    for depth in (0, 3):
        s, _ = check_all(ctxs, hard, path, 48, 36, depth, "quadrics/axis")
    want = hard.aov(path, 48, 36)
    assert np.isposinf(want["t"]).any()
    for name, c in ctxs.items():
        assert planes_equal(c.render_aov(s.frame), want) == [], name


# ---- the launch-camera kernels
def moved(frame):
    """Three moved cameras (yawed and moved, pitched and rolled and moved,
    slid sideways), then the first again."""
    return [cameras.turned(frame, cameras.rot(1, 7.0), (3.0, 0.5, -2.0)),
            cameras.turned(frame, cameras.rot(0, -6.0) @ cameras.rot(2, 20.0), (-4.0, 1.0, 2.0)),
            cameras.moving(frame, 2)[1], frame]


TINY = [("tiny_stress", seed, None) for seed in hs.SEEDS] + [("ties", 0, 3), ("ties", 0, 20)]


@pytest.mark.parametrize("family,seed,ntri", TINY, ids=lambda v: str(v))
def test_launch_camera_kernels(ctxs, hard, family, seed, ntri):
    w, h = hs.size(seed)
    path = hard.path(family, seed, ntri)
    s = rt_amd.Scene(path, w, h, 0)
    ctx, general = ctxs["default"], ctxs["launch_camera=0"]
    ctx.upload(s)
    general.upload(s)
    labels = set()
    for k, f in enumerate([s.frame] + moved(s.frame)):
        want = hard.want(path, w, h, 0, frame=None if f is s.frame else f).img
        assert np.isfinite(want).all()
        assert not check(general, f, want, (family, seed, "camera", k, "general")).startswith("rt_trace_tiny")
        for rep in range(3):  # the tile masks computed, computed and stored, read
            kernel = check(ctx, f, want, (family, seed, "camera", k, "render", rep))
            assert kernel.startswith("rt_trace_tiny"), kernel
            labels.add(kernel)
        assert np.array_equal(ctx.render(f), general.render(f))
    print(family, seed, ntri, sorted(labels))


def test_ties_of_21_triangles_take_the_general_kernels(ctxs, hard):
    s = rt_amd.Scene(hard.path("ties", 0, 21), 48, 36, 0)
    ctxs["default"].upload(s)
    ctxs["default"].render_float(s.frame)
    assert not is_tiny(ctxs["default"]), ctxs["default"].stats().kernel


# ---- the list-size edges: 20 | 21 (kTinyMax), 256 | 257 (kTricamMaxTriangles), 1024 | 1025 (clusters)
@pytest.mark.parametrize("ntri", [20, 21, 256, 257, 1024, 1025, 1026])
def test_ties_list_sizes(ctxs, hard, ntri):
    w, h = 48, 36
    path = hard.path("ties", 0, ntri)
    s, labels = check_all(ctxs, hard, path, w, h, 0, ("ties", ntri))
    assert labels["default"].startswith("rt_trace_tiny") == (ntri <= 20), labels
    # the id plane shows the tie-break directly
    want = hard.aov(path, w, h)
    for name, c in ctxs.items():
        assert planes_equal(c.render_aov(s.frame), want) == [], name
    counted = s.frame.copy()
    counted.flags |= rt_amd.FLAG_STATS
    counts = {}
    for name, c in ctxs.items():
        check(c, counted, hard.want(path, w, h, 0).img, ("counted", name))
        counts[name] = (c.stats().primary_rays, c.stats().shadow_rays)
    print("primary, shadow rays", counts)
    assert len(set(counts.values())) == 1 and counts["default"][0] == w * h, counts


def wf_counts(ctx):
    L = rt_amd.lib()
    L.rt_debug_wf_counts.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    out = np.zeros(3 * WF_LEVELS, np.uint32)
    assert L.rt_debug_wf_counts(ctx._h, out.ctypes.data, out.size) == 0, ctx._err()
    return out.reshape(WF_LEVELS, 3).astype(np.int64)  # [level] = rays, parents, stragglers


@pytest.mark.parametrize("ntri", [256, 1026])
def test_ties_bounces(ctxs, no_wavefront, no_bvh, hard, ntri):
    """Depth 2 over the reflective and refractive duplicates: the wavefront
    levels with their counts, the BVH megakernel, the plain bounce kernel."""
    w, h, depth = 47, 35, 2
    path = hard.path("ties", 0, ntri)
    want = hard.want(path, w, h, depth)
    assert want.rays[2] > 0 and np.isfinite(want.img).all()
    s = rt_amd.Scene(path, w, h, depth)
    labels = []
    for c in (ctxs["default"], no_wavefront, no_bvh):
        c.upload(s)
        labels.append(check(c, s.frame, want.img, ("ties", ntri, "depth 2")))
        if c is ctxs["default"]:
            got = wf_counts(c)
            assert got[1:, 0].tolist() == want.rays[1:WF_LEVELS].tolist(), "rays per level"
            assert got[:, 1].tolist() == want.parents[:WF_LEVELS].tolist(), "parents per level"
    print("ties", ntri, "depth 2", labels)
    assert labels[0].startswith("wavefront") and labels[0].endswith("+ 2 levels"), labels
    assert re.fullmatch(r"rt_trace_kernel<2,1,(269|270)>", labels[1]), labels
    assert re.fullmatch(r"rt_trace_kernel<2,1,0>", labels[2]), labels


# ---- materials: both children at every node, on each side of the stacks of 5 and 8
@pytest.mark.parametrize("depth", [5, 6, 8, 9])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_materials_depths(ctxs, hard, seed, depth):
    """rt_stats.stack_depth is the compiled stack that ran (rt.h): never under
    the deepest level the oracle's tree reaches; with a K >= 1 surface no
    level can be ruled out by the energy bound, so the stack is the one
    compiled for the requested depth — the depth itself at 5 and 8, the next
    capacity (8, 12) at 6 and 9."""
    w, h = 24, 18
    path = hard.path("materials", seed)
    want = hard.want(path, w, h, depth)
    assert np.isfinite(want.img).all()
    s = rt_amd.Scene(path, w, h, depth)
    for name, c in ctxs.items():
        c.upload(s)
        kernel = check(c, s.frame, want.img, ("materials", seed, depth, name))
        stack = c.stats().stack_depth
        print("materials", seed, depth, name, kernel, "stack", stack, "deepest level", want.deepest)
        assert stack >= want.deepest
        if hs.has_k_at_least_1(hs.hard_dat("materials", seed)):
            assert stack == min(d for d in STACKS if d >= depth)


def test_materials_depth_40_is_unsupported(ctxs, hard):
    """K = 1.2: every level is reachable, 40 of them exceed the deepest stack."""
    text = hs.hard_dat("materials", 0)
    assert "reflect: 1.200" in text
    s = rt_amd.Scene(hard.path("materials", 0), 8, 8, 40)
    ctxs["default"].upload(s)
    with pytest.raises(rt_amd.RtError) as e:
        ctxs["default"].render_float(s.frame)
    assert e.value.code == -6


# ---- whole scenes scaled by powers of two
@pytest.mark.parametrize("scale", hs.SCALES, ids=lambda s: "2^%d" % np.log2(s))
@pytest.mark.parametrize("family,seed", hs.SCALED)
def test_scaled(ctxs, hard, family, seed, scale):
    w, h = hs.size(seed)
    path = hard.path(family, seed, 20 if family == "ties" else None, scale)
    want = hard.want(path, w, h, 0).img
    assert np.isfinite(want).all()
    s = rt_amd.Scene(path, w, h, 0)
    labels = {}
    for name in ("default", "launch_camera=0"):
        ctxs[name].upload(s)
        for rep in range(3 if name == "default" else 1):
            labels[name] = check(ctxs[name], s.frame, want, (family, scale, name, rep))
    print(family, "scale", scale, labels)
    assert np.array_equal(ctxs["default"].render(s.frame), ctxs["launch_camera=0"].render(s.frame))
