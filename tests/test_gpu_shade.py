"""Radiance queries of arbitrary rays on the HIP path (include/rt.h
rt_shade_rays*, csrc/rt_shaderays.h rt_shade_rays_kernel<MAXD, LB, flags>).

Every expected colour comes from the oracle's own pixel loop pointed along the
ray (tests/shade_ref.py, through liboracle.so at test time) or from the
fixture tests/golden/shade.npz (the reference's own code through oracle/_ref)
— never from the code under test.  Comparison: word for word as uint32; in a
scene with a shininess (a dumped material with shin != 0: powf) within
test_gpu_parity's PHONG_ULP, with RGBA8 within 1 LSB.  The consistency sets
have no oracle expectation: there the CPU backend is the plain restatement and
the GPU must equal it bit for bit.  Which kernel ran is asserted by its name in
rt_stats."""
from __future__ import annotations

import contextlib
import ctypes
import gc
import os
import subprocess

import numpy as np
import pytest

import aov_ref
import rt_amd
import shade_ref
import shade_sets
from conftest import GOLDEN, REPO, bits_equal, rgba8, scene, ulp_diff
from test_gpu_parity import PHONG_ULP

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = 0x7FC12345  # a NaN pattern no query writes
EXE = os.path.join(REPO, "ray-tracing-gpu_amd", "lib", "rt_render")
DEPTHS = (0, 3)
# flags of the instance classes (rt_variant.h): kRayQuery alone; | kSmallList or kBigList (above 1024
# triangles); | kBvh | kSmallList or kBigList
PLAIN, LIT, BVH = "plain", "lit", "bvh"
FLAGS = {PLAIN: (16, 16), LIT: (21, 22), BVH: (277, 278)}
BVH_BIG = 278


def kernel(maxd: int, flags) -> str:
    return f"rt_shade_rays_kernel<{maxd},1,{FLAGS[flags][0] if flags in FLAGS else flags}>"


# scene -> (upload options, does the context hold the BVH).  The instance class follows rt.h's rule:
# with the tree, BVH at every depth; else with triangles LIT on a stack of 0 and PLAIN above; without
# triangles PLAIN.
CLASSES = {
    "scene2": ({}, False), "scene4": ({}, False), "scene7": ({}, False), "scene9": ({}, False),
    "hf1600": ({}, False),                      # 1600 triangles that cannot bounce: the big list, no tree
    "hf1600+ray_bvh": ({"ray_bvh": 1}, True),   # the depth-0 BVH instance
    "mixed63": ({}, False),                     # 63 triangles: no tree
    "mixed64": ({}, True), "mixed65": ({}, True), "chain96": ({}, True), "refract_only96": ({}, True),
    "soup1100": ({}, True), "split1024": ({}, True), "hf1600r": ({}, True),
}
SEEN = set()  # kernel names, for test_every_instance_class_ran
FIXTURE = ("scene2", "scene4", "scene7", "scene9", "mixed64", "soup1100")


def scene_of(key: str) -> str:
    return key.split("+")[0]


@pytest.fixture(scope="module")
def golden_shade():
    return np.load(os.path.join(GOLDEN, "shade.npz"))


@pytest.fixture(scope="module")
def tmpdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("shade"))


def has_bvh(ctx) -> bool:
    L = rt_amd.lib()
    L.rt_debug_bvh_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int]
    out = (ctypes.c_double * 5)()
    assert L.rt_debug_bvh_info(ctx._h, out, 5) == 0
    return out[0] == 1.0


class Made:
    def __init__(self, oracle, tmpdir, key):
        self.case = shade_sets.cases(oracle, scene_of(key), tmpdir)
        self.scene = rt_amd.Scene(self.case["path"], shade_sets.W, shade_sets.H, 3)
        self.ctx = rt_amd.Context(0, **CLASSES[key][0])
        self.ctx.upload(self.scene)
        surf, _, _ = oracle.dump(self.case["path"], shade_sets.W, shade_sets.H)
        self.phong = bool((surf[:, 7] != 0).any())
        self.ntri = int((surf[:, 0].astype(int) == 0).sum())
        self.big = self.ntri > 1024   # rt_dims.h kClusterMinTriangles
        self.bvh = has_bvh(self.ctx)
        assert self.bvh == CLASSES[key][1], key

    def cls(self, stack):
        return BVH if self.bvh else (LIT if self.ntri > 0 and stack == 0 else PLAIN)

    def kernel(self, maxd, cls):
        return kernel(maxd, FLAGS[cls][self.big])

    def frame(self, depth, min_energy=0.01, scene_ior=1.0):
        f = self.scene.frame.copy()
        f.max_bounces, f.min_energy, f.scene_ior = depth, min_energy, scene_ior
        return f


@pytest.fixture(scope="module")
def contexts(oracle, tmpdir):
    """One context per scene and option set for the whole module."""
    made = {}

    def get(key):
        if key not in made:
            made[key] = Made(oracle, tmpdir, key)
        return made[key]

    yield get
    for m in made.values():
        m.ctx.close()


def check(got, want, phong: bool, label=""):
    """Bit for bit; with a shininess in the scene within PHONG_ULP and RGBA8 within 1 LSB."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, label
    if not phong:
        assert shade_ref.colours_differ(got, want, label) == []
        return
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), label
    g, w = np.where(nan, F(0), got), np.where(nan, F(0), want)
    assert ulp_diff(g, w) <= PHONG_ULP, (label, ulp_diff(g, w))
    assert np.abs(rgba8(g).astype(int) - rgba8(w).astype(int)).max() <= 1, label


def device_out(torch, n):
    return torch.full((n, 3), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def words(v):
    return np.ascontiguousarray(v.cpu().numpy()).view(np.uint32)


def check_scene(oracle, m, key, expect=None):
    """Every oracle set at both depths.  The stack is the smallest compiled one that covers the
    REACHABLE depth (0 in a scene that cannot bounce, whatever the frame asks for), and the instance
    class follows it."""
    name = scene_of(key)
    for depth in DEPTHS:
        f = m.frame(depth)
        for label in shade_sets.ORACLE_SETS:
            want = shade_sets.expected(oracle, m.case, label, depth)
            rays = m.case["rays"][label]
            got = m.ctx.shade_rays(rays, f)
            st = m.ctx.stats()
            print(f"{key} depth {depth} {label}: {st.kernel} {st.kernel_ms:.3f} ms, "
                  f"{len(shade_ref.colours_differ(got, want))} sets differ in bits")
            check(got, want, m.phong, f"{key} {label} depth {depth}")
            assert st.stack_depth in ((0,) if depth == 0 else (0, 1, 2, 3)) and st.primary_rays == len(rays)
            if depth > 0 and (name in shade_sets.BOUNCE or name == "mixed63"):
                assert st.stack_depth > 0
            assert st.kernel == m.kernel(st.stack_depth, expect or m.cls(st.stack_depth)) and st.kernel_ms > 0
            SEEN.add(st.kernel)
            assert st.bounce_rays == 0 and st.shadow_rays == 0 and st.triangle_tests == 0


# ------------------------------------------------------------------ scenes
@pytest.mark.parametrize("key", list(CLASSES))
def test_every_set_matches_the_oracle(oracle, contexts, golden_shade, key):
    m = contexts(key)
    name = scene_of(key)
    c0 = shade_sets.expected(oracle, m.case, "base", 0)
    c3 = shade_sets.expected(oracle, m.case, "base", 3) if name in shade_sets.BOUNCE else None
    shade_sets.check_conditions(shade_sets.conditions(c0, c3, m.scene.frame.background[:]), name)
    if name in FIXTURE:  # the fixture's rays are these, and the reference's colours the oracle's
        g = golden_shade
        assert bits_equal(g[f"{name}_rays"], m.case["rays"]["base"])
        assert shade_ref.colours_differ(g[f"{name}_d0"], c0) == []
        assert shade_ref.colours_differ(g[f"{name}_d3"], shade_sets.expected(oracle, m.case, "base", 3)) == []
    check_scene(oracle, m, key)


def test_every_instance_class_ran():
    """(after the scenes above) every class of rt_variant.h's RT_SHADE_RAYS_VARIANTS was seen by name."""
    flags = {(k.split("<")[1].split(",")[0] != "0", int(k.rstrip(">").split(",")[2])) for k in SEEN}
    assert flags >= {(False, 16), (False, 21), (False, 22), (False, 277), (False, 278), (True, 16), (True, 277), (True, 278)}, SEEN


def test_reachable_depth_picks_the_smallest_stack(oracle, contexts):
    """scene2 cannot bounce (k_max = 0): depth 3 still takes the depth-0 stack.  scene9 (no triangles) at depth 4
    takes the stack of 5 (the thinner list), bit for bit the oracle's depth 4."""
    m = contexts("scene2")
    m.ctx.shade_rays(m.case["rays"]["base"], m.frame(3))
    assert m.ctx.stats().kernel == m.kernel(0, m.cls(0))
    m = contexts("scene9")
    got = m.ctx.shade_rays(m.case["rays"]["base"], m.frame(4, min_energy=-1.0))   # every depth reachable
    assert m.ctx.stats().kernel == kernel(5, PLAIN) and m.ctx.stats().stack_depth == 5
    check(got, shade_sets.expected(oracle, m.case, "base", 4, -1.0), m.phong)
    got = m.ctx.shade_rays(m.case["rays"]["base"], m.frame(3, min_energy=-1.0))
    check(got, shade_sets.expected(oracle, m.case, "base", 3, -1.0), m.phong)
    got = m.ctx.shade_rays(m.case["rays"]["base"], m.frame(3, scene_ior=1.33))
    check(got, shade_sets.expected(oracle, m.case, "base", 3, 0.01, 1.33), m.phong)
    f = m.frame(33, min_energy=-1.0)   # every depth reachable: above the deepest compiled stack
    out = np.zeros((4, 3), F)
    assert rt_amd.lib().rt_shade_rays(m.ctx._h, f, m.case["rays"]["base"].ctypes.data, 4, out.ctypes.data) == -6


@pytest.mark.parametrize("key,option", [("mixed65", "bvh"), ("soup1100", "bvh"), ("hf1600", "light_buffer"),
                                        ("mixed64", "light_buffer")])
def test_options_off_give_the_same_bits_through_the_plain_instances(oracle, contexts, key, option):
    m = contexts(key)
    m.ctx.set_option(option, 0)
    try:
        if option == "bvh":   # the light buffer stays: depth 0 lit, above it plain
            for depth, cls in ((0, LIT), (3, PLAIN)):
                got = m.ctx.shade_rays(m.case["rays"]["base"], m.frame(depth))
                st = m.ctx.stats()
                assert st.kernel == m.kernel(st.stack_depth, cls) and (st.stack_depth > 0) == (depth > 0)
                check(got, shade_sets.expected(oracle, m.case, "base", depth), m.phong)
        else:
            check_scene(oracle, m, key, expect=PLAIN)
    finally:
        m.ctx.set_option(option, 1)


def test_heightfield_50k_fixture_rays(golden_shade, heightfield_r05_path):
    """The 50,000-triangle heightfield with reflect 0.5 on its fixture's 128 rays (the expectation is
    the reference's own): the big-list BVH instances."""
    import hashlib

    g = golden_shade
    assert hashlib.sha256(open(heightfield_r05_path, "rb").read()).hexdigest() == str(g["hf50kr_sha256"])
    s = rt_amd.Scene(heightfield_r05_path, 64, 32, 3)
    ctx = rt_amd.Context(0)
    ctx.upload(s)
    for depth in DEPTHS:
        f = s.frame.copy()
        f.max_bounces = depth
        got = ctx.shade_rays(g["hf50kr_rays"], f)
        assert ctx.stats().kernel == kernel(depth, BVH_BIG)
        check(got, g[f"hf50kr_d{depth}"], False, f"hf50kr depth {depth}")
    ctx.close()


# ------------------------------------------------------- counts and pointers
@pytest.mark.parametrize("key", ["scene7", "mixed65"])
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_ray_counts_and_the_tail(oracle, contexts, key, depth, n):
    """The tail lanes, in whole waves (depth 0) and in partial waves (depth 3); a device output of
    n + 64 entries: nothing behind entry n is written."""
    torch = pytest.importorskip("torch")
    m = contexts(key)
    base = m.case["rays"]["base"]
    want = shade_sets.expected(oracle, m.case, "base", depth)
    pick = (np.arange(n) * 7 + n) % len(base)
    rays = np.ascontiguousarray(base[pick])
    dev = device_out(torch, n + 64)
    drays = torch.from_numpy(rays).cuda()
    torch.cuda.synchronize()
    assert rt_amd.lib().rt_shade_rays(m.ctx._h, m.frame(depth), drays.data_ptr(), n, dev.data_ptr()) == 0
    torch.cuda.synchronize()
    check(dev.cpu().numpy()[:n], want[pick], m.phong)
    assert (words(dev)[n:] == SENTINEL).all()
    assert m.ctx.stats().primary_rays == n


def test_mixed_pointers(oracle, contexts):
    """Host rays with a device output, device rays with a host output."""
    torch = pytest.importorskip("torch")
    m = contexts("mixed65")
    rays, want = m.case["rays"]["leaving"], shade_sets.expected(oracle, m.case, "leaving", 3)
    n = len(rays)
    L, f = rt_amd.lib(), m.frame(3)
    dev = device_out(torch, n)
    torch.cuda.synchronize()
    assert L.rt_shade_rays(m.ctx._h, f, rays.ctypes.data, n, dev.data_ptr()) == 0
    torch.cuda.synchronize()
    check(dev.cpu().numpy(), want, m.phong)
    host = np.zeros((n, 3), F)
    drays = torch.from_numpy(rays).cuda()
    torch.cuda.synchronize()
    assert L.rt_shade_rays(m.ctx._h, f, drays.data_ptr(), n, host.ctypes.data) == 0
    check(host, want, m.phong)


def test_argument_and_state_errors(contexts):
    torch = pytest.importorskip("torch")
    L = rt_amd.lib()
    m = contexts("scene7")
    ctx, f = m.ctx, m.frame(3)
    rays = m.case["rays"]["base"]
    out = np.full((len(rays), 3), SENTINEL, np.uint32)
    assert L.rt_shade_rays(ctx._h, None, rays.ctypes.data, 8, out.ctypes.data) == -1        # no params
    assert L.rt_shade_rays(ctx._h, f, rays.ctypes.data, 8, None) == -1
    assert L.rt_shade_rays(ctx._h, f, None, 8, out.ctypes.data) == -1
    assert L.rt_shade_rays(ctx._h, f, rays.ctypes.data, -1, out.ctypes.data) == -1
    assert L.rt_shade_rays(ctx._h, f, rays.ctypes.data, 2**31, out.ctypes.data) == -1
    assert L.rt_shade_rays(ctx._h, f, rays.ctypes.data, 0, out.ctypes.data) == 0
    assert L.rt_cpu_shade_rays(ctx._h, f, rays.ctypes.data, 8, out.ctypes.data) == -4       # the other backend's call
    assert (out == SENTINEL).all()
    drays = torch.from_numpy(np.concatenate([rays.ravel(), np.zeros(2, F)])).cuda()
    dev = device_out(torch, len(rays) + 2)
    torch.cuda.synchronize()
    assert L.rt_shade_rays_async(ctx._h, f, rays.ctypes.data, 8, dev.data_ptr(), None) == -1           # host rays
    assert L.rt_shade_rays_async(ctx._h, f, drays.data_ptr(), 8, out.ctypes.data, None) == -1          # host output
    assert L.rt_shade_rays_async(ctx._h, f, drays.data_ptr() + 4, 8, dev.data_ptr(), None) == -1       # misaligned
    assert L.rt_shade_rays_async(ctx._h, f, drays.data_ptr(), 8, dev.data_ptr() + 4, None) == -1
    assert L.rt_shade_rays_async(ctx._h, None, drays.data_ptr(), 8, dev.data_ptr(), None) == -1
    assert L.rt_shade_rays_async(ctx._h, f, None, 8, dev.data_ptr(), None) == -1
    assert L.rt_shade_rays_async(ctx._h, f, drays.data_ptr(), 8, None, None) == -1
    assert L.rt_shade_rays_async(ctx._h, f, drays.data_ptr(), -1, dev.data_ptr(), None) == -1
    assert L.rt_shade_rays(ctx._h, f, drays.data_ptr() + 4, 8, dev.data_ptr()) == -1
    assert L.rt_shade_rays(ctx._h, f, drays.data_ptr(), 8, dev.data_ptr() + 4) == -1
    assert L.rt_shade_rays_async(ctx._h, f, drays.data_ptr(), 0, dev.data_ptr(), None) == 0
    ctx.sync()
    torch.cuda.synchronize()
    assert (words(dev) == SENTINEL).all() and (out == SENTINEL).all()   # no refused call wrote anything
    fresh = rt_amd.Context(0)
    assert L.rt_shade_rays(fresh._h, f, rays.ctypes.data, 8, out.ctypes.data) == -4                    # before an upload
    assert L.rt_shade_rays_async(fresh._h, f, drays.data_ptr(), 8, dev.data_ptr(), None) == -4
    fresh.close()


def test_stats_flag_is_ignored(oracle, contexts):
    m = contexts("scene7")
    f = m.frame(3)
    f.flags |= 1  # RT_FLAG_STATS
    got = m.ctx.shade_rays(m.case["rays"]["base"], f)
    st = m.ctx.stats()
    assert st.stack_depth > 0 and st.kernel == kernel(st.stack_depth, PLAIN)
    assert st.primary_rays == 128 and st.shadow_rays == 0 and st.triangle_tests == 0
    check(got, shade_sets.expected(oracle, m.case, "base", 3), m.phong)


# ------------------------------------------------ a frame is a shade query
def camera_rays(f, w, h):
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    D = aov_ref.camera_dirs(aov_ref.Cam.from_frame(f), xs.ravel(), ys.ravel())
    O = np.broadcast_to(np.asarray(f.cam_pos[:], F), D.shape)
    return np.ascontiguousarray(np.concatenate([O, D], 1), F)


@pytest.mark.parametrize("key,depth,frame_kernel", [("scene2", 0, None), ("scene7", 3, None), ("hf1600", 0, None),
                                                    ("mixed64", 3, "wavefront")])
def test_a_frame_equals_the_query_of_its_camera_rays(contexts, key, depth, frame_kernel):
    """64 x 32: render_float against shade_rays of the frame's camera rays (mixed64 at depth 3: the
    frame takes the wavefront path, the query the single-kernel DFS)."""
    m = contexts(key)
    f = m.frame(depth)
    img = m.ctx.render_float(f)
    if frame_kernel:
        assert frame_kernel in m.ctx.stats().kernel
    got = m.ctx.shade_rays(camera_rays(f, 64, 32), f)
    assert "rt_shade_rays_kernel" in m.ctx.stats().kernel
    check(got.reshape(img.shape), img, m.phong, key)


# ------------------------------------------------------------------ async
@contextlib.contextmanager
def capture(torch, g):
    """torch.cuda.graph without the garbage collector (a collection could
    finalize a context, whose rt_destroy synchronises: illegal in a capture)."""
    gc.collect()
    gc.disable()
    try:
        with torch.cuda.graph(g):
            yield
    finally:
        gc.enable()


def test_two_streams_without_a_host_sync(oracle, contexts):
    torch = pytest.importorskip("torch")
    m = contexts("mixed65")
    ra, rb = m.case["rays"]["base"], m.case["rays"]["axis"]
    ea, eb = shade_sets.expected(oracle, m.case, "base", 3), shade_sets.expected(oracle, m.case, "axis", 0)
    da, db = torch.from_numpy(ra).cuda(), torch.from_numpy(rb).cuda()
    pa, pb, pc = device_out(torch, len(ra)), device_out(torch, len(rb)), device_out(torch, len(rb))
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    f3, f0 = m.frame(3), m.frame(0)
    m.ctx.shade_rays_async(f3, da.data_ptr(), len(ra), pa.data_ptr(), sa.cuda_stream)
    m.ctx.shade_rays_async(f0, db.data_ptr(), len(rb), pb.data_ptr(), sb.cuda_stream)
    m.ctx.shade_rays_async(f0, db.data_ptr(), len(rb), pc.data_ptr(), sa.cuda_stream)   # behind the first, on its stream
    m.ctx.sync()
    torch.cuda.synchronize()
    check(pa.cpu().numpy(), ea, m.phong)
    check(pb.cpu().numpy(), eb, m.phong)
    check(pc.cpu().numpy(), eb, m.phong)


@pytest.mark.parametrize("name,depth", [("scene7", 0), ("scene7", 3), ("mixed65", 3)])
def test_graph_capture_on_a_context_that_never_rendered(oracle, contexts, tmpdir, name, depth):
    """Captured on a fresh context, replayed twice with the device ray buffer rewritten in between:
    the outputs follow the buffer.  Depth 3: the instances with a bounce stack in scratch."""
    torch = pytest.importorskip("torch")
    c = shade_sets.cases(oracle, name, tmpdir)
    s = rt_amd.Scene(c["path"], 64, 32, depth)
    ctx = rt_amd.Context(0)
    ctx.upload(s)
    ra, rb = c["rays"]["base"], c["rays"]["axis"]
    ea, eb = shade_sets.expected(oracle, c, "base", depth), shade_sets.expected(oracle, c, "axis", depth)
    n = len(ra)
    assert len(rb) == n
    drays = torch.from_numpy(ra).cuda()
    dev = device_out(torch, n)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with capture(torch, g):
        ctx.shade_rays_async(s.frame, drays.data_ptr(), n, dev.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (words(dev) == SENTINEL).all()   # captured, not run
    for rays, exp in ((ra, ea), (rb, eb)):
        drays.copy_(torch.from_numpy(rays))
        g.replay()
        torch.cuda.synchronize()
        check(dev.cpu().numpy(), exp, contexts(name).phong)
    ctx.close()


# ------------------------------------------- consistency: GPU against CPU
@pytest.mark.parametrize("key", ["scene7", "scene9", "hf1600", "mixed65", "soup1100"])
def test_consistency_sets_equal_the_cpu_backend(contexts, key):
    """No oracle shades these (non-unit and infinite directions): consistency, not parity."""
    m = contexts(key)
    cpu = rt_amd.CpuContext(min(8, os.cpu_count() or 1))
    cpu.upload(m.scene)
    for depth in DEPTHS:
        f = m.frame(depth)
        for label, rays in m.case["consistency"].items():
            check(m.ctx.shade_rays(rays, f), cpu.shade_rays(rays, f), m.phong, f"{key} {label} depth {depth}")


# -------------------------------------------------------------- CLI, CScene
def test_cli_colours_hip(tmp_path, golden_shade):
    g = golden_shade
    src, dst = tmp_path / "rays.npy", tmp_path / "c.npy"
    np.save(src, g["scene7_rays"])
    r = subprocess.run([EXE, scene(7), "--backend", "hip", "-d", "3", "--rays", str(src), "--colours", str(dst)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert shade_ref.colours_differ(np.load(dst), g["scene7_d3"]) == []
    assert "rt_shade_rays_kernel<" in r.stdout and ",1,16>" in r.stdout


def test_cscene_colour_verb(golden_shade):
    c = rt_amd.CScene()
    c.AjusterResolution(64, 48)
    c.AjusterNbRebondsMax(3)
    c.TraiterFichierDeScene(scene(7))
    got = c.LancerListeDeRayonsCouleur(golden_shade["scene7_rays"])
    assert shade_ref.colours_differ(got, golden_shade["scene7_d3"]) == []
