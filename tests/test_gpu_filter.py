"""Shadow-filter queries of arbitrary segments on the HIP path (include/rt.h
rt_filter_rays*, csrc/rt_filter.h rt_filter_kernel<BVH>).

Every expected filter comes from tests/filter_ref.py through liboracle.so at
test time or from the fixture tests/golden/filter.npz (the reference's own
Intersection() through oracle/_ref) — never from the code under test.
Comparison: word for word as uint32; where the expectation is NaN the result
is NaN.  Which kernel ran is asserted by its name in rt_stats."""
from __future__ import annotations

import contextlib
import ctypes
import gc
import os
import subprocess

import numpy as np
import pytest

import aov_ref
import filter_ref
import filter_sets
import rt_amd
from conftest import GOLDEN, REPO, bits_equal, scene

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = 0x7FC12345  # a NaN pattern no query writes
EXE = os.path.join(REPO, "ray-tracing-gpu_amd", "lib", "rt_render")
K0, K1 = "rt_filter_kernel<0>", "rt_filter_kernel<1>"
KERNEL = {name: (K1 if name in filter_sets.BVH_SCENES else K0) for name in filter_sets.SCENES}


@pytest.fixture(scope="module")
def golden_filter():
    return np.load(os.path.join(GOLDEN, "filter.npz"))


@pytest.fixture(scope="module")
def tmpdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("filter"))


@pytest.fixture(scope="module")
def contexts(oracle, tmpdir):
    """One context per scene for the whole module: name -> (context, its cases)."""
    made = {}

    def get(name):
        if name not in made:
            c = filter_sets.cases(oracle, name, tmpdir)
            ctx = rt_amd.Context(0, **filter_sets.OPTIONS.get(name, {}))
            ctx.upload(rt_amd.Scene(c["path"], filter_sets.W, filter_sets.H))
            made[name] = (ctx, c)
        return made[name]

    yield get
    for ctx, _ in made.values():
        ctx.close()


def device_out(torch, n):
    return torch.full((n, 3), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def words(v):
    return np.ascontiguousarray(v.cpu().numpy()).view(np.uint32)


def has_bvh(ctx) -> bool:
    L = rt_amd.lib()
    L.rt_debug_bvh_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int]
    out = (ctypes.c_double * 5)()
    assert L.rt_debug_bvh_info(ctx._h, out, 5) == 0
    return out[0] == 1.0


def check_sets(ctx, c, kernel, other=None):
    for label, (segs, d) in c["sets"].items():
        got = ctx.filter_rays(segs)
        assert filter_ref.differ(got, d["filter"]) == [], label
        st = ctx.stats()
        assert st.kernel == kernel, label
        assert st.shadow_rays == len(segs) and st.primary_rays == 0 and st.bounce_rays == 0 and st.kernel_ms > 0
        assert st.triangle_tests == 0 and st.shadow_tests_skipped == 0 and st.bvh_nodes_visited == 0
        if other is not None:
            assert filter_ref.differ(got, other.filter_rays(segs)) == [], label


# ------------------------------------------------------------------ scenes
@pytest.mark.parametrize("name", filter_sets.SCENES)
def test_every_set_matches_the_oracle(contexts, name):
    ctx, c = contexts(name)
    filter_sets.check_conditions(name, c["sets"])
    check_sets(ctx, c, KERNEL[name])
    if KERNEL[name] == K1 or name == "layers_neg":
        assert has_bvh(ctx)   # (layers_neg: the tree is there, and the file-order product still runs)


@pytest.mark.parametrize("name", ["soup1100", "layers", "layers10"])
def test_bvh_option_off_gives_the_same_bits(contexts, name):
    ctx, c = contexts(name)
    ctx.set_option("bvh", 0)
    try:
        check_sets(ctx, c, K0)
    finally:
        ctx.set_option("bvh", 1)


def test_heightfield_1600_ray_bvh_option(contexts):
    """A non-reflective mesh: kernel <0> by default, with RT_OPT_RAY_BVH 1 the
    BVH and kernel <1>: the same bits.  Colour and AOV frames keep their
    kernels and bits under both."""
    ctx0, c = contexts("hf1600")
    assert not has_bvh(ctx0)
    ctx1 = rt_amd.Context(0, ray_bvh=1)
    s0 = rt_amd.Scene(c["path"], 64, 32, 0)
    s3 = rt_amd.Scene(c["path"], 64, 32, 3)
    ctx1.upload(s0)
    assert has_bvh(ctx1)
    check_sets(ctx1, c, K1, other=ctx0)
    assert ctx0.stats().kernel == K0
    for f in (s0.frame, s3.frame):
        a, ka = ctx0.render_float(f), ctx0.stats().kernel
        b, kb = ctx1.render_float(f), ctx1.stats().kernel
        assert ka == kb and "rt_filter" not in ka and bits_equal(a, b)
    a, ka = ctx0.render_aov(s0.frame), ctx0.stats().kernel
    b, kb = ctx1.render_aov(s0.frame), ctx1.stats().kernel
    assert ka == kb and aov_ref.planes_equal(a, b) == []
    ctx1.close()


def test_heightfield_50k_with_ray_bvh(golden_filter, heightfield_path):
    g = golden_filter
    ctx = rt_amd.Context(0, ray_bvh=1)
    ctx.upload(rt_amd.Scene(heightfield_path, 64, 32))
    got = ctx.filter_rays(g["hf50k_segs"])
    assert ctx.stats().kernel == K1
    assert filter_ref.differ(got, g["hf50k_filter"]) == []
    ctx.close()


@pytest.mark.parametrize("name,label", [("scene7", "lights"), ("layers", "cross"), ("mixed65", "through")])
def test_fixture_sets(contexts, golden_filter, name, label):
    ctx, _ = contexts(name)
    g = golden_filter
    assert filter_ref.differ(ctx.filter_rays(g[f"{name}_{label}_segs"]), g[f"{name}_{label}_filter"]) == []


# ------------------------------------------ the renderer's own shadow rays
def dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


@pytest.mark.parametrize("i", [2, 6])
def test_the_frames_own_shadow_rays_and_colour(oracle, i):
    """64 x 32, depth 0: for every pixel with a primary hit (the AOV planes)
    and every light whose N.L gate passes, the filter of the segment from
    float32(O + t D) to the light equals filter_ref's; and the pixel's colour,
    recomputed in float32 numpy from the AOV planes, THESE filters and
    ObtenirCouleurSurIntersection's formula (rt_oracle.c shade(), restated as
    in tests/golden/make_aov_golden.py), equals the rendered frame bit for bit."""
    path = scene(i)
    surf, cam_words, lights = oracle.dump(path, 64, 32)
    s = rt_amd.Scene(path, 64, 32, 0)
    ctx = rt_amd.Context(0)
    ctx.upload(s)
    f = s.frame
    aov = ctx.render_aov(f)
    img = ctx.render_float(f).reshape(-1, 3)
    ys, xs = np.meshgrid(np.arange(32), np.arange(64), indexing="ij")
    cam = aov_ref.Cam.from_frame(f)
    D = aov_ref.camera_dirs(cam, xs.ravel(), ys.ravel())
    ids, t, n = aov["id"].reshape(-1), aov["t"].reshape(-1), aov["n"].reshape(-1, 3)
    hit = ids >= 0
    assert hit.sum() >= 200
    powf = aov_ref.libm_powf()
    with np.errstate(all="ignore"):
        P = (cam.pos[None] + D * t[:, None]).astype(F)
        m = surf[np.where(hit, ids, 0)]
        color, ka, kd, ks, shin = m[:, 1:4], m[:, 4], m[:, 5], m[:, 6], m[:, 7]
        res = (color * ka[:, None]).astype(F)
        tinted = 0
        for L in lights:
            ld = (L[None, 0:3] - P).astype(F)
            gate = hit & (dot3(ld, n) > 0)
            k = np.flatnonzero(gate)
            segs = np.ascontiguousarray(np.concatenate([P[k], ld[k]], 1), F)
            Fg = ctx.filter_rays(segs)
            assert filter_ref.differ(Fg, filter_ref.filters(oracle.L.oracle_intersect, surf, segs)) == []
            assert filter_sets.white(Fg).any() and not filter_sets.white(Fg).all()
            tinted += int((~filter_sets.white(Fg) & ~filter_sets.black(Fg)).sum())
            dist, lrd = filter_ref.directions(segs)
            nk, dk = n[k], D[k]
            LC = (L[None, 3:6] * Fg).astype(F)
            g = L[6] * kd[k] * dot3(nk, lrd)
            r = res[k] + (color[k] * g[:, None]) * LC
            sc = F(2) * dot3(lrd, nk)
            rf = lrd - nk * sc[:, None]
            ps = dot3(rf, dk)
            pw = np.array([powf(float(a), float(b)) if a > 0 else 0.0 for a, b in zip(ps, shin[k])], F)
            pf = L[6] * ks[k] * pw
            r = np.where((ps > 0)[:, None], r + LC * pf[:, None], r)
            res[k] = r.astype(F)
        bg = np.asarray(f.background[:], F)
        want = np.where(hit[:, None], res, bg[None]).astype(F)
    if i == 6:
        assert tinted >= 5   # scene6: shadow rays through translucent surfaces
    assert bits_equal(np.ascontiguousarray(want), np.ascontiguousarray(img))
    ctx.close()


# ------------------------------------------------------- counts and pointers
@pytest.mark.parametrize("name", ["scene3", "layers"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 4097])
def test_segment_counts_and_the_tail(contexts, name, n):
    """A device output of n + 64 entries: nothing behind entry n is written."""
    torch = pytest.importorskip("torch")
    ctx, c = contexts(name)
    base, d = c["sets"]["cross" if name == "layers" else "through"]
    pick = (np.arange(n) * 7 + n) % len(base)
    segs = np.ascontiguousarray(base[pick])
    dev = device_out(torch, n + 64)
    dsegs = torch.from_numpy(segs).cuda()
    torch.cuda.synchronize()
    assert rt_amd.lib().rt_filter_rays(ctx._h, dsegs.data_ptr(), n, dev.data_ptr()) == 0
    torch.cuda.synchronize()
    assert filter_ref.differ(dev.cpu().numpy()[:n], d["filter"][pick]) == []
    assert (words(dev)[n:] == SENTINEL).all()
    assert ctx.stats().shadow_rays == n and ctx.stats().kernel == KERNEL[name]


def test_mixed_pointers(contexts):
    """Host segments with a device output, device segments with a host output."""
    torch = pytest.importorskip("torch")
    ctx, c = contexts("mixed65")
    segs, d = c["sets"]["through"]
    n = len(segs)
    L = rt_amd.lib()
    dev = device_out(torch, n)
    torch.cuda.synchronize()
    assert L.rt_filter_rays(ctx._h, segs.ctypes.data, n, dev.data_ptr()) == 0
    torch.cuda.synchronize()
    assert filter_ref.differ(dev.cpu().numpy(), d["filter"]) == []
    host = np.zeros((n, 3), F)
    dsegs = torch.from_numpy(segs).cuda()
    torch.cuda.synchronize()
    assert L.rt_filter_rays(ctx._h, dsegs.data_ptr(), n, host.ctypes.data) == 0
    assert filter_ref.differ(host, d["filter"]) == []


def test_argument_and_state_errors(contexts):
    torch = pytest.importorskip("torch")
    L = rt_amd.lib()
    ctx, c = contexts("scene3")
    segs = c["sets"]["through"][0]
    out = np.full((len(segs), 3), SENTINEL, np.uint32)
    assert L.rt_filter_rays(ctx._h, segs.ctypes.data, 8, None) == -1
    assert L.rt_filter_rays(ctx._h, None, 8, out.ctypes.data) == -1
    assert L.rt_filter_rays(ctx._h, segs.ctypes.data, -1, out.ctypes.data) == -1
    assert L.rt_filter_rays(ctx._h, segs.ctypes.data, 2**31, out.ctypes.data) == -1
    assert L.rt_filter_rays(ctx._h, segs.ctypes.data, 0, out.ctypes.data) == 0
    assert L.rt_cpu_filter_rays(ctx._h, segs.ctypes.data, 8, out.ctypes.data) == -4      # the other backend's call
    assert (out == SENTINEL).all()
    # async: device pointers only, 8-byte aligned
    dsegs = torch.from_numpy(np.concatenate([segs.ravel(), np.zeros(2, F)])).cuda()
    dev = device_out(torch, len(segs) + 2)
    torch.cuda.synchronize()
    assert L.rt_filter_rays_async(ctx._h, segs.ctypes.data, 8, dev.data_ptr(), None) == -1            # host segments
    assert L.rt_filter_rays_async(ctx._h, dsegs.data_ptr(), 8, out.ctypes.data, None) == -1           # host output
    assert L.rt_filter_rays_async(ctx._h, dsegs.data_ptr() + 4, 8, dev.data_ptr(), None) == -1        # misaligned
    assert L.rt_filter_rays_async(ctx._h, dsegs.data_ptr(), 8, dev.data_ptr() + 4, None) == -1
    assert L.rt_filter_rays_async(ctx._h, None, 8, dev.data_ptr(), None) == -1
    assert L.rt_filter_rays_async(ctx._h, dsegs.data_ptr(), 8, None, None) == -1
    assert L.rt_filter_rays_async(ctx._h, dsegs.data_ptr(), -1, dev.data_ptr(), None) == -1
    assert L.rt_filter_rays(ctx._h, dsegs.data_ptr() + 4, 8, dev.data_ptr()) == -1
    assert L.rt_filter_rays(ctx._h, dsegs.data_ptr(), 8, dev.data_ptr() + 4) == -1
    assert L.rt_filter_rays_async(ctx._h, dsegs.data_ptr(), 0, dev.data_ptr(), None) == 0
    ctx.sync()
    torch.cuda.synchronize()
    assert (words(dev) == SENTINEL).all() and (out == SENTINEL).all()   # no refused call wrote anything
    fresh = rt_amd.Context(0)
    assert L.rt_filter_rays(fresh._h, segs.ctypes.data, 8, out.ctypes.data) == -4                      # before an upload
    assert L.rt_filter_rays_async(fresh._h, dsegs.data_ptr(), 8, dev.data_ptr(), None) == -4
    fresh.close()


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


def test_two_streams_without_a_host_sync(contexts):
    torch = pytest.importorskip("torch")
    ctx, c = contexts("layers")
    (ra, ea), (rb, eb) = c["sets"]["cross"], c["sets"]["through"]
    da, db = torch.from_numpy(ra).cuda(), torch.from_numpy(rb).cuda()
    pa, pb, pc = device_out(torch, len(ra)), device_out(torch, len(rb)), device_out(torch, len(rb))
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx.filter_rays_async(da.data_ptr(), len(ra), pa.data_ptr(), sa.cuda_stream)
    ctx.filter_rays_async(db.data_ptr(), len(rb), pb.data_ptr(), sb.cuda_stream)
    ctx.filter_rays_async(db.data_ptr(), len(rb), pc.data_ptr(), sa.cuda_stream)   # behind the first, on its stream
    ctx.sync()
    torch.cuda.synchronize()
    assert filter_ref.differ(pa.cpu().numpy(), ea["filter"]) == []
    assert filter_ref.differ(pb.cpu().numpy(), eb["filter"]) == []
    assert filter_ref.differ(pc.cpu().numpy(), eb["filter"]) == []


@pytest.mark.parametrize("name", ["scene3", "layers"])
def test_graph_capture_on_a_context_that_never_rendered(oracle, tmpdir, name):
    """Captured on a fresh context, replayed twice with the device segment
    buffer rewritten in between: the outputs follow the buffer."""
    torch = pytest.importorskip("torch")
    c = filter_sets.cases(oracle, name, tmpdir)
    ctx = rt_amd.Context(0)
    ctx.upload(rt_amd.Scene(c["path"], 64, 32))
    (ra, ea), (rb, eb) = c["sets"]["through"], c["sets"]["axis"]
    n = len(ra)
    assert len(rb) == n
    dsegs = torch.from_numpy(ra).cuda()
    dev = device_out(torch, n)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with capture(torch, g):
        ctx.filter_rays_async(dsegs.data_ptr(), n, dev.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (words(dev) == SENTINEL).all()   # captured, not run
    for segs, exp in ((ra, ea), (rb, eb)):
        dsegs.copy_(torch.from_numpy(segs))
        g.replay()
        torch.cuda.synchronize()
        assert filter_ref.differ(dev.cpu().numpy(), exp["filter"]) == []
    ctx.close()


# -------------------------------------------------------------- CLI, CScene
def test_cli_segments_hip(tmp_path, golden_filter):
    g = golden_filter
    src, dst = tmp_path / "segs.npy", tmp_path / "filters.npy"
    np.save(src, g["scene7_through_segs"])
    r = subprocess.run([EXE, scene(7), "--backend", "hip", "--segments", str(src), "--filters", str(dst)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert filter_ref.differ(np.load(dst), g["scene7_through_filter"]) == []
    assert K0 in r.stdout


def test_cscene_shadow_ray_verb(golden_filter):
    c = rt_amd.CScene()
    c.AjusterResolution(64, 48)
    c.TraiterFichierDeScene(scene(7))
    got = c.LancerListeDeRayonsOmbre(golden_filter["scene7_lights_segs"])
    assert filter_ref.differ(got, golden_filter["scene7_lights_filter"]) == []
