"""Closest-hit queries of arbitrary rays on the HIP path (include/rt.h
rt_trace_rays*, csrc/rt_rays.h rt_rays_kernel<BVH>).

Every expected hit comes from tests/rays_ref.py through liboracle.so at test
time or from the fixture tests/golden/rays.npz (the reference's own
Intersection() through oracle/_ref) — never from the code under test.
Comparison: id equal, t and n word for word as uint32; where the expectation
is NaN the result is NaN.  Which kernel ran is asserted by its name in
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
import cameras
import ray_sets
import rays_ref
import rt_amd
from conftest import GOLDEN, REPO, bits_equal, scene

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC12345  # a NaN pattern no query writes
KEYS = ("t", "id", "n")
EXE = os.path.join(REPO, "ray-tracing-gpu_amd", "lib", "rt_render")
K0, K1 = "rt_rays_kernel<0>", "rt_rays_kernel<1>"
RAYS_BUDGET = 128  # csrc/rt_rays.h RT_RAYS_BUDGET: the serial walk's steps before the wave finishes a ray
# the kernel each scene's query takes with the default options
KERNEL = {**{f"scene{i}": K0 for i in range(1, 10)}, "mixed63": K0, "mixed64": K1, "mixed65": K1, "soup1100": K1,
          "ties3": K0, "ties1026": K1, "hf1600": K0}
# ties1026: the BVH whatever its materials are, so that the file-order tie-break goes through the tree's reordering
OPTIONS = {"ties1026": {"ray_bvh": 1}}


@pytest.fixture(scope="module")
def golden_rays():
    return np.load(os.path.join(GOLDEN, "rays.npz"))


@pytest.fixture(scope="module")
def tmpdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("rays"))


@pytest.fixture(scope="module")
def contexts(oracle, tmpdir):
    """One context per scene for the whole module: name -> (context, its cases)."""
    made = {}

    def get(name):
        if name not in made:
            c = ray_sets.cases(oracle, name, tmpdir)
            ctx = rt_amd.Context(0, **OPTIONS.get(name, {}))
            ctx.upload(rt_amd.Scene(c["path"], ray_sets.W, ray_sets.H))
            made[name] = (ctx, c)
        return made[name]

    yield get
    for ctx, _ in made.values():
        ctx.close()


def want_of(g, name):
    return {k: g[f"{name}_{k}"] for k in ("id", "t", "n")}


def device_planes(torch, n):
    d = {"t": torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32),
         "id": torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda"),
         "n": torch.full((n, 3), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)}
    return d


def to_host(d, n=None):
    return {k: v.cpu().numpy()[:n] for k, v in d.items()}


def words(v):
    return np.ascontiguousarray(v.cpu().numpy()).view(np.uint32)


def has_bvh(ctx) -> bool:
    L = rt_amd.lib()
    L.rt_debug_bvh_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int]
    out = (ctypes.c_double * 5)()
    assert L.rt_debug_bvh_info(ctx._h, out, 5) == 0
    return out[0] == 1.0


def debug_bvh_rays(ctx, rays):
    """rt_debug_bvh_rays: (return code, [triangle tests, inner nodes visited])."""
    L = rt_amd.lib()
    L.rt_debug_bvh_rays.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] + [ctypes.c_void_p] * 3
    r = np.ascontiguousarray(rays, np.float32)
    idx, t = np.zeros((len(r), 2), np.int32), np.zeros((len(r), 2), np.float32)
    tally = np.zeros(2, np.uint64)
    rc = L.rt_debug_bvh_rays(ctx._h, r.ctypes.data, len(r), idx.ctypes.data, t.ctypes.data, tally.ctypes.data)
    return rc, tally


# ------------------------------------------------------------------ scenes
@pytest.mark.parametrize("name", list(KERNEL))
def test_every_set_matches_the_oracle(contexts, name):
    ctx, c = contexts(name)
    for label, (rays, exp) in c["sets"].items():
        got = ctx.trace_rays(rays)
        assert rays_ref.hits_differ(got, exp) == [], label
        st = ctx.stats()
        assert st.kernel == KERNEL[name], label
        assert st.bounce_rays == len(rays) and st.primary_rays == 0 and st.kernel_ms > 0
    assert has_bvh(ctx) == (KERNEL[name] == K1)


def test_soup_walks_go_over_the_budget_and_bvh_off_gives_the_same_bits(contexts, oracle, tmpdir):
    """soup1100: some walks take more steps than the serial walk's budget (the
    kernel finishes them itself); RT_OPT_BVH 0 tests every surface: same bits."""
    ctx, c = contexts("soup1100")
    base = c["sets"]["base"][0]
    # A ray's unbudgeted serial walk (rt_debug_bvh_rays, one ray per call) takes at least
    # its inner nodes + a quarter of its triangle tests (a leaf holds up to 4) steps;
    # the budgeted walk is that walk cut short, so such a ray straggles.
    most = 0
    for k in range(0, len(base), 2):
        rc, tally = debug_bvh_rays(ctx, base[k:k + 1])
        assert rc == 0
        most = max(most, int(tally[1]) + (int(tally[0]) + 3) // 4)
    print(f"soup1100: the longest walk of {len(base) // 2} base rays takes at least {most} steps")
    assert most > RAYS_BUDGET, most
    ctx.set_option("bvh", 0)
    try:
        for label, (rays, exp) in c["sets"].items():
            assert rays_ref.hits_differ(ctx.trace_rays(rays), exp) == [], label
            assert ctx.stats().kernel == K0
    finally:
        ctx.set_option("bvh", 1)


def test_ties_report_the_earlier_surface(contexts):
    """Coincident surfaces: only the first of each group in file order ever wins."""
    import hard_scenes

    for name, ntri in (("ties3", 3), ("ties1026", 1026)):
        ctx, c = contexts(name)
        text = hard_scenes.hard_dat("ties", 0, ntri)
        # exact duplicates (rtri's members are the same triangle with its vertices rotated: their t may differ)
        groups = hard_scenes.groups(text, prefixes=("dtri", "dpln", "dqd"))
        first = {g[0] for g in groups.values()}
        later = {i for g in groups.values() for i in g[1:]}
        ids = np.concatenate([ctx.trace_rays(r)["id"] for r, _ in c["sets"].values()])
        want = np.concatenate([e["id"] for _, e in c["sets"].values()])
        assert np.array_equal(ids, want)
        assert len(first) == 3 and first <= set(ids.tolist()) and not later & set(ids.tolist())


def test_heightfield_1600_ray_bvh_option(contexts, oracle, tmpdir):
    """A non-reflective mesh: no BVH and kernel <0> by default; with
    RT_OPT_RAY_BVH 1 the BVH and kernel <1>: the same bits.  No colour frame,
    AOV frame or wavefront decision changes with the option."""
    ctx0, c = contexts("hf1600")
    rays, exp = c["sets"]["base"]
    assert ctx0.get_option("ray_bvh") == 0 and not has_bvh(ctx0)
    assert debug_bvh_rays(ctx0, rays[:4])[0] == -4
    ctx1 = rt_amd.Context(0, ray_bvh=1)
    s0 = rt_amd.Scene(c["path"], 64, 32, 0)
    s3 = rt_amd.Scene(c["path"], 64, 32, 3)
    ctx1.upload(s0)
    assert has_bvh(ctx1) and debug_bvh_rays(ctx1, rays[:4])[0] == 0
    for label, (r, e) in c["sets"].items():
        got = ctx1.trace_rays(r)
        assert ctx1.stats().kernel == K1
        assert rays_ref.hits_differ(got, e) == [], label
        assert rays_ref.hits_differ(got, ctx0.trace_rays(r)) == [], label
        assert ctx0.stats().kernel == K0
    # frames: the same kernels and the same images under both option values
    f3 = s3.frame.copy()
    fneg = s3.frame.copy()
    fneg.min_energy = -1.0          # every depth reachable, whatever the materials are
    for f in (s0.frame, f3, fneg):
        a, ka = ctx0.render_float(f), ctx0.stats().kernel
        b, kb = ctx1.render_float(f), ctx1.stats().kernel
        assert ka == kb and "rt_rays" not in ka and bits_equal(a, b)
    a, ka = ctx0.render_aov(s0.frame), ctx0.stats().kernel
    b, kb = ctx1.render_aov(s0.frame), ctx1.stats().kernel
    assert ka == kb and aov_ref.planes_equal(a, b) == []
    ctx1.close()


def test_heightfield_50k_with_ray_bvh(golden_rays, heightfield_path):
    g = golden_rays
    ctx = rt_amd.Context(0, ray_bvh=1)
    ctx.upload(rt_amd.Scene(heightfield_path, 64, 32))
    got = ctx.trace_rays(g["hf50k_rays"])
    assert ctx.stats().kernel == K1
    assert rays_ref.hits_differ(got, want_of(g, "hf50k")) == []
    ctx.close()


# ------------------------------------------------------- counts and pointers
@pytest.mark.parametrize("name", ["scene3", "soup1100"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 4097])
def test_ray_counts_and_the_tail(contexts, name, n):
    """Device planes of n + 64 entries: nothing behind entry n is written."""
    torch = pytest.importorskip("torch")
    ctx, c = contexts(name)
    base, exp = c["sets"]["base"]
    pick = (np.arange(n) * 7 + n) % len(base)
    rays = np.ascontiguousarray(base[pick])
    dev = device_planes(torch, n + 64)
    drays = torch.from_numpy(rays).cuda()
    torch.cuda.synchronize()
    aov = rt_amd.Aov(dev["t"].data_ptr(), dev["id"].data_ptr(), dev["n"].data_ptr())
    assert rt_amd.lib().rt_trace_rays(ctx._h, drays.data_ptr(), n, ctypes.byref(aov)) == 0
    torch.cuda.synchronize()
    assert rays_ref.hits_differ(to_host(dev, n), {k: exp[k][pick] for k in KEYS}) == []
    for k in KEYS:
        assert (words(dev[k])[n:] == SENTINEL).all(), k
    assert ctx.stats().bounce_rays == n


@pytest.mark.parametrize("only", KEYS)
def test_single_plane_and_mixed_pointers(contexts, only):
    """One plane alone; host rays with a device plane, device rays with a host plane."""
    torch = pytest.importorskip("torch")
    ctx, c = contexts("mixed65")
    rays, exp = c["sets"]["base"]
    n = len(rays)
    got = ctx.trace_rays(rays, **{k: k == only for k in KEYS})
    assert list(got) == [only] and rays_ref.hits_differ(got, exp, keys=(only,)) == []
    L = rt_amd.lib()
    dev = device_planes(torch, n)
    torch.cuda.synchronize()
    aov = rt_amd.Aov(*(dev[k].data_ptr() if k == only else None for k in KEYS))
    assert L.rt_trace_rays(ctx._h, rays.ctypes.data, n, ctypes.byref(aov)) == 0          # host rays, device plane
    torch.cuda.synchronize()
    assert rays_ref.hits_differ(to_host(dev), exp, keys=(only,)) == []
    for k in KEYS:
        if k != only:
            assert (words(dev[k]) == SENTINEL).all(), k
    host = {"t": np.zeros(n, np.float32), "id": np.zeros(n, np.int32), "n": np.zeros((n, 3), np.float32)}
    drays = torch.from_numpy(rays).cuda()
    torch.cuda.synchronize()
    aov = rt_amd.Aov(*(host[k].ctypes.data if k == only else None for k in KEYS))
    assert L.rt_trace_rays(ctx._h, drays.data_ptr(), n, ctypes.byref(aov)) == 0          # device rays, host plane
    assert rays_ref.hits_differ(host, exp, keys=(only,)) == []
    # every plane, each on the other side from the rays
    dev = device_planes(torch, n)
    torch.cuda.synchronize()
    aov = rt_amd.Aov(dev["t"].data_ptr(), host["id"].ctypes.data, dev["n"].data_ptr())
    assert L.rt_trace_rays(ctx._h, rays.ctypes.data, n, ctypes.byref(aov)) == 0
    torch.cuda.synchronize()
    mixed = {"t": dev["t"].cpu().numpy(), "id": host["id"], "n": dev["n"].cpu().numpy()}
    assert rays_ref.hits_differ(mixed, exp) == []


def test_argument_and_state_errors(contexts):
    torch = pytest.importorskip("torch")
    L = rt_amd.lib()
    ctx, c = contexts("scene3")
    rays = c["sets"]["base"][0]
    t = np.full(len(rays), SENTINEL, np.uint32)
    some = rt_amd.Aov(t.ctypes.data, None, None)
    none = rt_amd.Aov(None, None, None)
    assert L.rt_trace_rays(ctx._h, rays.ctypes.data, 8, ctypes.byref(none)) == -1
    assert L.rt_trace_rays(ctx._h, None, 8, ctypes.byref(some)) == -1
    assert L.rt_trace_rays(ctx._h, rays.ctypes.data, -1, ctypes.byref(some)) == -1
    assert L.rt_trace_rays(ctx._h, rays.ctypes.data, 2**31, ctypes.byref(some)) == -1
    assert L.rt_trace_rays(ctx._h, rays.ctypes.data, 0, ctypes.byref(some)) == 0 and (t == SENTINEL).all()
    assert L.rt_cpu_trace_rays(ctx._h, rays.ctypes.data, 8, ctypes.byref(some)) == -4      # the other backend's call
    # async: device pointers only, 8-byte aligned
    drays = torch.from_numpy(np.concatenate([rays.ravel(), np.zeros(2, np.float32)])).cuda()
    dev = device_planes(torch, len(rays) + 2)
    torch.cuda.synchronize()
    ok = rt_amd.Aov(dev["t"].data_ptr(), dev["id"].data_ptr(), dev["n"].data_ptr())
    assert L.rt_trace_rays_async(ctx._h, rays.ctypes.data, 8, ctypes.byref(ok), None) == -1            # host rays
    assert L.rt_trace_rays_async(ctx._h, drays.data_ptr(), 8, ctypes.byref(some), None) == -1          # host plane
    assert L.rt_trace_rays_async(ctx._h, drays.data_ptr() + 4, 8, ctypes.byref(ok), None) == -1        # misaligned rays
    off = rt_amd.Aov(dev["t"].data_ptr() + 4, None, None)
    assert L.rt_trace_rays_async(ctx._h, drays.data_ptr(), 8, ctypes.byref(off), None) == -1           # misaligned plane
    assert L.rt_trace_rays(ctx._h, drays.data_ptr() + 4, 8, ctypes.byref(ok)) == -1
    assert L.rt_trace_rays_async(ctx._h, drays.data_ptr(), 0, ctypes.byref(ok), None) == 0
    ctx.sync()
    torch.cuda.synchronize()
    for k in KEYS:
        assert (words(dev[k]) == SENTINEL).all(), k        # none of the refused calls wrote anything
    fresh = rt_amd.Context(0)
    assert L.rt_trace_rays(fresh._h, rays.ctypes.data, 8, ctypes.byref(some)) == -4                    # before an upload
    assert L.rt_trace_rays_async(fresh._h, drays.data_ptr(), 8, ctypes.byref(ok), None) == -4
    fresh.close()


# ------------------------------------------------- the AOV feature's frames
@pytest.mark.parametrize("which", ["scene2", "hf1600", "hf1600_moved"])
def test_camera_rays_equal_the_aov_frame(contexts, which):
    """trace_rays of a 64 x 32 frame's camera rays = render_aov of that frame."""
    name = which.split("_")[0]
    ctx, c = contexts(name)
    f = rt_amd.Scene(c["path"], 64, 32).frame.copy()
    if which.endswith("_moved"):
        f = cameras.cameras(f)[2]
    ys, xs = np.meshgrid(np.arange(32), np.arange(64), indexing="ij")
    cam = aov_ref.Cam.from_frame(f)
    D = aov_ref.camera_dirs(cam, xs.ravel(), ys.ravel())
    rays = np.ascontiguousarray(np.concatenate([np.tile(cam.pos, (len(D), 1)), D], 1), np.float32)
    got = ctx.trace_rays(rays)
    aov = ctx.render_aov(f)
    assert (aov["id"] >= 0).any()
    flat = {"t": aov["t"].reshape(-1), "id": aov["id"].reshape(-1), "n": aov["n"].reshape(-1, 3)}
    assert rays_ref.hits_differ(got, flat) == []


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
    ctx, c = contexts("soup1100")
    (ra, ea), (rb, eb) = c["sets"]["base"], c["sets"]["axis"]
    da, db = torch.from_numpy(ra).cuda(), torch.from_numpy(rb).cuda()
    pa, pb = device_planes(torch, len(ra)), device_planes(torch, len(rb))
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx.trace_rays_async(da.data_ptr(), len(ra), pa["t"].data_ptr(), pa["id"].data_ptr(), pa["n"].data_ptr(), sa.cuda_stream)
    ctx.trace_rays_async(db.data_ptr(), len(rb), pb["t"].data_ptr(), pb["id"].data_ptr(), pb["n"].data_ptr(), sb.cuda_stream)
    ctx.trace_rays_async(db.data_ptr(), len(rb), 0, pa["id"].data_ptr(), 0, sa.cuda_stream)   # behind the first, on its stream
    ctx.sync()
    torch.cuda.synchronize()
    assert rays_ref.hits_differ(to_host(pb), eb) == []
    assert rays_ref.hits_differ(to_host(pa), ea, keys=("t", "n")) == []
    assert np.array_equal(pa["id"].cpu().numpy(), eb["id"])


@pytest.mark.parametrize("name", ["scene3", "mixed65"])
def test_graph_capture_on_a_context_that_never_rendered(oracle, tmpdir, name):
    """Captured on a fresh context, replayed twice with the device ray buffer
    rewritten in between: the outputs follow the buffer."""
    torch = pytest.importorskip("torch")
    c = ray_sets.cases(oracle, name, tmpdir)
    ctx = rt_amd.Context(0)
    ctx.upload(rt_amd.Scene(c["path"], 64, 32))
    (ra, ea), (rb, eb) = c["sets"]["base"], c["sets"]["axis"]
    n = len(ra)
    assert len(rb) == n
    drays = torch.from_numpy(ra).cuda()
    dev = device_planes(torch, n)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with capture(torch, g):
        ctx.trace_rays_async(drays.data_ptr(), n, dev["t"].data_ptr(), dev["id"].data_ptr(), dev["n"].data_ptr(),
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for k in KEYS:
        assert (words(dev[k]) == SENTINEL).all()   # captured, not run
    for rays, exp in ((ra, ea), (rb, eb)):
        drays.copy_(torch.from_numpy(rays))
        g.replay()
        torch.cuda.synchronize()
        assert rays_ref.hits_differ(to_host(dev), exp) == []
    ctx.close()


# -------------------------------------------------------------- CLI, CScene
@pytest.mark.parametrize("backend", ["hip", "cpu"])
def test_cli_rays(tmp_path, golden_rays, backend):
    src, prefix = tmp_path / "in.npy", tmp_path / "h"
    np.save(src, golden_rays["scene7_rays"])
    r = subprocess.run([EXE, scene(7), "--backend", backend, "--rays", str(src), "--hits", str(prefix)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = {k: np.load(f"{prefix}_{k}.npy") for k in KEYS}
    assert rays_ref.hits_differ(got, want_of(golden_rays, "scene7")) == []
    assert ("rt_rays_kernel<0>" if backend == "hip" else "cpu_trace_rays") in r.stdout


def test_cscene_ray_verb(golden_rays):
    c = rt_amd.CScene()
    c.AjusterResolution(64, 48)
    c.TraiterFichierDeScene(scene(7))
    assert rays_ref.hits_differ(c.LancerListeDeRayons(golden_rays["scene7_rays"]), want_of(golden_rays, "scene7")) == []
