"""Primary-hit AOV renders on the HIP path (include/rt.h rt_render_aov*,
csrc/rt_aov.h rt_aov_kernel<WAVE>).

Every expected plane comes from the fixture tests/golden/aov.npz (the
reference's own Intersection() through oracle/_ref) or from tests/aov_ref.py
through liboracle.so at test time — never from the code under test — and
every comparison is bit for bit, quadric normals included.  Which kernel
variant ran is asserted by its name in rt_stats (or by rt_debug_cb_info)."""
from __future__ import annotations

import contextlib
import ctypes
import gc
import os

import numpy as np
import pytest

import aov_ref
import cameras
import rt_amd
from conftest import GOLDEN, CamRef, bits_equal, scene

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC12345  # a NaN pattern no render writes
KEYS = ("t", "id", "n")


@pytest.fixture(scope="module")
def golden_aov():
    return np.load(os.path.join(GOLDEN, "aov.npz"))


@pytest.fixture(scope="module")
def hf1280_path(tmp_path_factory):
    from rt_amd import synth

    return synth.write_heightfield(str(tmp_path_factory.mktemp("hf1280") / "heightfield_40x16.dat"), cols=40, rows=16)


@pytest.fixture(scope="module")
def hf96_path(tmp_path_factory):
    """96 triangles: past the launch-camera scenes (20), under the clustering threshold."""
    from rt_amd import synth

    return synth.write_heightfield(str(tmp_path_factory.mktemp("hf96") / "heightfield_8x6.dat"), cols=8, rows=6)


def want_of(g, name):
    return {k: g[f"{name}_{k}"] for k in ("id", "t", "n")}


def uploaded(path, w, h, depth=0, **options):
    s = rt_amd.Scene(path, w, h, depth)
    ctx = rt_amd.Context(0, **options)
    ctx.upload(s)
    return ctx, s.frame.copy()


def device_planes(torch, rows, w):
    """Sentinel-filled device planes and the pointers of an rt_aov."""
    i32 = SENTINEL  # (positive as an int32)
    d = {"t": torch.full((rows, w), i32, dtype=torch.int32, device="cuda").view(torch.float32),
         "id": torch.full((rows, w), i32, dtype=torch.int32, device="cuda"),
         "n": torch.full((rows, w, 3), i32, dtype=torch.int32, device="cuda").view(torch.float32)}
    return d


def to_host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def kernel_of(ctx):
    return ctx.stats().kernel


# ------------------------------------------------------------------ scenes
@pytest.mark.parametrize("i", range(1, 10))
def test_scenes_match_the_reference_fixture(golden_aov, i):
    """A scene whose colour frame renders with launch-camera records (scene2
    for one) and a scene without triangles (scenes 4-9) start on WAVE 0."""
    s = rt_amd.Scene(scene(i), 64, 48, 0)
    n_tri = int((s.arrays()[0] == rt_amd.TRIANGLE).sum())
    ctx, f = uploaded(scene(i), 64, 48)
    got = ctx.render_aov(f)
    assert aov_ref.planes_equal(got, want_of(golden_aov, f"scene{i}")) == []
    st = ctx.stats()
    assert st.primary_rays == 64 * 48 and st.kernel_ms > 0
    assert (st.bounce_rays, st.shadow_rays, st.triangle_tests, st.plane_tests, st.quadric_tests) == (0, 0, 0, 0, 0)
    ctx.render_float(f)
    tiny = kernel_of(ctx).startswith("rt_trace_tiny")
    assert tiny or i != 2
    assert st.kernel == ("rt_aov_kernel<0>" if tiny or n_tri == 0 else "rt_aov_kernel<9>")
    # behind the colour frame: the same planes, the same variant
    assert aov_ref.planes_equal(ctx.render_aov(f), want_of(golden_aov, f"scene{i}")) == []
    assert kernel_of(ctx) == st.kernel
    ctx.close()


@pytest.mark.parametrize("i", [1, 2, 3])
@pytest.mark.parametrize("cb", [1, 0])
def test_small_lists_with_device_camera_records(golden_aov, i, cb):
    """RT_OPT_LAUNCH_CAMERA 0: the wave-culling variants, with and without the camera buffer."""
    ctx, f = uploaded(scene(i), 64, 48, launch_camera=0, camera_buffer=cb)
    assert aov_ref.planes_equal(ctx.render_aov(f), want_of(golden_aov, f"scene{i}")) == []
    assert kernel_of(ctx) == ("rt_aov_kernel<9>" if cb else "rt_aov_kernel<1>")
    ctx.close()


@pytest.mark.parametrize("cb", [1, 0])
def test_96_triangles_wave_culling(oracle, hf96_path, cb):
    """A scene past the launch-camera limit: WAVE 9 / 1 by default; 61 x 43 (edge waves)."""
    ctx, f = uploaded(hf96_path, 61, 43, camera_buffer=cb)
    got = ctx.render_aov(f)
    assert kernel_of(ctx) == ("rt_aov_kernel<9>" if cb else "rt_aov_kernel<1>")
    surf, cam, _ = oracle.dump(hf96_path, 61, 43)
    ys, xs = np.meshgrid(np.arange(0, 43, 2), np.arange(0, 61, 2), indexing="ij")
    xs, ys = np.append(xs.ravel(), [60, 60, 0]), np.append(ys.ravel(), [42, 0, 42])
    ids, ts, ns, _ = aov_ref.aov_pixels(oracle.L.oracle_intersect, surf, aov_ref.Cam.from_words(cam), xs, ys)
    picked = {k: np.ascontiguousarray(got[k][ys, xs]) for k in got}
    assert aov_ref.planes_equal(picked, {"id": ids, "t": ts, "n": ns}) == []
    assert (ids > 0).any() and (ids == 0).any()
    ctx.close()


@pytest.mark.parametrize("i,options", [(2, {}), (2, {"launch_camera": 0}), (4, {}), (7, {})])
def test_edge_waves(oracle, i, options):
    """61 x 43: the last tile column and row are partial (clamped lanes dropped)."""
    ctx, f = uploaded(scene(i), 61, 43, **options)
    got = ctx.render_aov(f)
    assert got["id"].shape == (43, 61)
    assert aov_ref.planes_equal(got, aov_ref.oracle_aov(oracle, scene(i), 61, 43)) == []
    ctx.close()


# ------------------------------------------------------- slabs, bands, pointers
def render_both(ctx, f, rows, w):
    """The synchronous call into device planes and into host planes."""
    torch = pytest.importorskip("torch")
    L = rt_amd.lib()
    dev = device_planes(torch, rows, w)
    aov = rt_amd.Aov(dev["t"].data_ptr(), dev["id"].data_ptr(), dev["n"].data_ptr())
    assert L.rt_render_aov(ctx._h, ctypes.byref(f), ctypes.byref(aov)) == 0, ctx._err()
    torch.cuda.synchronize()
    host = {"t": np.full((rows, w), SENTINEL, np.uint32).view(np.float32),
            "id": np.full((rows, w), SENTINEL, np.uint32).view(np.int32),
            "n": np.full((rows, w, 3), SENTINEL, np.uint32).view(np.float32)}
    aov = rt_amd.Aov(host["t"].ctypes.data, host["id"].ctypes.data, host["n"].ctypes.data)
    assert L.rt_render_aov(ctx._h, ctypes.byref(f), ctypes.byref(aov)) == 0, ctx._err()
    return to_host(dev), host


@pytest.mark.parametrize("options", [{}, {"launch_camera": 0}])
def test_slab_rows(golden_aov, options):
    ctx, f = uploaded(scene(3), 64, 48, **options)
    f.row_begin, f.row_end = 16, 40
    dev, host = render_both(ctx, f, 24, 64)
    want = {k: v[16:40] for k, v in want_of(golden_aov, "scene3").items()}
    assert aov_ref.planes_equal(dev, want) == [] and aov_ref.planes_equal(host, want) == []
    assert ctx.stats().primary_rays == 24 * 64
    ctx.close()


@pytest.mark.parametrize("options", [{}, {"launch_camera": 0}])
@pytest.mark.parametrize("height,valid", [(80, 32), (72, 24)])
def test_band_set_and_rows_past_the_frame(oracle, options, height, valid):
    """band_rows 16, count 3, index 1: bands 1 and 4 = frame rows 16..32 and
    64..80, into sentinel-filled planes of 40 rows.  At 64 x 80 the set fills
    its 32 packed rows; at 64 x 72 rows 72..80 lie past the frame and the last
    8 packed rows keep the sentinel — in device and in host memory."""
    ctx, f = uploaded(scene(3), 64, height, **options)
    f.band_rows, f.band_count, f.band_index = 16, 3, 1
    assert rt_amd.frame_rows(f) == 32
    dev, host = render_both(ctx, f, 40, 64)
    rows = list(range(16, 32)) + list(range(64, min(80, height)))
    want = aov_ref.oracle_aov(oracle, scene(3), 64, height, rows=rows)
    for got in (dev, host):
        assert aov_ref.planes_equal({k: got[k][:valid] for k in got}, want) == []
        for k in got:
            assert (np.ascontiguousarray(got[k][valid:]).view(np.uint32) == SENTINEL).all(), (height, k)
    assert aov_ref.planes_equal(dev, host) == []
    assert ctx.stats().primary_rays == valid * 64
    ctx.close()


@pytest.mark.parametrize("only", KEYS)
def test_single_plane_and_mixed_pointers(golden_aov, only):
    """One plane alone; and one plane in device memory with the others in host memory."""
    torch = pytest.importorskip("torch")
    L = rt_amd.lib()
    ctx, f = uploaded(scene(8), 64, 48)
    want = want_of(golden_aov, "scene8")
    got = ctx.render_aov(f, **{k: k == only for k in KEYS})
    assert list(got) == [only] and aov_ref.planes_equal(got, want, keys=(only,)) == []
    dev = device_planes(torch, 48, 64)
    host = {"t": np.zeros((48, 64), np.float32), "id": np.zeros((48, 64), np.int32), "n": np.zeros((48, 64, 3), np.float32)}
    ptr = {k: (dev[k].data_ptr() if k == only else host[k].ctypes.data) for k in KEYS}
    aov = rt_amd.Aov(ptr["t"], ptr["id"], ptr["n"])
    assert L.rt_render_aov(ctx._h, ctypes.byref(f), ctypes.byref(aov)) == 0, ctx._err()
    torch.cuda.synchronize()
    mixed = {k: (dev[k].cpu().numpy() if k == only else host[k]) for k in KEYS}
    assert aov_ref.planes_equal(mixed, want) == []
    ctx.close()


def test_argument_and_state_errors():
    L = rt_amd.lib()
    s = rt_amd.Scene(scene(1), 64, 48, 0)
    ctx = rt_amd.Context(0)
    f = s.frame.copy()
    t = np.full((48, 64), 7, np.float32)
    some = rt_amd.Aov(t.ctypes.data, None, None)
    assert L.rt_render_aov(ctx._h, ctypes.byref(f), ctypes.byref(some)) == -4          # before upload
    assert L.rt_render_aov_async(ctx._h, ctypes.byref(f), ctypes.byref(some), None) == -4
    ctx.upload(s)
    none = rt_amd.Aov(None, None, None)
    assert L.rt_render_aov(ctx._h, ctypes.byref(f), ctypes.byref(none)) == -1
    assert L.rt_render_aov_async(ctx._h, ctypes.byref(f), ctypes.byref(none), None) == -1
    g = f.copy()
    g.flags = rt_amd.FLAG_STATS
    assert L.rt_render_aov(ctx._h, ctypes.byref(g), ctypes.byref(some)) == -1
    g = f.copy()
    g.row_end = 49
    assert L.rt_render_aov(ctx._h, ctypes.byref(g), ctypes.byref(some)) == -1
    g = f.copy()
    g.band_rows, g.band_count, g.band_index = 8, 2, 0
    assert L.rt_render_aov(ctx._h, ctypes.byref(g), ctypes.byref(some)) == -1
    assert (t == 7).all()
    assert L.rt_cpu_render_aov(ctx._h, ctypes.byref(f), ctypes.byref(some)) == -4       # the CPU backend's call
    assert L.rt_render_aov(ctx._h, ctypes.byref(f), ctypes.byref(some)) == 0
    ctx.close()


# ------------------------------------------------------------ big lists
def cb_info(ctx, n=10):
    L = rt_amd.lib()
    L.rt_debug_cb_info.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    info = (ctypes.c_double * n)()
    assert L.rt_debug_cb_info(ctx._h, info, n) == 0
    return list(info)


def cb_listed(ctx):
    L = rt_amd.lib()
    L.rt_debug_cb_verify.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    out = (ctypes.c_ulonglong * 3)()
    assert L.rt_debug_cb_verify(ctx._h, out) == 0, ctx._err()
    return list(out)


def test_heightfield_1280_clustered_with_camera_buffer(golden_aov, hf1280_path):
    ctx, f = uploaded(hf1280_path, 64, 32)
    assert aov_ref.planes_equal(ctx.render_aov(f), want_of(golden_aov, "hf1280")) == []
    assert kernel_of(ctx) == "rt_aov_kernel<10>"
    info = cb_info(ctx)
    assert info[0] == 1.0 and info[3] == 8 * 4
    bad, pairs, listed = cb_listed(ctx)
    assert bad == 0 and listed == 8 * 4          # every tile walked its list
    ctx.close()


def test_heightfield_1280_without_camera_buffer(golden_aov, hf1280_path):
    ctx, f = uploaded(hf1280_path, 64, 32, camera_buffer=0)
    assert aov_ref.planes_equal(ctx.render_aov(f), want_of(golden_aov, "hf1280")) == []
    assert kernel_of(ctx) == "rt_aov_kernel<2>"
    assert cb_info(ctx)[0] == 0.0
    ctx.close()


@pytest.mark.parametrize("cap", [1, 400])
def test_heightfield_1280_tiles_fall_back_per_wave(golden_aov, hf1280_path, cap):
    """RT_OPT_CB_CAPACITY too small for every list: the tiles that do not fit
    render by the per-wave path inside the camera-buffer kernel."""
    ctx, f = uploaded(hf1280_path, 64, 32, cb_capacity=cap)
    assert aov_ref.planes_equal(ctx.render_aov(f), want_of(golden_aov, "hf1280")) == []
    assert kernel_of(ctx) == "rt_aov_kernel<10>"
    # (first: a build that did not fit is marked for a rebuild once rt_debug_cb_info reads its totals back)
    bad, pairs, listed = cb_listed(ctx)
    assert bad == 0 and listed < 8 * 4
    info = cb_info(ctx)
    assert info[9] == cap and info[1] > cap
    ctx.close()


@pytest.mark.parametrize("deal", [0, 2, 3])
def test_heightfield_1280_tile_dealing_modes(golden_aov, hf1280_path, deal):
    """RT_OPT_XCD_DEAL's padded grids (tile_of_block) give the same planes."""
    ctx, f = uploaded(hf1280_path, 64, 32, xcd_deal=deal)
    assert aov_ref.planes_equal(ctx.render_aov(f), want_of(golden_aov, "hf1280")) == []
    assert kernel_of(ctx) == "rt_aov_kernel<10>"
    ctx.close()


def sparse_check(ctx, f, g, name):
    xs, ys = aov_ref.sparse_pixels(int(g[f"{name}_seed"]))
    assert np.array_equal(xs, g[f"{name}_x"]) and np.array_equal(ys, g[f"{name}_y"])
    got = ctx.render_aov(f)
    picked = {k: np.ascontiguousarray(got[k][ys, xs]) for k in got}
    assert aov_ref.planes_equal(picked, want_of(g, name)) == []
    return got


@pytest.mark.parametrize("cb", [1, 0])
def test_heightfield_50k_sparse_pixels(golden_aov, heightfield_path, cb):
    g = golden_aov
    ctx, f = uploaded(heightfield_path, 64, 32, camera_buffer=cb)
    got = sparse_check(ctx, f, g, "hf50k")
    assert kernel_of(ctx) == ("rt_aov_kernel<10>" if cb else "rt_aov_kernel<2>")
    assert not (got["id"] < 0).any()             # the ground plane fills this frame (hf50k_lacks)
    # the pitched and yawed camera of the fixture: sky in the frame
    f2 = cameras.cameras(f)[2]
    assert np.array_equal(np.asarray(cameras.words(f2), np.float32).view(np.uint32),
                          np.asarray(g["hf50kcam2_words"], np.float32).view(np.uint32))
    got = sparse_check(ctx, f2, g, "hf50kcam2")
    assert (got["id"] < 0).any() and (got["id"] > 0).any()
    ctx.close()


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


@pytest.mark.parametrize("which", ["scene3", "hf1280"])
def test_async_on_a_stream_equals_the_synchronous_call(golden_aov, hf1280_path, which):
    torch = pytest.importorskip("torch")
    path, w, h = (scene(3), 64, 48) if which == "scene3" else (hf1280_path, 64, 32)
    ctx, f = uploaded(path, w, h)
    sync = ctx.render_aov(f)
    assert aov_ref.planes_equal(sync, want_of(golden_aov, which)) == []
    st = torch.cuda.Stream()
    dev = device_planes(torch, h, w)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        ctx.render_aov_async(f, dev["t"].data_ptr(), dev["id"].data_ptr(), dev["n"].data_ptr(), st.cuda_stream)
        # a moved camera behind it on the same stream, then the first again: no host sync between
        f2 = cameras.cameras(f)[1]
        dev2 = device_planes(torch, h, w)
        ctx.render_aov_async(f2, dev2["t"].data_ptr(), dev2["id"].data_ptr(), dev2["n"].data_ptr(), st.cuda_stream)
        dev3 = device_planes(torch, h, w)
        ctx.render_aov_async(f, 0, dev3["id"].data_ptr(), 0, st.cuda_stream)
    ctx.sync()
    torch.cuda.synchronize()
    assert aov_ref.planes_equal(to_host(dev), sync) == []
    assert aov_ref.planes_equal(to_host(dev3), sync, keys=("id",)) == []
    assert (dev3["t"].view(torch.int32).cpu().numpy().view(np.uint32) == SENTINEL).all()
    assert aov_ref.planes_equal(to_host(dev2), ctx.render_aov(f2)) == []
    ctx.close()


@pytest.mark.parametrize("which", ["scene3", "hf1280"])
def test_graph_capture_and_replay(golden_aov, hf1280_path, which):
    """Captured after rt_prepare_camera, replayed twice: the same bits."""
    torch = pytest.importorskip("torch")
    path, w, h = (scene(3), 64, 48) if which == "scene3" else (hf1280_path, 64, 32)
    ctx, f = uploaded(path, w, h)
    ctx.prepare_camera(f)
    dev = device_planes(torch, h, w)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with capture(torch, g):
        ctx.render_aov_async(f, dev["t"].data_ptr(), dev["id"].data_ptr(), dev["n"].data_ptr(),
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for k in dev:
        assert (dev[k].view(torch.int32).cpu().numpy().view(np.uint32) == SENTINEL).all()   # captured, not run
    for _ in range(2):
        for k in dev:
            dev[k].view(torch.int32).fill_(0)
        g.replay()
        torch.cuda.synchronize()
        assert aov_ref.planes_equal(to_host(dev), want_of(golden_aov, which)) == []
    ctx.close()


# the refused capture leaves its graph empty, which torch warns about
@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_capture_with_an_unprepared_camera_is_refused(golden_aov, hf1280_path):
    torch = pytest.importorskip("torch")
    ctx, f = uploaded(hf1280_path, 64, 32)
    dev = device_planes(torch, 32, 64)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with capture(torch, g):
        with pytest.raises(rt_amd.RtError) as e:
            ctx.render_aov_async(f, dev["t"].data_ptr(), dev["id"].data_ptr(), dev["n"].data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
    assert e.value.code == -4
    ctx.sync()
    torch.cuda.synchronize()
    for k in dev:                                # nothing was enqueued
        assert (dev[k].view(torch.int32).cpu().numpy().view(np.uint32) == SENTINEL).all()
    # the context still renders
    assert aov_ref.planes_equal(ctx.render_aov(f), want_of(golden_aov, "hf1280")) == []
    ctx.close()


# ----------------------------------------------------------- state hazard
def strided_check(oracle, path, w, h, f, got, step=9):
    """got's planes on a pixel grid (and the frame's corners) against aov_ref for frame f."""
    surf, _, _ = oracle.dump(path, w, h)
    ys, xs = np.meshgrid(np.arange(0, h, step), np.arange(0, w, step), indexing="ij")
    xs, ys = np.append(xs.ravel(), [w - 1, w - 1, 0]), np.append(ys.ravel(), [h - 1, 0, h - 1])
    ids, ts, ns, _ = aov_ref.aov_pixels(oracle.L.oracle_intersect, surf, aov_ref.Cam.from_frame(f), xs, ys)
    picked = {k: np.ascontiguousarray(got[k][ys, xs]) for k in got}
    assert aov_ref.planes_equal(picked, {"id": ids, "t": ts, "n": ns}) == []


@pytest.mark.parametrize("lc", [1, 0])
def test_state_hazard_scene2(oracle, heightfield_path, lc):
    """AOV of A, colour of B, AOV of B, colour of A on one context: with the
    launch-camera records (the AOV pass builds no camera state behind the
    tiny-scene kernel) and with the device camera records (shared state)."""
    r = CamRef("scene2", heightfield_path)
    A, B = r.frames["cams"][1], r.frames["cams"][2]
    ctx = rt_amd.Context(0, launch_camera=lc)
    ctx.upload(r.scene)
    aov_a = ctx.render_aov(A)
    assert kernel_of(ctx) == ("rt_aov_kernel<0>" if lc else "rt_aov_kernel<9>")
    col_b = ctx.render_float(B)
    assert kernel_of(ctx).startswith("rt_trace_tiny" if lc else "rt_trace_kernel<0,")
    aov_b = ctx.render_aov(B)
    col_a = ctx.render_float(A)
    assert r.matches(col_b, "cams", 2) and r.matches(col_a, "cams", 1)
    strided_check(oracle, r.path, r.w, r.h, A, aov_a)
    strided_check(oracle, r.path, r.w, r.h, B, aov_b)
    ctx.close()


def oracle_colour(oracle, path, w, h, f):
    """liboracle's depth-0 frame under the explicit camera of rt_frame f."""
    L = oracle.L
    L.oracle_set_camera.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_float] * 4 + \
                                   [ctypes.c_int, ctypes.c_int]
    rc, p = oracle.load(path, w, h, 0)
    assert rc == 0
    pos, orient = np.array(f.cam_pos[:], np.float32), np.array(f.orient[:], np.float32)
    assert L.oracle_set_camera(p, pos.ctypes.data, orient.ctypes.data, f.half_w, f.half_h, f.inv_w, f.inv_h, w, h) == 0
    out = np.zeros((h, w, 3), np.float32)
    L.oracle_render_window(p, 0, h, 0, w, out.ctypes.data, 4)
    L.oracle_free(p)
    return out


def test_state_hazard_heightfield_1280(oracle, hf1280_path):
    """The same order on the clustered kernels, which share the device camera
    records and the camera buffer with the colour frames: cameras()[1] and
    [2] of tests/cameras.py at 64 x 32."""
    ctx, f = uploaded(hf1280_path, 64, 32)
    A, B = cameras.cameras(f)[1], cameras.cameras(f)[2]
    aov_a = ctx.render_aov(A)
    assert kernel_of(ctx) == "rt_aov_kernel<10>"
    col_b = ctx.render_float(B)
    assert kernel_of(ctx).startswith("rt_trace_kernel<0,1,")
    aov_b = ctx.render_aov(B)
    col_a = ctx.render_float(A)
    assert bits_equal(col_b, oracle_colour(oracle, hf1280_path, 64, 32, B))
    assert bits_equal(col_a, oracle_colour(oracle, hf1280_path, 64, 32, A))
    strided_check(oracle, hf1280_path, 64, 32, A, aov_a, step=5)
    strided_check(oracle, hf1280_path, 64, 32, B, aov_b, step=5)
    assert (aov_b["id"] < 0).any() and (aov_b["id"] > 0).any()     # B sees sky and mesh
    ctx.close()


# ------------------------------------------------------------ consistency
@pytest.mark.parametrize("i", [4, 3])
def test_misses_are_exactly_the_background_pixels(i):
    """id < 0 exactly where the depth-0 colour frame shows a background no shading produces."""
    ctx, f = uploaded(scene(i), 64, 48)
    f.background[0], f.background[1], f.background[2] = 0.123456, 7.5, -3.25
    col = ctx.render_float(f)
    bg = np.array(f.background[:], np.float32)
    is_bg = (col.view(np.uint32) == bg.view(np.uint32)).all(-1)
    ids = ctx.render_aov(f)["id"]
    assert is_bg.any() and not is_bg.all()
    assert np.array_equal(ids < 0, is_bg)
    ctx.close()


def test_supersampled_frame_is_the_sample_grid(golden_aov):
    """An AOV render of the sample frame is the AOVs of the sample grid."""
    c = rt_amd.CScene()
    c.AjusterResolution(32, 24)
    c.TraiterFichierDeScene(scene(7))
    c.AjusterSurEchantillonnage(2)
    assert aov_ref.planes_equal(c.LancerRayonsAOV(), want_of(golden_aov, "scene7")) == []


def test_cli_aov(tmp_path, golden_aov):
    import subprocess

    from conftest import REPO

    exe = os.path.join(REPO, "ray-tracing-gpu_amd", "lib", "rt_render")
    prefix = tmp_path / "s4"
    out = tmp_path / "s4.ppm"
    r = subprocess.run([exe, scene(4), "-x", "64", "-y", "48", "--aov", str(prefix), "-o", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert out.exists()
    got = {k: np.load(f"{prefix}_{k}.npy") for k in KEYS}
    assert aov_ref.planes_equal(got, want_of(golden_aov, "scene4")) == []
