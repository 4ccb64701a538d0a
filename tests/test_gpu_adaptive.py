"""Adaptive supersampling on the HIP path (include/rt.h rt_render_adaptive*,
csrc/rt_adaptive.h): the base frame and its AOV pass through the plain
kernels, rt_edge_classify_kernel, the scan, and rt_refine_kernel on the list
of flagged pixels.  Expected images: adaptive_ref.compose of the reference's
frame of the sample grid (tests/golden/images.npz) or the oracle's, under the
mask adaptive_ref.mask computes from reference data — bit for bit, except
scene4 (Phong: ocml powf against glibc powf, as in test_gpu_parity.py), whose
mask is taken from the same context's plain frame, whose colours must be
within PHONG_ULP and whose RGBA8 within 1 LSB."""
from __future__ import annotations

import contextlib
import ctypes
import gc
import math
import os
import subprocess

import numpy as np
import pytest

import adaptive_ref as ar
import rt_amd
from conftest import REPO, bits_equal, rgba8, scene, ulp_diff
from rt_amd import synth
from test_gpu_parity import PHONG_ULP

pytestmark = pytest.mark.gpu

PHONG_SCENES = {4}
ALL = ar.ALL
EXE = os.path.join(REPO, "ray-tracing-gpu_amd", "lib", "rt_render")


@pytest.fixture(scope="module")
def ctx():
    return rt_amd.Context(0)


@pytest.fixture(scope="module")
def hf_paths(tmp_path_factory):
    """The 40 x 20 heightfield (1600 triangles), plain and with reflect = 0.5."""
    d = tmp_path_factory.mktemp("adaptive_hf")
    return {"hf1600": synth.write_heightfield(str(d / "hf1600.dat"), 40, 20),
            "hf1600r": synth.write_heightfield(str(d / "hf1600r.dat"), 40, 20, reflect=0.5)}


def sample_frame(ctx, path, w, h, depth, rows=None):
    s = rt_amd.Scene(path, w, h, depth)
    ctx.upload(s)
    f = s.frame.copy()
    if rows:
        f.row_begin, f.row_end = rows
    return f


def check(got, want, m, phong=False):
    assert got["rgb"].shape == want.shape and got["mask"].shape == m.shape
    assert np.array_equal(got["mask"], m), f"{np.count_nonzero(got['mask'] != m)} mask bytes differ"
    if phong:
        assert ulp_diff(got["rgb"], want) <= PHONG_ULP
        assert np.abs(got["rgba"].astype(int) - rgba8(want).astype(int)).max() <= 1
    else:
        assert bits_equal(got["rgb"], want), f"{np.count_nonzero(got['rgb'] != want)} floats differ"
        assert np.array_equal(got["rgba"], rgba8(want))


def base_frame(path, w, h, depth):
    return rt_amd.Scene(path, w, h, depth).frame.copy()


@pytest.mark.parametrize("i", range(1, 10))
@pytest.mark.parametrize("depth", [0, 3])
def test_scene_images(ctx, oracle, golden_images, i, depth):
    """64 x 48 samples, s = 2, every criterion."""
    S = golden_images[f"scene{i}_64x48_d{depth}"]
    want, m = ar.expect(oracle, scene(i), S, 2, ALL)
    assert 0.2 <= np.count_nonzero(m) / m.size <= 0.6
    f = sample_frame(ctx, scene(i), 64, 48, depth)
    if i in PHONG_SCENES:  # the colour criterion sees this context's own plain frame
        a = ar.planes(oracle, scene(i), 32, 24)
        m = ar.mask(ctx.render_float(base_frame(scene(i), 32, 24, depth)), a["id"], a["n"], ALL, 0.9, 0.1)
        want = ar.compose(S, 2, m)
    check(ctx.render_adaptive(f, 2, ALL), want, m, i in PHONG_SCENES)
    st = ctx.stats()
    assert st.primary_rays == m.size + 4 * np.count_nonzero(m) and st.kernel_ms > 0
    # (the stack covers the depth the scene can reach: 0 where nothing reflects or refracts)
    assert st.kernel.startswith(f"rt_refine_kernel<{st.stack_depth},1,") and 0 <= st.stack_depth <= depth


@pytest.mark.parametrize("s", [4, 8])
def test_scene7_larger_factors(ctx, oracle, s):
    """128 x 96 and 256 x 192 samples: 4 pixels and one pixel per wave."""
    S = oracle.render(scene(7), 32 * s, 24 * s, 3)
    want, m = ar.expect(oracle, scene(7), S, s, ALL)
    f = sample_frame(ctx, scene(7), 32 * s, 24 * s, 3)
    check(ctx.render_adaptive(f, s, ALL), want, m)
    assert ctx.stats().primary_rays == m.size + s * s * np.count_nonzero(m)


@pytest.mark.parametrize("criteria", [ar.EDGE_ID, ar.EDGE_NORMAL, ar.EDGE_COLOUR])
def test_each_criterion_alone(ctx, oracle, golden_images, criteria):
    """ID and NORMAL alone read no colour plane, COLOUR alone runs no AOV pass."""
    S = golden_images["scene7_64x48_d3"]
    want, m = ar.expect(oracle, scene(7), S, 2, criteria)
    assert m.any() and set(np.unique(m)) == {0, criteria}
    f = sample_frame(ctx, scene(7), 64, 48, 3)
    check(ctx.render_adaptive(f, 2, criteria), want, m)


def test_kernel_tiny_scene_depth0(ctx, oracle, golden_images):
    """scene2 at depth 0: the base frame by the launch-camera kernel, the samples by the lit query instance."""
    S = golden_images["scene2_64x48_d0"]
    want, m = ar.expect(oracle, scene(2), S, 2, ALL)
    f = sample_frame(ctx, scene(2), 64, 48, 0)
    check(ctx.render_adaptive(f, 2, ALL), want, m)
    assert ctx.stats().kernel == "rt_refine_kernel<0,1,21>" and ctx.stats().stack_depth == 0
    ctx.render_float(base_frame(scene(2), 32, 24, 0))
    assert ctx.stats().kernel.startswith("rt_trace_tiny")


def test_kernel_dfs_depth3(ctx, oracle, golden_images):
    S = golden_images["scene7_64x48_d3"]
    want, m = ar.expect(oracle, scene(7), S, 2, ALL)
    f = sample_frame(ctx, scene(7), 64, 48, 3)
    check(ctx.render_adaptive(f, 2, ALL), want, m)
    assert ctx.stats().kernel == "rt_refine_kernel<3,1,16>" and ctx.stats().stack_depth == 3


def hf_expect(oracle, hf_paths, key, depth):
    S = oracle.render(hf_paths[key], 64, 48, depth)
    want, m = ar.expect(oracle, hf_paths[key], S, 2, ar.EDGE_NORMAL | ar.EDGE_COLOUR, key=("hf1600", 32, 24))
    assert 0.3 <= np.count_nonzero(m) / m.size <= 0.8
    return want, m


def test_kernel_big_list_depth0(ctx, oracle, hf_paths):
    """1600 triangles, depth 0: the lit big-list query instance."""
    want, m = hf_expect(oracle, hf_paths, "hf1600", 0)
    f = sample_frame(ctx, hf_paths["hf1600"], 64, 48, 0)
    check(ctx.render_adaptive(f, 2, ar.EDGE_NORMAL | ar.EDGE_COLOUR), want, m)
    assert ctx.stats().kernel == "rt_refine_kernel<0,1,22>"


def test_kernel_bvh_depth3_wavefront_base(ctx, oracle, hf_paths):
    """reflect = 0.5, depth 3: the samples walk the exact BVH, the base frame is a wavefront frame."""
    want, m = hf_expect(oracle, hf_paths, "hf1600r", 3)
    f = sample_frame(ctx, hf_paths["hf1600r"], 64, 48, 3)
    check(ctx.render_adaptive(f, 2, ar.EDGE_NORMAL | ar.EDGE_COLOUR), want, m)
    assert ctx.stats().kernel == "rt_refine_kernel<3,1,278>"
    ctx.render_float(base_frame(hf_paths["hf1600r"], 32, 24, 3))
    assert ctx.stats().kernel.startswith("wavefront")


def test_one_pixel_per_wave(ctx, oracle, golden_images):
    """s = 8 on 64 x 48 samples: an 8 x 6 image."""
    S = golden_images["scene7_64x48_d3"]
    want, m = ar.expect(oracle, scene(7), S, 8, ALL)
    assert want.shape == (6, 8, 3) and m.any()
    f = sample_frame(ctx, scene(7), 64, 48, 3)
    check(ctx.render_adaptive(f, 8, ALL), want, m)


@pytest.mark.parametrize("depth", [0, 3])
def test_ragged_last_wave(ctx, oracle, golden_images, depth):
    """s = 2: 16 pixels per wave, a flagged count that is no multiple of 16 —
    depth 0 keeps the wave whole with dead tail lanes, depth 3 runs only the valid ones."""
    S = golden_images[f"scene9_64x48_d{depth}"]
    want, m = ar.expect(oracle, scene(9), S, 2, ALL)
    assert np.count_nonzero(m) % 16 != 0
    f = sample_frame(ctx, scene(9), 64, 48, depth)
    check(ctx.render_adaptive(f, 2, ALL), want, m)


def test_nothing_and_everything_flagged(ctx, golden_images):
    f = sample_frame(ctx, scene(7), 64, 48, 3)
    none = ctx.render_adaptive(f, 2, ar.EDGE_COLOUR, colour_delta=math.inf)
    assert ctx.stats().primary_rays == 32 * 24
    assert not none["mask"].any()
    assert bits_equal(none["rgb"], ctx.render_float(base_frame(scene(7), 32, 24, 3)))
    assert bits_equal(none["rgb"], golden_images["scene7_64x48_d3"][::2, ::2])
    every = ctx.render_adaptive(f, 2, ar.EDGE_COLOUR, colour_delta=-1.0)
    assert ctx.stats().primary_rays == 5 * 32 * 24
    assert (every["mask"] == ar.EDGE_COLOUR).all()
    assert bits_equal(every["rgb"], ctx.render_ss_float(f, 2)) and np.array_equal(every["rgba"], ctx.render_ss(f, 2))


def test_slabs_stitch_to_the_whole_frame(ctx, oracle, golden_images):
    """As on the CPU backend: the seam rows look across the seam (the halo rows)."""
    S = golden_images["scene6_64x48_d3"]
    want, m = ar.expect(oracle, scene(6), S, 2, ALL)
    parts = []
    for rows in ((0, 16), (16, 48)):
        f = sample_frame(ctx, scene(6), 64, 48, 3, rows=rows)
        parts.append(ctx.render_adaptive(f, 2, ALL))
    assert parts[0]["mask"].shape == (8, 32) and parts[1]["mask"].shape == (16, 32)
    check({k: np.concatenate([parts[0][k], parts[1][k]]) for k in parts[0]}, want, m)


def test_host_and_device_pointers_mixed(ctx, oracle, golden_images):
    torch = pytest.importorskip("torch")
    L = rt_amd.lib()
    S = golden_images["scene7_64x48_d3"]
    want, m = ar.expect(oracle, scene(7), S, 2, ALL)
    f = sample_frame(ctx, scene(7), 64, 48, 3)
    a = rt_amd.Adaptive(2, ALL, 0.9, 0.1)
    d_rgb = torch.zeros((24, 32, 3), dtype=torch.float32, device="cuda")
    d_mask = torch.zeros((24, 32), dtype=torch.uint8, device="cuda")
    h_q = np.zeros((24, 32, 4), np.uint8)
    o = rt_amd.AdaptiveOut(h_q.ctypes.data, d_rgb.data_ptr(), d_mask.data_ptr())
    assert L.rt_render_adaptive(ctx._h, ctypes.byref(f), ctypes.byref(a), ctypes.byref(o)) == 0
    check({"rgb": d_rgb.cpu().numpy(), "rgba": h_q, "mask": d_mask.cpu().numpy()}, want, m)
    h_m = np.zeros((24, 32), np.uint8)
    o = rt_amd.AdaptiveOut(None, None, h_m.ctypes.data)       # the mask alone: no sample is traced
    assert L.rt_render_adaptive(ctx._h, ctypes.byref(f), ctypes.byref(a), ctypes.byref(o)) == 0
    assert np.array_equal(h_m, m) and ctx.stats().primary_rays == m.size


def test_two_streams_share_the_buffers(oracle):
    """render_adaptive_async of two sample frames (64 x 48, then 96 x 64: the
    second grows the context's buffers while the first may be in flight) on two
    streams, back to back with no host sync: every image is right."""
    torch = pytest.importorskip("torch")
    ctx = rt_amd.Context(0)
    a = sample_frame(ctx, scene(7), 64, 48, 3)
    b = rt_amd.Scene(scene(7), 96, 64, 3).frame.copy()
    want = {"a": ar.expect(oracle, scene(7), oracle.render(scene(7), 64, 48, 3), 2, ALL),
            "b": ar.expect(oracle, scene(7), oracle.render(scene(7), 96, 64, 3), 2, ALL)}
    frames = {"a": a, "b": b}
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for rep in range(3):
        for name, st in (("a", s1), ("b", s2), ("a", s2), ("b", s1)):
            h, w = want[name][1].shape
            o = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
            q = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
            k = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
            for t in (o, q, k):
                t.record_stream(st)
            ctx.render_adaptive_async(frames[name], 2, ALL, rgba_dev_ptr=q.data_ptr(), rgb_dev_ptr=o.data_ptr(),
                                      mask_dev_ptr=k.data_ptr(), stream=st.cuda_stream)
            outs.append((name, o, q, k))
    ctx.sync()
    torch.cuda.synchronize()
    for name, o, q, k in outs:
        check({"rgb": o.cpu().numpy(), "rgba": q.cpu().numpy(), "mask": k.cpu().numpy()}, *want[name])


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


# the refused capture leaves its graph empty, which torch warns about
@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_capturing_stream_is_refused(oracle, golden_images):
    """hipGraph capture is out of scope: RT_E_STATE, nothing recorded, and the context renders on."""
    torch = pytest.importorskip("torch")
    ctx = rt_amd.Context(0)
    f = sample_frame(ctx, scene(7), 64, 48, 3)
    warm = ctx.render_adaptive(f, 2, ALL)      # (buffers sized, camera prepared: still refused)
    out = torch.zeros((24, 32, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with capture(torch, g):
        with pytest.raises(rt_amd.RtError) as e:
            ctx.render_adaptive_async(f, 2, ALL, rgb_dev_ptr=out.data_ptr(),
                                      stream=torch.cuda.current_stream().cuda_stream)
    assert e.value.code == -4
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()
    again = ctx.render_adaptive(f, 2, ALL)
    assert bits_equal(again["rgb"], warm["rgb"])
    check(again, *ar.expect(oracle, scene(7), golden_images["scene7_64x48_d3"], 2, ALL))


def test_argument_errors_enqueue_nothing(ctx):
    torch = pytest.importorskip("torch")
    L = rt_amd.lib()
    f = sample_frame(ctx, scene(1), 64, 48, 0)
    rgb = np.full((24, 32, 3), 7, np.float32)
    q = np.full((24, 32, 4), 7, np.uint8)
    mk = np.full((24, 32), 7, np.uint8)
    out = rt_amd.AdaptiveOut(q.ctypes.data, rgb.ctypes.data, mk.ctypes.data)

    def call(frame, s=2, criteria=ALL, o=out):
        a = rt_amd.Adaptive(s, criteria, 0.9, 0.1)
        return L.rt_render_adaptive(ctx._h, ctypes.byref(frame), ctypes.byref(a), ctypes.byref(o))

    for s in (0, 1, 3, 5, 6, 7, 9):
        assert call(f, s=s) == -1, s
    assert call(sample_frame(ctx, scene(1), 64, 44, 0), s=8) == -1
    g = f.copy()
    g.row_begin = 2
    assert call(g, s=4) == -1
    g = f.copy()
    g.band_rows, g.band_count, g.band_index = 32, 2, 0
    assert call(g) == -1
    for criteria in (0, 8):
        assert call(f, criteria=criteria) == -1
    assert call(f, o=rt_amd.AdaptiveOut(None, None, None)) == -1
    g = f.copy()
    g.flags = rt_amd.FLAG_STATS
    assert call(g) == -1
    a = rt_amd.Adaptive(2, ALL, 0.9, 0.1)
    # a host pointer given to the async call
    assert L.rt_render_adaptive_async(ctx._h, ctypes.byref(f), ctypes.byref(a), ctypes.byref(out), None) == -1
    d = torch.full((24, 32, 3), 7.0, dtype=torch.float32, device="cuda")
    mixed = rt_amd.AdaptiveOut(q.ctypes.data, d.data_ptr(), None)
    assert L.rt_render_adaptive_async(ctx._h, ctypes.byref(f), ctypes.byref(a), ctypes.byref(mixed), None) == -1
    # beyond the deepest compiled stack, as for a render
    g = sample_frame(ctx, scene(9), 64, 48, 40)   # two facing mirrors: every depth is reachable
    g.min_energy = -1.0
    assert call(g) == -6
    # call order and backend
    fresh = rt_amd.Context(0)
    assert L.rt_render_adaptive(fresh._h, ctypes.byref(f), ctypes.byref(a), ctypes.byref(out)) == -4
    assert L.rt_cpu_render_adaptive(ctx._h, ctypes.byref(f), ctypes.byref(a), ctypes.byref(out)) == -4
    ctx.sync()
    torch.cuda.synchronize()
    assert (rgb == 7).all() and (q == 7).all() and (mk == 7).all() and bool((d == 7).all())


@pytest.mark.parametrize("i,depth", [(1, 0), (2, 0), (6, 3), (7, 3), (9, 3)])
def test_gpu_equals_the_cpu_backend(ctx, i, depth):
    cpu = rt_amd.CpuContext(min(8, os.cpu_count() or 1))
    f = sample_frame(ctx, scene(i), 64, 48, depth)
    sample_frame(cpu, scene(i), 64, 48, depth)
    got, want = ctx.render_adaptive(f, 4, ALL, 0.95, 0.05), cpu.render_adaptive(f, 4, ALL, 0.95, 0.05)
    assert np.array_equal(got["mask"], want["mask"]) and got["mask"].any()
    assert bits_equal(got["rgb"], want["rgb"]) and np.array_equal(got["rgba"], want["rgba"])


def test_cli_adaptive_both_backends(tmp_path, oracle, golden_images):
    want, m = ar.expect(oracle, scene(7), golden_images["scene7_64x48_d3"], 2, ALL)
    for backend in ("hip", "cpu"):
        out, mk = tmp_path / f"{backend}.ppm", tmp_path / f"{backend}.npy"
        r = subprocess.run([EXE, scene(7), "-x", "32", "-y", "24", "-d", "3", "--adaptive", "2", "--backend", backend,
                            "--threads", "4", "-o", str(out), "--mask", str(mk)], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
        head = open(out, "rb").read().split(b"\n", 3)
        assert head[1] == b"32 24"
        img = np.frombuffer(head[3], np.uint8).reshape(24, 32, 3)
        assert np.array_equal(img[::-1], rgba8(want)[..., :3]), backend
        assert np.array_equal(np.load(mk), m), backend
