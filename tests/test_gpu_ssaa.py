"""Supersampled anti-aliasing on the HIP path (include/rt.h rt_render_ss*):
the plain render's kernels into the context's float intermediate, then
rt_resolve_kernel (csrc/rt_resolve.h) on the same stream.  Expected images:
ssaa_ref.box of the reference's frame of the sample grid (tests/golden/
images.npz, made from the reference's sources) or of the oracle's — bit for
bit, except scene4 (Phong: ocml powf against glibc powf, as in
test_gpu_parity.py), whose RGBA8 must be within 1 LSB."""
from __future__ import annotations

import contextlib
import ctypes
import gc

import numpy as np
import pytest

import rt_amd
from conftest import bits_equal, rgba8, scene
from ssaa_ref import box

pytestmark = pytest.mark.gpu

PHONG_SCENES = {4}


@pytest.fixture(scope="module")
def ctx():
    return rt_amd.Context(0)


def sample_frame(ctx, path, w, h, depth, rows=None, bands=None, flags=0):
    s = rt_amd.Scene(path, w, h, depth)
    ctx.upload(s)
    f = s.frame.copy()
    f.flags = flags
    if rows:
        f.row_begin, f.row_end = rows
    if bands:
        f.band_rows, f.band_count, f.band_index = bands
    return f


def check(ctx, f, s, want, i=0):
    got = ctx.render_ss_float(f, s)
    q = ctx.render_ss(f, s)
    assert got.shape == want.shape and q.shape == want.shape[:2] + (4,)
    if i in PHONG_SCENES:
        assert np.abs(rgba8(got).astype(int) - rgba8(want).astype(int)).max() <= 1
        assert np.abs(q.astype(int) - rgba8(want).astype(int)).max() <= 1
    else:
        assert bits_equal(got, want), f"s {s}: {np.count_nonzero(got != want)} floats differ"
        assert np.array_equal(q, rgba8(want))
    return got, q


@pytest.mark.parametrize("i", range(1, 10))
@pytest.mark.parametrize("depth", [0, 1, 3, 5])
def test_scene_images(ctx, golden_images, i, depth):
    """64 x 48 samples (width % 4 == 0: the 16-byte loads), s = 2 and 4, and
    s = 8 on scenes 2 and 7: the tiny-record, small-list and DFS kernels."""
    f = sample_frame(ctx, scene(i), 64, 48, depth)
    ref = golden_images[f"scene{i}_64x48_d{depth}"]
    for s in (2, 4) + ((8,) if i in (2, 7) else ()):
        check(ctx, f, s, box(ref, s), i)


def test_factor_one_is_the_plain_render(ctx, golden_images):
    f = sample_frame(ctx, scene(7), 64, 48, 3)
    check(ctx, f, 1, golden_images["scene7_64x48_d3"])


def test_dword_path_odd_factor(ctx, oracle):
    """66 x 33 samples, s = 3: the row pitch is no multiple of 16 bytes."""
    f = sample_frame(ctx, scene(5), 66, 33, 3)
    check(ctx, f, 3, box(oracle.render(scene(5), 66, 33, 3), 3))


def test_vector_path_odd_factor(ctx, oracle):
    """72 x 24 samples, s = 3: runs of four pixels per lane, 16-byte loads."""
    f = sample_frame(ctx, scene(5), 72, 24, 3)
    check(ctx, f, 3, box(oracle.render(scene(5), 72, 24, 3), 3))


def test_whole_frame_into_one_pixel(ctx, oracle):
    f = sample_frame(ctx, scene(5), 8, 8, 3)
    check(ctx, f, 8, box(oracle.render(scene(5), 8, 8, 3), 8))


@pytest.mark.parametrize("s,w,h", [(5, 40, 20), (6, 48, 24), (7, 56, 28), (5, 35, 20), (6, 54, 24), (7, 42, 28)])
def test_other_factors_both_paths(ctx, oracle, s, w, h):
    """s = 5, 6, 7 (their own kernels), a width that is a multiple of 4 and one that is not."""
    f = sample_frame(ctx, scene(9), w, h, 1)
    check(ctx, f, s, box(oracle.render(scene(9), w, h, 1), s))


def test_big_list_kernel(ctx, oracle, heightfield_path):
    """The 50k-triangle heightfield, depth 1: the big-list kernel with its
    camera buffer and light buffer writes the samples."""
    f = sample_frame(ctx, heightfield_path, 64, 32, 1)
    check(ctx, f, 2, box(oracle.render(heightfield_path, 64, 32, 1), 2))
    assert ctx.stats().kernel.startswith("rt_trace")


def test_wavefront_levels(ctx, oracle, heightfield_r05_path):
    """reflect = 0.5 on every triangle, depth 3: a wavefront frame, whose
    pixels (here: samples) are written by the fold kernels."""
    f = sample_frame(ctx, heightfield_r05_path, 64, 32, 3)
    check(ctx, f, 2, box(oracle.render(heightfield_r05_path, 64, 32, 3), 2))
    assert ctx.stats().kernel.startswith("wavefront")


def test_chunked_equals_unchunked(golden_images):
    """RT_OPT_SS_CHUNK_ROWS = 16 on 64 x 48 samples, s = 2: chunks of 16 and
    8 output rows — the unchunked bits, float and RGBA8, into host memory and
    into device memory."""
    torch = pytest.importorskip("torch")
    L = rt_amd.lib()
    want = box(golden_images["scene7_64x48_d3"], 2)
    whole, chunked = rt_amd.Context(0), rt_amd.Context(0, ss_chunk_rows=16)
    assert chunked.get_option("ss_chunk_rows") == 16 and whole.get_option("ss_chunk_rows") == 0
    for c in (whole, chunked):
        f = sample_frame(c, scene(7), 64, 48, 3)
        got, q = check(c, f, 2, want)
        df = torch.zeros((24, 32, 3), dtype=torch.float32, device="cuda")
        dq = torch.zeros((24, 32, 4), dtype=torch.uint8, device="cuda")
        assert L.rt_render_ss_float(c._h, ctypes.byref(f), 2, ctypes.c_void_p(df.data_ptr())) == 0
        assert L.rt_render_ss(c._h, ctypes.byref(f), 2, ctypes.c_void_p(dq.data_ptr())) == 0
        assert bits_equal(df.cpu().numpy(), want) and np.array_equal(dq.cpu().numpy(), rgba8(want))
    # a chunk size that is no multiple of 16 is rounded up (17 -> 32: one chunk of 24 rows)
    chunked.set_option("ss_chunk_rows", 17)
    check(chunked, sample_frame(chunked, scene(7), 64, 48, 3), 2, want)


def test_slab_rows(ctx, golden_images):
    want = box(golden_images["scene7_64x48_d3"], 2)
    f = sample_frame(ctx, scene(7), 64, 48, 3, rows=(16, 48))
    check(ctx, f, 2, want[8:24])


@pytest.mark.parametrize("index", [0, 1])
def test_bands(ctx, golden_images, index):
    """As on the CPU: rank 1's band reaches past the frame; those 8 output rows stay unwritten."""
    want = box(golden_images["scene7_64x48_d3"], 2)
    f = sample_frame(ctx, scene(7), 64, 48, 3, bands=(32, 2, index))
    got, q = ctx.render_ss_float(f, 2), ctx.render_ss(f, 2)
    assert got.shape == (16, 32, 3)
    if index == 0:
        assert bits_equal(got, want[:16]) and np.array_equal(q, rgba8(want[:16]))
    else:
        assert bits_equal(got[:8], want[16:24]) and np.array_equal(q[:8], rgba8(want[16:24]))
        assert not got[8:].any() and not q[8:].any()


def test_argument_errors_enqueue_nothing(ctx):
    L = rt_amd.lib()
    f = sample_frame(ctx, scene(1), 64, 48, 0)
    out = np.full((48, 64, 4), 7, np.uint8)
    for s in (0, 9, 5):
        assert L.rt_render_ss(ctx._h, ctypes.byref(f), s, out.ctypes.data) == -1
        assert L.rt_render_ss_async(ctx._h, ctypes.byref(f), s, None, None, None) == -1
    g = f.copy()
    g.band_rows, g.band_count, g.band_index = 16, 2, 0
    assert L.rt_render_ss_float(ctx._h, ctypes.byref(g), 2, out.ctypes.data) == -1
    assert (out == 7).all()
    # the CPU backend's calls refuse a HIP context
    assert L.rt_cpu_render_ss(ctx._h, ctypes.byref(f), 2, out.ctypes.data) == -4
    assert L.rt_cpu_render_ss_float(ctx._h, ctypes.byref(f), 2, out.ctypes.data) == -4


def test_two_streams_share_the_intermediate(oracle):
    """render_ss_async of two sample frames (64 x 48 and 96 x 64: the second
    grows the intermediate while the first may be in flight) on two streams,
    back to back with no host sync: every image is right."""
    torch = pytest.importorskip("torch")
    ctx = rt_amd.Context(0)
    a = sample_frame(ctx, scene(7), 64, 48, 3)
    b = rt_amd.Scene(scene(7), 96, 64, 3).frame.copy()
    want = {"a": box(oracle.render(scene(7), 64, 48, 3), 2), "b": box(oracle.render(scene(7), 96, 64, 3), 2)}
    frames = {"a": a, "b": b}
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for rep in range(3):
        for name, st in (("a", s1), ("b", s2), ("a", s2), ("b", s1)):
            h, w = want[name].shape[:2]
            o = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
            q = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
            o.record_stream(st)
            q.record_stream(st)
            ctx.render_ss_async(frames[name], 2, q.data_ptr(), o.data_ptr(), st.cuda_stream)
            outs.append((name, o, q))
    ctx.sync()
    torch.cuda.synchronize()
    for k, (name, o, q) in enumerate(outs):
        assert bits_equal(o.cpu().numpy(), want[name]), (k, name)
        assert np.array_equal(q.cpu().numpy(), rgba8(want[name])), (k, name)


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
def test_graph_capture_and_replay(golden_images):
    """render_ss_async in a hipGraph after one warm call: two replays give the
    warm call's bits.  Without the warm call the intermediate is not sized:
    RT_E_STATE, as for an unprepared camera."""
    torch = pytest.importorskip("torch")
    want = box(golden_images["scene7_64x48_d3"], 2)
    ctx = rt_amd.Context(0)
    f = sample_frame(ctx, scene(7), 64, 48, 3)
    ctx.prepare_camera(f)
    out = torch.zeros((24, 32, 3), dtype=torch.float32, device="cuda")
    q = torch.zeros((24, 32, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g0 = torch.cuda.CUDAGraph()
    with capture(torch, g0):
        with pytest.raises(rt_amd.RtError) as e:
            ctx.render_ss_async(f, 2, q.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert e.value.code == -4
    warm = ctx.render_ss_float(f, 2)  # sizes the intermediate, prepares the camera
    assert bits_equal(warm, want)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with capture(torch, g):
        ctx.render_ss_async(f, 2, q.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        out.zero_()
        q.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert bits_equal(out.cpu().numpy(), warm)
        assert np.array_equal(q.cpu().numpy(), rgba8(want))


def test_stats_count_samples(ctx):
    f = sample_frame(ctx, scene(7), 64, 48, 3, flags=rt_amd.FLAG_STATS)
    ctx.render_ss(f, 2)
    st = ctx.stats()
    assert st.primary_rays == 64 * 48
    assert st.kernel_ms > 0
    ctx.render_ss_float(f, 4)
    assert ctx.stats().primary_rays == 64 * 48


def test_rgba8_is_quantised_float(ctx):
    for i in (1, 4, 7):
        f = sample_frame(ctx, scene(i), 96, 64, 5)
        assert np.array_equal(ctx.render_ss(f, 2), rgba8(ctx.render_ss_float(f, 2)))


def test_cli_ssaa(tmp_path, golden_images):
    import os
    import subprocess

    from conftest import REPO

    exe = os.path.join(REPO, "ray-tracing-gpu_amd", "lib", "rt_render")
    out = tmp_path / "s7.ppm"
    r = subprocess.run([exe, scene(7), "-x", "32", "-y", "24", "-d", "3", "--ssaa", "2", "-o", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    head = open(out, "rb").read().split(b"\n", 3)
    assert head[1] == b"32 24"
    img = np.frombuffer(head[3], np.uint8).reshape(24, 32, 3)
    assert np.array_equal(img[::-1], rgba8(box(golden_images["scene7_64x48_d3"], 2))[..., :3])
