"""The three ray queries' host path on the HIP backend (include/rt.h
rt_trace_rays*, rt_filter_rays*, rt_shade_rays*): the code and the exact
rt_last_error text of every refusal the GPU entry points make, the order of
shade's depth refusal against the pointer checks, the whole rt_stats record
after a synchronous call, and mixed host / device pointers against the
all-host call's bits.  The expectations are rt.h's and the strings the entry
points have always set, written down here.  What the kernels compute is
test_gpu_rays / test_gpu_filter / test_gpu_shade's business: scene3 at 64 x 32,
8 and 65 of its camera rays (their six floats serve as segments too).
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import aov_ref
import rt_amd
from conftest import scene
from test_query_errors_cpu import ARG, COUNTERS, NO_FRAME, QUERIES, SENTINEL, STATE, call, error, stats

pytestmark = pytest.mark.gpu

F = np.float32
UNSUPPORTED = -6
SIZES = (8, 65)
PLANES = {"trace": (1, 1, 3)}   # floats (or ints) per item of each output; the others: one (N, 3) plane
COUNTER = {"trace": "bounce_rays", "filter": "shadow_rays", "shade": "primary_rays"}


def planes(q):
    return PLANES.get(q, (3,))


def aligned(name):
    return f"{name}: device pointers must be 8-byte aligned".encode()


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def made():
    s = rt_amd.Scene(scene(3), 64, 32, 0)
    ctx = rt_amd.Context(0)
    ctx.upload(s)
    k = np.arange(max(SIZES)) * 31 % (64 * 32)
    D = aov_ref.camera_dirs(aov_ref.Cam.from_frame(s.frame), k % 64, k // 64)
    rays = np.ascontiguousarray(np.concatenate([np.broadcast_to(np.asarray(s.frame.cam_pos[:], F), D.shape), D], 1), F)
    yield s, ctx, rays
    ctx.close()


def host_out(q, n):
    return [np.full((n, w), SENTINEL, np.uint32) for w in planes(q)]


def device_out(torch, q, n, slack=2):
    """Sentinel-filled device planes of n items and `slack` words more."""
    return [torch.full((n * w + slack,), SENTINEL, dtype=torch.int32, device="cuda") for w in planes(q)]


def device_rays(torch, rays, slack=2):
    d = torch.from_numpy(np.concatenate([rays.ravel(), np.zeros(slack, F)])).cuda()
    torch.cuda.synchronize()
    return d


def words(v):
    return np.ascontiguousarray(v.cpu().numpy()).view(np.uint32)


def sync(q, ctx, f, rays, n, ptrs):
    return call(q, ctx._h, rays, n, ptrs, f, prefix="rt_")


def enqueue(q, ctx, f, rays, n, ptrs):
    return call(q, ctx._h, rays, n, ptrs, f, prefix="rt_", tail=(None,))


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("q", list(QUERIES))
def test_before_an_upload(torch, made, q):
    s, _, rays = made
    fresh = rt_amd.Context(0)
    try:
        d, dev, host = device_rays(torch, rays[:8]), device_out(torch, q, 8), host_out(q, 8)
        msg = f"{QUERIES[q][0]} before rt_upload_scene".encode()
        for n in (8, 0, -1):   # the state comes before the count
            assert sync(q, fresh, s.frame, rays.ctypes.data, n, [a.ctypes.data for a in host]) == STATE
            assert error(fresh._h) == msg
            assert enqueue(q, fresh, s.frame, d.data_ptr(), n, [v.data_ptr() for v in dev]) == STATE
            assert error(fresh._h) == msg
        torch.cuda.synchronize()
        assert all((a == SENTINEL).all() for a in host) and all((words(v) == SENTINEL).all() for v in dev)
    finally:
        fresh.close()


@pytest.mark.parametrize("q", list(QUERIES))
def test_counts_and_nulls(torch, made, q):
    s, ctx, rays = made
    name, noun, nulls = QUERIES[q]
    f, h = s.frame, ctx._h
    d, dev, host = device_rays(torch, rays[:8]), device_out(torch, q, 8), host_out(q, 8)
    hp, dp = [a.ctypes.data for a in host], [v.data_ptr() for v in dev]
    count, null = f"{name}: the {noun} count must be 0 .. INT32_MAX".encode(), f"{name}: {nulls}".encode()
    before = bytes(stats(h))
    for run, r, p in ((sync, rays.ctypes.data, hp), (enqueue, d.data_ptr(), dp)):
        for n in (-1, 2**31):
            assert run(q, ctx, f, r, n, p) == ARG and error(h) == count
        assert run(q, ctx, f, None, -1, p) == ARG and error(h) == count   # the count comes before the pointers
        assert run(q, ctx, f, None, 8, p) == ARG and error(h) == null
        assert run(q, ctx, f, r, 8, [None] * len(p)) == ARG and error(h) == null
        if q == "shade":   # the frame comes before the count and the pointers
            for n, rr in ((8, r), (-1, r), (0, r), (8, None)):
                assert run(q, ctx, None, rr, n, p) == ARG and error(h) == NO_FRAME.encode()
        assert run(q, ctx, f, r, 0, p) == 0                    # n == 0: RT_OK, nothing written,
        assert run(q, ctx, f, None, 0, [None] * len(p)) == 0   # whatever the pointers
    L = rt_amd.lib()
    if q == "trace":   # no rt_aov at all: as no plane
        assert L.rt_trace_rays(h, rays.ctypes.data, 8, None) == ARG and error(h) == null
        assert L.rt_trace_rays_async(h, d.data_ptr(), 8, None, None) == ARG and error(h) == null
    assert call(q, None, rays.ctypes.data, 8, hp, f, prefix="rt_") == ARG            # no context
    assert call(q, None, d.data_ptr(), 8, dp, f, prefix="rt_", tail=(None,)) == ARG
    assert call(q, h, rays.ctypes.data, 8, hp, f) == STATE                           # the other backend's call
    ctx.sync()
    torch.cuda.synchronize()
    assert all((a == SENTINEL).all() for a in host) and all((words(v) == SENTINEL).all() for v in dev)
    assert bytes(stats(h)) == before   # no refused call and no n == 0 touched the record


@pytest.mark.parametrize("q", list(QUERIES))
def test_async_takes_device_pointers(torch, made, q):
    s, ctx, rays = made
    name = QUERIES[q][0]
    d, dev, host = device_rays(torch, rays[:8]), device_out(torch, q, 8), host_out(q, 8)
    dp = [v.data_ptr() for v in dev]
    msg = f"{name}_async takes device pointers".encode()
    assert enqueue(q, ctx, s.frame, rays.ctypes.data, 8, dp) == ARG and error(ctx._h) == msg
    for i, a in enumerate(host):   # each output in turn
        p = list(dp)
        p[i] = a.ctypes.data
        assert enqueue(q, ctx, s.frame, d.data_ptr(), 8, p) == ARG and error(ctx._h) == msg
    # the input is looked at before the outputs: host rays and a misaligned output
    assert enqueue(q, ctx, s.frame, rays.ctypes.data, 8, [x + 4 for x in dp]) == ARG and error(ctx._h) == msg
    ctx.sync()
    torch.cuda.synchronize()
    assert all((a == SENTINEL).all() for a in host) and all((words(v) == SENTINEL).all() for v in dev)


@pytest.mark.parametrize("run", [sync, enqueue], ids=["sync", "async"])
@pytest.mark.parametrize("q", list(QUERIES))
def test_device_pointers_misaligned_by_4_bytes(torch, made, q, run):
    s, ctx, rays = made
    d, dev = device_rays(torch, rays[:8]), device_out(torch, q, 8)
    dp = [v.data_ptr() for v in dev]
    assert run(q, ctx, s.frame, d.data_ptr() + 4, 8, dp) == ARG and error(ctx._h) == aligned(QUERIES[q][0])
    for i in range(len(dp)):   # each output in turn
        p = list(dp)
        p[i] += 4
        assert run(q, ctx, s.frame, d.data_ptr(), 8, p) == ARG and error(ctx._h) == aligned(QUERIES[q][0])
    if q == "trace":   # a plane that is not requested is not looked at
        assert run(q, ctx, s.frame, d.data_ptr(), 8, [dp[0], None, None]) == 0
        ctx.sync()
        torch.cuda.synchronize()
        assert (words(dev[0])[:8] != SENTINEL).all() and (words(dev[0])[8:] == SENTINEL).all()
        dev[0].fill_(SENTINEL)
    ctx.sync()
    torch.cuda.synchronize()
    assert all((words(v) == SENTINEL).all() for v in dev)


@pytest.mark.parametrize("run", [sync, enqueue], ids=["sync", "async"])
def test_shade_depth_above_32_is_refused_before_the_pointers(torch, made, run):
    """scene9 with min_energy -1: every depth is reachable.  Depth 33 has no compiled stack: RT_E_UNSUPPORTED,
    also where a device pointer is misaligned (or, for the async call, a host pointer) — RT_E_ARG at depth 32."""
    _, _, rays = made
    s = rt_amd.Scene(scene(9), 64, 32, 3)
    ctx = rt_amd.Context(0)
    try:
        ctx.upload(s)
        d, dev = device_rays(torch, rays[:8]), device_out(torch, "shade", 8)
        f = s.frame.copy()
        f.max_bounces, f.min_energy = 33, -1.0
        msg = b"reachable bounce depth 33 exceeds the compiled stack (32)"
        for r, o in ((d.data_ptr() + 4, dev[0].data_ptr()), (d.data_ptr(), dev[0].data_ptr() + 4),
                     (d.data_ptr(), dev[0].data_ptr())):
            assert run("shade", ctx, f, r, 8, [o]) == UNSUPPORTED and error(ctx._h) == msg
        if run is enqueue:
            assert run("shade", ctx, f, rays.ctypes.data, 8, [dev[0].data_ptr()]) == UNSUPPORTED
        assert run("shade", ctx, f, None, 8, [dev[0].data_ptr()]) == ARG    # the nulls come before the depth,
        assert run("shade", ctx, f, d.data_ptr() + 4, 0, [dev[0].data_ptr()]) == 0   # and so does n == 0
        f.max_bounces = 32
        assert run("shade", ctx, f, d.data_ptr() + 4, 8, [dev[0].data_ptr()]) == ARG
        assert error(ctx._h) == aligned("rt_shade_rays")
        ctx.sync()
        torch.cuda.synchronize()
        assert (words(dev[0]) == SENTINEL).all()
    finally:
        ctx.close()


# ------------------------------------------------------- the stats record
def expected_kernel(q, s, ctx):
    """scene3 has no BVH (fewer than 64 triangles) and fewer than 1025 triangles: the <0> instances, and
    at a reachable depth of 0 the lit small-list shade instance (rt_variant.h: kRayQuery | kLightBuf | kSmallList)."""
    L = rt_amd.lib()
    L.rt_debug_bvh_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int]
    out = (ctypes.c_double * 5)()
    assert L.rt_debug_bvh_info(ctx._h, out, 5) == 0 and out[0] == 0.0
    ntri = sum(s.flat.type[i] == 0 for i in range(s.flat.n_surfaces))
    assert 0 < ntri < 64
    return {"trace": "rt_rays_kernel<0>", "filter": "rt_filter_kernel<0>", "shade": "rt_shade_rays_kernel<0,1,21>"}[q]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("q", list(QUERIES))
def test_the_whole_stats_record_after_a_sync_call(made, q, n):
    s, ctx, rays = made
    other = "filter" if q == "trace" else "trace"   # the record is reset, not added to
    assert sync(other, ctx, s.frame, rays.ctypes.data, n, [a.ctypes.data for a in host_out(other, n)]) == 0
    host = host_out(q, n)
    assert sync(q, ctx, s.frame, rays.ctypes.data, n, [a.ctypes.data for a in host]) == 0
    assert not any((a == SENTINEL).any() for a in host)
    st = stats(ctx._h)
    assert st.kernel == expected_kernel(q, s, ctx) and st.kernel_ms > 0
    want = {k: 0 for k in COUNTERS}
    want[COUNTER[q]] = n
    if q == "shade":
        want["light_batch"] = 1   # (stack_depth 0)
    assert {k: getattr(st, k) for k in COUNTERS} == want


# ------------------------------------------------------------ the pointers
@pytest.mark.parametrize("q", list(QUERIES))
def test_mixed_and_device_pointers_give_the_all_host_bits(torch, made, q):
    s, ctx, rays = made
    n = 65
    r = np.ascontiguousarray(rays[:n])
    want = host_out(q, n)
    assert sync(q, ctx, s.frame, r.ctypes.data, n, [a.ctypes.data for a in want]) == 0
    assert not any((a == SENTINEL).any() for a in want)
    d = device_rays(torch, r, slack=0)
    # host input, device outputs (64 words more: nothing behind item n is written)
    dev = device_out(torch, q, n, slack=64)
    assert sync(q, ctx, s.frame, r.ctypes.data, n, [v.data_ptr() for v in dev]) == 0
    torch.cuda.synchronize()
    for v, a in zip(dev, want):
        assert np.array_equal(words(v)[:a.size], a.ravel()) and (words(v)[a.size:] == SENTINEL).all()
    # device input, host outputs
    host = host_out(q, n)
    assert sync(q, ctx, s.frame, d.data_ptr(), n, [a.ctypes.data for a in host]) == 0
    assert all(np.array_equal(a, b) for a, b in zip(host, want))
    # device input, device outputs, enqueued
    dev = device_out(torch, q, n, slack=64)
    assert enqueue(q, ctx, s.frame, d.data_ptr(), n, [v.data_ptr() for v in dev]) == 0
    ctx.sync()
    torch.cuda.synchronize()
    for v, a in zip(dev, want):
        assert np.array_equal(words(v)[:a.size], a.ravel()) and (words(v)[a.size:] == SENTINEL).all()
    if q == "trace":   # host rays, one host plane and one device plane, one plane not requested
        h0, d2 = host_out(q, n)[0], device_out(torch, q, n, slack=64)[2]
        assert sync(q, ctx, s.frame, r.ctypes.data, n, [h0.ctypes.data, None, d2.data_ptr()]) == 0
        torch.cuda.synchronize()
        assert np.array_equal(h0, want[0]) and np.array_equal(words(d2)[:3 * n], want[2].ravel())
