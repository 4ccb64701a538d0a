"""The three ray queries' host contract on the CPU backend (include/rt.h
rt_cpu_trace_rays, rt_cpu_filter_rays, rt_cpu_shade_rays): the code and the
exact rt_last_error text of every refusal, the n == 0 rule, and the whole
rt_stats record after a good call.  The expectations are rt.h's and the
strings the entry points have always set — written down here, not read from
the code under test.  The scene: a triangle, a plane and a sphere with one
light, built as an rt_scene_flat; 8 rays towards it.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import rt_amd

F = np.float32
N = 8
SENTINEL = 0x7FC12345  # a NaN pattern no query writes
ARG, STATE = -1, -4    # RT_E_ARG, RT_E_STATE
COUNTERS = [name for name, _ in rt_amd.Stats._fields_ if name not in ("kernel_ms", "kernel_name")]

TYPES = np.array([0, 1, 2], np.int32)  # RT_TRIANGLE, RT_PLANE, RT_QUADRIC
GEOM = np.array([[-1, -1, -3, 1, -1, -3, 0, 1, -3, 0, 0, 1],    # a triangle in z = -3
                 [0, 1, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0],          # the plane y = -2
                 [1, 1, 1, 0, 0, 12, 0, 0, 0, 35, 0, 0]], F)    # the unit sphere around (0, 0, -6)
MATERIAL = np.array([[0.8, 0.2, 0.2, 0.1, 0.7, 0, 0, 0, 0, 1],
                     [0.2, 0.8, 0.2, 0.1, 0.7, 0, 0, 0, 0, 1],
                     [0.2, 0.2, 0.8, 0.1, 0.7, 0, 0, 0.5, 0, 1]], F)
LIGHTS = np.array([[0, 4, 0, 1, 1, 1, 1]], F)
RAYS = np.array([[0, 0, 0, 0, 0.05, -1], [0, 0, 0, 0.1, 0.05, -1],     # the triangle
                 [3, 0, -6, -1, 0, 0], [0, 0, -4, 0, 0, -1],           # the sphere
                 [0, 0, 0, 0, -1, 0], [0, 0, 0, 0.3, -1, -0.2],        # the plane
                 [0, 0, 0, 0, 1, 0], [0, 0, 0, 1, 1, 0]], F)           # nothing

# query -> (the call's name in messages, the noun of its count, its message for a null pointer)
QUERIES = {"trace": ("rt_trace_rays", "ray", "no rays or no output plane"),
           "filter": ("rt_filter_rays", "segment", "no segments or no output"),
           "shade": ("rt_shade_rays", "ray", "no rays or no output")}
NO_FRAME = "rt_shade_rays: no rt_frame (max_bounces, min_energy, scene_ior, background)"


def flat():
    ptr = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))
    return rt_amd.SceneFlat(3, 1, ptr(TYPES, ctypes.c_int32), ptr(GEOM, ctypes.c_float), ptr(MATERIAL, ctypes.c_float),
                            ptr(LIGHTS, ctypes.c_float))


def frame():
    f = rt_amd.Frame()
    f.max_bounces, f.min_energy, f.scene_ior = 2, 0.01, 1.0
    f.background[:] = [0.1, 0.2, 0.3]
    return f


class Out:
    """Sentinel-filled outputs of one query and the pointers to them."""

    def __init__(self, q):
        shapes = {"trace": [(N,), (N,), (N, 3)]}.get(q, [(N, 3)])
        self.arrays = [np.full(s, SENTINEL, np.uint32) for s in shapes]
        self.ptrs = [a.ctypes.data for a in self.arrays]

    def untouched(self):
        return all((a == SENTINEL).all() for a in self.arrays)


def call(q, h, rays, n, ptrs, f=None, prefix="rt_cpu_", tail=()):
    """One entry point of query q through the C ABI; ptrs: its output pointers (None: null)."""
    L = rt_amd.lib()
    fn = getattr(L, f"{prefix}{QUERIES[q][0][3:]}{'_async' if tail else ''}")
    if q == "trace":
        aov = rt_amd.Aov(*ptrs)
        return fn(h, rays, n, ctypes.byref(aov), *tail)
    if q == "filter":
        return fn(h, rays, n, ptrs[0], *tail)
    return fn(h, ctypes.byref(f) if f is not None else None, rays, n, ptrs[0], *tail)


def error(h):
    return rt_amd.lib().rt_last_error(h)


def stats(h):
    s = rt_amd.Stats()
    assert rt_amd.lib().rt_last_stats(h, ctypes.byref(s)) == 0
    return s


def record(s):
    return bytes(s)


@pytest.fixture(scope="module")
def cpu():
    c = rt_amd.CpuContext(2)
    assert rt_amd.lib().rt_upload_scene(c._h, ctypes.byref(flat())) == 0
    yield c
    c.close()


@pytest.mark.parametrize("q", list(QUERIES))
def test_before_an_upload(q):
    fresh = rt_amd.CpuContext(1)
    o = Out(q)
    try:
        for n in (N, 0, -1):   # the state comes before the count
            assert call(q, fresh._h, RAYS.ctypes.data, n, o.ptrs, frame()) == STATE
            assert error(fresh._h) == f"{QUERIES[q][0]} before rt_upload_scene".encode()
        assert o.untouched()
    finally:
        fresh.close()


@pytest.mark.parametrize("q", list(QUERIES))
def test_refusals_code_and_message(cpu, q):
    name, noun, nulls = QUERIES[q]
    o = Out(q)
    h, r, f = cpu._h, RAYS.ctypes.data, frame()
    count = f"{name}: the {noun} count must be 0 .. INT32_MAX".encode()
    for n in (-1, 2**31):
        assert call(q, h, r, n, o.ptrs, f) == ARG and error(h) == count
    assert call(q, h, None, N, o.ptrs, f) == ARG and error(h) == f"{name}: {nulls}".encode()
    assert call(q, h, r, N, [None] * len(o.ptrs), f) == ARG and error(h) == f"{name}: {nulls}".encode()
    # the count comes before the pointers
    assert call(q, h, None, -1, o.ptrs, f) == ARG and error(h) == count
    if q == "trace":   # no rt_aov at all: as no plane
        assert rt_amd.lib().rt_cpu_trace_rays(h, r, N, None) == ARG and error(h) == f"{name}: {nulls}".encode()
    if q == "shade":   # the frame comes before the count and the pointers
        for n, rays in ((N, r), (-1, r), (0, r), (N, None)):
            assert call(q, h, rays, n, o.ptrs, None) == ARG and error(h) == NO_FRAME.encode()
    assert call(q, None, r, N, o.ptrs, f) == ARG   # no context: no message to keep
    assert o.untouched()


@pytest.mark.parametrize("q", list(QUERIES))
def test_gpu_entry_points_refuse_the_cpu_context(cpu, q):
    o = Out(q)
    assert call(q, cpu._h, RAYS.ctypes.data, N, o.ptrs, frame(), prefix="rt_") == STATE
    assert call(q, cpu._h, RAYS.ctypes.data, N, o.ptrs, frame(), prefix="rt_", tail=(None,)) == STATE
    assert call(q, cpu._h, RAYS.ctypes.data, 0, o.ptrs, frame(), prefix="rt_") == STATE   # before the count
    assert o.untouched()


@pytest.mark.parametrize("q", list(QUERIES))
def test_good_call_fills_the_whole_record_and_n0_leaves_it(cpu, q):
    """After a good call: the query's counter is n, the kernel is the cpu_ name, kernel_ms the timer's,
    every other counter 0.  Then n == 0 (with null pointers too): RT_OK, nothing written, the record
    as the good call left it — and a refused call leaves it too."""
    o = Out(q)
    h, r, f = cpu._h, RAYS.ctypes.data, frame()
    other = "filter" if q == "trace" else "trace"   # the record is reset, not added to
    assert call(other, h, r, N, Out(other).ptrs, f) == 0
    assert call(q, h, r, N, o.ptrs, f) == 0
    assert not any((a == SENTINEL).any() for a in o.arrays)
    st = stats(h)
    counter = {"trace": "bounce_rays", "filter": "shadow_rays", "shade": "primary_rays"}[q]
    assert st.kernel == "cpu_" + QUERIES[q][0][3:] and st.kernel_ms >= 0
    assert {k: getattr(st, k) for k in COUNTERS} == {k: (N if k == counter else 0) for k in COUNTERS}
    assert st.kernel_name == st.kernel.encode() and bytes(st)[-48:].rstrip(b"\0") == st.kernel.encode()
    before = record(st)
    z = Out(q)
    assert call(q, h, r, 0, z.ptrs, f) == 0 and z.untouched()
    assert call(q, h, None, 0, [None] * len(z.ptrs), f) == 0
    assert record(stats(h)) == before
    assert call(q, h, r, -1, z.ptrs, f) == ARG and record(stats(h)) == before and z.untouched()


def test_outputs_are_the_scene_s(cpu):
    """(the scene is what the header says: the rays hit all three surfaces and the background)"""
    got = cpu.trace_rays(RAYS)
    assert got["id"].tolist() == [0, 0, 2, 2, 1, 1, -1, -1]
    rgb = cpu.shade_rays(RAYS, frame())
    assert np.array_equal(rgb[got["id"] == -1], np.tile(F([0.1, 0.2, 0.3]), ((got["id"] == -1).sum(), 1)))
