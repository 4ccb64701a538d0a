"""The expected colour of an arbitrary ray (include/rt.h rt_shade_rays), never
computed by the code under test: the oracle's own pixel loop, pointed along
the ray.

A camera with a zero film — half_w = half_h = 0, inv_w = inv_h = 1, one pixel
— and an orientation that is all zeros except row 2 = (-Rx, -Ry, -Rz, 0) makes
pixel(0, 0) of oracle/rt_oracle.c build the direction v3_normaliser(R): the
film point is (-0, -0, -1), v3_xform gives R, and oracle_render_window(0, 1,
0, 1) returns obtenir_couleur of the CRayon (O, that direction, energy 1, 0
bounces, IOR 1).  aov_ref.camera_dirs applied to the same camera restates
those steps in float32 and returns exactly that direction (unit_dirs): that D
is what the product is handed.  ref_set_camera / ref_render_window of
oracle/_ref have the same shape and feed the committed fixture
(tests/golden/make_shade_golden.py).
"""
from __future__ import annotations

import ctypes

import numpy as np

import aov_ref

F = np.float32
VP = ctypes.c_void_p
_CAM_ARGS = [VP, VP, VP, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_int]


def orient_of(r) -> np.ndarray:
    """The 16 orientation words whose row 2 is (-Rx, -Ry, -Rz, 0)."""
    m = np.zeros(16, F)
    m[8:11] = -np.asarray(r, F)
    return m


def unit_dirs(raw) -> np.ndarray:
    """v3_normaliser(R) per row of raw, by aov_ref.camera_dirs on the
    zero-film camera: the D the oracle shades (zero where |R| <= EPSILON, NaN
    where R holds a NaN or an inf)."""
    raw = np.ascontiguousarray(raw, F).reshape(-1, 3)
    out = np.zeros_like(raw)
    with np.errstate(invalid="ignore", over="ignore"):
        for k, r in enumerate(raw):
            cam = aov_ref.Cam(np.zeros(3, F), orient_of(r), 0, 0, 1, 1)
            out[k] = aov_ref.camera_dirs(cam, [0], [0])[0]
    return np.ascontiguousarray(out)


def shade_with(set_camera, render_pixel, O, raw) -> np.ndarray:
    """(N, 3) float32: one zero-film camera and one pixel per ray.
    set_camera(pos_addr, orient_addr); render_pixel(out_addr)."""
    O = np.ascontiguousarray(O, F).reshape(-1, 3)
    raw = np.ascontiguousarray(raw, F).reshape(-1, 3)
    assert O.shape == raw.shape
    out = np.zeros((len(O), 3), F)
    for k in range(len(O)):
        m = orient_of(raw[k])
        set_camera(O.ctypes.data + 12 * k, m.ctypes.data)
        render_pixel(out.ctypes.data + 12 * k)
    return out


def oracle_shade(oracle, path, depth, min_energy, scene_ior, O, raw) -> np.ndarray:
    """obtenir_couleur of (O[k], v3_normaliser(raw[k])) through liboracle.so
    (conftest.Oracle), with the given bounce depth, energy threshold and index
    of refraction; the background is the file's."""
    L = oracle.L
    L.oracle_set_camera.argtypes = _CAM_ARGS
    rc, p = oracle.load(path, 1, 1, depth)
    assert rc == 0, (path, rc)
    try:
        L.oracle_set_params(p, int(depth), float(min_energy), float(scene_ior))

        def set_camera(pos, orient):
            assert L.oracle_set_camera(p, pos, orient, 0.0, 0.0, 1.0, 1.0, 1, 1) == 0

        def render_pixel(out):
            assert L.oracle_render_window(p, 0, 1, 0, 1, out, 1) == 0

        return shade_with(set_camera, render_pixel, O, raw)
    finally:
        L.oracle_free(p)


def ref_shade(L, path, depth, O, raw) -> np.ndarray:
    """The same through oracle/_ref (the reference's own code; default
    min_energy and index of refraction): for the fixture generator."""
    L.ref_set_camera.argtypes = _CAM_ARGS
    p = VP()
    assert L.ref_load(path.encode(), 1, 1, int(depth), ctypes.byref(p)) == 0
    try:
        return shade_with(lambda pos, orient: L.ref_set_camera(p, pos, orient, 0.0, 0.0, 1.0, 1.0, 1, 1),
                          lambda out: L.ref_render_window(p, 0, 1, 0, 1, out), O, raw)
    finally:
        L.ref_free(p)


def colours_differ(got, want, label: str = "") -> list:
    """Word for word as uint32 (where the expectation is NaN the result is
    NaN); returns a description of the difference, or []."""
    a = np.ascontiguousarray(got, F)
    b = np.ascontiguousarray(want, F)
    if a.shape != b.shape:
        return [f"{label}: shape {a.shape} != {b.shape}"]
    d = ((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).any(-1) if a.size else np.zeros(0, bool)
    return [f"{label}: {int(d.sum())} of {d.size} colours differ, first at {int(np.argmax(d))}"] if d.any() else []
