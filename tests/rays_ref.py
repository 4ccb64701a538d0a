"""The expected closest hits of arbitrary rays (include/rt.h rt_trace_rays),
never computed by the code under test.

CScene::ObtenirCouleur's loop (Scene.cpp:1705-1715) — aov_ref.winner — over a
PER-PRIMITIVE intersect function applied to the dumped post-Pretraitement
geometry (aov_ref.Surfaces.intersect_all), for an origin and a direction the
caller chooses; the direction is handed over as given (CRayon::AjusterDirection
does not normalise).  The intersect function is `oracle_intersect` of
liboracle.so at test time and `ref_intersect` of oracle/_ref for the committed
fixture tests/golden/rays.npz (tests/golden/make_rays_golden.py).

A miss is the reference's empty CIntersection: id -1, t -1, n (0, 0, 0).
"""
from __future__ import annotations

import numpy as np

import aov_ref

F = np.float32


def trace(isect, surf, rays) -> dict:
    """{"id": (N,) int32, "t": (N,) float32, "n": (N, 3) float32} of the (N, 6)
    float32 rays [Ox Oy Oz Dx Dy Dz]."""
    S = surf if isinstance(surf, aov_ref.Surfaces) else aov_ref.Surfaces(surf)
    r = np.ascontiguousarray(rays, F)
    assert r.ndim == 2 and r.shape[1] == 6
    N = r.shape[0]
    ids = np.full(N, -1, np.int32)
    ts = np.full(N, -1, F)
    ns = np.zeros((N, 3), F)
    base = r.ctypes.data
    for k in range(N):
        S.intersect_all(isect, base + 24 * k, base + 24 * k + 12)
        i = aov_ref.winner(S.t[: S.n])
        if i >= 0:
            ids[k], ts[k], ns[k] = i, S.t[i], S.nrm[i]
    return {"id": ids, "t": ts, "n": ns}


def hits_differ(got: dict, want: dict, keys=("id", "t", "n")):
    """The comparison rule: id equal; t and n word for word as uint32, except
    that where the expectation is NaN the result must be NaN (any payload).
    Returns the list of planes that differ (with a count)."""
    bad = []
    for k in keys:
        a = np.ascontiguousarray(got[k])
        b = np.ascontiguousarray(want[k])
        if a.shape != b.shape or a.dtype != b.dtype:
            bad.append(f"{k}: shape/dtype {a.shape} {a.dtype} != {b.shape} {b.dtype}")
            continue
        d = a.view(np.uint32) != b.view(np.uint32)
        if k != "id":
            d &= ~(np.isnan(a) & np.isnan(b))
        if d.any():
            first = np.argwhere(d)[0]
            bad.append(f"{k}: {int(d.sum())} of {d.size} words differ, first at {tuple(int(v) for v in first)}: "
                       f"{a[tuple(first)]!r} != {b[tuple(first)]!r}")
    return bad
