"""The expected shadow filters of arbitrary segments (include/rt.h
rt_filter_rays), never computed by the code under test.

CScene::ObtenirFiltreDeSurface (Scene.cpp:1842-1861) in explicit float32
steps, as oracle/rt_oracle.c spells it (filtre, v3_norme, v3_div):

    dist = sqrtf((Lx*Lx + Ly*Ly) + Lz*Lz);  inv = 1.0f / dist;  D = L * inv
    F = (1, 1, 1)
    for every surface i in file order:  t_i = Intersection(P, D)
        if (t_i > EPSILON && t_i < dist)  F *= colour_i * Kt_i

over a PER-PRIMITIVE intersect function applied to the dumped
post-Pretraitement surfaces (oracle_dump / ref_dump rows: words 1-3 colour,
9 Kt, 11-22 geometry; aov_ref.Surfaces.intersect_all).  The intersect function
is `oracle_intersect` of liboracle.so at test time and `ref_intersect` of
oracle/_ref for the committed fixture tests/golden/filter.npz
(tests/golden/make_filter_golden.py).  No special cases: a NaN stays a NaN.
"""
from __future__ import annotations

import numpy as np

import aov_ref

F = np.float32
EPS = aov_ref.EPS


def factors(surf) -> np.ndarray:
    """colour x Kt per surface, (n, 3) float32 (Scene.cpp:1855: the colour scaled first)."""
    s = np.asarray(surf, F)
    return np.ascontiguousarray(s[:, 1:4] * s[:, 9:10], F)


def directions(segs):
    """(dist (N,), D (N, 3)) of the (N, 6) float32 segments: v3_norme and v3_div."""
    L = np.ascontiguousarray(segs, F)[:, 3:6]
    with np.errstate(all="ignore"):
        dist = np.sqrt((L[:, 0] * L[:, 0] + L[:, 1] * L[:, 1]) + L[:, 2] * L[:, 2])
        inv = F(1) / dist
        D = L * inv[:, None]
    assert dist.dtype == F and D.dtype == F
    return dist, np.ascontiguousarray(D)


def detail(isect, surf, segs) -> dict:
    """{"filter": (N, 3) float32, "count": (N,) factors multiplied, "reverse":
    (N, 3) the same factors multiplied in REVERSE file order} — the last two
    for the conditions the tests put on their own inputs."""
    S = aov_ref.Surfaces(surf)
    fc = factors(surf)
    s = np.ascontiguousarray(segs, F)
    assert s.ndim == 2 and s.shape[1] == 6
    N = s.shape[0]
    dist, D = directions(s)
    P = np.ascontiguousarray(s[:, 0:3])
    out = np.ones((N, 3), F)
    rev = np.ones((N, 3), F)
    count = np.zeros(N, np.int32)
    pa, da = P.ctypes.data, D.ctypes.data
    with np.errstate(all="ignore"):
        for k in range(N):
            S.intersect_all(isect, pa + 12 * k, da + 12 * k)
            t = S.t[: S.n]
            hit = np.flatnonzero((t > EPS) & (t < dist[k]))
            count[k] = hit.size
            f = np.ones(3, F)
            for i in hit:
                f = f * fc[i]
            out[k] = f
            f = np.ones(3, F)
            for i in hit[::-1]:
                f = f * fc[i]
            rev[k] = f
    return {"filter": out, "count": count, "reverse": rev}


def filters(isect, surf, segs) -> np.ndarray:
    """(N, 3) float32: the filter of each (N, 6) float32 segment [Px Py Pz Lx Ly Lz]."""
    return detail(isect, surf, segs)["filter"]


def differ(got, want):
    """The comparison rule: word for word as uint32, except that where the
    expectation is NaN the result must be NaN (any payload).  Returns a list of
    messages (empty: equal)."""
    a = np.ascontiguousarray(got)
    b = np.ascontiguousarray(want)
    if a.shape != b.shape or a.dtype != np.float32 or b.dtype != np.float32:
        return [f"shape/dtype {a.shape} {a.dtype} != {b.shape} {b.dtype}"]
    d = a.view(np.uint32) != b.view(np.uint32)
    d &= ~(np.isnan(a) & np.isnan(b))
    if not d.any():
        return []
    first = np.argwhere(d)[0]
    return [f"{int(d.sum())} of {d.size} words differ, first at {tuple(int(v) for v in first)}: "
            f"{a[tuple(first)]!r} != {b[tuple(first)]!r}"]
