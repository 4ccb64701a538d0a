"""The expected image of an adaptive supersampled render (include/rt.h
rt_render_adaptive*), in numpy from REFERENCE data only — the reference's (or
the oracle's) frame S of the sample grid and the oracle's primary-hit planes
(aov_ref.oracle_aov) — never from the code under test.

For s = 2, 4, 8 the base frame B is the sample lattice S[::s, ::s] bit for bit
(inv_w s is exact), so
    mask    = mask(S[::s, ::s], ids, normals, criteria, cos, delta)
    image   = compose(S, s, mask) = where(mask, ssaa_ref.box(S, s), S[::s, ::s])
Every step is one float32 operation."""
from __future__ import annotations

import numpy as np

from aov_ref import oracle_aov
from ssaa_ref import box

F = np.float32
EDGE_ID, EDGE_NORMAL, EDGE_COLOUR = 1, 2, 4
ALL = EDGE_ID | EDGE_NORMAL | EDGE_COLOUR


def _pair(base, ids, normals, p, q, criteria, cos, delta):
    """The criteria separating the pixels of view p from those of view q
    (p, q: index tuples selecting the two sides of every neighbour pair)."""
    m = np.zeros(ids[p].shape if ids is not None else base[p].shape[:2], np.uint8)
    if criteria & (EDGE_ID | EDGE_NORMAL):
        ip, iq = ids[p], ids[q]
        if criteria & EDGE_ID:
            m |= np.where(ip != iq, EDGE_ID, 0).astype(np.uint8)
        if criteria & EDGE_NORMAL:
            a, b = normals[p].astype(F), normals[q].astype(F)
            dot = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
            assert dot.dtype == F
            with np.errstate(invalid="ignore"):
                bent = (ip >= 0) & (iq >= 0) & (dot < F(cos))
            m |= np.where(((ip < 0) != (iq < 0)) | bent, EDGE_NORMAL, 0).astype(np.uint8)
    if criteria & EDGE_COLOUR:
        with np.errstate(invalid="ignore"):
            d = np.abs(base[p].astype(F) - base[q].astype(F))
            assert d.dtype == F
            m |= np.where((d > F(delta)).any(-1), EDGE_COLOUR, 0).astype(np.uint8)
    return m


def mask(base, ids, normals, criteria, cos, delta) -> np.ndarray:
    """mask(p) of every pixel of the WHOLE base frame: (H, W) uint8 of EDGE_*
    bits, the OR over the 4-neighbours inside the frame.  base (H, W, 3)
    float32; ids (H, W) int32 (-1: a miss); normals (H, W, 3) float32.  Every
    criterion is symmetric in p and q (a b == b a in IEEE), so each pair is
    evaluated once and marks both of its pixels."""
    h, w = base.shape[:2]
    out = np.zeros((h, w), np.uint8)
    left, right = (slice(None), slice(0, w - 1)), (slice(None), slice(1, w))
    m = _pair(base, ids, normals, left, right, criteria, cos, delta)
    out[left] |= m
    out[right] |= m
    low, high = (slice(0, h - 1), slice(None)), (slice(1, h), slice(None))
    m = _pair(base, ids, normals, low, high, criteria, cos, delta)
    out[low] |= m
    out[high] |= m
    return out


def compose(S, s: int, m) -> np.ndarray:
    """The expected float image: the boxed samples where the mask is set, the lattice sample elsewhere."""
    S = np.ascontiguousarray(S, F)
    return np.where((np.asarray(m) != 0)[..., None], box(S, s), S[::s, ::s]).astype(F)


_AOV = {}


def planes(oracle, path: str, w: int, h: int, key=None):
    """The oracle's primary-hit planes of the w x h frame of `path` (cached:
    they do not depend on the bounce depth)."""
    k = key or (path, w, h)
    if k not in _AOV:
        _AOV[k] = oracle_aov(oracle, path, w, h)
    return _AOV[k]


def expect(oracle, path: str, S, s: int, criteria: int, cos=0.9, delta=0.1, key=None):
    """(image, mask) expected from sample frame S (s H x s W x 3) of `path`."""
    S = np.ascontiguousarray(S, F)
    h, w = S.shape[0] // s, S.shape[1] // s
    a = planes(oracle, path, w, h, key)
    m = mask(S[::s, ::s], a["id"], a["n"], criteria, cos, delta)
    return compose(S, s, m), m
