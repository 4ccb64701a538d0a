"""The expected primary-hit AOVs (include/rt.h rt_render_aov), never computed
by the code under test.

The camera ray is restated here in explicit float32 steps — pixel()'s two
lines, then v3_xform and v3_normaliser of oracle/rt_oracle.c (Scene.cpp:
1543-1552) — and the winner is CScene::ObtenirCouleur's loop (Scene.cpp:
1705-1715) over a PER-PRIMITIVE intersect function applied to the dumped
post-Pretraitement geometry (oracle_dump / ref_dump rows):

    surface i replaces the winner when  t_i > EPSILON && (t_i < t_best || t_best < 0)

The intersect function is `oracle_intersect` of liboracle.so at test time
(the `oracle` fixture) and `ref_intersect` of oracle/_ref for the committed
fixture (tests/golden/make_aov_golden.py): both take
(type, geom12*, origin3*, dir3*, t_out*, n_out*) with every pointer argument
declared c_void_p, so plain addresses are passed.

A miss is the reference's empty CIntersection (Intersection.cpp:17-18):
id -1, t -1, n (0, 0, 0).
"""
from __future__ import annotations

import ctypes

import numpy as np

F = np.float32
EPS = F(1.0e-2)  # MathUtils.h:35 EPSILON


class Cam:
    """The camera words the pixel loop reads: position, orientation m[i][j],
    film half extents and pixel reciprocals, all float32."""

    def __init__(self, pos, orient, half_w, half_h, inv_w, inv_h):
        self.pos = np.ascontiguousarray(pos, F).reshape(3)
        self.m = np.ascontiguousarray(orient, F).reshape(4, 4)
        self.half_w, self.half_h, self.inv_w, self.inv_h = F(half_w), F(half_h), F(inv_w), F(inv_h)

    @classmethod
    def from_words(cls, c):
        """From an oracle_dump / ref_dump camera row (27 words)."""
        c = np.asarray(c, F)
        return cls(c[0:3], c[3:19], c[20], c[21], c[22], c[23])

    @classmethod
    def from_frame(cls, f):
        """From an rt_frame (a moved camera: the words the caller hands every backend)."""
        return cls(f.cam_pos[:], f.orient[:], f.half_w, f.half_h, f.inv_w, f.inv_h)


def camera_dirs(cam: Cam, xs, ys) -> np.ndarray:
    """Ray directions of pixels (xs[k], ys[k]): one float32 operation per step."""
    xs = np.asarray(xs, np.int64)
    ys = np.asarray(ys, np.int64)
    one = F(1)
    # v3((2 * px * inv_w - 1) * half_w, (2 * py * inv_h - 1) * half_h, -1): 2 * px is an int
    dx = ((2 * xs).astype(F) * cam.inv_w - one) * cam.half_w
    dy = ((2 * ys).astype(F) * cam.inv_h - one) * cam.half_h
    dz = np.full(dx.shape, -1, F)
    m = cam.m
    # v3_xform: m[0][j] x + m[1][j] y + m[2][j] z + m[3][j], left to right
    r = [((m[0, j] * dx + m[1, j] * dy) + m[2, j] * dz) + m[3, j] for j in range(3)]
    # v3_normaliser: ZERO if the length is <= EPSILON, else v * (1 / len)
    ln = np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
    assert ln.dtype == F
    ok = ln > EPS
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = one / ln
    out = np.stack([np.where(ok, c * inv, F(0)) for c in r], -1).astype(F)
    return np.ascontiguousarray(out)


class Surfaces:
    """Dumped post-Pretraitement surfaces (rows of 24 words) as the intersect
    function takes them: type and the 12 geometry words [11..22]."""

    def __init__(self, surf):
        surf = np.asarray(surf, F)
        self.n = surf.shape[0]
        self.types = [int(v) for v in surf[:, 0]]
        self.geom = np.ascontiguousarray(surf[:, 11:23], F)
        self._ga = [self.geom.ctypes.data + 48 * i for i in range(self.n)]
        self.t = np.zeros(max(self.n, 1), F)
        self.nrm = np.zeros((max(self.n, 1), 3), F)
        self._ta = [self.t.ctypes.data + 4 * i for i in range(self.n)]
        self._na = [self.nrm.ctypes.data + 12 * i for i in range(self.n)]

    def intersect_all(self, isect, o_addr: int, d_addr: int):
        """Every surface against one ray: fills self.t / self.nrm in file order."""
        for ty, g, t, n in zip(self.types, self._ga, self._ta, self._na):
            isect(ty, g, o_addr, d_addr, t, n)


def winner(t: np.ndarray) -> int:
    """ObtenirCouleur's loop over the distances in file order: the first index
    of the smallest t above EPSILON (a tie keeps the earlier surface; a NaN
    never passes t > EPSILON); -1: none."""
    with np.errstate(invalid="ignore"):
        valid = t > EPS
    if not valid.any():
        return -1
    tmin = t[valid].min()
    return int(np.argmax(valid & (t == tmin)))


def aov_pixels(isect, surf, cam: Cam, xs, ys):
    """(id, t, n, D) of the given pixels: int32 (N,), float32 (N,), (N, 3), (N, 3)."""
    S = surf if isinstance(surf, Surfaces) else Surfaces(surf)
    D = camera_dirs(cam, xs, ys)
    N = D.shape[0]
    ids = np.full(N, -1, np.int32)
    ts = np.full(N, -1, F)
    ns = np.zeros((N, 3), F)
    oa, da = cam.pos.ctypes.data, D.ctypes.data
    for k in range(N):
        S.intersect_all(isect, oa, da + 12 * k)
        i = winner(S.t[: S.n])
        if i >= 0:
            ids[k], ts[k], ns[k] = i, S.t[i], S.nrm[i]
    return ids, ts, ns, D


def aov_frame(isect, surf, cam: Cam, width: int, rows):
    """The planes of frame rows `rows` (an iterable of PixY, packed in that
    order): {"id": (R, W) int32, "t": (R, W), "n": (R, W, 3)}."""
    rows = list(rows)
    ys, xs = np.meshgrid(np.asarray(rows, np.int64), np.arange(width), indexing="ij")
    ids, ts, ns, _ = aov_pixels(isect, surf, cam, xs.ravel(), ys.ravel())
    R = len(rows)
    return {"id": ids.reshape(R, width), "t": ts.reshape(R, width), "n": ns.reshape(R, width, 3)}


def oracle_aov(oracle, path: str, w: int, h: int, rows=None, frame=None):
    """aov_frame through liboracle.so: geometry and camera from oracle_dump
    (frame: a moved camera's rt_frame instead of the file's)."""
    surf, cam, _ = oracle.dump(path, w, h)
    c = Cam.from_frame(frame) if frame is not None else Cam.from_words(cam)
    return aov_frame(oracle.L.oracle_intersect, surf, c, w, range(h) if rows is None else rows)


def planes_equal(got: dict, want: dict, keys=("id", "t", "n")):
    """Bit for bit; returns the list of planes that differ (with a count)."""
    bad = []
    for k in keys:
        a = np.ascontiguousarray(got[k])
        b = np.ascontiguousarray(want[k])
        if a.shape != b.shape or a.dtype != b.dtype:
            bad.append(f"{k}: shape/dtype {a.shape} {a.dtype} != {b.shape} {b.dtype}")
            continue
        d = a.view(np.uint32) != b.view(np.uint32)
        if d.any():
            bad.append(f"{k}: {int(d.sum())} of {d.size} words differ")
    return bad


# The 64 sparse pixels of a 64 x 32 frame (tests/golden/aov.npz hf50k_*):
# pixel k sits at in-tile position k of an 8 x 8 tile (lane k of its wave) and
# every one of the 32 tiles is used twice, dealt by a seeded shuffle.
def sparse_pixels(seed: int, width: int = 64, height: int = 32):
    tx, ty = width // 8, height // 8
    tiles = np.repeat(np.arange(tx * ty), 64 // (tx * ty))
    assert tiles.size == 64
    np.random.default_rng(seed).shuffle(tiles)
    k = np.arange(64)
    xs = (tiles % tx) * 8 + (k & 7)
    ys = (tiles // tx) * 8 + (k >> 3)
    return xs.astype(np.int32), ys.astype(np.int32)


def libm_powf():
    L = ctypes.CDLL("libm.so.6")
    L.powf.restype = ctypes.c_float
    L.powf.argtypes = [ctypes.c_float, ctypes.c_float]
    return L.powf
