"""Seeded ray sets and the scenes they are traced in, shared by the ray-query
tests (test_rays_cpu.py, test_gpu_rays.py) and the fixture generator
(tests/golden/make_rays_golden.py): all three build the very same rays.

Base set (n rays, default_rng(seed)):
 1. n / 2 random pixels of the scene's own 64 x 32 camera;
 2. their primary-hit points (aov_ref.aov_pixels; a miss counts as the point
    at t = 100);
 3. origins uniform in the bounding box of the triangle vertices, those points
    and the camera, grown by 25 % per side;
 4. the first half of the directions aim at those points, the second half is
    uniform on the sphere;
 5. normalised in float64, then cast to float32.
Conditions on every base case (conditions()): hit share within [0.25, 0.95],
winners of at least 2 surface kinds, at least 20 distinct winners where the
scene has 60 or more surfaces.  A scene that falls outside takes another seed
(BASE_SEED); the bounds stay.

Derived sets (derived()), each compared in full, no share condition:
 leaving     rays leaving the base set's hit points along the mirrored
             direction, the origin float32(O + t D): the t > EPSILON self-hit
             rejection;
 axis        directions with one or two exact zeros;
 scaled3 / scaled025   non-unit directions (t scales, id does not — the
             expectation still comes from the oracle, not from that rule);
 zero        the zero direction;
 nonfinite   NaN or inf in O or D on every fourth ray, so that every wave of
             64 holds finite and non-finite rays.
"""
from __future__ import annotations

import os

import numpy as np

import aov_ref

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
W, H = 64, 32  # the camera the base set's pixels come from
N_BASE = 256
HF50K_RAYS = 128  # the 50k heightfield: its fixture's rays only

# name -> (kind, arguments); file(): its .dat on disk
SCENES = {f"scene{i}": ("file", i) for i in range(1, 10)}
SCENES.update({f"mixed{n}": ("wf", "mixed", n) for n in (63, 64, 65)})
SCENES.update({"soup1100": ("wf", "soup", 1100), "ties3": ("ties", 3), "ties1026": ("ties", 1026),
               "hf1600": ("hf", 40, 20), "hf50k": ("hf", 250, 100)})
# The base set's seed per scene: 5 unless the conditions ask for another.
BASE_SEED = {}


def scene_text(name: str):
    """The scene's .dat text (None: a committed file)."""
    kind, *a = SCENES[name]
    if kind == "file":
        return None
    if kind == "wf":
        import wf_scenes

        return wf_scenes.wf_dat(a[0], a[1])
    if kind == "ties":
        import hard_scenes

        return hard_scenes.hard_dat("ties", 0, a[0])
    from rt_amd import synth

    return synth.heightfield_dat(a[0], a[1])


def file(name: str, tmpdir: str) -> str:
    text = scene_text(name)
    if text is None:
        return os.path.join(HERE, "golden", "scenes", f"scene{SCENES[name][1]}.dat")
    path = os.path.join(tmpdir, f"rays_{name}.dat")
    if not (os.path.exists(path) and open(path).read() == text):
        with open(path, "w") as f:
            f.write(text)
    return path


def _unit(v):
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.linalg.norm(v, axis=-1, keepdims=True)


def base_set(isect, surf, cam_words, n: int = N_BASE, seed: int = 5) -> np.ndarray:
    """(n, 6) float32; surf / cam_words: the scene's dump at W x H."""
    rng = np.random.default_rng(seed)
    h = n // 2
    xs, ys = rng.integers(0, W, h), rng.integers(0, H, h)
    cam = aov_ref.Cam.from_words(cam_words)
    ids, ts, _, D = aov_ref.aov_pixels(isect, surf, cam, xs, ys)
    t = np.where((ids >= 0) & np.isfinite(ts), ts, F(100)).astype(np.float64)
    P = cam.pos.astype(np.float64) + t[:, None] * D.astype(np.float64)
    rows = np.asarray(surf, F)  # the dump's rows: type, ..., geometry words [11..22]
    verts = rows[rows[:, 0].astype(int) == 0][:, 11:20].reshape(-1, 3).astype(np.float64)
    pts = np.concatenate([verts, P, cam.pos.astype(np.float64)[None]])
    lo, hi = pts.min(0), pts.max(0)
    lo, hi = lo - 0.25 * (hi - lo), hi + 0.25 * (hi - lo)
    O = rng.uniform(lo, hi, (n, 3))
    Dn = np.concatenate([_unit(P - O[:h]), _unit(rng.normal(size=(n - h, 3)))])
    rays = np.concatenate([O, Dn], 1).astype(F)
    assert np.isfinite(rays).all()
    return np.ascontiguousarray(rays)


def conditions(want: dict, types) -> dict:
    """The base case's figures: hit share, surface kinds among the winners,
    distinct winners."""
    ids = want["id"]
    hit = ids >= 0
    types = np.asarray(types, int)
    return {"share": float(hit.mean()), "kinds": len(set(types[ids[hit]].tolist())),
            "distinct": len(set(ids[hit].tolist())), "surfaces": len(types)}


def check_conditions(c: dict, name: str = ""):
    assert 0.25 <= c["share"] <= 0.95, (name, c)
    assert c["kinds"] >= 2, (name, c)
    assert c["surfaces"] < 60 or c["distinct"] >= 20, (name, c)


_NONFINITE = [(0, np.nan), (4, np.inf), (2, -np.inf), (3, np.nan), (1, np.inf), (5, -np.inf)]


def derived(base: np.ndarray, want: dict) -> dict:
    """name -> (N, 6) float32 rays from the base rays and their expected hits."""
    base = np.ascontiguousarray(base, F)
    n = base.shape[0]
    O, D = base[:, :3].astype(np.float64), base[:, 3:].astype(np.float64)
    out = {}
    # leaving the hit points along the mirrored direction
    N = want["n"].astype(np.float64)
    ok = (want["id"] >= 0) & np.isfinite(want["t"]) & np.isfinite(N).all(1)
    P = (O + want["t"].astype(np.float64)[:, None] * D)[ok]
    R = D[ok] - 2.0 * (D[ok] * N[ok]).sum(1, keepdims=True) * N[ok]
    out["leaving"] = np.concatenate([P, _unit(R)], 1).astype(F)
    # one or two exact zeros in the direction
    A = D.copy()
    for k in range(n):
        p = k % 6
        if p < 3:
            A[k, p] = 0.0
        else:
            A[k, [c for c in range(3) if c != p - 3]] = 0.0
            if A[k, p - 3] == 0.0:
                A[k, p - 3] = 1.0
    out["axis"] = np.concatenate([O, _unit(A)], 1).astype(F)
    assert ((out["axis"][:, 3:] == 0).sum(1) >= 1).all() and ((out["axis"][:, 3:] == 0).sum(1) == 2).any()
    # non-unit directions
    for label, s in (("scaled3", 3.0), ("scaled025", 0.25)):
        r = base.copy()
        r[:, 3:] = (base[:, 3:] * F(s)).astype(F)
        out[label] = r
    # the zero direction
    r = base[:64].copy()
    r[:, 3:] = 0.0
    r[1::2, 3:] = -0.0
    out["zero"] = r
    # NaN / inf in O or D, interleaved with finite rays
    r = base.copy()
    for j, k in enumerate(range(1, n, 4)):
        c, v = _NONFINITE[j % len(_NONFINITE)]
        r[k, c] = v
    out["nonfinite"] = r
    for k0 in range(0, n - 63, 64):
        fin = np.isfinite(r[k0:k0 + 64]).all(1)
        assert fin.any() and not fin.all()
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


_CASES = {}


def cases(oracle, name: str, tmpdir: str) -> dict:
    """{"path", "types", "sets": {set name: (rays, expected hits)}} of a scene,
    through liboracle.so (conftest.Oracle); computed once per process."""
    import rays_ref

    if name not in _CASES:
        path = file(name, tmpdir)
        surf, cam, _ = oracle.dump(path, W, H)
        S = aov_ref.Surfaces(surf)
        isect = oracle.L.oracle_intersect
        base = base_set(isect, surf, cam, seed=BASE_SEED.get(name, 5))
        want = rays_ref.trace(isect, S, base)
        sets = {"base": (base, want)}
        for k, r in derived(base, want).items():
            sets[k] = (r, rays_ref.trace(isect, S, r))
        _CASES[name] = {"path": path, "types": surf[:, 0].astype(int), "sets": sets}
    return _CASES[name]
