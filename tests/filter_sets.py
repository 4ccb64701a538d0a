"""The scenes and the seeded segment sets of the shadow-filter query tests
(test_filter_cpu.py, test_gpu_filter.py) and of the fixture generator
(tests/golden/make_filter_golden.py): all three build the very same segments.

Scenes (SCENES): ray_sets' scene1 .. scene9, mixed63 / 64 / 65, soup1100,
ties3, ties1026 (uploaded with ray_bvh = 1) and hf1600, and
 neg6        tests/golden/scenes/scene6.dat read at run time with every
             `refract:` coefficient negated: negative factors, shadow_split 0;
 layers      4 horizontal sheets at y = 0, 8, 16, 24 over x, z in [-40, 40],
             4 x 4 cells x 2 triangles each, the file order interleaving the
             sheets triangle by triangle, a random colour per triangle,
             `refract:` 0.9 / 0.7 / 0.8 / 0.6 (ior 1.3) by sheet, the top
             sheet's cells with (i + j) even opaque, a ground plane, a
             translucent sphere, two lights: 130 surfaces, 128 triangles, 113
             translucent;
 layers10    the same with 10 sheets (only the top one half opaque): an
             unoccluded crossing meets more than 8 translucent triangles;
 layers_neg  layers with the second sheet's coefficient negative: a scene with
             the BVH whose product still needs every factor in file order.

Segment sets per scene, from the 256 base rays of ray_sets.base_set [O D] and
their expected closest hit distance t (rays_ref.trace; 100 for a miss):
 through    L = D (1.5 t)        the segment passes the first surface
 short      L = D (0.5 t)        it ends in front of it
 touch      L = float32(t D)     the end point lies on the surface: the
                                 boundary of t < dist
 lights     from the float32 hit points float32(O + t D) to each of the first
            two lights: the renderer's own shadow rays, and the t > EPSILON
            self-hit rejection
 axis       `through` with one or two exact zeros in L
 zero       L = +0 / -0
 nonfinite  `through` with NaN / +-inf in P or L on every fourth segment
 scaled     `through` with L x 1e-30 and x 1e30, alternating: dist under- and
            overflows
 cross      (layers* only) 256 segments between random points below the
            lowest and above the highest sheet, every second one downwards
"""
from __future__ import annotations

import os

import numpy as np

import aov_ref
import filter_ref
import ray_sets
import rays_ref

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
W, H = ray_sets.W, ray_sets.H

RAY_SCENES = [f"scene{i}" for i in range(1, 10)] + ["mixed63", "mixed64", "mixed65", "soup1100", "ties3", "ties1026",
                                                      "hf1600"]
SCENES = RAY_SCENES + ["neg6", "layers", "layers10", "layers_neg"]
# upload options per scene (default: none)
OPTIONS = {"ties1026": {"ray_bvh": 1}}
# the scenes whose queries take rt_filter_kernel<1> (the BVH and only finite factors >= +0)
BVH_SCENES = ("mixed64", "mixed65", "soup1100", "ties1026", "layers", "layers10")
# scenes in which a translucent surface is hit
TINTED = ("scene5", "scene6", "scene7", "scene8", "mixed63", "mixed64", "mixed65")
LAYERS = {"layers": (4, None), "layers10": (10, None), "layers_neg": (4, 1)}  # sheets, the negative sheet
# The base set's seed per scene: ray_sets' unless the conditions ask for another.
BASE_SEED = {}
CROSS_SEED = 11
KT = (0.9, 0.7, 0.8, 0.6)


def layers_dat(sheets: int = 4, negative=None, seed: int = 3) -> str:
    rng = np.random.default_rng(seed)
    out = ["* shadow-filter test scene (tests/filter_sets.py): layers", "        background: 20 20 60",
           "        origin: 0.0 60.0 150.0", "        eye: 0.0 10.0 0.0", "        up:  0.0 1.0 0.0"]
    for i, (p, intens) in enumerate([((30.0, 120.0, 40.0), 0.7), ((-50.0, 100.0, -20.0), 0.4)]):
        out += [f"Lumiere: light_{i + 1}", "        position: %.3f %.3f %.3f" % p, "        intens:   %.3f" % intens]
    cells = [(i, j, h) for j in range(4) for i in range(4) for h in range(2)]
    for k, (i, j, h) in enumerate(cells):
        for s in range(sheets):
            y = 8.0 * s
            x0, x1, z0, z1 = -40.0 + 20.0 * i, -20.0 + 20.0 * i, -40.0 + 20.0 * j, -20.0 + 20.0 * j
            pts = [(x0, y, z0), (x1, y, z0), (x1, y, z1)] if h == 0 else [(x0, y, z0), (x1, y, z1), (x0, y, z1)]
            out.append(f"Poly: s{s}_t{k}")
            for q, p in enumerate(pts):
                out.append("        point: %d %.3f %.3f %.3f" % ((q,) + p))
            out.append("        color: %d %d %d" % tuple(int(v) for v in rng.integers(90, 256, 3)))
            if s == sheets - 1 and (i + j) % 2 == 0:
                continue  # opaque
            kt = KT[s % 4] * (-1.0 if s == negative else 1.0)
            out.append("        refract: %.3f 1.300" % kt)
    out += ["Plane: ground", "        v_linear: 0.0 1.0 0.0", "        v_const: 45.0", "        color: 10 200 10"]
    out += ["Quad: sphere", "        v_quad: 1.0 1.0 1.0", "        v_linear: 0.0 -24.0 0.0", "        v_const: 44.0",
            "        color: 230 200 250", "        refract: 0.500 1.400"]
    text = "\n".join(out) + "\n"
    assert max(len(l) for l in text.split("\n")) <= 78 and text.count("Poly:") == 32 * sheets
    return text


def neg6_dat() -> str:
    src = open(os.path.join(HERE, "golden", "scenes", "scene6.dat"), "rb").read().decode("latin-1")
    out, n = [], 0
    for line in src.split("\n"):
        if line.strip().startswith("refract:"):
            head, rest = line.split("refract:", 1)
            vals = rest.split()
            assert not vals[0].startswith("-")
            line = head + "refract:  -" + vals[0] + " " + " ".join(vals[1:])
            n += 1
        out.append(line)
    assert n >= 1
    return "\n".join(out)


def file(name: str, tmpdir: str) -> str:
    if name in RAY_SCENES:
        return ray_sets.file(name, tmpdir)
    text = neg6_dat() if name == "neg6" else layers_dat(*LAYERS[name])
    path = os.path.join(tmpdir, f"filter_{name}.dat")
    if not (os.path.exists(path) and open(path, encoding="latin-1", newline="").read() == text):
        with open(path, "w", encoding="latin-1", newline="") as f:
            f.write(text)
    return path


_NONFINITE = [(0, np.nan), (4, np.inf), (2, -np.inf), (3, np.nan), (1, np.inf), (5, -np.inf)]


def light_segments(rays, t, hit, lights, count: int = 2):
    """From the float32 hit points of the rays that hit to each of the first
    `count` lights: P = float32(O + t D) and L = light - P in float32 steps,
    as ObtenirCouleurSurIntersection forms them."""
    r = np.ascontiguousarray(rays, F)
    ok = hit & np.isfinite(t)
    P = (r[ok, :3] + t[ok, None].astype(F) * r[ok, 3:]).astype(F)
    out = [np.concatenate([P, (np.asarray(l[:3], F)[None] - P).astype(F)], 1) for l in lights[:count]]
    return np.ascontiguousarray(np.concatenate(out) if out else np.zeros((0, 6), F), F)


def segment_sets(base, want, lights) -> dict:
    """name -> (N, 6) float32 segments from the base rays [O D], their expected
    hits {"id", "t"} and the scene's light rows."""
    base = np.ascontiguousarray(base, F)
    n = base.shape[0]
    hit = want["id"] >= 0
    t = np.where(hit & np.isfinite(want["t"]), want["t"], F(100)).astype(F)
    O, D = base[:, :3], base[:, 3:]
    D64, t64 = D.astype(np.float64), t.astype(np.float64)[:, None]
    out = {}
    out["through"] = np.concatenate([O, (D64 * (1.5 * t64)).astype(F)], 1)
    out["short"] = np.concatenate([O, (D64 * (0.5 * t64)).astype(F)], 1)
    out["touch"] = np.concatenate([O, (t[:, None] * D).astype(F)], 1)
    out["lights"] = light_segments(base, want["t"], hit, lights)
    a = out["through"].copy()
    for k in range(n):
        p = k % 6
        if p < 3:
            a[k, 3 + p] = 0.0
        else:
            a[k, [3 + c for c in range(3) if c != p - 3]] = 0.0
            if a[k, p] == 0.0:
                a[k, p] = 1.0
    out["axis"] = a
    assert ((a[:, 3:] == 0).sum(1) >= 1).all() and ((a[:, 3:] == 0).sum(1) == 2).any()
    z = out["through"][:64].copy()
    z[:, 3:] = 0.0
    z[1::2, 3:] = -0.0
    out["zero"] = z
    r = out["through"].copy()
    for j, k in enumerate(range(1, n, 4)):
        c, v = _NONFINITE[j % len(_NONFINITE)]
        r[k, c] = v
    out["nonfinite"] = r
    for k0 in range(0, n - 63, 64):
        fin = np.isfinite(r[k0:k0 + 64]).all(1)
        assert fin.any() and not fin.all()
    s = out["through"].copy()
    s[0::2, 3:] = (s[0::2, 3:] * F(1e-30)).astype(F)
    with np.errstate(over="ignore"):
        s[1::2, 3:] = (s[1::2, 3:] * F(1e30)).astype(F)
    out["scaled"] = s
    return {k: np.ascontiguousarray(v, F) for k, v in out.items()}


def cross_set(sheets: int, n: int = 256, seed: int = CROSS_SEED) -> np.ndarray:
    rng = np.random.default_rng(seed)
    top = 8.0 * (sheets - 1)
    lo = np.stack([rng.uniform(-38, 38, n), rng.uniform(-6, -2, n), rng.uniform(-38, 38, n)], 1)
    hi = np.stack([rng.uniform(-38, 38, n), rng.uniform(top + 2, top + 6, n), rng.uniform(-38, 38, n)], 1)
    a, b = lo.copy(), hi.copy()
    a[1::2], b[1::2] = hi[1::2], lo[1::2]  # every second one runs downwards
    return np.ascontiguousarray(np.concatenate([a, b - a], 1), F)


def build(isect, surf, cam_words, lights, name: str) -> dict:
    """set name -> (segments, filter_ref.detail of them) for a scene's dump."""
    seed = BASE_SEED.get(name, ray_sets.BASE_SEED.get(name, 5))
    base = ray_sets.base_set(isect, surf, cam_words, seed=seed)
    want = rays_ref.trace(isect, aov_ref.Surfaces(surf), base)
    sets = segment_sets(base, want, lights)
    if name in LAYERS:
        sets["cross"] = cross_set(LAYERS[name][0])
    return {k: (s, filter_ref.detail(isect, surf, s)) for k, s in sets.items()}


def white(f):
    return (f == F(1)).all(1)


def black(f):
    return (f == F(0)).all(1)


def check_conditions(name: str, sets: dict):
    """What the tests assert on the EXPECTATION before they look at a result."""
    u = np.concatenate([sets["through"][1]["filter"], sets["lights"][1]["filter"]])
    share = float(white(u).mean())
    assert 0.05 <= share <= 0.95, (name, "white share", share)
    assert black(u).any(), (name, "no black result")
    if name in TINTED:
        assert int((~white(u) & ~black(u)).sum()) >= 5, (name, "tinted", int((~white(u) & ~black(u)).sum()))
    if name in ("neg6", "layers_neg"):
        allf = np.concatenate([d["filter"] for _, d in sets.values()])
        with np.errstate(invalid="ignore"):
            assert (allf < 0).any(), (name, "no negative component")
    if name == "layers":
        d = sets["cross"][1]
        f = d["filter"]
        open_ = ~black(f)
        assert 0.3 <= float(open_.mean()) <= 0.7, (name, float(open_.mean()))
        assert float((open_ & (d["count"] >= 3)).mean()) >= 0.3, name
        differs = (f.view(np.uint32) != d["reverse"].view(np.uint32)).any(1)
        assert int((open_ & differs).sum()) >= 50, (name, "order-sensitive", int((open_ & differs).sum()))
    if name == "layers10":
        d = sets["cross"][1]
        assert int((~black(d["filter"]) & (d["count"] > 8)).sum()) >= 20, name


_CASES = {}


def cases(oracle, name: str, tmpdir: str) -> dict:
    """{"path", "surf", "cam", "lights", "sets"} of a scene through liboracle.so
    (conftest.Oracle); computed once per process."""
    if name not in _CASES:
        path = file(name, tmpdir)
        surf, cam, lights = oracle.dump(path, W, H)
        sets = build(oracle.L.oracle_intersect, surf, cam, lights, name)
        _CASES[name] = {"path": path, "surf": surf, "cam": cam, "lights": lights, "sets": sets}
    return _CASES[name]
