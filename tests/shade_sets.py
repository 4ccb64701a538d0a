"""The scenes and the seeded ray sets of the radiance-query tests
(test_shade_cpu.py, test_gpu_shade.py) and of the fixture generator
(tests/golden/make_shade_golden.py): all three build the very same rays.

Scenes (SCENES): ray_sets' scene1 .. scene9, mixed63 / 64 / 65, soup1100 and
hf1600; wf_scenes' chain96, split1024 and refract_only96; hf1600r, the 40 x 20
heightfield with `reflect: 0.5` on every triangle; and — fixture only, brute
force over 50,000 triangles is too slow at test time — hf50kr, the 250 x 100
heightfield with `reflect: 0.5`.

A set is (O, R): origins and RAW directions.  The oracle shades
(O, v3_normaliser(R)) (shade_ref.oracle_shade), and the product is handed
[O, shade_ref.unit_dirs(R)] — exactly that direction.  Per scene, from the
N_BASE rays of ray_sets.base_set and their expected closest hits
(rays_ref.trace):
 base         the base rays, R their direction;
 leaving      from the hit points float32(O + t D) along the mirrored
              direction: the t > EPSILON self-hit rejection of the first
              search;
 axis         one or two exact zeros in R;
 zero         R = +0 / -0: D = 0 by the normaliser's rule;
 nonfinite_o  NaN / +-inf in O on every fourth ray, R the base direction;
 nan_d        NaN / +-inf in R on every fourth ray: the normaliser makes D zero
              (a NaN length fails its `> EPSILON`) or NaN (inf x 0).
The finite rays that share a wave of 64 with the non-finite ones are part of
the comparison.

Consistency sets (consistency()) have no oracle expectation — the oracle only
shades normalised directions: scaled3 / scaled025 (D x 3, D x 0.25) and inf_d
(+-inf written into D on every fourth ray).  For these the CPU backend is the
plain restatement and the GPU must equal it bit for bit.

Conditions (check_conditions), asserted on the expectation before any result
is looked at: on every base set the non-background share lies within [0.25,
0.97] and there are at least 40 distinct colours; on the bounce scenes
(BOUNCE) at least 0.04 of the depth-3 colours differ in bits from the depth-0
colours.  A scene that falls outside takes another seed (BASE_SEED); the
bounds stay.
"""
from __future__ import annotations

import os

import numpy as np

import aov_ref
import ray_sets
import rays_ref
import shade_ref

F = np.float32
W, H = ray_sets.W, ray_sets.H
N_BASE = 128
RAY_SCENES = [f"scene{i}" for i in range(1, 10)] + ["mixed63", "mixed64", "mixed65", "soup1100", "hf1600"]
EXTRA = {"chain96": ("wf", "chain", 96), "split1024": ("wf", "split", 1024),
         "refract_only96": ("wf", "refract_only", 96), "hf1600r": ("hf", 40, 20, 0.5), "hf50kr": ("hf", 250, 100, 0.5)}
SCENES = RAY_SCENES + [n for n in EXTRA if n != "hf50kr"]
BOUNCE = ("scene7", "scene8", "scene9", "refract_only96", "split1024", "hf1600r", "soup1100", "chain96", "mixed64",
          "mixed65")
ORACLE_SETS = ("base", "leaving", "axis", "zero", "nonfinite_o", "nan_d")
# The base set's seed per scene: 5 unless the conditions ask for another.
BASE_SEED = {}


def scene_text(name: str):
    if name in EXTRA:
        kind, *a = EXTRA[name]
        if kind == "wf":
            import wf_scenes

            return wf_scenes.wf_dat(a[0], a[1])
        from rt_amd import synth

        return synth.heightfield_dat(a[0], a[1], reflect=a[2])
    return ray_sets.scene_text(name)


def file(name: str, tmpdir: str) -> str:
    if name not in EXTRA:
        return ray_sets.file(name, tmpdir)
    text = scene_text(name)
    path = os.path.join(tmpdir, f"shade_{name}.dat")
    if not (os.path.exists(path) and open(path).read() == text):
        with open(path, "w") as f:
            f.write(text)
    return path


_NONFINITE = [np.nan, np.inf, -np.inf]


def base_rays(isect, surf, cam_words, name: str, n: int = N_BASE) -> np.ndarray:
    return ray_sets.base_set(isect, surf, cam_words, n=n, seed=BASE_SEED.get(name, 5))


def oracle_sets(base: np.ndarray, want: dict) -> dict:
    """label -> (O, R), both (N, 3) float32, from the base rays and their expected closest hits."""
    d = ray_sets.derived(base, want)
    out = {"base": base, "leaving": d["leaving"], "axis": d["axis"], "zero": d["zero"]}
    n = len(base)
    r = base.copy()
    for j, k in enumerate(range(1, n, 4)):
        r[k, j % 3] = _NONFINITE[(j // 3) % 3]
    out["nonfinite_o"] = r
    r = base.copy()
    for j, k in enumerate(range(2, n, 4)):
        r[k, 3 + j % 3] = _NONFINITE[(j // 3) % 3]
    out["nan_d"] = r
    for label in ("nonfinite_o", "nan_d"):
        for k0 in range(0, n - 63, 64):
            fin = np.isfinite(out[label][k0:k0 + 64]).all(1)
            assert fin.any() and not fin.all()
    return {k: (np.ascontiguousarray(v[:, :3]), np.ascontiguousarray(v[:, 3:])) for k, v in out.items()}


def rays_of(O, R) -> np.ndarray:
    """The (N, 6) array the product is handed: [O, v3_normaliser(R)]."""
    return np.ascontiguousarray(np.concatenate([O, shade_ref.unit_dirs(R)], 1), F)


def consistency(base: np.ndarray) -> dict:
    """label -> (N, 6) float32 rays that no oracle shades."""
    base = np.ascontiguousarray(base, F)
    out = {}
    for label, s in (("scaled3", 3.0), ("scaled025", 0.25)):
        r = base.copy()
        r[:, 3:] = (base[:, 3:] * F(s)).astype(F)
        out[label] = r
    r = base.copy()
    for j, k in enumerate(range(3, len(base), 4)):
        r[k, 3 + j % 3] = np.inf if j % 2 else -np.inf
    out["inf_d"] = r
    return out


def conditions(c0: np.ndarray, c3, background) -> dict:
    """The base set's figures from its depth-0 (and, on a bounce scene, depth-3) expectation."""
    bg = np.asarray(background, F)
    lit = (c0.view(np.uint32) != bg.view(np.uint32)).any(1)
    out = {"share": float(lit.mean()), "distinct": len({bytes(v) for v in np.ascontiguousarray(c0)})}
    if c3 is not None:
        out["bounced"] = float((c0.view(np.uint32) != c3.view(np.uint32)).any(1).mean())
    return out


def check_conditions(c: dict, name: str = ""):
    assert 0.25 <= c["share"] <= 0.97, (name, c)
    assert c["distinct"] >= 40, (name, c)
    assert "bounced" not in c or c["bounced"] >= 0.04, (name, c)


_CASES = {}
_WANT = {}


def cases(oracle, name: str, tmpdir: str) -> dict:
    """{"path", "sets": {label: (O, R)}, "rays": {label: (N, 6)}, "consistency": {label: (N, 6)}} of a
    scene through liboracle.so (conftest.Oracle); computed once per process."""
    if name not in _CASES:
        path = file(name, tmpdir)
        surf, cam, _ = oracle.dump(path, W, H)
        isect = oracle.L.oracle_intersect
        base = base_rays(isect, surf, cam, name)
        want = rays_ref.trace(isect, aov_ref.Surfaces(surf), base)
        sets = oracle_sets(base, want)
        rays = {k: rays_of(*v) for k, v in sets.items()}
        # the base rays are unit vectors already; the normaliser may still move their last bits
        _CASES[name] = {"name": name, "path": path, "sets": sets, "rays": rays, "consistency": consistency(rays["base"])}
    return _CASES[name]


def expected(oracle, case: dict, label: str, depth: int, min_energy: float = 0.01, scene_ior: float = 1.0,
             path=None) -> np.ndarray:
    """The oracle's colours of a set (cached, read-only)."""
    key = (path or case["path"], label, depth, float(min_energy), float(scene_ior))
    if key not in _WANT:
        O, R = case["sets"][label]
        w = shade_ref.oracle_shade(oracle, key[0], depth, min_energy, scene_ior, O, R)
        w.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]
