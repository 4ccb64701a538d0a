"""The ray-query fixture tests/golden/rays.npz, made by oracle/_ref (the
reference's own CTriangle / CPlan / CQuadrique::Intersection through
ref_intersect, and its post-Pretraitement state through ref_dump; see
make_golden.py and make_aov_golden.py).  Run in the build container:

    make -C oracle ref && python tests/golden/make_rays_golden.py

tests/ray_sets.py builds the rays and tests/rays_ref.py applies
CScene::ObtenirCouleur's loop (Scene.cpp:1705-1715) to the per-primitive
distances; this file only feeds them the reference's intersect function.

Contents (data only — inputs and expected outputs), per scene `name` of
ray_sets.SCENES:
  {name}_rays          (N, 6) float32: the base set (N = 256; the 50,000-
                       triangle heightfield: a base set of 128)
  {name}_{id,t,n}      (N,) int32, (N,) float32, (N, 3) float32
  {name}_sha256        of the scene's .dat text
  {name}_seed          the base set's seed
Before anything is written the base set's conditions are asserted
(ray_sets.check_conditions): hit share within [0.25, 0.95], winners of at
least 2 surface kinds, at least 20 distinct winners in scenes of 60 or more
surfaces.
"""
from __future__ import annotations

import hashlib
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden  # noqa: E402

import aov_ref  # noqa: E402
import ray_sets  # noqa: E402
import rays_ref  # noqa: E402


def main():
    L = make_golden.load_ref()
    out = {}
    t0 = time.time()
    with tempfile.TemporaryDirectory() as tmp:
        for name in ray_sets.SCENES:
            path = ray_sets.file(name, tmp)
            ref = make_golden.Ref(L, path, ray_sets.W, ray_sets.H, 0)
            surf, cam_words, _ = ref.dump()
            S = aov_ref.Surfaces(surf)
            seed = ray_sets.BASE_SEED.get(name, 5)
            n = ray_sets.HF50K_RAYS if name == "hf50k" else ray_sets.N_BASE
            rays = ray_sets.base_set(L.ref_intersect, surf, cam_words, n=n, seed=seed)
            want = rays_ref.trace(L.ref_intersect, S, rays)
            c = ray_sets.conditions(want, surf[:, 0].astype(int))
            ray_sets.check_conditions(c, name)
            out[f"{name}_rays"] = rays
            for k in ("id", "t", "n"):
                out[f"{name}_{k}"] = want[k]
            out[f"{name}_sha256"] = np.array(hashlib.sha256(open(path, "rb").read()).hexdigest())
            out[f"{name}_seed"] = np.int32(seed)
            print(f"{name}: {len(rays)} rays, {c} ({time.time() - t0:.0f} s)", flush=True)
    np.savez_compressed(os.path.join(HERE, "rays.npz"), **out)
    print(f"wrote rays.npz: {len(out)} arrays in {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
