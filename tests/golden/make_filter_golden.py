"""The shadow-filter fixture tests/golden/filter.npz, made by oracle/_ref (the
reference's own CTriangle / CPlan / CQuadrique::Intersection through
ref_intersect, and its post-Pretraitement state through ref_dump; see
make_golden.py and make_rays_golden.py).  Run in the build container:

    make -C oracle ref && python tests/golden/make_filter_golden.py

tests/filter_sets.py builds the segments and tests/filter_ref.py applies
CScene::ObtenirFiltreDeSurface's loop (Scene.cpp:1842-1861) to the
per-primitive distances; this file only feeds them the reference's intersect
function.

Contents (data only — inputs and expected outputs):
  scene7_{set}_segs / _filter    every set of filter_sets for scene7
  layers_cross_segs / _filter    the `cross` set of the layers scene
  mixed65_through_segs / _filter
  hf50k_segs / _filter           128 segments on the 50,000-triangle
                                 heightfield, from rays.npz's hf50k_rays:
                                 `through` of the first 64 rays; of the others
                                 the `lights` segment of the hit point (light
                                 0), `through` where the ray misses
  {scene}_sha256                 of the scene's .dat text
Before anything is written the conditions of filter_sets.check_conditions are
asserted on the scenes made in full.
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

import filter_ref  # noqa: E402
import filter_sets  # noqa: E402
import ray_sets  # noqa: E402

F = np.float32


def hf50k_segments(rays, t, ids, lights):
    rays = np.ascontiguousarray(rays, F)
    hit = ids >= 0
    tt = np.where(hit & np.isfinite(t), t, F(100)).astype(np.float64)[:, None]
    a = np.concatenate([rays[:, :3], (rays[:, 3:].astype(np.float64) * (1.5 * tt)).astype(F)], 1)
    b = filter_sets.light_segments(rays[64:], t[64:], hit[64:], lights, count=1)
    a[64:][hit[64:]] = b  # (a ray of the second half that misses keeps its `through` segment)
    assert len(a) == 128 and len(b) >= 16
    return np.ascontiguousarray(a, F)


def main():
    L = make_golden.load_ref()
    out = {}
    t0 = time.time()
    with tempfile.TemporaryDirectory() as tmp:
        for name, keep in (("scene7", None), ("layers", ("cross",)), ("mixed65", ("through",))):
            path = filter_sets.file(name, tmp)
            surf, cam, lights = make_golden.Ref(L, path, filter_sets.W, filter_sets.H, 0).dump()
            sets = filter_sets.build(L.ref_intersect, surf, cam, lights, name)
            filter_sets.check_conditions(name, sets)
            for label, (segs, d) in sets.items():
                if keep is None or label in keep:
                    out[f"{name}_{label}_segs"] = segs
                    out[f"{name}_{label}_filter"] = d["filter"]
            out[f"{name}_sha256"] = np.array(hashlib.sha256(open(path, "rb").read()).hexdigest())
            print(f"{name}: {sorted(sets)} ({time.time() - t0:.0f} s)", flush=True)
        path = ray_sets.file("hf50k", tmp)
        surf, cam, lights = make_golden.Ref(L, path, filter_sets.W, filter_sets.H, 0).dump()
        g = np.load(os.path.join(HERE, "rays.npz"))
        assert hashlib.sha256(open(path, "rb").read()).hexdigest() == str(g["hf50k_sha256"])
        segs = hf50k_segments(g["hf50k_rays"], g["hf50k_t"], g["hf50k_id"], lights)
        f = filter_ref.filters(L.ref_intersect, surf, segs)
        assert filter_sets.black(f).any() and filter_sets.white(f).any()
        out["hf50k_segs"], out["hf50k_filter"] = segs, f
        out["hf50k_sha256"] = g["hf50k_sha256"]
        print(f"hf50k: {len(segs)} segments, white {filter_sets.white(f).mean():.2f} ({time.time() - t0:.0f} s)",
              flush=True)
    np.savez_compressed(os.path.join(HERE, "filter.npz"), **out)
    print(f"wrote filter.npz: {len(out)} arrays in {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
