"""The primary-hit AOV fixture tests/golden/aov.npz, made by oracle/_ref (the
reference's own CTriangle / CPlan / CQuadrique::Intersection through
ref_intersect, and its post-Pretraitement state through ref_dump; see
make_golden.py).  Run in the build container:

    make -C oracle ref && python tests/golden/make_aov_golden.py

tests/aov_ref.py restates the camera ray in float32 steps and applies
CScene::ObtenirCouleur's loop (Scene.cpp:1705-1715) to the per-primitive
distances; this file only feeds it the reference's intersect function.

Contents (data only — expected outputs):
  scene{1..9}_{id,t,n}   64 x 48: (48, 64) int32, (48, 64) float32, (48, 64, 3) float32
  hf1280_{id,t,n}        synth.write_heightfield(cols=40, rows=16) (1,280
                         triangles, above the clustering threshold) at 64 x 32
  hf50k_{x,y,id,t,n}     the default 50,000-triangle heightfield at 64 x 32 on
                         the 64 pixels aov_ref.sparse_pixels(hf50k_seed): one
                         per in-tile position, every tile twice.  The scene's
                         ground plane fills that camera's frame: it has NO
                         miss anywhere (hf50k_lacks = "miss"), so the seed is
                         the first whose pixels hold at least 8 triangle and
                         at least 8 plane winners
  hf50kcam2_{x,y,id,t,n,words}
                         the same scene and size seen by tests/cameras.py
                         cameras()[2] (pitched and yawed: sky in the frame;
                         `words` are its 23 camera words): the sparse set with
                         at least 8 hits and 8 misses
  {name}_lacks           "" / "miss" / "hit": what a set does not contain
Row 0 = the bottom scanline.  A miss is id -1, t -1, n 0.

Before anything is written, two assertions:
 1. the restated ray is pinned: for every pixel the depth-0 colour is
    recomputed from the fixture's own (D, id, t, n) with the shading restated
    in float32 (shade() / filtre() of oracle/rt_oracle.c, glibc powf through
    ctypes, shadow rays through ref_intersect) and must equal
    ref_render_window bit for bit;
 2. coverage: every set has hits and misses or names what it lacks; the
    moved camera's sparse pixels hold at least 8 of each, the file camera's
    at least 8 winners of either kind (the seeds are raised until they do).
"""
from __future__ import annotations

import ctypes
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden  # noqa: E402
from make_golden import synth  # noqa: E402

import aov_ref  # noqa: E402
import cameras  # noqa: E402
import rt_amd  # noqa: E402
from aov_ref import EPS, F  # noqa: E402

SCENES = os.path.join(HERE, "scenes")
POWF = aov_ref.libm_powf()


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def shade0(isect, S: aov_ref.Surfaces, surf, lights, bg, o, d, idx, t, n):
    """obtenir_couleur's tail + shade() of rt_oracle.c at depth 0 (no bounce
    can pass `bounces < max_bounces`), every step one float32 operation."""
    if idx < 0:
        return bg
    s = surf[idx]
    color, ka, kd, ks, shin = s[1:4], s[4], s[5], s[6], s[7]
    res = [color[0] * ka, color[1] * ka, color[2] * ka]
    P = np.array([o[k] + d[k] * t for k in range(3)], F)
    lrd = np.zeros(3, F)
    for L in lights:
        pos, lcol, intens = L[0:3], L[3:6], L[6]
        ld = [pos[k] - P[k] for k in range(3)]
        if not dot(ld, n) > 0:
            continue
        # filtre(): the ray is normalised in place (v3_div: reciprocal, then multiply)
        dist = np.sqrt((ld[0] * ld[0] + ld[1] * ld[1]) + ld[2] * ld[2])
        inv = F(1) / dist
        lrd[:] = [ld[0] * inv, ld[1] * inv, ld[2] * inv]
        S.intersect_all(isect, P.ctypes.data, lrd.ctypes.data)
        Fc = [F(1), F(1), F(1)]
        for i in range(S.n):
            ti = S.t[i]
            if ti > EPS and ti < dist:
                kt = surf[i][9]
                for k in range(3):
                    Fc[k] = Fc[k] * (surf[i][1 + k] * kt)
        LC = [lcol[k] * Fc[k] for k in range(3)]
        g = intens * kd * dot(n, lrd)
        for k in range(3):
            res[k] = res[k] + (color[k] * g) * LC[k]
        sc = F(2) * dot(lrd, n)
        rf = [lrd[k] - n[k] * sc for k in range(3)]
        ps = dot(rf, d)
        if ps > 0:
            pf = intens * ks * F(POWF(float(ps), float(shin)))
            for k in range(3):
                res[k] = res[k] + LC[k] * pf
    return np.array(res, F)


def check_colour(ref, isect, S, surf, lights, cam_words, xs, ys, ids, ts, ns, D):
    """Assertion 1 on the given pixels; returns the number of pixels checked."""
    bg = np.asarray(cam_words[24:27], F)
    o = np.asarray(cam_words[0:3], F)
    bad = 0
    with np.errstate(all="ignore"):
        for k in range(len(xs)):
            want = ref.window(int(ys[k]), int(ys[k]) + 1, int(xs[k]), int(xs[k]) + 1)[0, 0]
            got = np.asarray(shade0(isect, S, surf, lights, bg, o, D[k], int(ids[k]), ts[k], ns[k]), F)
            bad += int(not np.array_equal(got.view(np.uint32), want.view(np.uint32)))
    assert bad == 0, f"{bad} of {len(xs)} pixels: restated colour != ref_render_window"
    return len(xs)


def lacks(ids) -> str:
    hit, miss = bool((ids >= 0).any()), bool((ids < 0).any())
    assert hit or miss
    return "" if hit and miss else ("miss" if hit else "hit")


def one_set(L, path, w, h, xs=None, ys=None, words=None):
    """words: an explicit camera (cameras.words of a moved frame) handed to the
    reference's pixel loop with ref_set_camera, as make_camera_golden.py does."""
    ref = make_golden.Ref(L, path, w, h, 0)
    if words is not None:
        wd = np.asarray(words, F)
        pos, orient = np.ascontiguousarray(wd[:3]), np.ascontiguousarray(wd[3:19])
        assert L.ref_set_camera(ref.p, pos.ctypes.data, orient.ctypes.data, *[float(v) for v in wd[19:23]], w, h) == 0
    surf, cam_words, lights = ref.dump()
    S = aov_ref.Surfaces(surf)
    cam = aov_ref.Cam.from_words(cam_words)
    if words is not None:
        assert np.array_equal(cam_words[:19], wd[:19]) and np.array_equal(cam_words[20:24], wd[19:23])
    if xs is None:
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        xs, ys = xx.ravel(), yy.ravel()
    ids, ts, ns, D = aov_ref.aov_pixels(L.ref_intersect, S, cam, xs, ys)
    n = check_colour(ref, L.ref_intersect, S, surf, lights, cam_words, xs, ys, ids, ts, ns, D)
    return ids, ts, ns, n


def main():
    L = make_golden.load_ref()
    L.ref_set_camera.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_float] * 4 + \
                                [ctypes.c_int, ctypes.c_int]
    out = {}
    t0 = time.time()
    for i in range(1, 10):
        ids, ts, ns, n = one_set(L, os.path.join(SCENES, f"scene{i}.dat"), 64, 48)
        out[f"scene{i}_id"], out[f"scene{i}_t"] = ids.reshape(48, 64), ts.reshape(48, 64)
        out[f"scene{i}_n"] = ns.reshape(48, 64, 3)
        out[f"scene{i}_lacks"] = np.array(lacks(ids))
        print(f"scene{i}: {n} pixels, colour pinned, lacks '{lacks(ids)}' ({time.time() - t0:.0f} s)", flush=True)
    hf = synth.write_heightfield(os.path.join("/tmp", "rt_amd_heightfield_40x16.dat"), cols=40, rows=16)
    ids, ts, ns, n = one_set(L, hf, 64, 32)
    out["hf1280_id"], out["hf1280_t"], out["hf1280_n"] = ids.reshape(32, 64), ts.reshape(32, 64), ns.reshape(32, 64, 3)
    out["hf1280_lacks"] = np.array(lacks(ids))
    print(f"hf1280: {n} pixels, colour pinned, lacks '{lacks(ids)}' ({time.time() - t0:.0f} s)", flush=True)
    hf = synth.write_heightfield(os.path.join("/tmp", "rt_amd_heightfield.dat"))
    seed = 1
    while True:
        xs, ys = aov_ref.sparse_pixels(seed)
        ids, ts, ns, n = one_set(L, hf, 64, 32, xs, ys)
        tri, pla = int((ids > 0).sum()), int((ids == 0).sum())
        print(f"hf50k seed {seed}: {tri} triangle, {pla} plane winners, {64 - tri - pla} misses "
              f"({time.time() - t0:.0f} s)", flush=True)
        if tri >= 8 and pla >= 8:
            break
        seed += 1
    out["hf50k_seed"] = np.int32(seed)
    out["hf50k_x"], out["hf50k_y"] = xs, ys
    out["hf50k_id"], out["hf50k_t"], out["hf50k_n"] = ids, ts, ns
    out["hf50k_lacks"] = np.array(lacks(ids))
    words = cameras.words(cameras.cameras(rt_amd.Scene(hf, 64, 32, 0).frame)[2])
    seed = 1
    while True:
        xs, ys = aov_ref.sparse_pixels(seed)
        ids, ts, ns, n = one_set(L, hf, 64, 32, xs, ys, words)
        hits = int((ids >= 0).sum())
        print(f"hf50kcam2 seed {seed}: {hits} hits, {64 - hits} misses ({time.time() - t0:.0f} s)", flush=True)
        if hits >= 8 and 64 - hits >= 8:
            break
        seed += 1
    out["hf50kcam2_seed"] = np.int32(seed)
    out["hf50kcam2_words"] = np.asarray(words, F)
    out["hf50kcam2_x"], out["hf50kcam2_y"] = xs, ys
    out["hf50kcam2_id"], out["hf50kcam2_t"], out["hf50kcam2_n"] = ids, ts, ns
    out["hf50kcam2_lacks"] = np.array(lacks(ids))
    np.savez_compressed(os.path.join(HERE, "aov.npz"), **out)
    print(f"wrote aov.npz: {len(out)} arrays in {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
