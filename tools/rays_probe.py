#!/usr/bin/env python3
"""Measurements of the ray queries (include/rt.h rt_trace_rays_async).

One config per process, each under its own time limit, chained:

    timeout -k 10 240 python tools/rays_probe.py --config coherent_scene2 && \\
    timeout -k 10 300 python tools/rays_probe.py --config coherent_hf && \\
    timeout -k 10 300 python tools/rays_probe.py --config incoherent_hf && \\
    timeout -k 10 300 python tools/rays_probe.py --config incoherent_soup && \\
    timeout -k 10 300 python tools/rays_probe.py --config bvh_vs_brute

Configs (device buffers, one stream, rt_trace_rays_async with t, id and n):

  coherent_scene2 / coherent_hf
      the 1920 x 1080 camera rays in pixel order against rt_render_aov_async
      (all planes) of the same frame — the AOV kernel has the camera's culling
      structures, the query has not; hf: the 50,000-triangle heightfield with
      RT_OPT_RAY_BVH 1.  The two legs alternate within every rep.
  incoherent_hf / incoherent_soup
      --rays (default 2 M) rays of the tests' base recipe (tests/ray_sets.py:
      half aimed at primary-hit points — here taken from the library's own AOV
      frame, this tool measures and does not verify —, half uniform on the
      sphere, origins in the grown bounding box) on the heightfield and on
      wf_dat("soup", 1600): Mray/s.
  bvh_vs_brute
      64 K of the heightfield's rays with RT_OPT_RAY_BVH 1 and 0, alternating.

Each figure: the median, minimum and maximum of --reps timed runs of --iters
back-to-back launches between two events, after --warmup untimed launches
(tools/aov_probe.py's convention).  With RT_AMD_LIB set to another build's
librt_amd.so the same figures are taken there (-DRT_RAYS_BUDGET / -DRT_RAYS_CAP
builds).  One JSON line per figure on stdout.  Kernel times come from a
separate `rocprofv3 --kernel-trace --stats` run of the same command with
--reps 1.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "ray-tracing-gpu_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

CONFIGS = ("coherent_scene2", "coherent_hf", "incoherent_hf", "incoherent_soup", "bvh_vs_brute")


def camera_rays(np, f, w, h):
    """The frame's camera rays in pixel order, as float32 steps (tests/aov_ref.py)."""
    import aov_ref

    cam = aov_ref.Cam.from_frame(f)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    D = aov_ref.camera_dirs(cam, xs.ravel(), ys.ravel())
    return np.ascontiguousarray(np.concatenate([np.tile(cam.pos, (len(D), 1)), D], 1), np.float32)


def recipe_rays(np, ctx, scene, n, seed=5):
    """The base recipe at any size; hit points from the context's own AOV frame at 64 x 32."""
    import aov_ref

    rng = np.random.default_rng(seed)
    h = n // 2
    f = scene.frame
    cam = aov_ref.Cam.from_frame(f)
    aov = ctx.render_aov(f)
    xs, ys = rng.integers(0, f.width, h), rng.integers(0, f.height, h)
    D = aov_ref.camera_dirs(cam, xs, ys).astype(np.float64)
    t = aov["t"][ys, xs]
    t = np.where((aov["id"][ys, xs] >= 0) & np.isfinite(t), t, np.float32(100)).astype(np.float64)
    P = cam.pos.astype(np.float64) + t[:, None] * D
    ty, g, _, _ = scene.arrays()
    verts = g[ty == 0][:, :9].reshape(-1, 3).astype(np.float64)
    pts = np.concatenate([verts, P, cam.pos.astype(np.float64)[None]])
    lo, hi = pts.min(0), pts.max(0)
    lo, hi = lo - 0.25 * (hi - lo), hi + 0.25 * (hi - lo)
    O = rng.uniform(lo, hi, (n, 3))
    d = np.concatenate([P - O[:h], rng.normal(size=(n - h, 3))])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray(np.concatenate([O, d], 1), np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", required=True, choices=CONFIGS)
    ap.add_argument("--rays", type=int, default=2_000_000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--tmp", default="/tmp/rays_probe")
    args = ap.parse_args()

    import numpy as np
    import torch

    import rt_amd
    from rt_amd import synth

    assert torch.cuda.is_available(), "rays_probe needs a HIP device"
    os.makedirs(args.tmp, exist_ok=True)
    hf = lambda: synth.write_heightfield(os.path.join(args.tmp, "heightfield.dat"))  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    calls, info = {}, {}

    def query(ctx, rays):
        n = len(rays)
        d = torch.from_numpy(rays).cuda()
        t = torch.empty(n, dtype=torch.float32, device="cuda")
        ids = torch.empty(n, dtype=torch.int32, device="cuda")
        nrm = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        ctx.trace_rays(rays[:64])
        kernel = ctx.stats().kernel
        keep = (d, t, ids, nrm)
        return (lambda: ctx.trace_rays_async(d.data_ptr(), n, t.data_ptr(), ids.data_ptr(), nrm.data_ptr(), st)), kernel, keep

    if args.config.startswith("coherent"):
        w, h = 1920, 1080
        path = hf() if args.config.endswith("hf") else os.path.join(REPO, "tests", "golden", "scenes", "scene2.dat")
        scene = rt_amd.Scene(path, w, h, 0)
        ctx = rt_amd.Context(0, ray_bvh=1)
        ctx.upload(scene)
        f = scene.frame
        rays = camera_rays(np, f, w, h)
        calls["rays"], info["rays_kernel"], keep = query(ctx, rays)
        t = torch.empty((h, w), dtype=torch.float32, device="cuda")
        ids = torch.empty((h, w), dtype=torch.int32, device="cuda")
        nrm = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        ctx.render_aov(f, t=False, id=True, n=False)
        info["aov_kernel"] = ctx.stats().kernel
        calls["aov_all"] = lambda: ctx.render_aov_async(f, t.data_ptr(), ids.data_ptr(), nrm.data_ptr(), st)
        count = {"rays": len(rays), "aov_all": w * h}
    elif args.config.startswith("incoherent"):
        if args.config.endswith("hf"):
            path = hf()
        else:
            import wf_scenes

            path = os.path.join(args.tmp, "soup1600.dat")
            with open(path, "w") as fh:
                fh.write(wf_scenes.wf_dat("soup", 1600))
        scene = rt_amd.Scene(path, 64, 32, 0)
        ctx = rt_amd.Context(0, ray_bvh=1)
        ctx.upload(scene)
        rays = recipe_rays(np, ctx, scene, args.rays)
        calls["rays"], info["rays_kernel"], keep = query(ctx, rays)
        count = {"rays": len(rays)}
    else:
        path = hf()
        scene = rt_amd.Scene(path, 64, 32, 0)
        ctxs = {}
        keep = []
        count = {}
        for label, opt in (("bvh", 1), ("brute", 0)):
            ctxs[label] = rt_amd.Context(0, ray_bvh=opt)
            ctxs[label].upload(scene)
        rays = recipe_rays(np, ctxs["bvh"], scene, 65536)
        for label in ctxs:
            calls[label], info[label + "_kernel"], k = query(ctxs[label], rays)
            keep.append(k)
            count[label] = len(rays)

    for _ in range(args.warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(args.reps):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.iters)
    base = {"config": args.config, **info,
            "lib": os.path.basename(os.path.dirname(rt_amd.LIB_PATH)) + "/" + os.path.basename(rt_amd.LIB_PATH)}
    first = statistics.median(next(iter(times.values())))
    for name, v in times.items():
        med = statistics.median(v)
        print(json.dumps({**base, "what": name, "n": count[name], "ms_median": round(med, 4), "ms_min": round(min(v), 4),
                          "ms_max": round(max(v), 4), "mray_s": round(count[name] / med / 1e3, 1),
                          "vs_first": round(med / first, 3)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
