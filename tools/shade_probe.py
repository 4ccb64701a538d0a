#!/usr/bin/env python3
"""Measurements of the radiance queries (include/rt.h rt_shade_rays_async).

Every leg puts the shade query next to its yardstick, on one stream with
device buffers (rays_probe.py's rays and conventions):

  coherent_scene2   scene2's 1920 x 1080 camera rays at depth 0 against
                    rt_render_async of the same frame (float output)
  coherent_scene7   scene7's camera rays at depth 3 and depth 5 against the
  coherent_scene9   same frames' renders (scene9 likewise)
  coherent_hf       the 50,000-triangle heightfield with reflect 0.5, camera
                    rays at depth 0 and depth 3, against its frames (camera
                    buffer, wavefront levels)
  incoherent_hf     --rays base-recipe rays (rays_probe.recipe_rays) on that
  incoherent_soup   heightfield / on wf_dat("soup", 1600) at depth 3, against
                    rt_trace_rays_async on the same rays — the first search
                    alone, the floor a shade query cannot beat

Each figure: the median, minimum and maximum of --reps timed runs of --iters
back-to-back launches between two events, after --warmup untimed launches, the
legs alternating.  One JSON line per figure on stdout; `vs_yardstick` is the
query's median over its yardstick's.
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
sys.path.insert(0, HERE)

CONFIGS = ("coherent_scene2", "coherent_scene7", "coherent_scene9", "coherent_hf", "incoherent_hf", "incoherent_soup")
DEPTHS = {"coherent_scene2": (0,), "coherent_scene7": (3, 5), "coherent_scene9": (3, 5), "coherent_hf": (0, 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", required=True, choices=CONFIGS)
    ap.add_argument("--rays", type=int, default=2_000_000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--tmp", default="/tmp/shade_probe")
    args = ap.parse_args()

    import numpy as np
    import torch

    import rays_probe
    import rt_amd
    from rt_amd import synth

    assert torch.cuda.is_available(), "shade_probe needs a HIP device"
    os.makedirs(args.tmp, exist_ok=True)
    st = torch.cuda.current_stream().cuda_stream
    legs, keep = [], []   # (label, yardstick label or None, call, n, kernel)

    def shade_leg(ctx, f, rays, label, yard):
        n = len(rays)
        d = torch.from_numpy(rays).cuda()
        rgb = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        keep.append((d, rgb, f))
        ctx.shade_rays(rays[:64], f)
        legs.append((label, yard, lambda: ctx.shade_rays_async(f, d.data_ptr(), n, rgb.data_ptr(), st), n,
                     ctx.stats().kernel))

    if args.config.startswith("coherent"):
        w, h = 1920, 1080
        if args.config.endswith("hf"):
            path = synth.write_heightfield(os.path.join(args.tmp, "heightfield_r05.dat"), reflect=0.5)
        else:
            path = os.path.join(REPO, "tests", "golden", "scenes", args.config.split("_")[1] + ".dat")
        scene = rt_amd.Scene(path, w, h, 0)
        ctx = rt_amd.Context(0)
        ctx.upload(scene)
        rays = rays_probe.camera_rays(np, scene.frame, w, h)
        img = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        keep.append(img)
        for depth in DEPTHS[args.config]:
            f = scene.frame.copy()
            f.max_bounces = depth
            ctx.render_float(f)
            legs.append((f"frame_d{depth}", None,
                         (lambda f=f: ctx.render_async(f, rgb_dev_ptr=img.data_ptr(), stream=st)), w * h,
                         ctx.stats().kernel))
            shade_leg(ctx, f, rays, f"shade_d{depth}", f"frame_d{depth}")
    else:
        if args.config.endswith("hf"):
            path = synth.write_heightfield(os.path.join(args.tmp, "heightfield_r05.dat"), reflect=0.5)
        else:
            import wf_scenes

            path = os.path.join(args.tmp, "soup1600.dat")
            with open(path, "w") as fh:
                fh.write(wf_scenes.wf_dat("soup", 1600))
        scene = rt_amd.Scene(path, 64, 32, 3)
        ctx = rt_amd.Context(0, ray_bvh=1)
        ctx.upload(scene)
        rays = rays_probe.recipe_rays(np, ctx, scene, args.rays)
        n = len(rays)
        d = torch.from_numpy(rays).cuda()
        t = torch.empty(n, dtype=torch.float32, device="cuda")
        ids = torch.empty(n, dtype=torch.int32, device="cuda")
        nrm = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        keep.append((d, t, ids, nrm))
        ctx.trace_rays(rays[:64])
        legs.append(("trace", None,
                     lambda: ctx.trace_rays_async(d.data_ptr(), n, t.data_ptr(), ids.data_ptr(), nrm.data_ptr(), st), n,
                     ctx.stats().kernel))
        shade_leg(ctx, scene.frame, rays, "shade_d3", "trace")

    for _ in range(args.warmup):
        for leg in legs:
            leg[2]()
    torch.cuda.synchronize()
    times = {leg[0]: [] for leg in legs}
    for _ in range(args.reps):
        for label, _, fn, _, _ in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[label].append(e0.elapsed_time(e1) / args.iters)
    med = {k: statistics.median(v) for k, v in times.items()}
    for label, yard, _, n, kernel in legs:
        v = times[label]
        line = {"config": args.config, "what": label, "kernel": kernel, "n": n, "ms_median": round(med[label], 4),
                "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "mray_s": round(n / med[label] / 1e3, 1)}
        if yard:
            line["yardstick"] = yard
            line["vs_yardstick"] = round(med[label] / med[yard], 3)
        print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
