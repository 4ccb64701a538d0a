#!/usr/bin/env python3
"""Measurements of the shadow-filter queries (include/rt.h rt_filter_rays_async).

One config per process, each under its own time limit, chained:

    timeout -k 10 240 python tools/filter_probe.py --config scene2 && \\
    timeout -k 10 300 python tools/filter_probe.py --config hf && \\
    timeout -k 10 300 python tools/filter_probe.py --config soup && \\
    timeout -k 10 240 python tools/filter_probe.py --config layers && \\
    timeout -k 10 240 python tools/filter_probe.py --config layers10

Configs (device buffers, one stream):

  scene2   the 1920 x 1080 frame's shadow segments towards light 0, from the
           library's own AOV planes (hit pixels; this tool measures and does
           not verify): rt_filter_kernel<0> against rt_rays_kernel<0>.
  hf       --segs (default 1 M) segments on the 50,000-triangle heightfield
           with RT_OPT_RAY_BVH 1: half `lights`-style (from the hit points of
           tools/rays_probe.py's recipe rays to the scene's lights), half
           `cross`-style (between random points of the grown bounding box).
  soup     the same on wf_dat("soup", 1100).
  layers / layers10
           tests/filter_sets.py's `cross` set tiled to --segs.

Legs, alternating within every rep: filter_bvh (rt_filter_kernel<1>),
filter_all (a second context with RT_OPT_BVH 0: rt_filter_kernel<0>) and rays
(rt_trace_rays_async with t, id and n of the same segments given as rays
[P, L / |L|]: rt_rays_kernel<1>, the yardstick for "the any-hit walk pays").
Each figure: the median, minimum and maximum of --reps timed runs of --iters
back-to-back launches between two events, after --warmup untimed launches
(tools/rays_probe.py's convention); (max - min) / median is the run-to-run
spread the comparison allows.  One JSON line per figure on stdout.

--steps (with RT_AMD_LIB naming a -DRT_FILTER_STEPS build of librt_amd.so,
whose <1> kernel writes its walk's tallies instead of the filter): one run,
no timing; per config the longest and the mean walk in steps (inner nodes +
leaves) and the share of lanes whose list of translucent hits overflowed.
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

CONFIGS = ("scene2", "hf", "soup", "layers", "layers10")


def mesh_segments(np, ctx, scene, n, seed=5):
    """Half lights-style, half cross-style (the docstring's recipe)."""
    import rays_probe

    h = n // 2
    rays = rays_probe.recipe_rays(np, ctx, scene, h, seed)
    got = ctx.trace_rays(rays, n=False)
    ok = (got["id"] >= 0) & np.isfinite(got["t"])
    P = (rays[ok, :3] + got["t"][ok, None] * rays[ok, 3:]).astype(np.float32)
    _, g, _, lights = scene.arrays()
    to = lights[np.arange(len(P)) % len(lights), :3]
    a = np.concatenate([P, (to - P).astype(np.float32)], 1)
    rng = np.random.default_rng(seed + 1)
    lo, hi = rays[:, :3].min(0), rays[:, :3].max(0)
    A, B = rng.uniform(lo, hi, (n - len(a), 3)), rng.uniform(lo, hi, (n - len(a), 3))
    b = np.concatenate([A, B - A], 1).astype(np.float32)
    segs = np.concatenate([a, b])
    return np.ascontiguousarray(segs[rng.permutation(len(segs))], np.float32), len(a)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", required=True, choices=CONFIGS)
    ap.add_argument("--segs", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", action="store_true")
    ap.add_argument("--tmp", default="/tmp/filter_probe")
    args = ap.parse_args()

    import numpy as np
    import torch

    import rt_amd
    from rt_amd import synth

    assert torch.cuda.is_available(), "filter_probe needs a HIP device"
    os.makedirs(args.tmp, exist_ok=True)
    st = torch.cuda.current_stream().cuda_stream
    info = {}
    if args.config == "scene2":
        import aov_ref

        w, h = 1920, 1080
        scene = rt_amd.Scene(os.path.join(REPO, "tests", "golden", "scenes", "scene2.dat"), w, h, 0)
        ctx = rt_amd.Context(0)
        ctx.upload(scene)
        aov = ctx.render_aov(scene.frame, n=False)
        cam = aov_ref.Cam.from_frame(scene.frame)
        ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        D = aov_ref.camera_dirs(cam, xs.ravel(), ys.ravel())
        t, ids = aov["t"].reshape(-1), aov["id"].reshape(-1)
        P = (cam.pos[None] + D[ids >= 0] * t[ids >= 0, None]).astype(np.float32)
        light = scene.arrays()[3][0, :3]
        segs = np.ascontiguousarray(np.concatenate([P, (light[None] - P).astype(np.float32)], 1), np.float32)
        info["lights_style"] = len(segs)
    elif args.config in ("hf", "soup"):
        if args.config == "hf":
            path = synth.write_heightfield(os.path.join(args.tmp, "heightfield.dat"))
        else:
            import wf_scenes

            path = os.path.join(args.tmp, "soup1100.dat")
            with open(path, "w") as fh:
                fh.write(wf_scenes.wf_dat("soup", 1100))
        scene = rt_amd.Scene(path, 64, 32, 0)
        ctx = rt_amd.Context(0, ray_bvh=1)
        ctx.upload(scene)
        segs, info["lights_style"] = mesh_segments(np, ctx, scene, args.segs)
    else:
        import filter_sets

        path = filter_sets.file(args.config, args.tmp)
        scene = rt_amd.Scene(path, 64, 32, 0)
        ctx = rt_amd.Context(0)
        ctx.upload(scene)
        base = filter_sets.cross_set(filter_sets.LAYERS[args.config][0])
        segs = np.ascontiguousarray(np.tile(base, (-(-args.segs // len(base)), 1))[: args.segs])
    n = len(segs)
    dsegs = torch.from_numpy(segs).cuda()
    out = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    base = {"config": args.config, "n": n, **info,
            "lib": os.path.basename(os.path.dirname(rt_amd.LIB_PATH)) + "/" + os.path.basename(rt_amd.LIB_PATH)}

    if args.steps:
        ctx.filter_rays(segs[:64])
        assert ctx.stats().kernel == "rt_filter_kernel<1>", ctx.stats().kernel
        ctx.filter_rays_async(dsegs.data_ptr(), n, out.data_ptr(), st)
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        steps = o[:, 0]
        print(json.dumps({**base, "what": "steps", "steps_max": int(steps.max()), "steps_mean": round(float(steps.mean()), 2),
                          "steps_p99": int(np.percentile(steps, 99)), "over_128": round(float((steps > 128).mean()), 5),
                          "overflow_share": round(float((o[:, 1] != 0).mean()), 5)}), flush=True)
        return 0

    calls, keep = {}, []
    ctx.filter_rays(segs[:64])
    info["filter_kernel"] = ctx.stats().kernel
    calls["filter_bvh" if info["filter_kernel"].endswith("<1>") else "filter_all"] = \
        lambda: ctx.filter_rays_async(dsegs.data_ptr(), n, out.data_ptr(), st)
    if info["filter_kernel"].endswith("<1>"):
        ctx0 = rt_amd.Context(0, ray_bvh=1, bvh=0)
        ctx0.upload(scene)
        ctx0.filter_rays(segs[:64])
        info["filter_all_kernel"] = ctx0.stats().kernel
        out0 = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        keep.append(out0)
        calls["filter_all"] = lambda: ctx0.filter_rays_async(dsegs.data_ptr(), n, out0.data_ptr(), st)
    with np.errstate(all="ignore"):
        L = segs[:, 3:].astype(np.float64)
        rays = np.concatenate([segs[:, :3], (L / np.linalg.norm(L, axis=1, keepdims=True)).astype(np.float32)], 1)
    rays = np.ascontiguousarray(rays, np.float32)
    drays = torch.from_numpy(rays).cuda()
    t = torch.empty(n, dtype=torch.float32, device="cuda")
    ids = torch.empty(n, dtype=torch.int32, device="cuda")
    nrm = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    ctx.trace_rays(rays[:64])
    info["rays_kernel"] = ctx.stats().kernel
    calls["rays"] = lambda: ctx.trace_rays_async(drays.data_ptr(), n, t.data_ptr(), ids.data_ptr(), nrm.data_ptr(), st)

    for _ in range(args.warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    # (the brute-force leg of a big mesh takes far longer per launch: fewer of them)
    iters = {k: (max(1, args.iters // 10) if k == "filter_all" and "filter_bvh" in calls else args.iters) for k in calls}
    times = {k: [] for k in calls}
    for _ in range(args.reps):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters[name]):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / iters[name])
    o = out.cpu().numpy()
    base.update(info)
    base["white"] = round(float((o == 1).all(1).mean()), 4)
    base["black"] = round(float((o == 0).all(1).mean()), 4)
    rays_med = statistics.median(times["rays"])
    for name, v in times.items():
        med = statistics.median(v)
        print(json.dumps({**base, "what": name, "ms_median": round(med, 4), "ms_min": round(min(v), 4),
                          "ms_max": round(max(v), 4), "spread": round((max(v) - min(v)) / med, 4),
                          "mseg_s": round(n / med / 1e3, 1), "vs_rays": round(med / rays_med, 3)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
