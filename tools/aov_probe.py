#!/usr/bin/env python3
"""Measurements of the primary-hit AOV pass (include/rt.h rt_render_aov_async).

One config per process, each under its own time limit, chained:

    timeout -k 10 240 python tools/aov_probe.py --config scene2_1080p && \\
    timeout -k 10 300 python tools/aov_probe.py --config hf_1080p && \\
    timeout -k 10 420 python tools/aov_probe.py --config hf_4320p

Per config, on one context and one stream, after a synchronous render of each
kind (the camera state as every later frame finds it):

  colour   rt_render_async into float RGB at depth 0 — the yardstick: the
           same closest hit, plus the shading the AOV pass leaves out
  aov_all  rt_render_aov_async with t, id and n (20 B per pixel)
  aov_id   rt_render_aov_async with id only (4 B per pixel)

Each figure: the median and the minimum of --reps timed runs of --iters
back-to-back launches between two events, after --warmup untimed launches;
the three calls alternate within every rep, so drift hits them alike.
--options passes context options (e.g. launch_camera=0: a tiny scene on the
device camera records, the AOV pass then on WAVE 9).  With RT_AMD_LIB set to
another build's librt_amd.so the same figures are taken there (store-policy
builds, -DRT_AOV_NT=0 / 1).  One JSON line per figure on stdout.
Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of
the same command with --reps 1.
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

CONFIGS = {"scene2_1080p": ("scene2", 1920, 1080), "hf_1080p": ("hf", 1920, 1080), "hf_4320p": ("hf", 7680, 4320)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", required=True, choices=sorted(CONFIGS))
    ap.add_argument("--options", default="", help="context options, name=value,...")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--tmp", default="/tmp/aov_probe")
    args = ap.parse_args()

    import numpy as np
    import torch

    import rt_amd
    from rt_amd import synth

    assert torch.cuda.is_available(), "aov_probe needs a HIP device"
    which, w, h = CONFIGS[args.config]
    if which == "hf":
        os.makedirs(args.tmp, exist_ok=True)
        path = synth.write_heightfield(os.path.join(args.tmp, "heightfield.dat"))
    else:
        path = os.path.join(REPO, "tests", "golden", "scenes", "scene2.dat")
    options = {k: float(v) for k, v in (kv.split("=") for kv in args.options.split(",") if kv)}
    scene = rt_amd.Scene(path, w, h, 0)
    ctx = rt_amd.Context(0, **options)
    ctx.upload(scene)
    f = scene.frame
    st = torch.cuda.current_stream().cuda_stream
    rgb = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    t = torch.empty((h, w), dtype=torch.float32, device="cuda")
    ids = torch.empty((h, w), dtype=torch.int32, device="cuda")
    n = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")

    ctx.render_aov(f, t=False, id=True, n=False)
    k_aov = ctx.stats().kernel
    ctx.render_float(f)
    k_col = ctx.stats().kernel
    calls = {"colour": lambda: ctx.render_async(f, 0, rgb.data_ptr(), st),
             "aov_all": lambda: ctx.render_aov_async(f, t.data_ptr(), ids.data_ptr(), n.data_ptr(), st),
             "aov_id": lambda: ctx.render_aov_async(f, 0, ids.data_ptr(), 0, st)}
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
    # what was timed is what the tests pin: misses exactly where the colour frame shows the background
    bg = np.array(f.background[:], np.float32)
    rows = slice(0, h, max(1, h // 64))
    same = bool(np.array_equal(ids[rows].cpu().numpy() < 0, (rgb[rows].cpu().numpy() == bg).all(-1)))
    base = {"config": args.config, "options": args.options,
            "lib": os.path.basename(os.path.dirname(rt_amd.LIB_PATH)) + "/" + os.path.basename(rt_amd.LIB_PATH),
            "aov_kernel": k_aov, "colour_kernel": k_col, "miss_is_background": same}
    col = statistics.median(times["colour"])
    for name, v in times.items():
        med = statistics.median(v)
        print(json.dumps({**base, "what": name, "ms_median": round(med, 4), "ms_min": round(min(v), 4),
                          "ms_max": round(max(v), 4), "vs_colour": round(med / col, 3)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
