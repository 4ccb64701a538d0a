#!/usr/bin/env python
"""Measurements of the adaptive supersampled renders (DESIGN.md "Adaptive
supersampling", profiles/r18/adaptive/).

    python tools/adaptive_probe.py compile REMARKS.txt
    timeout -k 10 300 python tools/adaptive_probe.py frame --config c2 --s 2

compile  the compiler's facts: REMARKS.txt is the stderr of one device
         compile of csrc/rt_kernels.hip with
         -Rpass-analysis=kernel-resource-usage.  One row per query variant:
         VGPRs, scratch bytes per lane, occupancy and LDS of rt_refine_kernel
         beside the same rt_shade_rays_kernel instance.  No GPU.
frame    a whole frame: 1920 x 1080 output, factor --s, asynchronous on one
         stream (c2: scene2 depth 3; scene7: depth 3; c3: the 50k heightfield,
         depth 1), every criterion at the default thresholds.  Timed in
         rounds that alternate the three calls, after a warm-up of each:
         rt_render_adaptive_async (RGBA8), rt_render_async of the base frame B
         and rt_render_ss_async of the sample frame — the two existing entry
         points are the yardsticks.  The medians over the rounds, the flagged
         share, and the phases of one synchronous call (base + AOV, classify +
         scan, refine: rt_debug_adaptive_phases).  From them the break-even
         share: the flagged share below which the adaptive call beats full
         supersampling when the refine time scales with the share,
             (t_ss - t_base - t_classify) / (t_refine / share).

One JSON line per measurement on stdout.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import re
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "ray-tracing-gpu_amd"))


def emit(**kw):
    print(json.dumps(kw), flush=True)


def step_compile(args):
    """Parse the remarks: {kernel stem: {(maxd, lb, flags): {field: value}}}."""
    fields = {"VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy",
              "LDS Size [bytes/block]": "lds", "VGPRs Spill": "vgpr_spill", "SGPRs Spill": "sgpr_spill"}
    table = {"rt_refine_kernel": {}, "rt_shade_rays_kernel": {}}
    cur = None
    for line in open(args.remarks, errors="replace"):
        m = re.search(r"Function Name: _ZN2rt\d+(rt_refine_kernel|rt_shade_rays_kernel)ILi(\d+)ELi(\d+)ELi(\d+)EEE", line)
        if m:
            cur = table[m.group(1)].setdefault(tuple(int(m.group(k)) for k in (2, 3, 4)), {})
            continue
        if "Function Name:" in line:
            cur = None
            continue
        m = re.search(r"remark:\s+(.*?): (\d+) \[", line)
        if cur is not None and m and m.group(1) in fields:
            cur[fields[m.group(1)]] = int(m.group(2))
    assert table["rt_refine_kernel"] and set(table["rt_refine_kernel"]) == set(table["rt_shade_rays_kernel"])
    for v in sorted(table["rt_refine_kernel"], key=lambda v: (v[2], v[0])):
        r, q = table["rt_refine_kernel"][v], table["rt_shade_rays_kernel"][v]
        emit(step="compile", variant="<%d,%d,%d>" % v, refine=r, query=q,
             more_scratch=r["scratch"] - q["scratch"], more_vgprs=r["vgprs"] - q["vgprs"])
    return 0


def step_frame(args):
    import torch

    import rt_amd
    from rt_amd import synth

    s, wo, ho = args.s, 1920, 1080
    scenes = os.path.join(REPO, "tests", "golden", "scenes")
    if args.config == "c3":
        os.makedirs(args.tmp, exist_ok=True)
        path, depth = synth.write_heightfield(os.path.join(args.tmp, "heightfield.dat")), 1
    else:
        path, depth = os.path.join(scenes, "scene2.dat" if args.config == "c2" else "scene7.dat"), 3
    samples = rt_amd.Scene(path, wo * s, ho * s, depth)
    base = rt_amd.Scene(path, wo, ho, depth).frame.copy()
    ctx = rt_amd.Context(0)
    ctx.upload(samples)
    f = samples.frame
    crit = rt_amd.EDGE_ID | rt_amd.EDGE_NORMAL | rt_amd.EDGE_COLOUR
    L = rt_amd.lib()
    L.rt_debug_adaptive_phases.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float),
                                           ctypes.POINTER(ctypes.c_ulonglong)]
    st = torch.cuda.current_stream().cuda_stream
    out = torch.empty((ho, wo), dtype=torch.int32, device="cuda")
    a = rt_amd.Adaptive(s, crit, 0.9, 0.1)
    o = rt_amd.AdaptiveOut(out.data_ptr(), None, None)
    # one synchronous call: the phases and the flagged share (and every buffer sized)
    phases = []
    n = ctypes.c_ulonglong()
    for _ in range(max(1, args.warmup)):
        assert L.rt_render_adaptive(ctx._h, ctypes.byref(f), ctypes.byref(a), ctypes.byref(o)) == 0
        ms = (ctypes.c_float * 3)()
        L.rt_debug_adaptive_phases(ctx._h, ms, ctypes.byref(n))
        phases.append(list(ms))
    kernel = ctx.stats().kernel  # the synchronous call's: the refine kernel
    ph = [statistics.median(p[i] for p in phases) for i in range(3)]
    share = n.value / (wo * ho)
    ctx.render_ss(f, s)  # sizes the sample intermediate
    calls = {
        "adaptive": lambda: ctx.render_adaptive_async(f, s, crit, rgba_dev_ptr=out.data_ptr(), stream=st),
        "base": lambda: ctx.render_async(base, out.data_ptr(), 0, st),
        "ss": lambda: ctx.render_ss_async(f, s, out.data_ptr(), 0, st),
    }
    for fn in calls.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(args.reps):       # alternating: every round times each call once
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / args.iters)
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: (max(v) - min(v)) / statistics.median(v) for k, v in times.items()}
    per_share = ph[2] / share if share > 0 else float("nan")
    emit(step="frame", config=args.config, s=s, output="1920x1080", depth=depth, flagged_share=round(share, 4),
         kernel=kernel, sync_base_aov_ms=round(ph[0], 4), sync_classify_scan_ms=round(ph[1], 4),
         sync_refine_ms=round(ph[2], 4), adaptive_ms=round(med["adaptive"], 4), base_ms=round(med["base"], 4),
         ss_ms=round(med["ss"], 4), adaptive_over_ss=round(med["adaptive"] / med["ss"], 3),
         adaptive_over_base=round(med["adaptive"] / med["base"], 3),
         break_even_share=round((med["ss"] - ph[0] - ph[1]) / per_share, 4) if per_share == per_share else None,
         spread={k: round(v, 3) for k, v in spread.items()}, reps=args.reps, iters=args.iters)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("step", choices=["compile", "frame"])
    ap.add_argument("remarks", nargs="?", help="compile: the file of compiler remarks")
    ap.add_argument("--config", default="c2", choices=["c2", "scene7", "c3"])
    ap.add_argument("--s", type=int, default=2, choices=[2, 4, 8])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tmp", default="/tmp/adaptive_probe")
    args = ap.parse_args()
    return step_compile(args) if args.step == "compile" else step_frame(args)


if __name__ == "__main__":
    sys.exit(main())
