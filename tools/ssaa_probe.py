#!/usr/bin/env python3
"""Measurements of the supersampled render (include/rt.h rt_render_ss*).

Two steps, each its own process, each under its own time limit, chained:

    timeout -k 10 240 python tools/ssaa_probe.py resolve && \\
    timeout -k 10 300 python tools/ssaa_probe.py frame --config c2 && \\
    timeout -k 10 300 python tools/ssaa_probe.py frame --config c3

resolve  the resolve kernel alone (rt_debug_resolve) at 3840 x 2160 samples,
         s = 2, and 7680 x 4320, s = 4, against hipMemcpyAsync device to
         device of the sample frame's bytes on the same buffers (the
         runtime's copy: the yardstick).  The resolve moves
         (1 + 16 / (12 s^2)) N bytes where the copy moves 2 N.
frame    a whole frame: 1920 x 1080 output, s = 2 (--s; c2: scene2 depth 3; c3:
         the heightfield, depth 1) by rt_render_ss_async with RGBA8 output,
         whole and in chunks (--chunks: RT_OPT_SS_CHUNK_ROWS values), against
         rt_render_async of the same 3840 x 2160 samples.  With RT_AMD_LIB set
         to another build's librt_amd.so (the parent commit's) and --plain-only
         the same plain render is timed there.

Each figure: the median and the minimum of --reps timed runs of --iters
back-to-back calls between two events, after --warmup untimed calls.  One
JSON line per measurement on stdout.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "ray-tracing-gpu_amd"))


def timed(torch, fn, iters, reps, warmup):
    """ms per call: median and min over `reps` runs of `iters` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return statistics.median(out), min(out)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def step_resolve(args):
    import torch

    import rt_amd

    L = rt_amd.lib()
    L.rt_debug_resolve.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    hip = ctypes.CDLL("libamdhip64.so.7")  # the runtime already loaded (torch's)
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    ctx = rt_amd.Context(0)
    st = torch.cuda.current_stream().cuda_stream
    for w, h, s in ((3840, 2160, 2), (7680, 4320, 4), (3840, 2160, 3), (3838, 2160, 2)):
        n = w * h * 3
        src = torch.rand(n, dtype=torch.float32, device="cuda")
        dst = torch.empty(n, dtype=torch.float32, device="cuda")
        rgb = torch.empty((h // s) * (w // s) * 3, dtype=torch.float32, device="cuda")
        rgba = torch.empty((h // s) * (w // s), dtype=torch.int32, device="cuda")
        nbytes = n * 4

        def copy():
            rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, st)  # 3 = device to device
            assert rc == 0, rc

        def resolve(f=True, q=True):
            rc = L.rt_debug_resolve(ctx._h, src.data_ptr(), w, s, h // s, rgb.data_ptr() if f else None,
                                    rgba.data_ptr() if q else None, st)
            assert rc == 0, rc

        t_copy = timed(torch, copy, args.iters, args.reps, args.warmup)
        rows = {"copy_d2d": t_copy,
                "resolve_rgba8": timed(torch, lambda: resolve(False, True), args.iters, args.reps, args.warmup),
                "resolve_float": timed(torch, lambda: resolve(True, False), args.iters, args.reps, args.warmup),
                "resolve_both": timed(torch, lambda: resolve(True, True), args.iters, args.reps, args.warmup)}
        # the image against numpy on a few rows (the probe measures what the tests pin)
        resolve(True, False)
        torch.cuda.synchronize()
        a = src.view(h, w, 3)[: 4 * s].cpu().numpy()
        acc = None
        for j in range(s):
            for i in range(s):
                t = a[j::s, i::s]
                acc = t.copy() if acc is None else acc + t
        import numpy as np

        same = np.array_equal((acc / np.float32(s * s)).view(np.uint32),
                              rgb.view(h // s, w // s, 3)[:4].cpu().numpy().view(np.uint32))
        for name, (med, mn) in rows.items():
            moved = 2 * nbytes if name == "copy_d2d" else nbytes + (h // s) * (w // s) * (
                {"resolve_rgba8": 4, "resolve_float": 12, "resolve_both": 16}[name])
            emit(step="resolve", samples=f"{w}x{h}", s=s, what=name, ms_median=round(med, 4), ms_min=round(mn, 4),
                 gb_per_s=round(moved / med / 1e6, 1), vs_copy=round(med / t_copy[0], 3), exact=bool(same),
                 path="16-byte" if w % 4 == 0 else "dword")
        del src, dst, rgb, rgba
    return 0


def step_frame(args):
    import torch

    import rt_amd
    from rt_amd import synth

    if args.plain_only:  # another build's library may predate the supersampled calls
        L = ctypes.CDLL(rt_amd.LIB_PATH)
        for name in [n for n in rt_amd.SIGNATURES if not hasattr(L, n)]:
            del rt_amd.SIGNATURES[name]
    s, wo, ho = args.s, 1920, 1080
    w, h = wo * s, ho * s
    if args.config == "c2":
        path, depth = os.path.join(REPO, "tests", "golden", "scenes", "scene2.dat"), 3
    else:
        os.makedirs(args.tmp, exist_ok=True)
        path, depth = synth.write_heightfield(os.path.join(args.tmp, "heightfield.dat")), 1
    scene = rt_amd.Scene(path, w, h, depth)
    ctx = rt_amd.Context(0)
    ctx.upload(scene)
    f = scene.frame
    st = torch.cuda.current_stream().cuda_stream
    samples_q = torch.empty((h, w), dtype=torch.int32, device="cuda")
    samples_f = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    ctx.render(f)  # the camera state, as every later frame finds it
    base = {"lib": os.path.basename(os.path.dirname(rt_amd.LIB_PATH)) + "/" + os.path.basename(rt_amd.LIB_PATH)}
    plain_q = timed(torch, lambda: ctx.render_async(f, samples_q.data_ptr(), 0, st), args.iters, args.reps, args.warmup)
    plain_f = timed(torch, lambda: ctx.render_async(f, 0, samples_f.data_ptr(), st), args.iters, args.reps, args.warmup)
    emit(step="frame", config=args.config, what=f"plain_rgba8_{w}x{h}", ms_median=round(plain_q[0], 4),
         ms_min=round(plain_q[1], 4), **base)
    emit(step="frame", config=args.config, what=f"plain_float_{w}x{h}", ms_median=round(plain_f[0], 4),
         ms_min=round(plain_f[1], 4), **base)
    if args.plain_only:
        return 0
    out_q = torch.empty((ho, wo), dtype=torch.int32, device="cuda")
    for chunk in [int(c) for c in args.chunks.split(",")]:
        ctx.set_option("ss_chunk_rows", chunk)
        ctx.render_ss(f, s)  # sizes the intermediate
        t = timed(torch, lambda: ctx.render_ss_async(f, s, out_q.data_ptr(), 0, st), args.iters, args.reps, args.warmup)
        emit(step="frame", config=args.config, what=f"ss{s}_rgba8_1920x1080", chunk_rows=chunk, ms_median=round(t[0], 4),
             ms_min=round(t[1], 4), over_plain_float_us=round((t[0] - plain_f[0]) * 1e3, 1),
             over_plain_float_pct=round((t[0] / plain_f[0] - 1) * 100, 2),
             over_plain_rgba8_us=round((t[0] - plain_q[0]) * 1e3, 1),
             over_plain_rgba8_pct=round((t[0] / plain_q[0] - 1) * 100, 2), **base)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("step", choices=["resolve", "frame"])
    ap.add_argument("--config", default="c2", choices=["c2", "c3"])
    ap.add_argument("--chunks", default="0,1080,544,272,144,64",
                    help="frame: RT_OPT_SS_CHUNK_ROWS values (0 = auto; 1080 = one chunk)")
    ap.add_argument("--s", type=int, default=2, help="frame: the factor (samples: 1920 s x 1080 s)")
    ap.add_argument("--plain-only", action="store_true", help="frame: only the plain renders (another build's library)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--tmp", default="/tmp/ssaa_probe")
    args = ap.parse_args()
    return step_resolve(args) if args.step == "resolve" else step_frame(args)


if __name__ == "__main__":
    sys.exit(main())
