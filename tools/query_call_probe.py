#!/usr/bin/env python3
"""Host cost of one query call (include/rt.h rt_trace_rays*, rt_filter_rays*, rt_shade_rays*).

Wall time per call of 64-item queries on scene3 through the C ABI: the
synchronous calls with host pointers (upload, kernel, copy back, sync), the
async calls with device pointers (the enqueue alone, the stream synchronised
outside the timed loop), and a call with n == 0 (the checks alone).  Medians,
minimum and maximum of 9 runs of 400 calls after 50 untimed calls, the legs
alternating.  One JSON line per leg on stdout.

usage: query_call_probe.py [ROOT [LABEL]]   ROOT: the tree whose rt_amd and
librt_amd.so to load (default: this one), LABEL: the lines' "build" field.
"""
import ctypes
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
root = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(HERE)
label = sys.argv[2] if len(sys.argv) > 2 else "this"
sys.path.insert(0, os.path.join(root, "ray-tracing-gpu_amd"))
import numpy as np
import torch
import rt_amd
assert rt_amd.__file__.startswith(root), rt_amd.__file__
L = rt_amd.lib()
scene = os.path.join(root, "tests", "golden", "scenes", "scene3.dat")
s = rt_amd.Scene(scene, 64, 32, 0)
ctx = rt_amd.Context(0)
ctx.upload(s)
n = 64
rng = np.random.default_rng(1)
rays = np.ascontiguousarray(np.concatenate([np.tile(np.asarray(s.frame.cam_pos[:], np.float32), (n, 1)),
                                            rng.normal(size=(n, 3)).astype(np.float32)], 1))
d = torch.from_numpy(rays).cuda()
t_, i_, n_ = (torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n * 3, device="cuda"))
rgb = torch.zeros(n * 3, device="cuda")
ht, hi, hn, hrgb = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
dev_aov = rt_amd.Aov(t_.data_ptr(), i_.data_ptr(), n_.data_ptr())
host_aov = rt_amd.Aov(ht.ctypes.data, hi.ctypes.data, hn.ctypes.data)
f = ctypes.byref(s.frame)
h = ctx._h
st = torch.cuda.Stream()
sp = st.cuda_stream
legs = {
    "trace_sync_host": lambda: L.rt_trace_rays(h, rays.ctypes.data, n, ctypes.byref(host_aov)),
    "filter_sync_host": lambda: L.rt_filter_rays(h, rays.ctypes.data, n, hrgb.ctypes.data),
    "shade_sync_host": lambda: L.rt_shade_rays(h, f, rays.ctypes.data, n, hrgb.ctypes.data),
    "trace_async": lambda: L.rt_trace_rays_async(h, d.data_ptr(), n, ctypes.byref(dev_aov), sp),
    "filter_async": lambda: L.rt_filter_rays_async(h, d.data_ptr(), n, rgb.data_ptr(), sp),
    "shade_async": lambda: L.rt_shade_rays_async(h, f, d.data_ptr(), n, rgb.data_ptr(), sp),
    "rejected_n0": lambda: L.rt_filter_rays(h, rays.ctypes.data, 0, hrgb.ctypes.data),
}
torch.cuda.synchronize()
REPS, ITERS = 9, 400
res = {k: [] for k in legs}
for k, fn in legs.items():
    for _ in range(50):
        assert fn() == 0
    torch.cuda.synchronize()
for rep in range(REPS):
    for k, fn in legs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(ITERS):
            fn()
        if k.endswith("async"):
            t1 = time.perf_counter()   # the enqueue cost alone
            torch.cuda.synchronize()
        else:
            t1 = time.perf_counter()
        res[k].append((t1 - t0) / ITERS * 1e6)
for k, v in res.items():
    print(json.dumps({"build": label, "leg": k, "n": n, "us_per_call_median": round(statistics.median(v), 3),
                      "us_min": round(min(v), 3), "us_max": round(max(v), 3)}), flush=True)
ctx.close()
