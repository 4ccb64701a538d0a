#!/usr/bin/env python3
"""How many light-buffer lookups of a frame find an empty cell, and how many
the occupied-direction bound (RT_OPT_LB_REGION) removes.

    python tools/lb_region_shares.py [--scene tests/golden/scenes/scene2.dat] [--size 1920x1080]

Needs a device: the light buffer is built at upload and its cell offsets and
bounds are read back (rt_debug_lb_offsets, rt_debug_lb_region).  The primary
hits (planes and triangles; quadrics are not handled), the shadow rays' gates
and their cells are recomputed here in numpy, float64 for the hits and the
lookup's float32 steps for the cell: figures for a README, not a parity check.
Prints one JSON line: per light and in total the shares of
  (a) gated shadow rays whose cell is empty,
  (b) (8 x 8 tile, light) pairs, of those with a gated lane, in which every
      gated lane's cell is empty,
  (c) such pairs in which no gated lane lies inside the bound (skipped waves),
  (d) gated shadow rays outside the bound (skipped lookups)."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ray-tracing-gpu_amd"))
import rt_amd  # noqa: E402


def lb_cell(d, R):
    d = d.astype(np.float32)
    ax, ay, az = np.abs(d[..., 0]), np.abs(d[..., 1]), np.abs(d[..., 2])
    fx = (ax >= ay) & (ax >= az)
    fy = ~fx & (ay >= az)
    fz = ~fx & ~fy
    face = np.where(fx, np.where(d[..., 0] >= 0, 0, 1), np.where(fy, np.where(d[..., 1] >= 0, 2, 3),
                                                                 np.where(d[..., 2] >= 0, 4, 5)))
    m = np.where(fx, ax, np.where(fy, ay, az))
    a = np.where(fx, d[..., 1], np.where(fy, d[..., 2], d[..., 0]))
    b = np.where(fx, d[..., 2], np.where(fy, d[..., 0], d[..., 1]))
    assert fz.shape == fx.shape
    inv = (np.float32(1) / np.maximum(m, np.float32(1e-30))).astype(np.float32)
    h = np.float32(0.5 * R)
    i = np.clip(np.floor((a * inv + np.float32(1)) * h).astype(np.int64), 0, R - 1)
    j = np.clip(np.floor((b * inv + np.float32(1)) * h).astype(np.int64), 0, R - 1)
    return (face * R + j) * R + i


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default=os.path.join(REPO, "tests", "golden", "scenes", "scene2.dat"))
    ap.add_argument("--size", default="1920x1080")
    args = ap.parse_args()
    w, h = (int(x) for x in args.size.split("x"))
    s = rt_amd.Scene(args.scene, w, h, 0)
    ctx = rt_amd.Context(0)
    ctx.upload(s)
    L = rt_amd.lib()
    nl = s.flat.n_lights
    info = np.zeros(3 + 3 * nl)
    L.rt_debug_lb_info.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    assert L.rt_debug_lb_info(ctx._h, info.ctypes.data, info.size) == 0 and info[0] == 1.0
    reg = np.zeros(6 * nl)
    L.rt_debug_lb_region.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    assert L.rt_debug_lb_region(ctx._h, reg.ctypes.data, reg.size) == 0, ctx._err()
    reg = reg.reshape(nl, 6)
    L.rt_debug_lb_offsets.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]

    # primary hits, float64
    f = s.frame
    t_, g, m, lights = s.arrays()
    px, py = np.meshgrid(np.arange(w), np.arange(h))
    d0 = np.stack([(2 * px * f.inv_w - 1) * f.half_w, (2 * py * f.inv_h - 1) * f.half_h, -np.ones_like(px, float)], -1)
    M = np.array(f.orient[:], np.float64).reshape(4, 4)[:3, :3]
    D = d0 @ M
    D /= np.linalg.norm(D, axis=-1, keepdims=True)
    O = np.array(f.cam_pos[:], np.float64)
    best = np.full((h, w), np.inf)
    N = np.zeros((h, w, 3))
    for k in range(len(t_)):
        if t_[k] == rt_amd.PLANE:
            n, cst = g[k, :3].astype(float), float(g[k, 3])
            vd = D @ n
            with np.errstate(divide="ignore", invalid="ignore"):
                t = -(n @ O + cst) / vd
        elif t_[k] == rt_amd.TRIANGLE:
            p0, p1, p2, n = (g[k, 3 * q: 3 * q + 3].astype(float) for q in range(4))
            e1, e2 = p1 - p0, p2 - p0
            pv = np.cross(D, e2)
            det = pv @ e1
            with np.errstate(divide="ignore", invalid="ignore"):
                tv = O - p0
                u = (pv @ tv) / det
                qv = np.cross(tv, e1)
                v = (D @ qv) / det
                t = (qv @ e2) / det
            t = np.where((u >= 0) & (v >= 0) & (u + v <= 1), t, np.inf)
        else:
            raise SystemExit("quadrics are not handled")
        ok = (t > 1e-4) & (t < best)
        best = np.where(ok, t, best)
        N[ok] = n
    hit = np.isfinite(best)
    P = O + np.where(hit, best, 0.0)[..., None] * D

    th, tw = -(-h // 8), -(-w // 8)
    tile = (py // 8) * tw + px // 8
    out = {"scene": os.path.basename(args.scene), "size": [w, h], "hit_share": float(hit.mean()), "lights": []}
    tot = np.zeros(7)
    for j in range(nl):
        R = int(info[3 + 3 * j])
        dcov = info[5 + 3 * j]
        off = np.zeros(6 * R * R + 1, np.uint32)
        assert L.rt_debug_lb_offsets(ctx._h, j, off.ctypes.data, off.size) == 0, ctx._err()
        occupied = off[1:] > off[:-1]
        assert int(occupied.sum()) == int(reg[j, 4])
        Lr = lights[j, :3].astype(float) - P
        dist = np.linalg.norm(Lr, axis=-1)
        gate = hit & ((Lr * N).sum(-1) > 0) & (dist <= dcov)
        d = -Lr / np.maximum(dist, 1e-30)[..., None]
        cell = lb_cell(d, R)
        empty = ~occupied[cell]
        inside = (d.astype(np.float32) @ reg[j, :3].astype(np.float32)) >= np.float32(reg[j, 3])
        pairs = np.bincount(tile[gate], minlength=th * tw) > 0
        any_full = np.bincount(tile[gate & ~empty], minlength=th * tw) > 0
        any_in = np.bincount(tile[gate & inside], minlength=th * tw) > 0
        row = np.array([gate.sum(), (gate & empty).sum(), pairs.sum(), (pairs & ~any_full).sum(),
                        (pairs & ~any_in).sum(), (gate & ~inside).sum(), occupied.sum()], float)
        tot += row
        out["lights"].append({"R": R, "cosB": float(reg[j, 3]), "cells_with_entries": int(row[6]),
                              "gated_rays": int(row[0]), "a_empty_cell": row[1] / max(row[0], 1),
                              "gated_pairs": int(row[2]), "b_pairs_all_empty": row[3] / max(row[2], 1),
                              "c_pairs_outside_bound": row[4] / max(row[2], 1),
                              "d_rays_outside_bound": row[5] / max(row[0], 1),
                              # (0 on the device by construction; here up to this script's float64 hit points)
                              "outside_bound_with_entries": int((gate & ~inside & ~empty).sum())})
    out["total"] = {"gated_rays": int(tot[0]), "a_empty_cell": tot[1] / max(tot[0], 1), "gated_pairs": int(tot[2]),
                    "b_pairs_all_empty": tot[3] / max(tot[2], 1), "c_pairs_outside_bound": tot[4] / max(tot[2], 1),
                    "d_rays_outside_bound": tot[5] / max(tot[0], 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
