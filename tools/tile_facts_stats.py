"""Counts of the stored tile facts (rt_cull.h tile_facts_pack) of C2, C4 and
C1 after a camera's second frame, read back through rt_debug_tiny_words and
rt_debug_tiny_facts: tiles by kind, and per light the no-op and all-gated
pairs against the light's class; and the lean tiles (rt_tile.h): by the rule,
from the two words, and as the stored lean records flag them
(rt_debug_tiny_lean).  One JSON line.

    python tools/tile_facts_stats.py > profiles/r13/tile_facts/fact_stats.json
"""
import ctypes, json, os, sys
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ray-tracing-gpu_amd")); sys.path.insert(0, REPO)
import bench, rt_amd
out = {}
for cfg in ("c2", "c4", "c1"):
    name, W, H, depth = bench.CONFIGS[cfg]
    s = rt_amd.Scene(bench.scene_path(name), W, H, depth)
    c = rt_amd.Context(0)
    c.upload(s)
    labels = []
    for _ in range(3):
        c.render(s.frame); labels.append(c.stats().kernel)
    L = rt_amd.lib()
    ty, tx = (H + 7) // 8, (W + 7) // 8
    res = {}
    for fn in ("rt_debug_tiny_words", "rt_debug_tiny_facts"):
        f = getattr(L, fn); f.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int]; f.restype = ctypes.c_int
        a = np.zeros(ty * tx, np.uint32)
        assert f(c._h, None, a.ctypes.data, a.size) == 0
        res[fn] = a
    wd, fx = res["rt_debug_tiny_words"], res["rt_debug_tiny_facts"]
    kind = fx & 7
    nl = 3 if cfg != "c1" else 1
    d = {"tiles": int(fx.size), "labels": labels, "kind_none": int((kind == 0).sum()), "plane_slot0": int(((kind == 1) & ((fx >> 3 & 31) == 0)).sum()),
         "plane_slot1": int(((kind == 1) & ((fx >> 3 & 31) == 1)).sum()), "triangle": int((kind == 2).sum()),
         "search": int((kind == 3).sum()), "miss": int((kind == 4).sum()), "lights": []}
    for li in range(nl):
        b = fx >> (8 + 2 * li) & 3; k = wd >> (20 + 2 * li) & 3
        d["lights"].append({"noop": int((b & 1 != 0).sum()), "all_gated": int((b & 2 != 0).sum()),
                            "all_gated_class1": int(((b & 2 != 0) & (k == 1)).sum()),
                            "noop_class": [int(((b & 1 != 0) & (k == q)).sum()) for q in range(3)],
                            "class": [int((k == q).sum()) for q in range(3)]})
    # lean: one plane or kept triangle with a known index, every light classed (a no-op counts), no translucent surface
    lean = ((kind == 1) | (kind == 2)) & (fx >> 20 != 0)
    for li in range(nl):
        lean &= ((wd >> (20 + 2 * li) & 3) != 0) | ((fx >> (8 + 2 * li) & 1) != 0)
    if (s.arrays()[2][:, 8] != 0).any() or nl > 6:
        lean[:] = False
    d["lean_by_rule"] = int(lean.sum())
    d["lean_plane"], d["lean_triangle"] = int((lean & (kind == 1)).sum()), int((lean & (kind == 2)).sum())
    f = L.rt_debug_tiny_lean; f.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int]; f.restype = ctypes.c_int
    rec = np.zeros(ty * tx * 16, np.uint32)
    assert f(c._h, None, rec.ctypes.data, ty * tx) == 0
    rk = rec.reshape(-1, 16)[:, 1] & 7
    d["lean_stored"] = int(((rk == 5) | (rk == 6)).sum())
    out[cfg] = d
print(json.dumps(out))
