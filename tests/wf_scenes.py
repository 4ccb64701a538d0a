"""Seeded small scenes for the wavefront bounce levels (test input
generator), in the reference's .dat format: %.3f numbers, lines <= 78
characters (Scene.cpp:231-501).  The meshes are rt_amd.synth.heightfield_dat's
triangles (the same vertices, its camera and ground plane) with a colour per
triangle from the seed — a ray that lands in another ray's slot shows — and
the family's materials:

* chain         every triangle `reflect: 0.7`: one child per node, and
                0.7^8 = 0.058 > 0.01, so level 8 is alive — the ground plane
                reflects 0.7 too, or no ray would bounce eight times: an open
                heightfield sends its reflections to the sky, the mirror
                below it keeps them between the two;
* split         every triangle `reflect: 0.3`, every other one also
                `refract: 0.4 1.5`: 2-child nodes, inside/out IOR flips
                (0.4^5 = 0.01024 > 0.01: level 5 is alive, level 6 is not);
* refract_only  every third triangle `refract: 0.6 1.3` and no reflect (nodes
                with a refracted child only), the rest opaque;
* mixed         split, a reflective ground plane, a reflective sphere and a
                refractive ellipsoid with v_mixte terms above the mesh: bounce
                rays hit planes and quadrics, translucent surfaces filter
                shadow rays;
* soup          long, mutually overlapping triangles and slivers (scales 0.05
                to 400 across an 80-unit box, all `reflect: 0.6`), a plane and
                a sphere, one light: BVH walks of many steps.

Triangle counts: a grid of the table below, with triangles dropped from or
added to the end of the file (63 / 64 / 65 around the BVH's minimum, 1,024 /
1,026 around the cluster threshold)."""
from __future__ import annotations

import hashlib

import numpy as np

from rt_amd import synth

FAMILIES = ("chain", "split", "refract_only", "mixed", "soup")
# triangles -> (cols, rows) of the heightfield grid they are cut from / added to
GRIDS = {63: (8, 4), 64: (8, 4), 65: (8, 4), 96: (8, 6), 1024: (32, 16), 1026: (32, 16), 1600: (40, 20)}
LIGHTS = [((100.0, 400.0, 360.0), 0.7), ((-200.0, 300.0, 100.0), 0.4), ((0.0, 250.0, -300.0), 0.3)]


def _triangles(cols: int, rows: int):
    """heightfield_dat's triangles: per triangle its three `point:` lines."""
    out = []
    for line in synth.heightfield_dat(cols, rows).split("\n"):
        if line.startswith("Poly:"):
            out.append([])
        elif line.startswith("        point:"):
            out[-1].append(line)
    assert len(out) == 2 * cols * rows and all(len(t) == 3 for t in out)
    return out


def _extra(k: int):
    """Triangle k past the grid's: a tilted one floating above the mesh."""
    x = -100.0 + 30.0 * k
    return ["        point: 0 %.3f 10.000 -150.000" % x, "        point: 1 %.3f 10.000 -110.000" % x,
            "        point: 2 %.3f 18.000 -150.000" % (x + 30.0)]


def _header(lights: int, plane_reflect: float = 0.0):
    out = ["* wavefront test scene (tests/wf_scenes.py)", "        background: 0 0 150",
           "        origin: 0.0 120.0 250.0", "        eye: 0.0 0.0 -80.0", "        up:  0.0 1.0 0.0"]
    for i, (p, intens) in enumerate(LIGHTS[:lights]):
        out += [f"Lumiere: light_{i + 1}", "        position: %.3f %.3f %.3f" % p, "        intens:   %.3f" % intens]
    out += ["Plane: plane_1", "        v_linear: 0.0 1.0 0.0", "        v_const:  45.0", "        color:   10 255 11",
            "        ambient: 0.3", "        diffus:  0.7"]
    if plane_reflect:
        out.append("        reflect: %.3f" % plane_reflect)
    return out


def _material(family: str, i: int):
    if family == "chain":
        return ["        reflect: 0.700"]
    if family in ("split", "mixed"):
        return ["        reflect: 0.300"] + (["        refract: 0.400 1.500"] if i % 2 == 0 else [])
    if family == "refract_only":
        return ["        refract: 0.600 1.300"] if i % 3 == 0 else []
    raise ValueError(family)


def _soup(ntri: int, lights: int, seed: int, spread: float):
    """The random soup of test_bvh_walk_equals_brute_force_on_random_meshes.
    spread scales its two long classes of triangles (30 and 400 units at 1.0,
    that test's): their boxes overlap most of the 80-unit scene, every walk
    visits them, so spread sets how many walks go over the trace launch's
    budget."""
    rng = np.random.default_rng(seed)
    out = ["* wavefront test scene (tests/wf_scenes.py): soup", "        background: 10 10 30",
           "        origin: 0.0 4.0 95.0", "        eye: 0.0 0.0 0.0", "        up:  0.0 1.0 0.0"]
    for i, (p, intens) in enumerate([((10.0, 50.0, 40.0), 0.8), ((-60.0, 20.0, 70.0), 0.3)][:lights]):
        out += [f"Lumiere: light_{i + 1}", "        position: %.3f %.3f %.3f" % p, "        intens:   %.3f" % intens]
    for i in range(ntri):
        c = rng.uniform(-40, 40, 3)
        sc = [0.05, 2.0, 30.0 * spread, 400.0 * spread][i % 4] if i % 7 else 0.5
        pts = c + rng.normal(size=(3, 3)) * sc
        if i % 5 == 0:  # sliver
            pts[2] = pts[0] + (pts[1] - pts[0]) * 0.5 + rng.normal(size=3) * 1e-2
        out.append(f"Poly: t{i}")
        for j in range(3):
            out.append("        point: %d %.3f %.3f %.3f" % ((j,) + tuple(pts[j])))
        out.append("        color: %d %d %d" % tuple(rng.integers(40, 256, 3)))
        out.append("        reflect: 0.600")
    out += ["Plane: p", "        v_linear: 0.0 1.0 0.0", "        v_const: 45.0", "        color: 10 200 10"]
    out += ["Quad: q", "        v_quad: 1.0 1.0 1.0", "        v_const: -25.0", "        color: 10 10 200",
            "        reflect: 0.300"]
    return out


def wf_dat(family: str, ntri: int, lights: int = 2, seed: int = 1, spread: float = 1.0) -> str:
    """spread: the soup's only (see _soup)."""
    if family not in FAMILIES:
        raise ValueError(family)
    if family == "soup":
        assert ntri >= 1025
        out = _soup(ntri, min(lights, 2), seed, spread)
    else:
        rng = np.random.default_rng(seed)
        cols, rows = GRIDS[ntri]
        tris = _triangles(cols, rows)
        tris = tris[:ntri] + [_extra(k) for k in range(ntri - len(tris))]
        out = _header(lights, plane_reflect={"mixed": 0.4, "chain": 0.7}.get(family, 0.0))
        for i, pts in enumerate(tris):
            out += [f"Poly: t{i}"] + pts + ["        color:  %d %d %d" % tuple(rng.integers(40, 256, 3))]
            out += _material(family, i)
        if family == "mixed":
            # a sphere of radius 22 about (-60, 15, -90); an ellipsoid about
            # (70, 12, -60) with mixed terms (still positive definite)
            out += ["Quad: sphere", "        v_quad: 1.0 1.0 1.0", "        v_linear: 120.0 -30.0 180.0",
                    "        v_const: 11441.0", "        color: 230 230 250", "        reflect: 0.500"]
            out += ["Quad: ellipsoid", "        v_quad: 1.0 2.0 1.5", "        v_mixte: 0.200 0.100 -0.150",
                    "        v_linear: -140.0 -48.0 180.0", "        v_const: 9988.0", "        color: 250 200 120",
                    "        refract: 0.500 1.400"]
    text = "\n".join(out) + "\n"
    assert max(len(l) for l in text.split("\n")) <= 78
    assert text.count("Poly:") == ntri
    return text


def text_sha(text: str) -> str:
    return hashlib.sha256(text.encode()).hexdigest()


# The frames pinned to the reference's own code (tests/golden/wf_small.npz,
# make_wf_golden.py): (family, triangles, width, height, depth), two lights.
GOLDEN_FRAMES = [("split", 1600, 96, 64, 3), ("split", 1600, 96, 64, 5), ("split", 96, 96, 64, 3),
                 ("mixed", 1600, 96, 64, 4), ("chain", 1600, 96, 64, 8)]


def golden_key(family, ntri, w, h, depth) -> str:
    return f"wf_{family}_{ntri}_{w}x{h}_d{depth}"


def sha_key(family, ntri) -> str:
    return f"sha256_{family}_{ntri}"
