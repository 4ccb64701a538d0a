"""Seeded hard scenes in the reference's .dat format (test input generator):
what the other generators (fuzz_scenes.py, cull_scenes.py, wf_scenes.py)
never draw.  No `specular:`, so every comparison is bit-exact.

    hard_dat(family, seed, ntri=None, scale=1.0) -> str

families

* ties          groups of coincident surfaces written 2-3 times, far apart in
                the file (first member near the top, last at the very end),
                with different colours and materials (one opaque, one
                `refract`, one `reflect`): the reference keeps the first in
                file order among equal distances, so the winner changes
                shading, shadow filtering and the bounce tree.  Groups (the
                group's name is the surface's name up to the last `_`):
                dtri (a triangle, identical vertex order), rtri (the same
                triangle with its vertices rotated: a near-tie, the distances
                may differ in the last bit), dpln (a plane), dqd (a sphere);
                then a fan of differently coloured triangles about one vertex
                and two sharing an edge.  ntri (NTRI_TIES) pads with small
                filler triangles scattered in view to the exact count; 3
                keeps the dtri group alone.
* tiny_stress   1-20 triangles of the kinds of TINY_KINDS (the surface's name
                is its kind and a number): cull_scenes.py's edge-on, oversized,
                sliver and speck geometry, a triangle straddling the camera
                along the view axis, one with a vertex within 0.02 of the
                camera, a light within 0.02 of a triangle, a light 3,000 units
                away; 0-3 planes, one oblique with a non-unit normal.  Seed 3
                draws every kind and three planes, seed 5 a single triangle;
                a scene without planes has a backdrop triangle, so that every
                scene has a receiver in shadow from each of its lights.
* quadrics      1-4 of QUADRIC_KINDS (named by kind), opaque, refractive or
                reflective, some transformed, the camera or a light inside a
                closed one on some seeds, and 1-3 triangles.
  quadrics/axis a level camera looks along the `v_quad: 0 0 0` quadric, so
                its middle pixel row has B == 0: hits at t = +inf.
* materials     a closed set — two facing planes, a sphere between them, two
                nested refractive spheres of equal ior, a few triangles —
                whose materials carry both `reflect` and `refract`, K from
                K_SET and ior from IOR_SET; one plane always has K >= 0.999.

scale multiplies every coordinate by a power of two (SCALES): points, light
and camera positions, `translate:`, plane constants, quadric `v_linear` (and
`v_const` by its square).  At scale 1 numbers are %.3f; a scaled scene prints
the %.3f values times the scale as %.9g.  Lines <= 78 characters.
"""
from __future__ import annotations

import numpy as np

FAMILIES = ("ties", "tiny_stress", "quadrics", "materials")
NTRI_TIES = (3, 20, 21, 256, 257, 1024, 1025, 1026)
SCALES = (2.0 ** -6, 2.0 ** 6, 2.0 ** 12)
TINY_KINDS = ("edge_cam", "edge_l0", "edge_l1", "oversized", "sliver", "speck", "straddle", "near_cam", "near_light",
              "plain")
QUADRIC_KINDS = ("cone", "hyp1", "hyp2", "parab", "cylx", "cylz", "ellmix", "lin", "slab")
K_SET = (0.0, 0.3, 0.999, 1.0, 1.2)
IOR_SET = (0.5, 1.0, 1.5, 2.4)


def _unit(v):
    return v / np.linalg.norm(v)


class _Scene:
    """Objects in file order; text() prints them at a scale."""

    def __init__(self, title, background, origin, eye=(0.0, 0.0, 0.0)):
        self.title, self.background = title, background
        self.origin, self.eye = np.asarray(origin, float), np.asarray(eye, float)
        self.lights, self.surfaces = [], []

    def light(self, pos, intens):
        self.lights.append((np.asarray(pos, float), intens))

    # material: a list of finished lines ("color: 1 2 3", "reflect: 0.500", ...)
    def tri(self, name, pts, material):
        self.surfaces.append(("Poly", name, [np.asarray(p, float) for p in pts], material, []))

    def plane(self, name, normal, const, material):
        self.surfaces.append(("Plane", name, (np.asarray(normal, float), float(const)), material, []))

    def quad(self, name, q, lin, const, material, mix=None, xform=()):
        self.surfaces.append(("Quad", name, (np.asarray(q, float), None if mix is None else np.asarray(mix, float),
                                             np.asarray(lin, float), float(const)), material, list(xform)))

    def text(self, scale=1.0):
        if scale == 1.0:
            def v(x, k=1.0):
                return " ".join("%.3f" % c for c in np.atleast_1d(x))
        else:
            def v(x, k=scale):
                return " ".join("%.9g" % (round(float(c), 3) * k) for c in np.atleast_1d(x))
        out = [f"* {self.title} (tests/hard_scenes.py)", "        background: %d %d %d" % tuple(self.background),
               "        origin: " + v(self.origin), "        eye: " + v(self.eye), "        up:  0.0 1.0 0.0"]
        for i, (p, intens) in enumerate(self.lights):
            out += [f"Lumiere: l{i}", "        position: " + v(p), "        intens: %.3f" % intens]
        for kind, name, g, material, xform in self.surfaces:
            out.append(f"{kind}: {name}")
            if kind == "Poly":
                out += ["        point: %d " % j + v(p) for j, p in enumerate(g)]
            elif kind == "Plane":
                out += ["        v_linear: " + v(g[0], 1.0), "        v_const: " + v(g[1])]
            else:
                q, mix, lin, const = g
                out.append("        v_quad: " + " ".join("%.6f" % c for c in q))
                if mix is not None:
                    out.append("        v_mixte: " + " ".join("%.6f" % c for c in mix))
                out += ["        v_linear: " + v(lin), "        v_const: " + v(const, scale * scale)]
            out += ["        " + m for m in material]
            for op, val in xform:
                out.append(f"        {op}: " + (v(val) if op == "translate" else v(val, 1.0)))
        text = "\n".join(out) + "\n"
        assert max(len(l) for l in text.split("\n")) <= 78
        assert "specular" not in text
        return text


def _color(rng, lo=30):
    return "color: %d %d %d" % tuple(rng.integers(lo, 256, 3))


def _opaque(rng):
    return [_color(rng)]


def _refract(rng):
    return [_color(rng, 120), "refract: %.3f %.3f" % (rng.uniform(0.4, 0.7), rng.uniform(1.1, 1.6))]


def _reflect(rng):
    return [_color(rng), "reflect: %.3f" % rng.uniform(0.4, 0.7)]


def _three(rng):
    """An opaque, a refractive and a reflective material, in a seeded order."""
    m = [_opaque(rng), _refract(rng), _reflect(rng)]
    return [m[i] for i in rng.permutation(3)]


def _sphere(c, r, q=(1.0, 1.0, 1.0)):
    """v_quad, v_linear, v_const of sum q (p - c)^2 = r^2."""
    q, c = np.asarray(q, float), np.asarray(c, float)
    return q, -2.0 * q * c, float((q * c * c).sum() - r * r)


# ---------------------------------------------------------------------- ties
def _ties(rng, ntri):
    ntri = 20 if ntri is None else ntri
    if ntri not in NTRI_TIES:
        raise ValueError(f"ties: ntri is one of {NTRI_TIES}")
    S = _Scene("hard scene: ties", (15, 20, 60), rng.uniform([-25, 25, 150], [25, 45, 170]))
    S.light((60.0, 120.0, 90.0), 0.6)
    S.light((-80.0, 50.0, 60.0), 0.4)
    mid, last = [], []  # (add, name, material, k, is a triangle) of the groups' later members

    def group(name, add, count, is_tri=False):
        mats = _three(rng)[:count]
        add(f"{name}_0", mats[0], 0)
        for k in range(1, count):
            (last if k == count - 1 else mid).append((add, f"{name}_{k}", mats[k], k, is_tri))

    a = rng.uniform([-38, -12, -10], [-30, -6, 0])
    pts = [a, a + rng.uniform([28, -2, -4], [36, 4, 4]), a + rng.uniform([10, 26, -6], [20, 34, 6])]
    group("dtri", lambda n, m, k: S.tri(n, pts, m), 3, is_tri=True)
    if ntri > 3:
        b = rng.uniform([2, -14, 0], [8, -8, 12])
        rp = [b, b + rng.uniform([26, -3, -5], [34, 3, 5]), b + rng.uniform([8, 22, -8], [18, 30, 8])]
        group("rtri", lambda n, m, k: S.tri(n, rp[k:] + rp[:k], m), 3, is_tri=True)
    group("dpln", lambda n, m, k: S.plane(n, (0.0, 1.0, 0.0), 24.0, m), int(rng.integers(2, 4)))
    sq = _sphere(rng.uniform([-14, 24, -30], [14, 32, -10]), rng.uniform(11, 15))
    group("dqd", lambda n, m, k: S.quad(n, *sq, m), int(rng.integers(2, 4)))
    if ntri > 3:
        hub = rng.uniform([-6, 2, 28], [6, 8, 36])
        ring = [hub + 11.0 * np.array([np.cos(t), np.sin(t), 0.15 * np.sin(3 * t)])
                for t in np.linspace(0.3, 0.3 + 2 * np.pi * 4 / 5, 5)]
        for k in range(4):  # a fan about the hub: every triangle shares an edge with the next
            S.tri(f"fan_{k}", [hub, ring[k], ring[k + 1]], _opaque(rng))
        e0, e1 = rng.uniform([-40, 28, 10], [-34, 32, 20]), rng.uniform([-22, 36, 10], [-16, 42, 20])
        for k, side in enumerate((1.0, -1.0)):  # two triangles sharing the edge e0 e1
            S.tri(f"edge_{k}", [e0, e1, (e0 + e1) / 2 + side * np.array([7.0, -7.0, 3.0])], _opaque(rng))
    nfill = ntri - sum(1 for s in S.surfaces if s[0] == "Poly") - sum(1 for m in mid + last if m[4])
    assert nfill >= 0
    size = min(2.5, 45.0 / np.sqrt(max(nfill, 1)))
    for i in range(nfill):
        if i == nfill // 2:
            for add, n, m, k, _ in mid:
                add(n, m, k)
            mid = []
        c = rng.uniform([-45, -20, -25], [45, 50, 45])
        S.tri(f"fill{i}", [c + rng.normal(size=3) * size for _ in range(3)], _opaque(rng))
    for add, n, m, k, _ in mid + last:
        add(n, m, k)
    assert sum(1 for s in S.surfaces if s[0] == "Poly") == ntri
    return S


# --------------------------------------------------------------- tiny_stress
# The draw of each seed, chosen so that every scene of SEEDS meets the
# conditions of test_hard_scenes.py (a shadow boundary of every light, every
# kind but the speck seen) and not only the set as a whole.
# Seeds 2 and 3, the scaled ones: at 2^-6 its light 0.02 from a triangle is 0.0003
# from it, and the reference's own code stops on an assertion when it shades
# a point within 0.01 of a light; in these draws no pixel's ray hits one.
_TINY_DRAW = [10, 4, 22, 0, 12, 3]


def _tiny_stress(seed):
    rng = np.random.default_rng([FAMILIES.index("tiny_stress"), seed, _TINY_DRAW[seed % len(_TINY_DRAW)]])
    cam = rng.uniform([-30, 0, 55], [30, 30, 80])
    S = _Scene("hard scene: tiny_stress", (10, 10, 120), cam)
    view = _unit(-cam)
    side = _unit(np.cross(view, [0.0, 1.0, 0.0]))
    up = np.cross(side, view)
    l0 = rng.uniform([-60, 40, 20], [60, 90, 60])
    l1 = rng.uniform([-30, 5, -10], [30, 30, 20])
    n = rng.normal(size=3)  # the far light: above and in front of the scene
    far = _unit([n[0], abs(n[1]) + 0.5, abs(n[2]) + 0.5]) * 3000.0
    nplanes = seed % 4
    # every seed draws another window of the kinds' cycle, 3 to 10 kinds wide;
    # every sixth a single triangle, the lower edge of the list's size
    kinds = [TINY_KINDS[(3 * seed + k) % len(TINY_KINDS)] for k in range(3 + (seed * 5) % 8)]
    if seed % 6 == 5:
        kinds = ["plain"]
    elif nplanes == 0 and "plain" not in kinds:  # without a plane a triangle receives the shadows
        kinds.append("plain")
    budget = 1 if len(kinds) == 1 else int(rng.integers(len(kinds), 21))
    tris = []

    def edge_on(apex, off, size=12.0):
        """In the plane through a point `off` beside the apex (0: edge-on)."""
        q = rng.uniform([-20, -10, -20], [20, 15, 10])
        a = _unit(apex - q)
        w = _unit(np.cross(a, rng.normal(size=3)))
        n = np.cross(a, w)
        s = size * rng.uniform(0.4, 1.0)
        return [q + off * n + s * (x * a + y * w) for x, y in rng.uniform(-1, 1, (3, 2))]

    def make(kind):
        if kind == "edge_cam":
            # exact, or seen about a pixel wide; long, so that it is seen in a handful of pixels
            return edge_on(cam, rng.choice([0.0, 1.5, 4.0]), 30.0)
        if kind == "edge_l0":
            return edge_on(l0, 0.0)
        if kind == "edge_l1":
            return edge_on(l1, 0.0)
        if kind == "oversized":
            c = rng.uniform([-40, -10, -120], [40, 30, -40])
            d = _unit(rng.normal(size=3))
            e = _unit(np.cross(d, rng.normal(size=3)))
            return [c - 200 * d - 60 * e, c + 200 * d - 60 * e, c + 170 * e]
        if kind == "sliver":
            c = rng.uniform([-20, -10, -20], [20, 15, 10])
            d = _unit(rng.normal(size=3)) * rng.uniform(5, 30)
            if rng.random() < 0.5:  # across the view near the camera: wide enough there to meet some pixels' rays
                a = rng.uniform(0, np.pi)
                d = _unit(np.cos(a) * side + np.sin(a) * up + rng.uniform(-0.3, 0.3) * view) * rng.uniform(5, 30)
                c = cam + view * rng.uniform(3, 8) + side * rng.uniform(-1, 1) + up * rng.uniform(-1, 1) - d / 2
            e = _unit(np.cross(d, view)) * rng.uniform(0.005, 0.05)
            return [c, c + d, c + d * 0.5 + e]
        if kind == "speck":
            c = cam + view * rng.uniform(1.0, 2.5) - side * rng.uniform(0.05, 0.2) + up * rng.uniform(0.05, 0.2)
            return [c, c + 0.05 * side, c + 0.05 * up]
        if kind == "straddle":  # from behind the camera to far ahead of it, under the view axis
            b = cam - up * rng.uniform(1.5, 4.0)
            return [b - 25 * view - 6 * side, b - 25 * view + 6 * side, b + 90 * view + rng.uniform(-4, 4) * side]
        if kind == "near_cam":  # a vertex within 0.02 of the camera, the rest ahead and to one side
            v0 = cam + 0.012 * _unit(rng.normal(size=3))
            return [v0, cam + 30 * view + 12 * side + 2 * up, cam + 30 * view + 7 * side - 4 * up]
        if kind == "near_light":  # its plane passes within 0.02 of light 1
            n = _unit(rng.normal(size=3))
            a = _unit(np.cross(n, [0.3, 1.0, 0.2]))
            b = np.cross(n, a)
            c = l1 - 0.015 * n
            return [c - 9 * a - 6 * b, c + 9 * a - 6 * b, c + 11 * b]
        if nplanes == 0 and not any(k == "plain" for k, _ in tris):  # a backdrop facing the camera and the lights
            c = rng.uniform([-10, -5, -45], [10, 5, -35])
            return [c + [x, y, rng.uniform(-5, 5)] for x, y in ((-75.0, -60.0), (75.0, -60.0), (0.0, 70.0))]
        c = rng.uniform([-25, -10, -25], [25, 15, 5])
        return [c + rng.normal(size=3) * 9.0 for _ in range(3)]

    for kind in kinds:
        tris.append((kind, make(kind)))
    while len(tris) < budget:
        kind = kinds[int(rng.integers(len(kinds)))]
        tris.append((kind, make(kind)))
    S.light(l0, 0.5)
    S.light(l1, 0.4)
    S.light(far, 0.3)
    if nplanes >= 1:
        S.plane("ground", (0.0, 1.0, 0.0), 20.0, ["color: 10 235 30", "ambient: 0.300", "diffus: 0.700"])
    if nplanes >= 2:  # oblique, |n| = 3.2: the loader normalises it and rescales the constant; a ramp behind the origin
        S.plane("oblique", (0.6, 2.9, 1.2), 64.0, [_color(rng)])
    if nplanes >= 3:
        S.plane("wall", (0.0, 0.0, 1.0), 150.0, [_color(rng)])
    opaque_at = int(rng.integers(len(tris)))
    for i, (kind, pts) in enumerate(tris):
        r = rng.random()
        m = _opaque(rng) if (i == opaque_at or r < 0.7) else (_refract(rng) if r < 0.85 else _reflect(rng))
        S.tri(f"{kind}_{i}", pts, m)
    assert 1 <= len(tris) <= 20
    return S


# ------------------------------------------------------------------ quadrics
def _quadric(S, rng, kind, name, c, material, xform):
    r = rng.uniform(7, 12)
    k = rng.uniform(0.15, 0.4)
    mix = None
    if kind == "cone":
        q, lin, const = _sphere(c, 0.0, (1.0, -k, 1.0))
    elif kind == "hyp1":
        q, lin, const = _sphere(c, r * 0.6, (1.0, -k, 1.0))
    elif kind == "hyp2":
        q, lin, const = _sphere(c, r * 0.6, (-1.0, k * 4, -1.0))
    elif kind == "parab":  # (x - cx)^2 + (z - cz)^2 = a (y - cy)
        a = rng.uniform(6, 14)
        q, lin, const = np.array([1.0, 0.0, 1.0]), np.array([-2 * c[0], -a, -2 * c[2]]), c[0] ** 2 + c[2] ** 2 + a * c[1]
    elif kind == "cylx":
        q, lin, const = _sphere(c, r * 0.7, (0.0, 1.0, 1.0))
        mix = rng.uniform(-0.3, 0.3, 3) * [1.0, 0.0, 0.0]
    elif kind == "cylz":
        q, lin, const = _sphere(c, r * 0.7, (1.0, 1.0, 0.0))
    elif kind == "ellmix":
        q, lin, const = _sphere(c, r * 1.3, rng.uniform(0.6, 2.0, 3))
        mix = rng.uniform(-0.25, 0.25, 3)
    elif kind == "lin":  # no quadratic term: every ray takes A == 0, t = -C / 2B
        n = np.array([rng.uniform(-0.2, 0.2), 1.0, rng.uniform(-0.2, 0.2)])
        q, lin, const, xform = np.zeros(3), n, rng.uniform(16, 26), ()
    elif kind == "slab":  # x^2 = R^2: two parallel planes, the camera between them (A == 0 for a ray with d.x == 0)
        q, lin, const, xform = *_sphere((0.0, 0.0, 0.0), r * 5.0, (1.0, 0.0, 0.0)), [x for x in xform if x[0] != "scale"]
    else:
        raise ValueError(kind)
    S.quad(name, q, lin, const, material, mix=mix, xform=xform)


def _quadrics(rng, seed):
    counts = (4, 3, 4, 2, 4, 1)
    n = counts[seed % len(counts)]
    first = sum(counts[: seed % len(counts)]) + seed // len(counts)
    kinds = [QUADRIC_KINDS[(first + i) % len(QUADRIC_KINDS)] for i in range(n)]
    cam = rng.uniform([-30, 5, 90], [30, 35, 120])
    S = _Scene("hard scene: quadrics", (25, 25, 45), cam, eye=(0.0, 4.0, 0.0))
    lights = [rng.uniform([-70, 40, 30], [70, 90, 80]), rng.uniform([-50, 10, -20], [50, 40, 60])]
    centres = [np.array([x, rng.uniform(-4, 12), rng.uniform(-25, 15)])
               for x in (np.linspace(-30, 30, n) if n > 1 else [0.0])]
    if seed % 3 == 1:  # the camera inside a closed quadric (a big sphere about it)
        S.quad("shell", *_sphere(cam + rng.uniform(-3, 3, 3), 260.0), [_color(rng, 90)])
    if seed % 3 == 2:  # a light inside a closed, refractive quadric
        S.quad("lamp", *_sphere(lights[1] + rng.uniform(-1, 1, 3), 6.0, (1.0, 0.7, 1.3)),
               [_color(rng, 150), "refract: 0.700 1.300"])
    for i, (kind, c) in enumerate(zip(kinds, centres)):
        material = (_opaque, _refract, _reflect)[int(rng.integers(3))](rng)
        xform = []
        if rng.random() < 0.5:
            xform.append(("rotate", rng.uniform(-25, 25, 3)))
        if rng.random() < 0.4:
            xform.append(("translate", rng.uniform(-6, 6, 3)))
        if rng.random() < 0.3:
            xform.append(("scale", rng.uniform(0.7, 1.4, 3)))
        _quadric(S, rng, kind, f"{kind}_{i}", c, material, xform)
    for i in range(1 + seed % 3):
        c = rng.uniform([-30, -5, 20], [30, 25, 45])
        S.tri(f"t{i}", [c + rng.normal(size=3) * 7.0 for _ in range(3)],
              _opaque(rng) if i == 0 else (_refract, _reflect)[i % 2](rng))
    for p, intens in zip(lights, (0.6, 0.4)):
        S.light(p, intens)
    return S


def _quadrics_axis():
    """A level camera on the z axis and `v_quad: 0 0 0`, `v_linear: 0 1 0`: the
    rays of the middle row (2 py == h, h even) have d.y == 0, so B == 0 and
    t = -C / 2B = +inf with the camera under the surface (C < 0): a hit at
    infinity, whose point has a NaN; a sphere and a triangle are ordinary."""
    S = _Scene("hard scene: quadrics/axis", (25, 25, 45), (0.0, 10.0, 120.0), eye=(0.0, 10.0, 0.0))
    S.light((40.0, 90.0, 60.0), 0.6)
    S.quad("lin_0", np.zeros(3), (0.0, 1.0, 0.0), -30.0, ["color: 200 180 90"])  # y = 30, above the camera
    S.quad("ball", *_sphere((-18.0, 4.0, 0.0), 14.0), ["color: 90 120 220", "reflect: 0.400"])
    S.tri("t0", [(8.0, -10.0, 10.0), (34.0, -8.0, 0.0), (20.0, 22.0, 5.0)], ["color: 220 60 60"])
    return S


# ----------------------------------------------------------------- materials
def _materials(rng, seed):
    S = _Scene("hard scene: materials", (30, 40, 70), rng.uniform([-30, 0, 110], [30, 30, 140]))
    S.light((30.0, 50.0, 80.0), 0.6)
    S.light((-50.0, 20.0, 30.0), 0.3)

    def both(kr=None, kt=None):
        kr = float(rng.choice(K_SET)) if kr is None else kr
        kt = float(rng.choice(K_SET)) if kt is None else kt
        return [_color(rng, 80), "reflect: %.3f" % kr, "refract: %.3f %.3f" % (kt, float(rng.choice(IOR_SET)))]

    # the facing planes y = -40 and y = 70; one of them keeps rays alive at
    # any depth: K >= 1 on even seeds, 0.999 on odd ones (no K >= 1 anywhere)
    ks = [k for k in K_SET if k < 1.0] if seed % 2 else K_SET
    def pick():
        return float(rng.choice(ks))
    strong = (1.2 if seed % 4 == 0 else 1.0) if seed % 2 == 0 else 0.999
    S.plane("floor", (0.0, 1.0, 0.0), 40.0, both(kr=strong, kt=pick()))
    S.plane("ceiling", (0.0, -1.0, 0.0), 70.0, both(kr=pick(), kt=pick()))
    S.quad("ball", *_sphere(rng.uniform([-25, 0, -10], [-10, 20, 10]), 16.0), both(kr=pick(), kt=pick()))
    # two nested refractive spheres of equal ior: the reference's inside test
    # (rior == m.ior) is true at the inner sphere's first hit
    c = rng.uniform([12, 5, -5], [28, 20, 15])
    ior = float(rng.choice([i for i in IOR_SET if i != 1.0]))
    for name, r in (("outer", 17.0), ("inner", 8.0)):
        S.quad(name, *_sphere(c, r), [_color(rng, 120), "reflect: %.3f" % pick(), "refract: 0.999 %.3f" % ior])
    for i in range(int(rng.integers(3, 7))):
        p = rng.uniform([-35, -25, -20], [35, 45, 40])
        S.tri(f"t{i}", [p + rng.normal(size=3) * 10.0 for _ in range(3)], both(kr=pick(), kt=pick()))
    return S


def has_k_at_least_1(text: str) -> bool:
    """A `reflect:` or `refract:` coefficient >= 1 somewhere in the scene."""
    for line in text.split("\n"):
        w = line.split()
        if w and w[0] in ("reflect:", "refract:") and float(w[1]) >= 1.0:
            return True
    return False


def hard_dat(family: str, seed: int, ntri=None, scale: float = 1.0) -> str:
    """The scene of a family and seed (see the module docstring); ntri: the
    triangle count of `ties`; scale: a power of two applied to every
    coordinate (the `scale` family is any family at a scale other than 1)."""
    rng = np.random.default_rng([FAMILIES.index(family.split("/")[0]), seed])
    if ntri is not None and family != "ties":
        raise ValueError("ntri is for the ties family")
    if family == "ties":
        S = _ties(rng, ntri)
    elif family == "tiny_stress":
        S = _tiny_stress(seed)
    elif family == "quadrics":
        S = _quadrics(rng, seed)
    elif family == "quadrics/axis":
        S = _quadrics_axis()
    elif family == "materials":
        S = _materials(rng, seed)
    else:
        raise ValueError(family)
    return S.text(scale)


# ---- views of a scene's text, for the tests' conditions
def surfaces(text: str):
    """[(keyword, name)] of the surfaces in file order: the index is the id
    the renderers report."""
    out = []
    for line in text.split("\n"):
        w = line.split()
        if len(w) == 2 and w[0] in ("Poly:", "Plane:", "Quad:"):
            out.append((w[0][:-1], w[1]))
    return out


def groups(text: str, prefixes=("dtri", "rtri", "dpln", "dqd")):
    """{group: [file indices of its members, in file order]} of a ties scene."""
    out = {}
    for i, (_, name) in enumerate(surfaces(text)):
        g = name.rsplit("_", 1)[0]
        if g in prefixes:
            out.setdefault(g, []).append(i)
    return out


def without(text: str, drop) -> str:
    """The scene without the objects (surfaces or lights) whose name drop(name) accepts."""
    out, keep = [], True
    for line in text.split("\n"):
        w = line.split()
        if len(w) == 2 and w[0] in ("Poly:", "Plane:", "Quad:", "Lumiere:"):
            keep = not drop(w[1])
        if keep:
            out.append(line)
    return "\n".join(out)


# ---- the frames pinned to the reference's own code (tests/golden/hard.npz,
# make_hard_golden.py): (family, seed, ntri, scale, width, height, depth).
# Even seeds render 48 x 36, odd ones the ragged 47 x 35.
DEPTH = {"ties": 3, "tiny_stress": 3, "quadrics": 4, "materials": 6}  # the depth with bounces of a family
SEEDS = range(6)


def size(seed: int):
    return (47, 35) if seed % 2 else (48, 36)


# the scaled scenes: the ties at 20 triangles, the tiny_stress seed whose
# oblique plane is in view, and the one that draws every kind and three planes
# (where the oversized triangle hides that plane from the camera)
SCALED = (("ties", 0), ("tiny_stress", 2), ("tiny_stress", 3))


GOLDEN_FRAMES = (
    [(fam, seed, None, 1.0, *size(seed), 0) for fam in FAMILIES for seed in range(4)] +
    [(fam, seed, None, 1.0, *size(seed), DEPTH[fam]) for fam in FAMILIES for seed in range(2)] +
    [("ties", 0, n, 1.0, 48, 36, 0) for n in (3, 21, 257, 1025)] + [("ties", 0, 1026, 1.0, 47, 35, 2)] +
    [("tiny_stress", 3, None, 1.0, 47, 35, DEPTH["tiny_stress"])] +
    [(fam, seed, None, s, *size(seed), 0) for fam, seed in SCALED for s in SCALES] +
    [("quadrics/axis", 0, None, 1.0, 48, 36, 0), ("quadrics/axis", 0, None, 1.0, 48, 36, 3),
     ("materials", 0, None, 1.0, 24, 18, 9)])


def golden_key(family, seed, ntri, scale, w, h, depth) -> str:
    return "%s_s%d_n%s_x%d_%dx%d_d%d" % (family.replace("/", "-"), seed, ntri or 0, int(np.log2(scale)), w, h, depth)


def text_sha(text: str) -> str:
    import hashlib

    return hashlib.sha256(text.encode()).hexdigest()
