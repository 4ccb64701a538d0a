"""The hard scenes (tests/hard_scenes.py) on the CPU: the oracle against the
frames the reference's own code rendered (tests/golden/hard.npz,
make_hard_golden.py), the CPU backend against the oracle, bit for bit, and —
on the oracle alone — the conditions that give each family its point, so that
a scene that lost it fails here and not silently:

* ties: inside a group of exact duplicates the winner is always the lowest
  file index; the groups' members win >= 15 % of the frame, every group wins
  somewhere, and without the duplicates that sit first in the file >= 15 % of
  the pixels change colour (the tie-break is visible in RGB).  The rtri group
  (rotated vertices) is a near-tie: its three distances are computed from
  other edges and may differ in the last bit, so any member may win a pixel;
  which one does is pinned by the id plane, not by a rule.
* tiny_stress: every kind of TINY_KINDS is the primary hit of at least four
  pixels in some seed — but `speck`: its |e1 x e2| = 0.0025 is under the
  reference's determinant cut (EPSILON = 0.01, Triangle.cpp:127-172), so no
  ray ever hits it; it stays in the lists the kernels cull — and in every
  seed every light has a shadow boundary (two neighbouring pixels of one
  planar surface, one lit by the light and one not).  One seed has a single
  triangle; the seed of the scaled scenes draws every kind.
* quadrics: every kind wins >= 1 % of some frame, the `v_quad: 0 0 0` kind
  >= 10 % of each of its frames.  quadrics/axis looks along that quadric so
  that B == 0 occurs: there t = -C / 2B = +inf is a hit (the id and t planes
  show it), the hit point has a NaN, `dot(light - P, n) > 0` is false for
  every light, and the pixel keeps its ambient term alone — so this frame is
  finite too, in the reference's own render (hard.npz), and is compared bit
  for bit like every other.
* materials: at the deepest depth used there are rays at that level and
  parents with two children.
"""
from __future__ import annotations

import os

import numpy as np
import pytest

import hard_scenes as hs
import rt_amd
from aov_ref import planes_equal
from conftest import GOLDEN
from hard_frames import Frames

W, H = 48, 36
DEEPEST = 9  # materials: the deepest depth any test here or on the GPU renders


@pytest.fixture(scope="module")
def hard(oracle, tmp_path_factory):
    return Frames(oracle, tmp_path_factory.mktemp("hard"))


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "hard.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def cpu():
    return rt_amd.CpuContext(4)


def same_frame(got, want):
    """Bit for bit, and the expected frame is finite."""
    assert np.isfinite(want).all()
    bad = (got.view(np.uint32) != want.view(np.uint32)).any(-1)
    assert got.shape == want.shape and not bad.any(), \
        f"{int(bad.sum())} pixels differ, first (row, col) {np.argwhere(bad)[:4].tolist()}"


# ---- the oracle against the reference's frames
@pytest.mark.parametrize("case", hs.GOLDEN_FRAMES, ids=lambda c: hs.golden_key(*c))
def test_oracle_matches_reference(hard, golden, case):
    family, seed, ntri, scale, w, h, depth = case
    key = hs.golden_key(*case)
    path = hard.path(family, seed, ntri, scale)
    with open(path) as f:
        assert str(golden["sha256_" + key]) == hs.text_sha(f.read()), "hard_scenes.py drifted"
    same_frame(hard.want(path, w, h, depth).img, golden[key])


# ---- the CPU backend against the oracle
def cpu_case(cpu, hard, family, seed, ntri=None, scale=1.0, depths=None, aov=False, wh=None):
    w, h = wh or hs.size(seed)
    path = hard.path(family, seed, ntri, scale)
    for depth in depths if depths is not None else (0, hs.DEPTH[family.split("/")[0]]):
        s = rt_amd.Scene(path, w, h, depth)
        cpu.upload(s)
        same_frame(cpu.render_float(s.frame), hard.want(path, w, h, depth).img)
        if aov and depth == 0:
            assert planes_equal(cpu.render_aov(s.frame), hard.aov(path, w, h)) == []


@pytest.mark.parametrize("seed", hs.SEEDS)
@pytest.mark.parametrize("family", hs.FAMILIES)
def test_cpu_backend_matches_oracle(cpu, hard, family, seed):
    cpu_case(cpu, hard, family, seed, aov=family in ("ties", "quadrics"))


def test_cpu_backend_on_the_infinite_hits(cpu, hard):
    cpu_case(cpu, hard, "quadrics/axis", 0, depths=(0, 3), aov=True, wh=(W, H))


@pytest.mark.parametrize("ntri", hs.NTRI_TIES)
def test_cpu_backend_ties_list_sizes(cpu, hard, ntri):
    cpu_case(cpu, hard, "ties", 0, ntri=ntri, depths=(0, 2), aov=ntri <= 257)


@pytest.mark.parametrize("scale", hs.SCALES, ids=lambda s: "2^%d" % np.log2(s))
@pytest.mark.parametrize("family,seed", hs.SCALED)
def test_cpu_backend_scaled(cpu, hard, family, seed, scale):
    cpu_case(cpu, hard, family, seed, scale=scale)


@pytest.mark.parametrize("depth", [5, 8, DEEPEST])
def test_cpu_backend_materials_deep(cpu, hard, depth):
    cpu_case(cpu, hard, "materials", 0, depths=(depth,), wh=(24, 18))
    cpu_case(cpu, hard, "materials", 1, depths=(depth,), wh=(24, 18))


# ---- the generator's conditions, on the oracle alone
def shares(ids, text):
    """{surface name up to its last `_`: share of the frame its members win}."""
    out = {}
    for i, (_, name) in enumerate(hs.surfaces(text)):
        kind = name.rsplit("_", 1)[0]
        out[kind] = out.get(kind, 0.0) + float((ids == i).mean())
    return out


@pytest.mark.parametrize("seed,ntri", [(seed, 20) for seed in hs.SEEDS] + [(0, n) for n in (3, 21, 257, 1025)])
def test_ties_conditions(hard, seed, ntri):
    w, h = hs.size(seed)
    text = hs.hard_dat("ties", seed, ntri)
    path = hard.path("ties", seed, ntri)
    ids = hard.aov(path, w, h)["id"]
    groups = hs.groups(text)
    assert set(groups) == ({"dtri", "dpln", "dqd"} | ({"rtri"} if ntri > 3 else set()))
    names = hs.surfaces(text)
    members = [i for g in groups.values() for i in g]
    won = {g: [int((ids == i).sum()) for i in m] for g, m in groups.items()}
    share = float(np.isin(ids, members).mean())
    print("ties", seed, ntri, "pixels won", won, "share of the frame %.3f" % share)
    for g, m in groups.items():
        assert len(m) in (2, 3) and m[0] < 8 and m[-1] >= len(names) - len(groups), (g, m, "far apart in the file")
        assert sum(won[g]) > 0, (g, "wins nowhere")
        if g != "rtri":  # exact duplicates: the first in file order
            assert won[g][0] > 0 and not any(won[g][1:]), (g, won[g])
    assert share >= 0.15
    # without the duplicates that sit first in the file
    first = {names[m[0]][1] for m in groups.values()}
    rest = hard.text(f"ties_rest_{seed}_{ntri}", hs.without(text, lambda n: n in first))
    for depth in (0, hs.DEPTH["ties"]):
        a, b = hard.want(path, w, h, depth).img, hard.want(rest, w, h, depth).img
        assert np.isfinite(a).all() and np.isfinite(b).all()
        changed = float((a != b).any(-1).mean())
        print("  depth", depth, "pixels that change without the first duplicates %.3f" % changed)
        assert changed >= 0.15


def lit_by(hard, text, path, name, w, h, j):
    """Pixels whose colour light j changes."""
    dark = hard.text(f"{name}_without_l{j}", hs.without(text, lambda n: n == f"l{j}"))
    return (hard.want(path, w, h, 0).img != hard.want(dark, w, h, 0).img).any(-1)


def test_tiny_stress_conditions(hard):
    seen, counts = {}, []
    for seed in hs.SEEDS:
        w, h = hs.size(seed)
        text = hs.hard_dat("tiny_stress", seed)
        path = hard.path("tiny_stress", seed)
        names = hs.surfaces(text)
        ntri = sum(1 for k, _ in names if k == "Poly")
        counts.append(ntri)
        assert 1 <= ntri <= 20 and text.count("Lumiere:") == 3 and sum(1 for k, _ in names if k == "Plane") == seed % 4
        for depth in (0, hs.DEPTH["tiny_stress"]):
            assert np.isfinite(hard.want(path, w, h, depth).img).all()
        ids = hard.aov(path, w, h)["id"]
        for kind, share in shares(ids, text).items():
            seen[kind] = max(seen.get(kind, 0), round(share * w * h))
        planar = np.isin(ids, [i for i, (k, _) in enumerate(names) if k in ("Poly", "Plane")])
        per_light = []
        for j in range(3):
            lit = lit_by(hard, text, path, f"tiny_{seed}", w, h, j)
            n = 0
            for a, b in ((np.s_[:, 1:], np.s_[:, :-1]), (np.s_[1:], np.s_[:-1])):  # right and upper neighbours
                n += int(((ids[a] == ids[b]) & planar[a] & (lit[a] != lit[b])).sum())
            per_light.append(n)
        print("tiny_stress", seed, ntri, "triangles; shadow boundary pairs per light", per_light)
        assert min(per_light) > 0, (seed, per_light)
    print("most pixels of a frame per kind", seen)
    for kind in hs.TINY_KINDS:
        if kind != "speck":  # under the determinant cut: see the module docstring
            assert seen.get(kind, 0) >= 4, kind  # more than a pixel that a rounding gave it
    assert seen["speck"] == 0
    assert min(counts) == 1 and max(counts) >= 16, counts
    all_kinds = {n.rsplit("_", 1)[0] for _, n in hs.surfaces(hs.hard_dat(*hs.SCALED[2]))}
    assert all_kinds == set(hs.TINY_KINDS) | {"ground", "oblique", "wall"}, "a scaled seed draws every kind"
    text = hs.hard_dat(*hs.SCALED[1])
    oblique = shares(hard.aov(hard.path(*hs.SCALED[1]), *hs.size(hs.SCALED[1][1]))["id"], text)["oblique"]
    print("the oblique plane's share of the other scaled seed's frame %.3f" % oblique)
    assert oblique >= 0.10


def test_quadrics_conditions(hard):
    seen, inside_cam, inside_light = {}, 0, 0
    for seed in hs.SEEDS:
        w, h = hs.size(seed)
        text = hs.hard_dat("quadrics", seed)
        path = hard.path("quadrics", seed)
        for depth in (0, hs.DEPTH["quadrics"]):
            assert np.isfinite(hard.want(path, w, h, depth).img).all()
        sh = shares(hard.aov(path, w, h)["id"], text)
        print("quadrics", seed, {k: round(v, 4) for k, v in sh.items()})
        assert 1 <= sum(1 for k in sh if k in hs.QUADRIC_KINDS) <= 4
        if "lin" in sh:
            assert sh["lin"] >= 0.10
        inside_cam += "shell" in sh
        inside_light += "lamp" in sh
        for kind, share in sh.items():
            seen[kind] = max(seen.get(kind, 0.0), share)
    for kind in hs.QUADRIC_KINDS:
        assert seen.get(kind, 0.0) >= 0.01, kind
    assert inside_cam and inside_light
    # quadrics/axis: B == 0 along the middle row, hits at t = +inf where
    # nothing nearer is hit (and a finite colour: see the module docstring)
    text = hs.hard_dat("quadrics/axis", 0)
    path = hard.path("quadrics/axis", 0)
    aov = hard.aov(path, W, H)
    lin = [n for _, n in hs.surfaces(text)].index("lin_0")
    at_inf = np.isposinf(aov["t"]) & (aov["id"] == lin)
    print("quadrics/axis: hits at infinity in the middle row", int(at_inf[H // 2].sum()), "of", W)
    assert at_inf[H // 2].sum() >= W // 4 and not np.delete(at_inf, H // 2, 0).any()
    assert shares(aov["id"], text)["lin"] >= 0.10
    for depth in (0, 3):
        assert np.isfinite(hard.want(path, W, H, depth).img).all()


@pytest.mark.parametrize("seed", hs.SEEDS)
def test_materials_conditions(hard, seed):
    text = hs.hard_dat("materials", seed)
    path = hard.path("materials", seed)
    assert hs.has_k_at_least_1(text) == (seed % 2 == 0)
    for line in text.split("\n"):  # both coefficients on every surface, from the sets
        w = line.split()
        if w and w[0] in ("reflect:", "refract:"):
            assert float(w[1]) in hs.K_SET
            assert w[0] == "reflect:" or float(w[2]) in hs.IOR_SET
    assert text.count("reflect:") == text.count("refract:") == len(hs.surfaces(text))
    for (w, h), depth in ((hs.size(seed), hs.DEPTH["materials"]), ((24, 18), DEEPEST)):
        want = hard.want(path, w, h, depth)
        assert np.isfinite(want.img).all()
        print("materials", seed, depth, "rays", want.rays[:depth + 1].tolist(), "parents",
              want.parents[:depth + 1].tolist())
        assert want.deepest == depth and want.rays[depth] > 0
        # a level with more rays than the level above has parents: two children somewhere
        assert (want.rays[1:depth + 1] > want.parents[:depth]).any()
        assert want.rays[depth] > want.parents[depth - 1], "parents with two children at the deepest level"
