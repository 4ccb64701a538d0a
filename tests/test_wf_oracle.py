"""The checkers of tests/test_gpu_wavefront.py, on the CPU:

* oracle_level_counts (the oracle's bounce tree by depth: rays traced and
  hits that spawned a child) against the CPU backend's ray count — an
  independent implementation — and against itself across depths;
* the small wavefront scenes (tests/wf_scenes.py) against the frames the
  reference's own code rendered (tests/golden/wf_small.npz,
  make_wf_golden.py): the scene texts' SHA-256 first, then the oracle's and
  the CPU backend's whole frames, bit for bit in float32.

The reference harness has no setter for the energy floor: frames with a
min_energy other than 0.01 (the negative one that spawns both children at
every hit) are checked against the oracle's restatement only."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

import rt_amd
import wf_scenes
from conftest import GOLDEN, bits_equal

LEVELS = 16


def level_counts(oracle, p):
    L = oracle.L
    L.oracle_level_counts.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    rays, parents = np.zeros(LEVELS, np.uint64), np.zeros(LEVELS, np.uint64)
    assert L.oracle_level_counts(p, rays.ctypes.data, parents.ctypes.data, LEVELS) == 0
    return rays, parents


def oracle_frame(oracle, path, w, h, depth, threads=8):
    rc, p = oracle.load(path, w, h, depth)
    assert rc == 0
    img = np.zeros((h, w, 3), np.float32)
    oracle.L.oracle_render_window(p, 0, h, 0, w, img.ctypes.data, threads)
    rays, parents = level_counts(oracle, p)
    oracle.L.oracle_free(p)
    return img, rays, parents


@pytest.fixture(scope="module")
def wf_golden():
    with np.load(os.path.join(GOLDEN, "wf_small.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def scene_file(tmp_path_factory):
    d = tmp_path_factory.mktemp("wf")
    made = {}

    def get(family, ntri, lights=2):
        k = (family, ntri, lights)
        if k not in made:
            made[k] = str(d / f"{family}_{ntri}_{lights}.dat")
            with open(made[k], "w") as f:
                f.write(wf_scenes.wf_dat(family, ntri, lights))
        return made[k]

    return get


@pytest.mark.parametrize("family,ntri,lights,depth", [("split", 96, 2, 5), ("mixed", 1600, 3, 3), ("chain", 65, 1, 8)])
def test_level_counts_against_the_cpu_backend(oracle, scene_file, family, ntri, lights, depth):
    w, h = 48, 36
    path = scene_file(family, ntri, lights)
    img, rays, parents = oracle_frame(oracle, path, w, h, depth)
    s = rt_amd.Scene(path, w, h, depth)
    cpu = rt_amd.CpuContext(4)
    cpu.upload(s)
    f = s.frame.copy()
    f.flags = rt_amd.FLAG_STATS
    assert bits_equal(cpu.render_float(f), img)
    st = cpu.stats()
    assert rays[0] == st.primary_rays == w * h
    assert st.bounce_rays > 0 and int(rays[1:].sum()) == st.bounce_rays
    # a level's rays are the children of the level above: one or two per parent
    for L in range(depth):
        assert parents[L] <= rays[L + 1] <= 2 * parents[L], L
        assert parents[L] <= rays[L]
    assert rays[1] > 0 and parents[depth] == 0 and not rays[depth + 1:].any()
    # the counts do not depend on the threads, and the image not on the counting
    img1, rays1, parents1 = oracle_frame(oracle, path, w, h, depth, threads=1)
    assert bits_equal(img1, img) and np.array_equal(rays1, rays) and np.array_equal(parents1, parents)
    # depth d's tree is the top of depth d + 1's
    _, rays_d, parents_d = oracle_frame(oracle, path, w, h, depth - 1)
    assert np.array_equal(rays_d[:depth], rays[:depth]) and np.array_equal(parents_d[:depth - 1], parents[:depth - 1])
    assert rays_d[depth] == 0 and parents_d[depth - 1] == 0


def test_level_counts_of_a_window(oracle, scene_file):
    """A window's counts are its own pixels': two halves add up to the frame."""
    path = scene_file("split", 96)
    _, rays, parents = oracle_frame(oracle, path, 48, 36, 3)
    tot_r, tot_p = np.zeros(LEVELS, np.uint64), np.zeros(LEVELS, np.uint64)
    rc, p = oracle.load(path, 48, 36, 3)
    assert rc == 0
    for r0, r1 in ((0, 17), (17, 36)):
        img = np.zeros((r1 - r0, 48, 3), np.float32)
        oracle.L.oracle_render_window(p, r0, r1, 0, 48, img.ctypes.data, 4)
        r, q = level_counts(oracle, p)
        tot_r += r
        tot_p += q
    oracle.L.oracle_free(p)
    assert np.array_equal(tot_r, rays) and np.array_equal(tot_p, parents)


@pytest.mark.parametrize("frame", wf_scenes.GOLDEN_FRAMES, ids=lambda f: wf_scenes.golden_key(*f))
def test_oracle_and_cpu_backend_match_the_reference_frames(oracle, scene_file, wf_golden, frame):
    family, ntri, w, h, depth = frame
    text = wf_scenes.wf_dat(family, ntri)
    assert str(wf_golden[wf_scenes.sha_key(family, ntri)]) == wf_scenes.text_sha(text), "wf_scenes.py drifted"
    want = wf_golden[wf_scenes.golden_key(*frame)]
    assert want.shape == (h, w, 3) and want.dtype == np.float32
    path = scene_file(family, ntri)
    img, rays, _ = oracle_frame(oracle, path, w, h, depth)
    assert rays[min(depth, 4)] > 0
    assert bits_equal(img, want), f"oracle: {int((img != want).any(-1).sum())} pixels differ"
    s = rt_amd.Scene(path, w, h, depth)
    cpu = rt_amd.CpuContext(8)
    cpu.upload(s)
    got = cpu.render_float(s.frame)
    assert bits_equal(got, want), f"CPU backend: {int((got != want).any(-1).sum())} pixels differ"
