"""Adaptive supersampling (include/rt.h rt_render_adaptive*, csrc/rt_adaptive.h)
on the CPU backend, the argument contract, the CLI and the CScene verb.

The expected image is adaptive_ref.compose of a reference frame of the sample
grid (tests/golden/images.npz, made from the reference's sources, or the
oracle's frame) under the mask adaptive_ref.mask computes from that frame's
lattice samples and the oracle's primary-hit planes: bit for bit on this
backend, float, RGBA8 and mask.  Before any result is looked at, the
expectation itself must be worth testing against: a third to a half of the
pixels on an edge, some of them found by the colour criterion alone."""
from __future__ import annotations

import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import adaptive_ref as ar
import rt_amd
from conftest import REPO, bits_equal, rgba8, scene

THREADS = min(8, os.cpu_count() or 1)
EXE = os.path.join(REPO, "ray-tracing-gpu_amd", "lib", "rt_render")
ALL = ar.ALL


@pytest.fixture(scope="module")
def cpu():
    return rt_amd.CpuContext(THREADS)


def sample_frame(ctx, path, w, h, depth, rows=None):
    s = rt_amd.Scene(path, w, h, depth)
    ctx.upload(s)
    f = s.frame.copy()
    if rows:
        f.row_begin, f.row_end = rows
    return f


def check(got, want, m):
    assert got["rgb"].shape == want.shape and got["mask"].shape == m.shape
    assert np.array_equal(got["mask"], m), f"{np.count_nonzero(got['mask'] != m)} mask bytes differ"
    assert bits_equal(got["rgb"], want), f"{np.count_nonzero(got['rgb'] != want)} floats differ"
    assert np.array_equal(got["rgba"], rgba8(want))


def test_header_defines():
    text = open(os.path.join(REPO, "include", "rt.h")).read()
    assert "#define RT_HAS_ADAPTIVE_SS 1" in text
    assert "enum { RT_EDGE_ID = 1, RT_EDGE_NORMAL = 2, RT_EDGE_COLOUR = 4 };" in text
    assert "#define RT_ABI_VERSION 8" in text and rt_amd.lib().rt_abi_version() == 8
    assert (rt_amd.EDGE_ID, rt_amd.EDGE_NORMAL, rt_amd.EDGE_COLOUR) == (1, 2, 4)
    assert ctypes.sizeof(rt_amd.Adaptive) == 16 and ctypes.sizeof(rt_amd.AdaptiveOut) == 3 * ctypes.sizeof(ctypes.c_void_p)


def test_reference_mask_by_hand():
    """adaptive_ref.mask on a 3 x 3 frame worked out by hand."""
    base = np.zeros((3, 3, 3), np.float32)
    ids = np.zeros((3, 3), np.int32)
    nrm = np.zeros((3, 3, 3), np.float32)
    nrm[..., 2] = 1
    ids[1, 1] = 5                      # the centre is another surface
    ids[0, 0] = -1                     # a corner misses
    nrm[0, 0] = 0
    nrm[2, 2] = (0, 1, 0)              # a corner's normal turned by 90 degrees, same surface
    base[0, 2] = np.nan                # a NaN never flags
    base[2, 0, 0] = 0.5                # a colour step at the other corner
    m = ar.mask(base, ids, nrm, ALL, 0.9, 0.1)
    want = np.array([[3, 3, 0], [7, 1, 3], [4, 7, 2]], np.uint8)
    # (0,0) miss: its neighbours differ by id and by hit/miss ((1,0) also by colour from (2,0)); the centre
    # only by id (equal normals);
    # (2,0): colour only; (2,1): colour from (2,0), id from the centre, normal from (2,2); (1,2): id, normal from (2,2)
    assert np.array_equal(m, want), m
    assert not ar.mask(base, ids, nrm, ar.EDGE_COLOUR, 0.9, math.inf).any()
    one = ar.mask(base, ids, nrm, ar.EDGE_COLOUR, 0.9, -1.0)
    assert one[0, 2] == 0 and one[0, 1] == 4 and np.count_nonzero(one) == 8   # NaN - x compares false both ways


@pytest.mark.parametrize("i", range(1, 10))
@pytest.mark.parametrize("depth", [0, 3])
def test_scene_images(cpu, oracle, golden_images, i, depth):
    """64 x 48 samples, s = 2, every criterion."""
    S = golden_images[f"scene{i}_64x48_d{depth}"]
    want, m = ar.expect(oracle, scene(i), S, 2, ALL)
    share = np.count_nonzero(m) / m.size
    assert 0.2 <= share <= 0.6, share
    assert np.count_nonzero(m == ar.EDGE_COLOUR) / m.size >= 0.04
    f = sample_frame(cpu, scene(i), 64, 48, depth)
    check(cpu.render_adaptive(f, 2, ALL), want, m)
    st = cpu.stats()
    assert st.primary_rays == m.size + 4 * np.count_nonzero(m) and st.kernel == "cpu_render_adaptive"


@pytest.mark.parametrize("s", [4, 8])
def test_scene7_larger_factors(cpu, oracle, s):
    S = oracle.render(scene(7), 32 * s, 24 * s, 3)
    want, m = ar.expect(oracle, scene(7), S, s, ALL)
    assert 0.2 <= np.count_nonzero(m) / m.size <= 0.6
    f = sample_frame(cpu, scene(7), 32 * s, 24 * s, 3)
    check(cpu.render_adaptive(f, s, ALL), want, m)


@pytest.mark.parametrize("criteria", [ar.EDGE_ID, ar.EDGE_NORMAL, ar.EDGE_COLOUR])
def test_each_criterion_alone(cpu, oracle, golden_images, criteria):
    S = golden_images["scene7_64x48_d3"]
    want, m = ar.expect(oracle, scene(7), S, 2, criteria)
    assert m.any() and set(np.unique(m)) == {0, criteria}
    f = sample_frame(cpu, scene(7), 64, 48, 3)
    check(cpu.render_adaptive(f, 2, criteria), want, m)


def test_thresholds_other_than_the_defaults(cpu, oracle, golden_images):
    S = golden_images["scene9_64x48_d3"]
    want, m = ar.expect(oracle, scene(9), S, 2, ar.EDGE_NORMAL | ar.EDGE_COLOUR, cos=0.999, delta=0.02)
    _, m0 = ar.expect(oracle, scene(9), S, 2, ar.EDGE_NORMAL | ar.EDGE_COLOUR)
    assert np.count_nonzero(m) > np.count_nonzero(m0)
    f = sample_frame(cpu, scene(9), 64, 48, 3)
    check(cpu.render_adaptive(f, 2, ar.EDGE_NORMAL | ar.EDGE_COLOUR, normal_cos=0.999, colour_delta=0.02), want, m)


def test_nothing_flagged_is_the_plain_frame(cpu):
    """colour_delta = +inf, COLOUR only: the bits of render_float(B), an all-zero mask."""
    f = sample_frame(cpu, scene(7), 64, 48, 3)
    got = cpu.render_adaptive(f, 2, ar.EDGE_COLOUR, colour_delta=math.inf)
    B = rt_amd.Scene(scene(7), 32, 24, 3).frame.copy()
    assert not got["mask"].any()
    assert bits_equal(got["rgb"], cpu.render_float(B)) and np.array_equal(got["rgba"], cpu.render(B))
    assert cpu.render_adaptive(f, 2, ar.EDGE_COLOUR, colour_delta=math.inf)["rgb"].shape == (24, 32, 3)


def test_everything_flagged_is_full_supersampling(cpu):
    """colour_delta = -1: |a - b| > -1 everywhere, the bits of render_ss_float."""
    f = sample_frame(cpu, scene(7), 64, 48, 3)
    got = cpu.render_adaptive(f, 2, ar.EDGE_COLOUR, colour_delta=-1.0)
    assert cpu.stats().primary_rays == 5 * 32 * 24
    assert (got["mask"] == ar.EDGE_COLOUR).all()
    assert bits_equal(got["rgb"], cpu.render_ss_float(f, 2)) and np.array_equal(got["rgba"], cpu.render_ss(f, 2))


def test_slabs_stitch_to_the_whole_frame(cpu, oracle, golden_images):
    """Sample rows [0, 16) + [16, 48) are output rows [0, 8) + [8, 24).  The
    neighbours are the whole frame's: scene6 has pixels on both sides of the
    seam that only their neighbour ACROSS the seam flags, and each is flagged
    in its slab too."""
    S = golden_images["scene6_64x48_d3"]
    want, m = ar.expect(oracle, scene(6), S, 2, ALL)
    a = ar.planes(oracle, scene(6), 32, 24)
    B = S[::2, ::2]
    below = ar.mask(B[:8], a["id"][:8], a["n"][:8], ALL, 0.9, 0.1)   # each slab taken for a frame of its own
    above = ar.mask(B[8:], a["id"][8:], a["n"][8:], ALL, 0.9, 0.1)
    seam_lo = np.flatnonzero((m[7] != 0) & (below[7] == 0))
    seam_hi = np.flatnonzero((m[8] != 0) & (above[0] == 0))
    assert seam_lo.size > 0 and seam_hi.size > 0
    parts = []
    for rows in ((0, 16), (16, 48)):
        f = sample_frame(cpu, scene(6), 64, 48, 3, rows=rows)
        parts.append(cpu.render_adaptive(f, 2, ALL))
    lo, hi = parts
    assert lo["mask"].shape == (8, 32) and hi["mask"].shape == (16, 32)
    assert (lo["mask"][7, seam_lo] != 0).all() and (hi["mask"][0, seam_hi] != 0).all()
    whole = {k: np.concatenate([lo[k], hi[k]]) for k in lo}
    check(whole, want, m)


def test_each_output_alone(cpu, oracle, golden_images):
    L = rt_amd.lib()
    S = golden_images["scene2_64x48_d0"]
    want, m = ar.expect(oracle, scene(2), S, 2, ALL)
    f = sample_frame(cpu, scene(2), 64, 48, 0)
    a = rt_amd.Adaptive(2, ALL, 0.9, 0.1)
    rgb = np.zeros((24, 32, 3), np.float32)
    q = np.zeros((24, 32, 4), np.uint8)
    mk = np.zeros((24, 32), np.uint8)
    for o in (rt_amd.AdaptiveOut(None, rgb.ctypes.data, None), rt_amd.AdaptiveOut(q.ctypes.data, None, None),
              rt_amd.AdaptiveOut(None, None, mk.ctypes.data)):
        assert L.rt_cpu_render_adaptive(cpu._h, ctypes.byref(f), ctypes.byref(a), ctypes.byref(o)) == 0
    check({"rgb": rgb, "rgba": q, "mask": mk}, want, m)
    assert cpu.stats().primary_rays == m.size    # the mask alone traced no sample


def test_argument_errors_leave_the_output_untouched(cpu):
    L = rt_amd.lib()
    f = sample_frame(cpu, scene(1), 64, 48, 0)
    rgb = np.full((24, 32, 3), 7, np.float32)
    q = np.full((24, 32, 4), 7, np.uint8)
    mk = np.full((24, 32), 7, np.uint8)
    out = rt_amd.AdaptiveOut(q.ctypes.data, rgb.ctypes.data, mk.ctypes.data)

    def call(frame, s=2, criteria=ALL, o=out, h=None):
        a = rt_amd.Adaptive(s, criteria, 0.9, 0.1)
        return L.rt_cpu_render_adaptive(cpu._h if h is None else h, ctypes.byref(frame), ctypes.byref(a),
                                        ctypes.byref(o))

    for s in (0, 1, 3, 5, 6, 7, 9, 16, -2):          # s not in {2, 4, 8}
        assert call(f, s=s) == -1, s
    g = sample_frame(cpu, scene(1), 60, 44, 0)
    assert call(g, s=8) == -1                        # 8 divides neither 60 nor 44
    g = sample_frame(cpu, scene(1), 64, 44, 0)
    assert call(g, s=8) == -1                        # 8 does not divide the height
    g = sample_frame(cpu, scene(1), 60, 48, 0)
    assert call(g, s=8) == -1                        # nor the width
    for rows in ((2, 48), (0, 46)):                  # s does not divide row_begin / row_end
        g = f.copy()
        g.row_begin, g.row_end = rows
        assert call(g, s=4) == -1, rows
    g = f.copy()
    g.band_rows, g.band_count, g.band_index = 32, 2, 0
    assert call(g) == -1                             # bands are out of scope
    for criteria in (0, 8, 15, -1):
        assert call(f, criteria=criteria) == -1, criteria
    assert call(f, o=rt_amd.AdaptiveOut(None, None, None)) == -1
    g = f.copy()
    g.flags = rt_amd.FLAG_STATS
    assert call(g) == -1
    assert b"rt_render_adaptive" in L.rt_last_error(cpu._h)
    a = rt_amd.Adaptive(2, ALL, 0.9, 0.1)
    assert L.rt_cpu_render_adaptive(None, ctypes.byref(f), ctypes.byref(a), ctypes.byref(out)) == -1
    assert L.rt_cpu_render_adaptive(cpu._h, None, ctypes.byref(a), ctypes.byref(out)) == -1
    assert L.rt_cpu_render_adaptive(cpu._h, ctypes.byref(f), None, ctypes.byref(out)) == -1
    assert L.rt_cpu_render_adaptive(cpu._h, ctypes.byref(f), ctypes.byref(a), None) == -1
    assert L.rt_render_adaptive(None, None, None, None) == -1
    assert L.rt_render_adaptive_async(None, None, None, None, None) == -1
    # call order and backend: RT_E_STATE
    fresh = rt_amd.CpuContext(1)
    assert call(f, h=fresh._h) == -4                 # before rt_upload_scene
    assert L.rt_render_adaptive(cpu._h, ctypes.byref(f), ctypes.byref(a), ctypes.byref(out)) == -4
    assert L.rt_render_adaptive_async(cpu._h, ctypes.byref(f), ctypes.byref(a), ctypes.byref(out), None) == -4
    assert (rgb == 7).all() and (q == 7).all() and (mk == 7).all()
    with pytest.raises(rt_amd.RtError) as e:
        cpu.render_adaptive(f, 3, ALL)
    assert e.value.code == -1


def test_empty_slab(cpu):
    f = sample_frame(cpu, scene(1), 64, 48, 0, rows=(16, 16))
    got = cpu.render_adaptive(f, 2, ALL)
    assert got["rgb"].shape == (0, 32, 3) and cpu.stats().primary_rays == 0


def read_ppm(path):
    head = open(path, "rb").read().split(b"\n", 3)
    assert head[0] == b"P6" and head[2] == b"255"
    w, h = map(int, head[1].split())
    return np.frombuffer(head[3], np.uint8).reshape(h, w, 3)


def test_cli_adaptive_cpu_backend(tmp_path, oracle, golden_images):
    want, m = ar.expect(oracle, scene(7), golden_images["scene7_64x48_d3"], 2, ALL)
    out, mk = tmp_path / "s7.ppm", tmp_path / "mask.npy"
    base = [EXE, scene(7), "-x", "32", "-y", "24", "-d", "3", "--backend", "cpu", "--threads", str(THREADS)]
    r = subprocess.run(base + ["--adaptive", "2", "-o", str(out), "--mask", str(mk)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(read_ppm(out)[::-1], rgba8(want)[..., :3])     # the PPM's top row first
    got = np.load(mk)
    assert got.dtype == np.uint8 and np.array_equal(got, m)
    want_n, m_n = ar.expect(oracle, scene(7), golden_images["scene7_64x48_d3"], 2, ar.EDGE_NORMAL | ar.EDGE_COLOUR,
                            cos=0.5, delta=0.25)
    r = subprocess.run(base + ["--adaptive", "2", "--edge", "normal,colour", "--edge-cos", "0.5", "--edge-delta",
                               "0.25", "-o", str(out), "--mask", str(mk)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.load(mk), m_n) and np.array_equal(read_ppm(out)[::-1], rgba8(want_n)[..., :3])
    for extra in (["--adaptive", "3"], ["--adaptive", "2", "--ssaa", "2"], ["--adaptive", "2", "-g", "2"],
                  ["--adaptive", "2", "--edge", "depth"], ["--mask", str(mk)]):
        bad = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 1 and "[ERREUR]" in bad.stderr, extra


def test_cscene_adaptive_verb(oracle, golden_images):
    want, m = ar.expect(oracle, scene(7), golden_images["scene7_64x48_d3"], 2, ALL)
    c = rt_amd.CScene(backend="cpu", threads=THREADS)
    c.AjusterResolution(32, 24)
    c.AjusterNbRebondsMax(3)
    c.TraiterFichierDeScene(scene(7))
    c.AjusterSurEchantillonnage(2)
    check(c.LancerRayonsAdaptatif(), want, m)
    assert np.array_equal(c.LancerRayonsAdaptatif(criteria=ar.EDGE_ID)["mask"],
                          ar.expect(oracle, scene(7), golden_images["scene7_64x48_d3"], 2, ar.EDGE_ID)[1])


def test_adaptive_under_asan_ubsan(tmp_path):
    """cpu_render_adaptive and the shared classification (rt_adaptive.h
    edge_mask, what both backends run) in a stand-alone host program built
    with AddressSanitizer and UBSan: every plane and output allocated at its
    exact size, slabs with and without halo rows, every factor and criterion."""
    exe = tmp_path / "adaptive_check"
    csrc = os.path.join(REPO, "ray-tracing-gpu_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-I", csrc,
                    os.path.join(REPO, "tools", "adaptive", "adaptive_check.cpp"), os.path.join(csrc, "rt_cpu.cpp"),
                    "-o", str(exe)], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "adaptive_check: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
