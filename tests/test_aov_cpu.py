"""Primary-hit AOV renders (include/rt.h rt_render_aov*) on the CPU backend,
the argument contract, the CLI and the CScene verb.

The expected planes are never computed by the code under test: they are the
fixture tests/golden/aov.npz (made from the reference's own Intersection()
through oracle/_ref by tests/golden/make_aov_golden.py) or tests/aov_ref.py
through liboracle.so's oracle_intersect at test time.  Every comparison is
bit for bit, quadric normals included.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

import aov_ref
import rt_amd
from conftest import GOLDEN, REPO, scene

THREADS = min(8, os.cpu_count() or 1)
EXE = os.path.join(REPO, "ray-tracing-gpu_amd", "lib", "rt_render")
CSRC = os.path.join(REPO, "ray-tracing-gpu_amd", "csrc")
SENTINEL = 0x7FC12345  # a NaN pattern no render writes


@pytest.fixture(scope="module")
def cpu():
    return rt_amd.CpuContext(THREADS)


@pytest.fixture(scope="module")
def golden_aov():
    return np.load(os.path.join(GOLDEN, "aov.npz"))


@pytest.fixture(scope="module")
def hf1280_path(tmp_path_factory):
    from rt_amd import synth

    return synth.write_heightfield(str(tmp_path_factory.mktemp("hf1280") / "heightfield_40x16.dat"), cols=40, rows=16)


def want_of(g, name):
    return {k: g[f"{name}_{k}"] for k in ("id", "t", "n")}


def frame_of(ctx, path, w, h, depth=0, rows=None, bands=None):
    s = rt_amd.Scene(path, w, h, depth)
    ctx.upload(s)
    f = s.frame.copy()
    if rows:
        f.row_begin, f.row_end = rows
    if bands:
        f.band_rows, f.band_count, f.band_index = bands
    return f


def test_header_and_binding_declare_the_feature():
    text = open(os.path.join(REPO, "include", "rt.h")).read()
    assert "#define RT_HAS_AOV 1" in text and "#define RT_ABI_VERSION 8" in text
    assert rt_amd.lib().rt_abi_version() == 8
    for name in ("rt_render_aov", "rt_render_aov_async", "rt_cpu_render_aov"):
        assert name in rt_amd.SIGNATURES and f"int {name}(" in text


@pytest.mark.parametrize("i", range(1, 10))
def test_scenes_match_the_reference_fixture(cpu, golden_aov, i):
    f = frame_of(cpu, scene(i), 64, 48)
    got = cpu.render_aov(f)
    assert got["t"].shape == (48, 64) and got["id"].dtype == np.int32 and got["n"].shape == (48, 64, 3)
    assert aov_ref.planes_equal(got, want_of(golden_aov, f"scene{i}")) == []
    st = cpu.stats()
    assert st.primary_rays == 64 * 48 and st.bounce_rays == 0 and st.shadow_rays == 0


def test_heightfield_1280_matches_the_reference_fixture(cpu, golden_aov, hf1280_path):
    f = frame_of(cpu, hf1280_path, 64, 32)
    assert rt_amd.Scene(hf1280_path, 64, 32).n_surfaces == 1281
    assert aov_ref.planes_equal(cpu.render_aov(f), want_of(golden_aov, "hf1280")) == []


def test_heightfield_50k_sparse_pixels(cpu, golden_aov, heightfield_path):
    g = golden_aov
    xs, ys = aov_ref.sparse_pixels(int(g["hf50k_seed"]))
    assert np.array_equal(xs, g["hf50k_x"]) and np.array_equal(ys, g["hf50k_y"])
    # the ground plane fills this camera's frame (no miss anywhere, hf50k_lacks):
    # the pixels hold both kinds of winner instead
    assert (g["hf50k_id"] > 0).sum() >= 8 and (g["hf50k_id"] == 0).sum() >= 8 and str(g["hf50k_lacks"]) == "miss"
    f = frame_of(cpu, heightfield_path, 64, 32)
    got = cpu.render_aov(f)
    picked = {k: np.ascontiguousarray(got[k][ys, xs]) for k in got}
    assert aov_ref.planes_equal(picked, want_of(g, "hf50k")) == []


def cam2_frame(g, base):
    """cameras()[2] of the heightfield's 64 x 32 frame, checked against the
    fixture's own camera words."""
    import cameras

    f = cameras.cameras(base)[2]
    assert np.array_equal(np.asarray(cameras.words(f), np.float32).view(np.uint32),
                          np.asarray(g["hf50kcam2_words"], np.float32).view(np.uint32))
    return f


def test_heightfield_50k_sparse_pixels_with_sky(cpu, golden_aov, heightfield_path):
    """The 50k heightfield under a pitched and yawed camera: hits and misses."""
    g = golden_aov
    xs, ys = aov_ref.sparse_pixels(int(g["hf50kcam2_seed"]))
    assert np.array_equal(xs, g["hf50kcam2_x"]) and np.array_equal(ys, g["hf50kcam2_y"])
    assert (g["hf50kcam2_id"] >= 0).sum() >= 8 and (g["hf50kcam2_id"] < 0).sum() >= 8
    f = cam2_frame(g, frame_of(cpu, heightfield_path, 64, 32))
    got = cpu.render_aov(f)
    picked = {k: np.ascontiguousarray(got[k][ys, xs]) for k in got}
    assert aov_ref.planes_equal(picked, want_of(g, "hf50kcam2")) == []


def test_fixture_coverage_is_declared(golden_aov):
    """Every set has hits and misses, or says which it lacks."""
    g = golden_aov
    for name in [f"scene{i}" for i in range(1, 10)] + ["hf1280", "hf50k", "hf50kcam2"]:
        ids = g[f"{name}_id"]
        hit, miss = bool((ids >= 0).any()), bool((ids < 0).any())
        assert str(g[f"{name}_lacks"]) == ("" if hit and miss else ("miss" if hit else "hit")), name
    assert any(str(g[f"scene{i}_lacks"]) == "" for i in range(1, 10))
    # a quadric's normal is per pixel: the fixture holds many distinct ones
    assert len(np.unique(g["scene4_n"].reshape(-1, 3), axis=0)) > 100


@pytest.mark.parametrize("i", [1, 3, 4, 7])
def test_aov_ref_through_liboracle_matches_the_fixture(oracle, golden_aov, i):
    """The transitive pin: aov_ref + oracle_intersect (what the other tests
    use for sizes the fixture does not hold) reproduces the oracle/_ref fixture."""
    assert aov_ref.planes_equal(aov_ref.oracle_aov(oracle, scene(i), 64, 48), want_of(golden_aov, f"scene{i}")) == []


def test_aov_ref_through_liboracle_on_sparse_heightfield_pixels(oracle, golden_aov, hf1280_path):
    g = golden_aov
    surf, cam, _ = oracle.dump(hf1280_path, 64, 32)
    xs, ys = aov_ref.sparse_pixels(7)
    ids, ts, ns, _ = aov_ref.aov_pixels(oracle.L.oracle_intersect, surf, aov_ref.Cam.from_words(cam), xs, ys)
    want = {k: np.ascontiguousarray(g[f"hf1280_{k}"][ys, xs]) for k in ("id", "t", "n")}
    assert aov_ref.planes_equal({"id": ids, "t": ts, "n": ns}, want) == []


def test_miss_encoding(cpu, golden_aov):
    f = frame_of(cpu, scene(4), 64, 48)
    got = cpu.render_aov(f)
    miss = got["id"] < 0
    assert miss.any() and not miss.all()
    assert (got["id"][miss] == -1).all()
    assert (got["t"][miss].view(np.uint32) == np.float32(-1.0).view(np.uint32)).all()
    assert (got["n"][miss].view(np.uint32) == 0).all()       # +0.0, not -0.0
    assert (got["t"][~miss] > aov_ref.EPS).all() and (got["id"][~miss] < 4).all()


def test_independent_of_bounces_and_shading_parameters(cpu):
    a = cpu.render_aov(frame_of(cpu, scene(7), 64, 48, depth=0))
    f = frame_of(cpu, scene(7), 64, 48, depth=5)
    assert f.max_bounces == 5
    f.min_energy, f.scene_ior = 0.5, 1.3
    f.background[0] = 0.25
    assert aov_ref.planes_equal(cpu.render_aov(f), a) == []


@pytest.mark.parametrize("only", ["t", "id", "n"])
def test_any_single_plane_alone(cpu, golden_aov, only):
    f = frame_of(cpu, scene(3), 64, 48)
    got = cpu.render_aov(f, **{k: k == only for k in ("t", "id", "n")})
    assert list(got) == [only]
    assert aov_ref.planes_equal(got, want_of(golden_aov, "scene3"), keys=(only,)) == []


def test_argument_errors(cpu):
    L = rt_amd.lib()
    f = frame_of(cpu, scene(1), 64, 48)
    t = np.zeros((48, 64), np.float32)
    none = rt_amd.Aov(None, None, None)
    some = rt_amd.Aov(t.ctypes.data, None, None)
    assert L.rt_cpu_render_aov(cpu._h, ctypes.byref(f), ctypes.byref(none)) == -1
    assert L.rt_cpu_render_aov(cpu._h, ctypes.byref(f), None) == -1
    assert L.rt_cpu_render_aov(cpu._h, None, ctypes.byref(some)) == -1
    assert L.rt_cpu_render_aov(None, ctypes.byref(f), ctypes.byref(some)) == -1
    assert L.rt_render_aov(None, ctypes.byref(f), ctypes.byref(some)) == -1
    assert L.rt_render_aov_async(None, ctypes.byref(f), ctypes.byref(some), None) == -1
    g = f.copy()
    g.flags = rt_amd.FLAG_STATS
    assert L.rt_cpu_render_aov(cpu._h, ctypes.byref(g), ctypes.byref(some)) == -1
    g = f.copy()
    g.row_begin, g.row_end = 40, 49            # a slab past the frame
    assert L.rt_cpu_render_aov(cpu._h, ctypes.byref(g), ctypes.byref(some)) == -1
    g = f.copy()
    g.band_rows, g.band_count, g.band_index = 8, 2, 0     # not a multiple of 16
    assert L.rt_cpu_render_aov(cpu._h, ctypes.byref(g), ctypes.byref(some)) == -1
    g.band_rows, g.band_index = 16, 2                     # index out of range
    assert L.rt_cpu_render_aov(cpu._h, ctypes.byref(g), ctypes.byref(some)) == -1
    assert L.rt_cpu_render_aov(cpu._h, ctypes.byref(f), ctypes.byref(some)) == 0


def test_render_before_upload_is_a_state_error():
    L = rt_amd.lib()
    h = ctypes.c_void_p()
    assert L.rt_create_cpu(1, ctypes.byref(h)) == 0
    try:
        f = rt_amd.Scene(scene(1), 16, 16).frame
        t = np.zeros((16, 16), np.float32)
        some = rt_amd.Aov(t.ctypes.data, None, None)
        assert L.rt_cpu_render_aov(h, ctypes.byref(f), ctypes.byref(some)) == -4
    finally:
        L.rt_destroy(h)


def test_backend_is_explicit(cpu):
    """The HIP AOV calls refuse a CPU context."""
    L = rt_amd.lib()
    f = frame_of(cpu, scene(1), 16, 16)
    t = np.zeros((16, 16), np.float32)
    some = rt_amd.Aov(t.ctypes.data, None, None)
    assert L.rt_render_aov(cpu._h, ctypes.byref(f), ctypes.byref(some)) == -4
    assert L.rt_render_aov_async(cpu._h, ctypes.byref(f), ctypes.byref(some), None) == -4
    assert b"rt_cpu_render" in L.rt_last_error(cpu._h)


def test_slab_rows(cpu, golden_aov):
    f = frame_of(cpu, scene(3), 64, 48, rows=(16, 40))
    got = cpu.render_aov(f)
    assert got["id"].shape == (24, 64)
    want = {k: v[16:40] for k, v in want_of(golden_aov, "scene3").items()}
    assert aov_ref.planes_equal(got, want) == []
    assert cpu.stats().primary_rays == 24 * 64


def sentinel_planes(rows, w):
    return {"t": np.full((rows, w), SENTINEL, np.uint32).view(np.float32),
            "id": np.full((rows, w), SENTINEL, np.uint32).view(np.int32),
            "n": np.full((rows, w, 3), SENTINEL, np.uint32).view(np.float32)}


def test_band_set_and_rows_past_the_frame(cpu, oracle):
    """band_rows 16, count 3, index 1: bands 1 and 4 = frame rows 16..32 and
    64..80.  At 64 x 80 the set fills its 32 packed rows (and nothing behind
    them); at 64 x 72 band 4's rows 72..80 lie past the frame: the last 8
    packed rows keep the sentinel."""
    L = rt_amd.lib()
    for height, valid in ((80, 32), (72, 24)):
        f = frame_of(cpu, scene(3), 64, height, bands=(16, 3, 1))
        assert rt_amd.frame_rows(f) == 32
        buf = sentinel_planes(40, 64)
        aov = rt_amd.Aov(buf["t"].ctypes.data, buf["id"].ctypes.data, buf["n"].ctypes.data)
        assert L.rt_cpu_render_aov(cpu._h, ctypes.byref(f), ctypes.byref(aov)) == 0
        rows = list(range(16, 32)) + list(range(64, min(80, height)))
        want = aov_ref.oracle_aov(oracle, scene(3), 64, height, rows=rows)
        assert aov_ref.planes_equal({k: buf[k][:valid] for k in buf}, want) == []
        for k in buf:
            assert (buf[k][valid:].view(np.uint32) == SENTINEL).all(), (height, k)
        assert cpu.stats().primary_rays == valid * 64


def read_npy_v1(path):
    """A strict NumPy format 1.0 reader: what the CLI promises."""
    raw = open(path, "rb").read()
    assert raw[:6] == b"\x93NUMPY" and raw[6:8] == b"\x01\x00"
    hlen = int.from_bytes(raw[8:10], "little")
    assert (10 + hlen) % 64 == 0 and raw[10 + hlen - 1:10 + hlen] == b"\n"
    return np.load(path)


def test_cli_aov_cpu_backend(tmp_path, cpu, golden_aov):
    prefix = tmp_path / "s4"
    out = tmp_path / "s4.ppm"
    r = subprocess.run([EXE, scene(4), "-x", "64", "-y", "48", "--backend", "cpu", "--threads", str(THREADS),
                        "--aov", str(prefix), "-o", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert out.exists()                                    # the colour output is still written
    got = {k: read_npy_v1(f"{prefix}_{k}.npy") for k in ("t", "id", "n")}
    assert got["t"].dtype == np.dtype("<f4") and got["id"].dtype == np.dtype("<i4") and got["n"].dtype == np.dtype("<f4")
    lib = cpu.render_aov(frame_of(cpu, scene(4), 64, 48))
    assert aov_ref.planes_equal(got, lib) == []
    assert aov_ref.planes_equal(got, want_of(golden_aov, "scene4")) == []
    for extra in (["-g", "2"], ["--bands"]):
        bad = subprocess.run([EXE, scene(4), "-x", "32", "-y", "24", "--aov", str(prefix)] + extra,
                             capture_output=True, text=True, timeout=60)
        assert bad.returncode == 1 and "[ERREUR]" in bad.stderr and "--aov" in bad.stderr, extra


def test_cscene_aov_verb(golden_aov):
    c = rt_amd.CScene(backend="cpu", threads=THREADS)
    c.AjusterResolution(64, 48)
    c.AjusterNbRebondsMax(3)
    c.TraiterFichierDeScene(scene(7))
    got = c.LancerRayonsAOV()
    assert aov_ref.planes_equal(got, want_of(golden_aov, "scene7")) == []
    # with supersampling: the AOVs of the sample grid
    c.AjusterResolution(32, 24)
    c.AjusterSurEchantillonnage(2)
    assert aov_ref.planes_equal(c.LancerRayonsAOV(), want_of(golden_aov, "scene7")) == []


def test_cpu_render_aov_under_asan_ubsan(tmp_path):
    """cpu_render_aov (rt_cpu.cpp) in a stand-alone host program built with
    AddressSanitizer and UBSan: planes allocated at their exact sizes, full
    frames, slabs, band sets reaching past the frame, every subset of planes."""
    exe = tmp_path / "aov_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-I", CSRC,
                    os.path.join(REPO, "tools", "aov", "aov_check.cpp"), os.path.join(CSRC, "rt_cpu.cpp"),
                    "-o", str(exe)], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "aov_check: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
