"""Radiance queries of arbitrary rays (include/rt.h rt_shade_rays*) on the CPU
backend, the argument contract, the CLI and the CScene verb.

The expected colours are never computed by the code under test: the oracle's
own pixel loop pointed along each ray (tests/shade_ref.py, through
liboracle.so at test time), pinned where the fixture covers it to
tests/golden/shade.npz (the reference's own code through oracle/_ref, made by
tests/golden/make_shade_golden.py).  Comparison: word for word as uint32 — the
CPU backend calls the same libm powf as the oracle, so scenes with a shininess
are exact too.  The consistency sets (non-unit and infinite directions) have no
oracle expectation: they only have to run, and their finite lanes to stay
finite.
"""
from __future__ import annotations

import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

import aov_ref
import cameras
import rt_amd
import shade_ref
import shade_sets
from conftest import GOLDEN, REPO, bits_equal, scene

THREADS = min(8, os.cpu_count() or 1)
EXE = os.path.join(REPO, "ray-tracing-gpu_amd", "lib", "rt_render")
CSRC = os.path.join(REPO, "ray-tracing-gpu_amd", "csrc")
INT32_MAX = 2**31 - 1
F = np.float32
FIXTURE = ("scene2", "scene4", "scene7", "scene9", "mixed64", "soup1100")
# (depth, min_energy) of every scene; scene_ior 1.33 on top for the refracting ones
PARAMS = [(0, 0.01), (1, 0.01), (3, 0.01), (5, 0.01), (3, 0.5), (3, -1.0)]
IOR_SCENES = ("scene9", "refract_only96")


@pytest.fixture(scope="module")
def cpu():
    return rt_amd.CpuContext(THREADS)


@pytest.fixture(scope="module")
def golden_shade():
    return np.load(os.path.join(GOLDEN, "shade.npz"))


@pytest.fixture(scope="module")
def tmpdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("shade"))


def frame_of(s, depth, min_energy=0.01, scene_ior=1.0):
    f = s.frame.copy()
    f.max_bounces, f.min_energy, f.scene_ior = depth, min_energy, scene_ior
    return f


def test_header_and_binding_declare_the_feature():
    text = open(os.path.join(REPO, "include", "rt.h")).read()
    assert "#define RT_HAS_SHADE_RAYS 1" in text and "#define RT_ABI_VERSION 8" in text
    assert rt_amd.lib().rt_abi_version() == 8
    for name in ("rt_shade_rays", "rt_shade_rays_async", "rt_cpu_shade_rays"):
        assert name in rt_amd.SIGNATURES and f"int {name}(" in text
    variant = open(os.path.join(CSRC, "rt_variant.h")).read()
    assert "constexpr int kRayQuery = 16;" in variant and "RT_SHADE_RAYS_VARIANTS" in variant


@pytest.mark.parametrize("name", shade_sets.SCENES)
def test_every_set_matches_the_oracle(cpu, oracle, golden_shade, tmpdir, name):
    """CpuContext.shade_rays on every oracle set of the scene at every parameter
    set, bit for bit; the base set meets its conditions first, and where the
    fixture covers the scene its rays and colours are the oracle's."""
    c = shade_sets.cases(oracle, name, tmpdir)
    s = rt_amd.Scene(c["path"], shade_sets.W, shade_sets.H, 3)
    c0 = shade_sets.expected(oracle, c, "base", 0)
    c3 = shade_sets.expected(oracle, c, "base", 3)
    cond = shade_sets.conditions(c0, c3 if name in shade_sets.BOUNCE else None, s.frame.background[:])
    shade_sets.check_conditions(cond, name)
    if name in FIXTURE:
        g = golden_shade
        assert hashlib.sha256(open(c["path"], "rb").read()).hexdigest() == str(g[f"{name}_sha256"])
        assert bits_equal(g[f"{name}_rays"], c["rays"]["base"])
        assert shade_ref.colours_differ(c0, g[f"{name}_d0"]) == [] and shade_ref.colours_differ(c3, g[f"{name}_d3"]) == []
    cpu.upload(s)
    params = [(d, e, 1.0) for d, e in PARAMS] + ([(3, 0.01, 1.33), (5, 0.01, 1.33)] if name in IOR_SCENES else [])
    for depth, me, ior in params:
        f = frame_of(s, depth, me, ior)
        for label in shade_sets.ORACLE_SETS:
            rays = c["rays"][label]
            got = cpu.shade_rays(rays, f)
            assert got.shape == (len(rays), 3) and got.dtype == np.float32
            want = shade_sets.expected(oracle, c, label, depth, me, ior)
            assert shade_ref.colours_differ(got, want, f"{label} depth {depth} e {me} ior {ior}") == []
            st = cpu.stats()
            assert st.primary_rays == len(rays) and st.kernel == "cpu_shade_rays"


def test_sets_exercise_what_they_are_for(oracle, tmpdir):
    c = shade_sets.cases(oracle, "scene7", tmpdir)
    rays = c["rays"]
    assert len(rays["base"]) == shade_sets.N_BASE and len(rays["leaving"]) >= 32 and len(rays["zero"]) == 64
    assert (rays["zero"][:, 3:] == 0).all()
    ax = rays["axis"][:, 3:]
    assert ((ax == 0).sum(1) >= 1).all() and ((ax == 0).sum(1) == 2).any()
    o = rays["nonfinite_o"]
    assert (~np.isfinite(o[:, :3]).all(1)).sum() == 32 and np.isfinite(o[:, 3:]).all()
    d = rays["nan_d"]
    bad = ~np.isfinite(c["sets"]["nan_d"][1]).all(1)
    # the normaliser's rule: a NaN length fails `> EPSILON` (D = 0), an infinite one gives inf * 0 = NaN
    assert bad.sum() == 32 and np.isfinite(d[~bad]).all()
    assert ((d[bad, 3:] == 0) | np.isnan(d[bad, 3:])).all() and np.isnan(d[bad, 3:]).any() and (d[bad, 3:] == 0).all(1).any()
    # unit directions: the normaliser's own, within a few ulps of length 1
    n = np.linalg.norm(rays["base"][:, 3:].astype(np.float64), axis=1)
    assert np.abs(n - 1).max() < 1e-6
    # a bounce changes what leaves a reflecting surface
    assert (shade_sets.expected(oracle, c, "leaving", 0) != shade_sets.expected(oracle, c, "leaving", 3)).any()


def test_background_comes_from_params(cpu, oracle, tmpdir):
    """A copy of scene7's text with another `background:` line: the oracle reads it from the file,
    the product from params — and from nowhere else."""
    c = shade_sets.cases(oracle, "scene7", tmpdir)
    src = open(scene(7), "rb").read().decode("latin-1").split("\n")
    k = [i for i, l in enumerate(src) if l.strip().startswith("background:")]
    assert len(k) == 1
    src[k[0]] = src[k[0]].split("background:")[0] + "background: 200 30 90"
    path = os.path.join(tmpdir, "scene7_bg.dat")
    with open(path, "w", encoding="latin-1") as f:
        f.write("\n".join(src))
    s_old, s_new = rt_amd.Scene(scene(7), 64, 32, 3), rt_amd.Scene(path, 64, 32, 3)
    assert s_old.frame.background[:] != s_new.frame.background[:]
    cpu.upload(s_old)   # the OLD file's scene, the new file's parameters
    for label in ("base", "leaving"):
        want = shade_sets.expected(oracle, c, label, 3, path=path)
        assert (want != shade_sets.expected(oracle, c, label, 3)).any()
        assert shade_ref.colours_differ(cpu.shade_rays(c["rays"][label], frame_of(s_new, 3)), want, label) == []


@pytest.mark.parametrize("name", ["scene7", "scene9", "mixed65", "hf1600r"])
def test_consistency_sets_run_and_stay_finite(cpu, oracle, tmpdir, name):
    """Consistency, not parity: no oracle shades a non-unit or an infinite direction.  The sets run,
    lanes with finite rays give finite colours, and a scaled direction that hits the same first
    surface still sees a lit scene."""
    c = shade_sets.cases(oracle, name, tmpdir)
    s = rt_amd.Scene(c["path"], 64, 32, 3)
    cpu.upload(s)
    for depth in (0, 3):
        f = frame_of(s, depth)
        for label, rays in c["consistency"].items():
            got = cpu.shade_rays(rays, f)
            fin = np.isfinite(rays).all(1)
            assert got.shape == (len(rays), 3) and np.isfinite(got[fin]).all(), label
            assert bits_equal(got, cpu.shade_rays(rays, f)), label   # and deterministic


@pytest.mark.parametrize("which,depth", [("scene2", 0), ("scene7", 3), ("moved", 3)])
def test_a_frame_equals_the_query_of_its_camera_rays(cpu, which, depth):
    """64 x 32: render_float equals shade_rays of the frame's camera rays (aov_ref.camera_dirs)."""
    s = rt_amd.Scene(scene(7 if which == "moved" else int(which[-1])), 64, 32, depth)
    f = s.frame
    if which == "moved":
        f = cameras.cameras(s.frame)[2]   # moved, yawed and pitched
        assert f.cam_pos[:] != s.frame.cam_pos[:] or f.orient[:] != s.frame.orient[:]
    cpu.upload(s)
    img = cpu.render_float(f)
    ys, xs = np.meshgrid(np.arange(32), np.arange(64), indexing="ij")
    D = aov_ref.camera_dirs(aov_ref.Cam.from_frame(f), xs.ravel(), ys.ravel())
    O = np.broadcast_to(np.asarray(f.cam_pos[:], F), D.shape)
    got = cpu.shade_rays(np.concatenate([O, D], 1), f)
    assert bits_equal(got.reshape(img.shape), img)


def test_argument_errors(cpu, golden_shade):
    L = rt_amd.lib()
    s = rt_amd.Scene(scene(7), 64, 32, 3)
    cpu.upload(s)
    f = s.frame
    rays = np.ascontiguousarray(golden_shade["scene7_rays"][:8])
    SENT = 0x7FC12345
    out = np.full((8, 3), SENT, np.uint32)
    assert L.rt_cpu_shade_rays(None, f, rays.ctypes.data, 8, out.ctypes.data) == -1
    assert L.rt_shade_rays(None, f, rays.ctypes.data, 8, out.ctypes.data) == -1
    assert L.rt_shade_rays_async(None, f, rays.ctypes.data, 8, out.ctypes.data, None) == -1
    assert L.rt_cpu_shade_rays(cpu._h, None, rays.ctypes.data, 8, out.ctypes.data) == -1     # no params
    assert L.rt_cpu_shade_rays(cpu._h, f, None, 8, out.ctypes.data) == -1
    assert L.rt_cpu_shade_rays(cpu._h, f, rays.ctypes.data, 8, None) == -1
    assert L.rt_cpu_shade_rays(cpu._h, f, rays.ctypes.data, -1, out.ctypes.data) == -1
    assert L.rt_cpu_shade_rays(cpu._h, f, rays.ctypes.data, INT32_MAX + 1, out.ctypes.data) == -1
    assert L.rt_cpu_shade_rays(cpu._h, f, rays.ctypes.data, 0, out.ctypes.data) == 0          # n == 0: nothing written
    assert (out == SENT).all()
    assert L.rt_cpu_shade_rays(cpu._h, f, rays.ctypes.data, 8, out.ctypes.data) == 0
    assert shade_ref.colours_differ(out.view(np.float32), golden_shade["scene7_d3"][:8]) == []
    assert cpu.shade_rays(np.zeros((0, 6), np.float32), f).shape == (0, 3)
    with pytest.raises(ValueError):
        cpu.shade_rays(np.zeros((4, 5), np.float32), f)


def test_shade_before_upload_is_a_state_error():
    L = rt_amd.lib()
    h = ctypes.c_void_p()
    assert L.rt_create_cpu(1, ctypes.byref(h)) == 0
    try:
        f = rt_amd.Scene(scene(1), 16, 16).frame
        rays, out = np.zeros((4, 6), np.float32), np.zeros((4, 3), np.float32)
        assert L.rt_cpu_shade_rays(h, f, rays.ctypes.data, 4, out.ctypes.data) == -4
        assert L.rt_cpu_shade_rays(h, f, rays.ctypes.data, 0, out.ctypes.data) == -4
    finally:
        L.rt_destroy(h)


def test_backend_is_explicit(cpu):
    """The HIP shade calls refuse a CPU context."""
    L = rt_amd.lib()
    s = rt_amd.Scene(scene(1), 16, 16)
    cpu.upload(s)
    rays, out = np.zeros((4, 6), np.float32), np.zeros((4, 3), np.float32)
    assert L.rt_shade_rays(cpu._h, s.frame, rays.ctypes.data, 4, out.ctypes.data) == -4
    assert L.rt_shade_rays_async(cpu._h, s.frame, rays.ctypes.data, 4, out.ctypes.data, None) == -4


def test_one_thread_and_many_threads_agree(golden_shade):
    one, many = rt_amd.CpuContext(1), rt_amd.CpuContext(THREADS)
    s = rt_amd.Scene(scene(9), 64, 32, 3)
    one.upload(s)
    many.upload(s)
    rays = np.ascontiguousarray(np.tile(golden_shade["scene9_rays"], (10, 1))[:1237])  # not a multiple of the chunk
    a, b = one.shade_rays(rays, s.frame), many.shade_rays(rays, s.frame)
    assert bits_equal(a, b)
    assert shade_ref.colours_differ(a[:128], golden_shade["scene9_d3"]) == []


def test_cscene_colour_verb(golden_shade):
    c = rt_amd.CScene(backend="cpu", threads=THREADS)
    c.AjusterResolution(64, 48)
    c.AjusterNbRebondsMax(3)
    c.TraiterFichierDeScene(scene(7))
    assert shade_ref.colours_differ(c.LancerListeDeRayonsCouleur(golden_shade["scene7_rays"]), golden_shade["scene7_d3"]) == []
    c.AjusterNbRebondsMax(0)
    assert shade_ref.colours_differ(c.LancerListeDeRayonsCouleur(golden_shade["scene7_rays"]), golden_shade["scene7_d0"]) == []


# ---- the CLI: --rays IN.npy --colours OUT.npy
def run_cli(*args, timeout=120):
    return subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, timeout=timeout)


def test_cli_colours_cpu_backend(tmp_path, golden_shade):
    g = golden_shade
    src, dst, prefix = tmp_path / "in.npy", tmp_path / "c.npy", tmp_path / "h"
    np.save(src, g["scene7_rays"])
    # alone, at -d 3
    r = run_cli(scene(7), "--backend", "cpu", "--threads", THREADS, "-d", 3, "--rays", src, "--colours", dst)
    assert r.returncode == 0, r.stderr
    got = np.load(dst)
    assert got.dtype == np.dtype("<f4") and shade_ref.colours_differ(got, g["scene7_d3"]) == []
    assert "cpu_shade_rays" in r.stdout and not list(tmp_path.glob("*.ppm")) and not os.path.exists(f"{prefix}_t.npy")
    # beside --hits, at the default depth 0
    os.remove(dst)
    r = run_cli(scene(7), "--backend", "cpu", "--rays", src, "--hits", prefix, "--colours", dst)
    assert r.returncode == 0, r.stderr
    assert shade_ref.colours_differ(np.load(dst), g["scene7_d0"]) == [] and np.load(f"{prefix}_id.npy").shape == (128,)
    # an empty ray list
    np.save(src, np.zeros((0, 6), np.float32))
    r = run_cli(scene(7), "--backend", "cpu", "--rays", src, "--colours", dst)
    assert r.returncode == 0 and np.load(dst).shape == (0, 3)


def test_cli_refusals(tmp_path, golden_shade):
    src, dst = tmp_path / "in.npy", tmp_path / "c.npy"
    np.save(src, golden_shade["scene7_rays"][:16])
    for args in (["--colours", dst],                                   # no --rays
                 ["--rays", src],                                      # neither --hits nor --colours
                 ["--rays", src, "--colours"],                         # no file name
                 ["--rays", src, "--colours", dst, "-g", "2"],         # one GPU only
                 ["--rays", src, "--colours", dst, "--bands"],
                 ["--rays", tmp_path / "missing.npy", "--colours", dst]):
        r = run_cli(scene(7), "--backend", "cpu" if "-g" not in args and "--bands" not in args else "hip", *args, timeout=60)
        assert r.returncode == 1 and "[ERREUR]" in r.stderr, (args, r.stderr)
        assert not os.path.exists(dst), args


def test_cpu_shade_rays_under_asan_ubsan(tmp_path):
    """cpu_shade_rays (rt_cpu.cpp) in a stand-alone host program built with AddressSanitizer and
    UBSan: arrays allocated at their exact sizes, n = 0, counts that are no multiple of the chunk,
    bounce depths 0 .. 5, degenerate rays."""
    exe = tmp_path / "shade_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-I", CSRC,
                    os.path.join(REPO, "tools", "shade", "shade_check.cpp"), os.path.join(CSRC, "rt_cpu.cpp"),
                    "-o", str(exe)], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "shade_check: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
