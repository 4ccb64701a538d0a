"""Closest-hit queries of arbitrary rays (include/rt.h rt_trace_rays*) on the
CPU backend, the argument contract, the .npy reader, the CLI and the CScene
verb.

The expected hits are never computed by the code under test: tests/rays_ref.py
(ObtenirCouleur's loop over per-primitive distances) through liboracle.so's
oracle_intersect at test time, pinned where the fixture covers it to
tests/golden/rays.npz (made from the reference's own Intersection() through
oracle/_ref by tests/golden/make_rays_golden.py).  Comparison: id equal, t and
n word for word as uint32; where the expectation is NaN the result is NaN.
"""
from __future__ import annotations

import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

import ray_sets
import rays_ref
import rt_amd
from conftest import GOLDEN, REPO, scene

THREADS = min(8, os.cpu_count() or 1)
EXE = os.path.join(REPO, "ray-tracing-gpu_amd", "lib", "rt_render")
CSRC = os.path.join(REPO, "ray-tracing-gpu_amd", "csrc")
SMALL = [n for n in ray_sets.SCENES if n != "hf50k"]
INT32_MAX = 2**31 - 1


@pytest.fixture(scope="module")
def cpu():
    return rt_amd.CpuContext(THREADS)


@pytest.fixture(scope="module")
def golden_rays():
    return np.load(os.path.join(GOLDEN, "rays.npz"))


@pytest.fixture(scope="module")
def tmpdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("rays"))


def want_of(g, name):
    return {k: g[f"{name}_{k}"] for k in ("id", "t", "n")}


def test_header_and_binding_declare_the_feature():
    text = open(os.path.join(REPO, "include", "rt.h")).read()
    assert "#define RT_HAS_RAYS 1" in text and "#define RT_ABI_VERSION 8" in text
    assert "#define RT_OPT_RAY_BVH 22" in text
    assert rt_amd.lib().rt_abi_version() == 8
    for name in ("rt_trace_rays", "rt_trace_rays_async", "rt_cpu_trace_rays"):
        assert name in rt_amd.SIGNATURES and f"int {name}(" in text
    assert rt_amd.RAY_OPTIONS == {"ray_bvh": 22}
    taken = {**rt_amd.OPTIONS, **rt_amd.SS_OPTIONS, **rt_amd.LB_OPTIONS}
    assert not set(rt_amd.RAY_OPTIONS) & set(taken) and 22 not in taken.values()


def test_ray_bvh_option_defaults_to_off_and_round_trips(cpu):
    L = rt_amd.lib()
    v = ctypes.c_double(-1)
    assert L.rt_get_option(cpu._h, 22, ctypes.byref(v)) == 0 and v.value == 0.0
    assert L.rt_set_option(cpu._h, 22, 1.0) == 0
    assert L.rt_get_option(cpu._h, 22, ctypes.byref(v)) == 0 and v.value == 1.0
    assert L.rt_set_option(cpu._h, 22, 0.0) == 0


@pytest.mark.parametrize("name", SMALL)
def test_every_set_matches_the_oracle(cpu, oracle, golden_rays, tmpdir, name):
    """CpuContext.trace_rays on every set of the scene, bit for bit; the base
    set meets its conditions, and its rays and oracle-made expectation are the
    fixture's (made by the reference's own code)."""
    c = ray_sets.cases(oracle, name, tmpdir)
    base, want = c["sets"]["base"]
    ray_sets.check_conditions(ray_sets.conditions(want, c["types"]), name)
    assert hashlib.sha256(open(c["path"], "rb").read()).hexdigest() == str(golden_rays[f"{name}_sha256"])
    assert np.array_equal(base.view(np.uint32), golden_rays[f"{name}_rays"].view(np.uint32))
    assert rays_ref.hits_differ(want, want_of(golden_rays, name)) == []
    cpu.upload(rt_amd.Scene(c["path"], ray_sets.W, ray_sets.H))
    for label, (rays, exp) in c["sets"].items():
        got = cpu.trace_rays(rays)
        assert got["t"].shape == (len(rays),) and got["id"].dtype == np.int32 and got["n"].shape == (len(rays), 3)
        assert rays_ref.hits_differ(got, exp) == [], label
        st = cpu.stats()
        assert st.bounce_rays == len(rays) and st.primary_rays == 0 and st.kernel == "cpu_trace_rays"


def test_derived_sets_exercise_what_they_are_for(oracle, tmpdir):
    c = ray_sets.cases(oracle, "scene7", tmpdir)
    sets = c["sets"]
    # leaving a surface: no ray reports the surface it starts on at t ~ 0
    rays, want = sets["leaving"]
    assert len(rays) >= 64 and ((want["id"] < 0) | (want["t"] > np.float32(1e-2))).all()
    # scaled directions: t in units of |D| (the oracle's own values, to rounding)
    b, s3 = sets["base"][1], sets["scaled3"][1]
    hit = (b["id"] >= 0) & (s3["id"] == b["id"])
    assert hit.sum() >= 64 and np.allclose(s3["t"][hit] * 3, b["t"][hit], rtol=1e-4)
    # the zero direction hits nothing in this scene's oracle; non-finite rays sit beside finite ones
    assert len(sets["zero"][0]) == 64
    fin = np.isfinite(sets["nonfinite"][0]).all(1)
    assert fin.sum() >= 128 and (~fin).sum() >= 32


def test_heightfield_50k_fixture_rays(cpu, golden_rays, heightfield_path):
    """The 50,000-triangle heightfield on its fixture's 128 rays (the
    expectation is the reference's own, from rays.npz)."""
    g = golden_rays
    text = open(heightfield_path, "rb").read()
    assert hashlib.sha256(text).hexdigest() == str(g["hf50k_sha256"])
    rays = g["hf50k_rays"]
    assert rays.shape == (ray_sets.HF50K_RAYS, 6)
    cpu.upload(rt_amd.Scene(heightfield_path, 64, 32))
    assert rays_ref.hits_differ(cpu.trace_rays(rays), want_of(g, "hf50k")) == []


@pytest.mark.parametrize("only", ["t", "id", "n"])
def test_any_single_plane_alone(cpu, golden_rays, only):
    cpu.upload(rt_amd.Scene(scene(3), 64, 32))
    got = cpu.trace_rays(golden_rays["scene3_rays"], **{k: k == only for k in ("t", "id", "n")})
    assert list(got) == [only]
    assert rays_ref.hits_differ(got, want_of(golden_rays, "scene3"), keys=(only,)) == []


def test_argument_errors(cpu, golden_rays):
    L = rt_amd.lib()
    cpu.upload(rt_amd.Scene(scene(1), 64, 32))
    rays = np.ascontiguousarray(golden_rays["scene1_rays"][:8])
    SENT = 0x7FC12345
    t = np.full(8, SENT, np.uint32)
    none = rt_amd.Aov(None, None, None)
    some = rt_amd.Aov(t.ctypes.data, None, None)
    assert L.rt_cpu_trace_rays(None, rays.ctypes.data, 8, ctypes.byref(some)) == -1
    assert L.rt_trace_rays(None, rays.ctypes.data, 8, ctypes.byref(some)) == -1
    assert L.rt_trace_rays_async(None, rays.ctypes.data, 8, ctypes.byref(some), None) == -1
    assert L.rt_cpu_trace_rays(cpu._h, rays.ctypes.data, 8, ctypes.byref(none)) == -1
    assert L.rt_cpu_trace_rays(cpu._h, rays.ctypes.data, 8, None) == -1
    assert L.rt_cpu_trace_rays(cpu._h, None, 8, ctypes.byref(some)) == -1
    assert L.rt_cpu_trace_rays(cpu._h, rays.ctypes.data, -1, ctypes.byref(some)) == -1
    assert L.rt_cpu_trace_rays(cpu._h, rays.ctypes.data, INT32_MAX + 1, ctypes.byref(some)) == -1
    # n == 0: RT_OK, nothing written
    assert L.rt_cpu_trace_rays(cpu._h, rays.ctypes.data, 0, ctypes.byref(some)) == 0
    assert (t == SENT).all()
    assert L.rt_cpu_trace_rays(cpu._h, rays.ctypes.data, 8, ctypes.byref(some)) == 0
    assert (t != SENT).all()
    assert cpu.trace_rays(np.zeros((0, 6), np.float32))["id"].shape == (0,)
    with pytest.raises(ValueError):
        cpu.trace_rays(np.zeros((4, 5), np.float32))


def test_trace_before_upload_is_a_state_error():
    L = rt_amd.lib()
    h = ctypes.c_void_p()
    assert L.rt_create_cpu(1, ctypes.byref(h)) == 0
    try:
        rays = np.zeros((4, 6), np.float32)
        t = np.zeros(4, np.float32)
        some = rt_amd.Aov(t.ctypes.data, None, None)
        assert L.rt_cpu_trace_rays(h, rays.ctypes.data, 4, ctypes.byref(some)) == -4
        assert L.rt_cpu_trace_rays(h, rays.ctypes.data, 0, ctypes.byref(some)) == -4
    finally:
        L.rt_destroy(h)


def test_backend_is_explicit(cpu):
    """The HIP ray calls refuse a CPU context."""
    L = rt_amd.lib()
    cpu.upload(rt_amd.Scene(scene(1), 16, 16))
    rays = np.zeros((4, 6), np.float32)
    t = np.zeros(4, np.float32)
    some = rt_amd.Aov(t.ctypes.data, None, None)
    assert L.rt_trace_rays(cpu._h, rays.ctypes.data, 4, ctypes.byref(some)) == -4
    assert L.rt_trace_rays_async(cpu._h, rays.ctypes.data, 4, ctypes.byref(some), None) == -4
    assert b"rt_cpu_render" in L.rt_last_error(cpu._h)


def test_one_thread_and_many_threads_agree(golden_rays):
    one, many = rt_amd.CpuContext(1), rt_amd.CpuContext(THREADS)
    s = rt_amd.Scene(scene(9), 64, 32)
    one.upload(s)
    many.upload(s)
    rays = np.ascontiguousarray(np.tile(golden_rays["scene9_rays"], (5, 1))[:1237])  # not a multiple of the chunk
    assert rays_ref.hits_differ(one.trace_rays(rays), many.trace_rays(rays)) == []


def test_cscene_ray_verb(golden_rays):
    c = rt_amd.CScene(backend="cpu", threads=THREADS)
    c.AjusterResolution(64, 48)
    c.AjusterNbRebondsMax(3)
    c.TraiterFichierDeScene(scene(7))
    got = c.LancerListeDeRayons(golden_rays["scene7_rays"])
    assert rays_ref.hits_differ(got, want_of(golden_rays, "scene7")) == []


# ---- the CLI: --rays IN.npy --hits PREFIX
def read_npy_v1(path):
    raw = open(path, "rb").read()
    assert raw[:6] == b"\x93NUMPY" and raw[6:8] == b"\x01\x00"
    hlen = int.from_bytes(raw[8:10], "little")
    assert (10 + hlen) % 64 == 0 and raw[10 + hlen - 1:10 + hlen] == b"\n"
    return np.load(path)


def run_cli(*args, timeout=120):
    return subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, timeout=timeout)


def test_cli_rays_cpu_backend(tmp_path, golden_rays):
    rays = golden_rays["scene7_rays"]
    prefix = tmp_path / "h"
    for version in ((1, 0), (2, 0)):
        src = tmp_path / f"in{version[0]}.npy"
        with open(src, "wb") as f:
            np.lib.format.write_array(f, rays, version=version)
        r = run_cli(scene(7), "--backend", "cpu", "--threads", THREADS, "--rays", src, "--hits", prefix)
        assert r.returncode == 0, r.stderr
        assert not list(tmp_path.glob("*.ppm"))                      # -o is optional with --rays
        got = {k: read_npy_v1(f"{prefix}_{k}.npy") for k in ("t", "id", "n")}
        assert got["t"].dtype == np.dtype("<f4") and got["id"].dtype == np.dtype("<i4") and got["n"].shape == (256, 3)
        assert rays_ref.hits_differ(got, want_of(golden_rays, "scene7")) == []
        for k in ("t", "id", "n"):
            os.remove(f"{prefix}_{k}.npy")
    # with -o the frame is rendered too; --ray-bvh is accepted; an empty ray list is fine
    src = tmp_path / "empty.npy"
    np.save(src, np.zeros((0, 6), np.float32))
    out = tmp_path / "f.ppm"
    r = run_cli(scene(7), "-x", 32, "-y", 16, "--backend", "cpu", "--rays", src, "--hits", prefix, "--ray-bvh", "-o", out)
    assert r.returncode == 0, r.stderr
    assert out.exists() and read_npy_v1(f"{prefix}_n.npy").shape == (0, 3) and read_npy_v1(f"{prefix}_t.npy").shape == (0,)


def test_cli_refuses_what_the_reader_does_not_take(tmp_path, golden_rays):
    rays = golden_rays["scene7_rays"][:16]
    prefix = tmp_path / "h"
    bad = {
        "f8": rays.astype(np.float64),
        "big_endian": rays.astype(">f4"),
        "int32": np.zeros((16, 6), np.int32),
        "one_dim": rays.ravel(),
        "five_columns": np.ascontiguousarray(rays[:, :5]),
        "three_dims": rays.reshape(4, 4, 6),
        "fortran": np.asfortranarray(rays),
    }
    files = {}
    for k, a in bad.items():
        files[k] = tmp_path / f"{k}.npy"
        np.save(files[k], a)
    good = tmp_path / "good.npy"
    np.save(good, rays)
    raw = open(good, "rb").read()
    files["truncated"] = tmp_path / "truncated.npy"
    open(files["truncated"], "wb").write(raw[:-5])
    files["trailing"] = tmp_path / "trailing.npy"
    open(files["trailing"], "wb").write(raw + b"\0\0\0\0")
    files["version3"] = tmp_path / "version3.npy"
    open(files["version3"], "wb").write(raw[:6] + b"\x03\x00" + raw[8:])
    files["not_npy"] = tmp_path / "not_npy.npy"
    open(files["not_npy"], "wb").write(b"P6\n1 1\n255\n\0\0\0")
    files["missing"] = tmp_path / "missing.npy"
    for k, path in files.items():
        r = run_cli(scene(7), "--backend", "cpu", "--rays", path, "--hits", prefix, timeout=60)
        assert r.returncode == 1 and "[ERREUR]" in r.stderr and "--rays" in r.stderr, (k, r.stderr)
        assert not os.path.exists(f"{prefix}_t.npy"), k
    for extra in (["-g", "2"], ["--bands"]):
        r = run_cli(scene(7), "--rays", good, "--hits", prefix, *extra, timeout=60)
        assert r.returncode == 1 and "[ERREUR]" in r.stderr and "--rays" in r.stderr, extra
    r = run_cli(scene(7), "--backend", "cpu", "--rays", good, timeout=60)           # --hits missing
    assert r.returncode == 1 and "[ERREUR]" in r.stderr
    r = run_cli(scene(7), "--backend", "cpu", "--rays", good, "--hits", prefix, timeout=60)
    assert r.returncode == 0, r.stderr


def test_cpu_trace_rays_under_asan_ubsan(tmp_path):
    """cpu_trace_rays (rt_cpu.cpp) in a stand-alone host program built with
    AddressSanitizer and UBSan: arrays allocated at their exact sizes, n = 0,
    counts that are no multiple of the chunk, single planes, degenerate rays."""
    exe = tmp_path / "rays_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-I", CSRC,
                    os.path.join(REPO, "tools", "rays", "rays_check.cpp"), os.path.join(CSRC, "rt_cpu.cpp"),
                    "-o", str(exe)], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "rays_check: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
