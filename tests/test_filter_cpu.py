"""Shadow-filter queries of arbitrary segments (include/rt.h rt_filter_rays*)
on the CPU backend, the argument contract, the CLI and the CScene verb.

The expected filters are never computed by the code under test:
tests/filter_ref.py (ObtenirFiltreDeSurface's loop over per-primitive
distances) through liboracle.so's oracle_intersect at test time, pinned where
the fixture covers it to tests/golden/filter.npz (made from the reference's own
Intersection() through oracle/_ref by tests/golden/make_filter_golden.py).
Comparison: word for word as uint32; where the expectation is NaN the result
is NaN.
"""
from __future__ import annotations

import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

import filter_ref
import filter_sets
import rt_amd
from conftest import GOLDEN, REPO, scene

THREADS = min(8, os.cpu_count() or 1)
EXE = os.path.join(REPO, "ray-tracing-gpu_amd", "lib", "rt_render")
CSRC = os.path.join(REPO, "ray-tracing-gpu_amd", "csrc")
INT32_MAX = 2**31 - 1
FIXTURE_SETS = [("scene7", None), ("layers", "cross"), ("mixed65", "through")]


@pytest.fixture(scope="module")
def cpu():
    return rt_amd.CpuContext(THREADS)


@pytest.fixture(scope="module")
def golden_filter():
    return np.load(os.path.join(GOLDEN, "filter.npz"))


@pytest.fixture(scope="module")
def tmpdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("filter"))


def test_header_and_binding_declare_the_feature():
    text = open(os.path.join(REPO, "include", "rt.h")).read()
    assert "#define RT_HAS_FILTER_RAYS 1" in text and "#define RT_ABI_VERSION 8" in text
    assert rt_amd.lib().rt_abi_version() == 8
    for name in ("rt_filter_rays", "rt_filter_rays_async", "rt_cpu_filter_rays"):
        assert name in rt_amd.SIGNATURES and f"int {name}(" in text


def test_generated_scenes_are_what_the_sets_assume(oracle, tmpdir):
    """layers: 130 surfaces, 128 triangles, 113 translucent; the loader and
    the oracle keep neg6's negated coefficients."""
    surf = filter_sets.cases(oracle, "layers", tmpdir)["surf"]
    fc = filter_ref.factors(surf)
    assert len(surf) == 130 and int((surf[:, 0] == 0).sum()) == 128 and int((fc != 0).any(1).sum()) == 113
    assert len(filter_sets.cases(oracle, "layers10", tmpdir)["surf"]) == 322
    s6 = oracle.dump(scene(6), 64, 32)[0]
    n6 = filter_sets.cases(oracle, "neg6", tmpdir)["surf"]
    assert (s6[:, 9] > 0).sum() >= 1 and np.array_equal(n6[:, 9], -s6[:, 9]) and (n6[:, 9] == np.float32(-0.9)).any()
    material = rt_amd.Scene(filter_sets.file("neg6", tmpdir), 64, 32).arrays()[2]
    assert np.array_equal(material[:, 8], n6[:, 9])
    ln = filter_sets.cases(oracle, "layers_neg", tmpdir)["surf"]
    assert int((ln[:, 9] < 0).sum()) == 32


@pytest.mark.parametrize("name", filter_sets.SCENES)
def test_every_set_matches_the_oracle(cpu, oracle, tmpdir, name):
    """CpuContext.filter_rays on every set of the scene, bit for bit, after
    the conditions on the expectation itself."""
    c = filter_sets.cases(oracle, name, tmpdir)
    filter_sets.check_conditions(name, c["sets"])
    cpu.upload(rt_amd.Scene(c["path"], filter_sets.W, filter_sets.H))
    for label, (segs, d) in c["sets"].items():
        got = cpu.filter_rays(segs)
        assert got.shape == (len(segs), 3) and got.dtype == np.float32
        assert filter_ref.differ(got, d["filter"]) == [], label
        st = cpu.stats()
        assert st.shadow_rays == len(segs) and st.primary_rays == 0 and st.bounce_rays == 0
        assert st.kernel == "cpu_filter_rays"


@pytest.mark.parametrize("name,only", FIXTURE_SETS)
def test_fixture_sets(cpu, oracle, golden_filter, tmpdir, name, only):
    """The segments and the oracle-made expectation are the fixture's (made by
    the reference's own code), and the CPU backend returns its filters."""
    g = golden_filter
    c = filter_sets.cases(oracle, name, tmpdir)
    assert hashlib.sha256(open(c["path"], "rb").read()).hexdigest() == str(g[f"{name}_sha256"])
    cpu.upload(rt_amd.Scene(c["path"], filter_sets.W, filter_sets.H))
    labels = [only] if only else list(c["sets"])
    for label in labels:
        segs, d = c["sets"][label]
        assert np.array_equal(segs.view(np.uint32), g[f"{name}_{label}_segs"].view(np.uint32)), label
        assert filter_ref.differ(d["filter"], g[f"{name}_{label}_filter"]) == [], label
        assert filter_ref.differ(cpu.filter_rays(g[f"{name}_{label}_segs"]), g[f"{name}_{label}_filter"]) == [], label


def test_heightfield_50k_fixture_segments(cpu, golden_filter, heightfield_path):
    g = golden_filter
    assert hashlib.sha256(open(heightfield_path, "rb").read()).hexdigest() == str(g["hf50k_sha256"])
    segs = g["hf50k_segs"]
    assert segs.shape == (128, 6)
    want = g["hf50k_filter"]
    assert filter_sets.white(want).sum() >= 16 and filter_sets.black(want).sum() >= 16
    cpu.upload(rt_amd.Scene(heightfield_path, 64, 32))
    assert filter_ref.differ(cpu.filter_rays(segs), want) == []


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_counts(cpu, golden_filter, n):
    g = golden_filter
    cpu.upload(rt_amd.Scene(scene(7), 64, 32))
    reps = -(-max(n, 1) // 256)
    segs = np.ascontiguousarray(np.tile(g["scene7_through_segs"], (reps, 1))[:n])
    want = np.tile(g["scene7_through_filter"], (reps, 1))[:n]
    got = cpu.filter_rays(segs)
    assert got.shape == (n, 3) and filter_ref.differ(got, want) == []


def test_argument_errors(cpu, golden_filter):
    L = rt_amd.lib()
    cpu.upload(rt_amd.Scene(scene(1), 64, 32))
    segs = np.ascontiguousarray(golden_filter["scene7_through_segs"][:8])
    SENT = 0x7FC12345
    f = np.full(24, SENT, np.uint32)
    assert L.rt_cpu_filter_rays(None, segs.ctypes.data, 8, f.ctypes.data) == -1
    assert L.rt_filter_rays(None, segs.ctypes.data, 8, f.ctypes.data) == -1
    assert L.rt_filter_rays_async(None, segs.ctypes.data, 8, f.ctypes.data, None) == -1
    assert L.rt_cpu_filter_rays(cpu._h, segs.ctypes.data, 8, None) == -1
    assert L.rt_cpu_filter_rays(cpu._h, None, 8, f.ctypes.data) == -1
    assert L.rt_cpu_filter_rays(cpu._h, segs.ctypes.data, -1, f.ctypes.data) == -1
    assert L.rt_cpu_filter_rays(cpu._h, segs.ctypes.data, INT32_MAX + 1, f.ctypes.data) == -1
    # n == 0: RT_OK, nothing written (null pointers included)
    assert L.rt_cpu_filter_rays(cpu._h, segs.ctypes.data, 0, f.ctypes.data) == 0
    assert L.rt_cpu_filter_rays(cpu._h, None, 0, None) == 0
    assert (f == SENT).all()
    assert L.rt_cpu_filter_rays(cpu._h, segs.ctypes.data, 8, f.ctypes.data) == 0
    assert (f != SENT).all()
    assert cpu.filter_rays(np.zeros((0, 6), np.float32)).shape == (0, 3)
    with pytest.raises(ValueError):
        cpu.filter_rays(np.zeros((4, 5), np.float32))


def test_filter_before_upload_is_a_state_error():
    L = rt_amd.lib()
    h = ctypes.c_void_p()
    assert L.rt_create_cpu(1, ctypes.byref(h)) == 0
    try:
        segs = np.zeros((4, 6), np.float32)
        f = np.zeros(12, np.float32)
        assert L.rt_cpu_filter_rays(h, segs.ctypes.data, 4, f.ctypes.data) == -4
        assert L.rt_cpu_filter_rays(h, segs.ctypes.data, 0, f.ctypes.data) == -4
    finally:
        L.rt_destroy(h)


def test_backend_is_explicit(cpu):
    """The HIP filter calls refuse a CPU context."""
    L = rt_amd.lib()
    cpu.upload(rt_amd.Scene(scene(1), 16, 16))
    segs = np.zeros((4, 6), np.float32)
    f = np.zeros(12, np.float32)
    assert L.rt_filter_rays(cpu._h, segs.ctypes.data, 4, f.ctypes.data) == -4
    assert L.rt_filter_rays_async(cpu._h, segs.ctypes.data, 4, f.ctypes.data, None) == -4
    assert b"rt_cpu_render" in L.rt_last_error(cpu._h)


def test_one_thread_and_many_threads_agree(golden_filter):
    one, many = rt_amd.CpuContext(1), rt_amd.CpuContext(THREADS)
    s = rt_amd.Scene(scene(7), 64, 32)
    one.upload(s)
    many.upload(s)
    segs = np.ascontiguousarray(np.tile(golden_filter["scene7_lights_segs"], (12, 1))[:1237])  # no multiple of the chunk
    assert len(segs) == 1237
    assert filter_ref.differ(one.filter_rays(segs), many.filter_rays(segs)) == []


def test_cscene_shadow_ray_verb(golden_filter):
    c = rt_amd.CScene(backend="cpu", threads=THREADS)
    c.AjusterResolution(64, 48)
    c.AjusterNbRebondsMax(3)
    c.TraiterFichierDeScene(scene(7))
    got = c.LancerListeDeRayonsOmbre(golden_filter["scene7_through_segs"])
    assert filter_ref.differ(got, golden_filter["scene7_through_filter"]) == []


# ---- the CLI: --segments IN.npy --filters OUT.npy
def run_cli(*args, timeout=120):
    return subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, timeout=timeout)


def test_cli_segments_cpu_backend(tmp_path, golden_filter):
    g = golden_filter
    src, dst = tmp_path / "segs.npy", tmp_path / "filters.npy"
    np.save(src, g["scene7_through_segs"])
    r = run_cli(scene(7), "--backend", "cpu", "--threads", THREADS, "--segments", src, "--filters", dst)
    assert r.returncode == 0, r.stderr
    assert "cpu_filter_rays" in r.stdout and not list(tmp_path.glob("*.ppm"))
    got = np.load(dst)
    assert got.dtype == np.dtype("<f4") and got.shape == (256, 3)
    assert filter_ref.differ(got, g["scene7_through_filter"]) == []
    # an empty list is fine; --rays can be combined; a missing half is refused
    np.save(src, np.zeros((0, 6), np.float32))
    r = run_cli(scene(7), "--backend", "cpu", "--segments", src, "--filters", dst, "--rays", src, "--hits",
                tmp_path / "h")
    assert r.returncode == 0, r.stderr
    assert np.load(dst).shape == (0, 3) and np.load(tmp_path / "h_t.npy").shape == (0,)
    r = run_cli(scene(7), "--backend", "cpu", "--segments", src)
    assert r.returncode == 1 and "[ERREUR]" in r.stderr
    np.save(src, np.zeros((4, 5), np.float32))
    r = run_cli(scene(7), "--backend", "cpu", "--segments", src, "--filters", dst)
    assert r.returncode == 1 and "[ERREUR]" in r.stderr and "--segments" in r.stderr


def test_cpu_filter_rays_under_asan_ubsan(tmp_path):
    """cpu_filter_rays (rt_cpu.cpp) in a stand-alone host program built with
    AddressSanitizer and UBSan: arrays allocated at their exact sizes, n = 0,
    counts that are no multiple of the chunk, degenerate segments."""
    exe = tmp_path / "filter_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-I", CSRC,
                    os.path.join(REPO, "tools", "filter", "filter_check.cpp"), os.path.join(CSRC, "rt_cpu.cpp"),
                    "-o", str(exe)], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "filter_check: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
