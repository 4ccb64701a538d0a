"""Supersampled anti-aliasing (include/rt.h rt_render_ss*, csrc/rt_resolve.h)
on the CPU backend, the argument contract, the CLI and the CScene verb.  The
sample grid of a W x H image with factor s is the reference's own frame at
s W x s H, so the expected image is ssaa_ref.box of a fixture made from the
reference's sources (tests/golden/images.npz) or of the oracle's frame: bit
for bit on this backend, scene4's Phong highlights included (glibc powf, as
in test_cpu_backend.py)."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

import rt_amd
from conftest import REPO, bits_equal, rgba8, scene
from ssaa_ref import box

THREADS = min(8, os.cpu_count() or 1)
EXE = os.path.join(REPO, "ray-tracing-gpu_amd", "lib", "rt_render")
CSRC = os.path.join(REPO, "ray-tracing-gpu_amd", "csrc")


@pytest.fixture(scope="module")
def cpu():
    return rt_amd.CpuContext(THREADS)


def sample_frame(ctx, path, w, h, depth, rows=None, bands=None):
    s = rt_amd.Scene(path, w, h, depth)
    ctx.upload(s)
    f = s.frame.copy()
    if rows:
        f.row_begin, f.row_end = rows
    if bands:
        f.band_rows, f.band_count, f.band_index = bands
    return f


def test_box_reference_is_the_contract():
    """The numpy reference itself, on numbers worked out by hand: the sum
    starts as the first sample, runs row-major, and ends in a division (at
    s = 3 a multiply by the rounded 1/9 gives other bits)."""
    a = np.zeros((3, 3, 3), np.float32)
    a[..., 0] = np.float32(1.0)                                 # 9 / 9
    a[..., 1] = np.arange(9, dtype=np.float32).reshape(3, 3)    # 36 / 9
    big, one = np.float32(2.0 ** 24), np.float32(1.0)
    a[..., 2] = one
    a[0, 0, 2] = big                                            # 2^24 + 1 + ... stays 2^24 sequentially
    got = box(a, 3)
    assert got.shape == (1, 1, 3)
    assert got[0, 0, 0] == np.float32(1.0) and got[0, 0, 1] == np.float32(4.0)
    assert got[0, 0, 2] == big / np.float32(9.0)
    x = np.full((3, 3, 3), np.float32(0.1), np.float32)
    acc = np.float32(0.1)
    for _ in range(8):
        acc = np.float32(acc + np.float32(0.1))
    assert box(x, 3)[0, 0, 0] == np.float32(acc / np.float32(9.0))
    # the division is not a multiply by the reciprocal for some float32 sums
    sums = np.arange(1, 200, dtype=np.float32)
    assert np.any(sums / np.float32(9.0) != sums * np.float32(np.float32(1.0) / np.float32(9.0)))


@pytest.mark.parametrize("i", range(1, 10))
@pytest.mark.parametrize("depth", [0, 3])
@pytest.mark.parametrize("s", [2, 4, 8])
def test_scene_images_match_boxed_reference(cpu, golden_images, i, depth, s):
    f = sample_frame(cpu, scene(i), 64, 48, depth)
    want = box(golden_images[f"scene{i}_64x48_d{depth}"], s)
    got = cpu.render_ss_float(f, s)
    assert got.shape == (48 // s, 64 // s, 3)
    assert bits_equal(got, want)
    assert np.array_equal(cpu.render_ss(f, s), rgba8(want))


def test_filter_is_not_subsampling(golden_images):
    """The fixtures can tell the filter from picking one sample."""
    a = golden_images["scene7_64x48_d3"]
    assert np.mean(np.any(box(a, 2) != a[::2, ::2], axis=-1)) > 0.5


def test_factor_one_is_the_plain_render(cpu):
    f = sample_frame(cpu, scene(7), 64, 48, 3)
    assert bits_equal(cpu.render_ss_float(f, 1), cpu.render_float(f))
    assert np.array_equal(cpu.render_ss(f, 1), cpu.render(f))


def test_odd_factor_and_ragged_width(cpu, oracle):
    """66 x 33 samples, s = 3: a 22 x 11 image (no multiple of 4 or 8 anywhere)."""
    f = sample_frame(cpu, scene(5), 66, 33, 3)
    got = cpu.render_ss_float(f, 3)
    assert got.shape == (11, 22, 3)
    assert bits_equal(got, box(oracle.render(scene(5), 66, 33, 3), 3))


def test_whole_frame_into_one_pixel(cpu, oracle):
    f = sample_frame(cpu, scene(5), 8, 8, 3)
    got = cpu.render_ss_float(f, 8)
    assert got.shape == (1, 1, 3)
    assert bits_equal(got, box(oracle.render(scene(5), 8, 8, 3), 8))


def test_slab_rows(cpu, golden_images):
    """Sample rows [16, 48) at s = 2 are output rows 8..24."""
    want = box(golden_images["scene7_64x48_d3"], 2)
    f = sample_frame(cpu, scene(7), 64, 48, 3, rows=(16, 48))
    assert rt_amd.ss_rows(f, 2) == 16
    assert bits_equal(cpu.render_ss_float(f, 2), want[8:24])
    assert np.array_equal(cpu.render_ss(f, 2), rgba8(want[8:24]))


@pytest.mark.parametrize("index", [0, 1])
def test_bands(cpu, golden_images, index):
    """band_rows 32, two ranks, s = 2: rank 0 has sample rows 0..32 (output
    0..16); rank 1 has 32..64, of which 32..48 are in the frame (output
    16..24) — its other 8 output rows stay unwritten, as in rt_render."""
    want = box(golden_images["scene7_64x48_d3"], 2)
    f = sample_frame(cpu, scene(7), 64, 48, 3, bands=(32, 2, index))
    got = cpu.render_ss_float(f, 2)
    assert got.shape == (16, 32, 3)
    if index == 0:
        assert bits_equal(got, want[:16])
    else:
        assert bits_equal(got[:8], want[16:24])
        assert not got[8:].any()


def test_ss_rows_and_argument_errors(cpu):
    L = rt_amd.lib()
    f = sample_frame(cpu, scene(1), 64, 48, 0)
    out = np.zeros((48, 64, 4), np.float32)
    for s, rows in ((1, 48), (2, 24), (4, 12), (8, 6)):
        assert L.rt_ss_rows(ctypes.byref(f), s) == rows == rt_amd.ss_rows(f, s)
    assert L.rt_ss_rows(None, 2) == -1

    def bad(frame, s):
        assert L.rt_ss_rows(ctypes.byref(frame), s) == -1
        assert L.rt_cpu_render_ss(cpu._h, ctypes.byref(frame), s, out.ctypes.data) == -1
        assert L.rt_cpu_render_ss_float(cpu._h, ctypes.byref(frame), s, out.ctypes.data) == -1
        with pytest.raises(ValueError):
            rt_amd.ss_rows(frame, s)

    for s in (0, -1, 9, 64):           # s outside 1..8
        bad(f, s)
    bad(f, 5)                          # 5 does not divide 64
    bad(f, 7)
    bad(f, 3)                          # 3 divides the height only
    g = sample_frame(cpu, scene(1), 64, 44, 0)
    bad(g, 8)                          # 8 divides the width, not the height 44
    g = f.copy()
    g.row_begin = 2
    bad(g, 4)                          # s does not divide row_begin
    g = f.copy()
    g.row_end = 46
    bad(g, 4)                          # s does not divide row_end
    assert L.rt_ss_rows(ctypes.byref(g), 2) == 23
    g = f.copy()
    g.band_rows, g.band_count, g.band_index = 16, 2, 0
    bad(g, 2)                          # band_rows must be a multiple of 16 s
    g.band_rows = 48
    bad(g, 2)
    assert L.rt_ss_rows(ctypes.byref(g), 1) == 48   # (48 = 16 x 3: fine for s = 1, and for s = 3 of a width 3 divides)
    g.band_rows = 32
    assert L.rt_ss_rows(ctypes.byref(g), 2) == 16
    g.band_index = 2                   # a bad band layout is a bad pair
    bad(g, 2)
    assert L.rt_cpu_render_ss(cpu._h, ctypes.byref(f), 2, None) == -1
    assert L.rt_cpu_render_ss(None, ctypes.byref(f), 2, out.ctypes.data) == -1
    assert L.rt_render_ss(None, None, 2, None) == -1
    assert L.rt_render_ss_async(None, None, 2, None, None, None) == -1


def test_backend_is_explicit(cpu):
    """The HIP supersampled calls refuse a CPU context."""
    L = rt_amd.lib()
    f = sample_frame(cpu, scene(1), 16, 16, 0)
    out = np.zeros((8, 8, 4), np.float32)
    assert L.rt_render_ss(cpu._h, ctypes.byref(f), 2, out.ctypes.data) == -4
    assert L.rt_render_ss_float(cpu._h, ctypes.byref(f), 2, out.ctypes.data) == -4
    assert L.rt_render_ss_async(cpu._h, ctypes.byref(f), 2, None, None, None) == -4
    assert b"rt_cpu_render" in L.rt_last_error(cpu._h)


def test_chunk_option_round_trips_on_a_cpu_context():
    """RT_OPT_SS_CHUNK_ROWS = 20 (rt.h; a macro beside ABI 8's option enum) is
    host state: it round-trips without a GPU and rejects bad values."""
    text = open(os.path.join(REPO, "include", "rt.h")).read()
    assert "#define RT_OPT_SS_CHUNK_ROWS 20" in text and "#define RT_HAS_SUPERSAMPLE 1" in text
    assert rt_amd.SS_OPTIONS == {"ss_chunk_rows": 20} and not set(rt_amd.SS_OPTIONS) & set(rt_amd.OPTIONS)
    L = rt_amd.lib()
    h = ctypes.c_void_p()
    assert L.rt_create_cpu(1, ctypes.byref(h)) == 0
    try:
        got = ctypes.c_double(-1)
        assert L.rt_get_option(h, 20, ctypes.byref(got)) == 0 and got.value == 0   # auto
        for v in (16, 40, 0):
            assert L.rt_set_option(h, 20, ctypes.c_double(v)) == 0
            assert L.rt_get_option(h, 20, ctypes.byref(got)) == 0 and got.value == v
        assert L.rt_set_option(h, 20, ctypes.c_double(-16)) == -1
        assert L.rt_set_option(h, 20, ctypes.c_double(7.5)) == -1
    finally:
        L.rt_destroy(h)


def read_ppm(path):
    head = open(path, "rb").read().split(b"\n", 3)
    assert head[0] == b"P6" and head[2] == b"255"
    w, h = map(int, head[1].split())
    return np.frombuffer(head[3], np.uint8).reshape(h, w, 3)


def test_cli_ssaa_cpu_backend(tmp_path, golden_images):
    out = tmp_path / "s7.ppm"
    r = subprocess.run([EXE, scene(7), "-x", "32", "-y", "24", "-d", "3", "--ssaa", "2", "--backend", "cpu",
                        "--threads", str(THREADS), "-o", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = rgba8(box(golden_images["scene7_64x48_d3"], 2))
    img = read_ppm(out)
    assert img.shape == (24, 32, 3)
    assert np.array_equal(img[::-1], want[..., :3])    # the PPM's top row first
    for extra in (["--ssaa", "2", "-g", "2"], ["--ssaa", "9"], ["--ssaa", "0"], ["--ssaa", "2", "--bands"]):
        bad = subprocess.run([EXE, scene(7), "-x", "32", "-y", "24"] + extra, capture_output=True, text=True,
                             timeout=60)
        assert bad.returncode == 1 and "[ERREUR]" in bad.stderr and "--ssaa" in bad.stderr, extra


def test_cscene_supersampling_verb(golden_images):
    c = rt_amd.CScene(backend="cpu", threads=THREADS)
    c.AjusterResolution(32, 24)
    c.AjusterNbRebondsMax(3)
    c.TraiterFichierDeScene(scene(7))
    c.AjusterSurEchantillonnage(2)
    want = box(golden_images["scene7_64x48_d3"], 2)
    img = c.LancerRayons()
    assert img.shape == (24, 32, 4) and np.array_equal(img, rgba8(want))
    assert bits_equal(c.LancerRayonsFloat(), want)
    c.AjusterSurEchantillonnage(1)
    c.AjusterResolution(64, 48)
    assert bits_equal(c.LancerRayonsFloat(), golden_images["scene7_64x48_d3"])
    with pytest.raises(ValueError):
        c.AjusterSurEchantillonnage(9)


def test_shared_resolve_under_asan_ubsan(tmp_path):
    """The shared resolve function (rt_resolve.h resolve_px, what both
    backends run) in a stand-alone host program built with AddressSanitizer
    and UBSan: a synthetic sample buffer allocated at its exact size, every
    factor, against sums the program computes itself."""
    exe = tmp_path / "resolve_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-fast-math", "-I", CSRC,
                    os.path.join(REPO, "tools", "ssaa", "resolve_check.cpp"), "-o", str(exe)], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "resolve_check: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
