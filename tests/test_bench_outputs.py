"""bench.py's plain run and --dump-outputs: the plain line carries the headline
figure and none of the --full legs, and the dumped frame is the last timed
step's RGBA8 frame — for scene2 the reference's digest — the same from run
to run."""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

FULL_ONLY = ("roofline", "hbm", "rays_per_frame", "frame_ms", "host_boundary", "frame_costs", "cpu_baseline",
             "cpu_baseline_allcores", "light_buffer", "camera_buffer")


def test_dump_writes_small_frames_whole(tmp_path):
    torch = pytest.importorskip("torch")
    import bench

    px = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (33, 47, 4), dtype=np.uint8))
    bench.dump_outputs(str(tmp_path / "d"), px)
    assert os.listdir(tmp_path / "d") == ["frame_rgba8.npy"]
    got = np.load(tmp_path / "d" / "frame_rgba8.npy")
    assert got.dtype == np.float32 and np.array_equal(got, px.numpy().astype(np.float32))


def test_dump_samples_big_frames_the_same_way_every_time(tmp_path):
    torch = pytest.importorskip("torch")
    import bench

    h, w = 1501, 2003  # 3.0 Mpx: 48.1 MB as float32, just over the whole-frame limit
    assert h * w * 16 > bench.DUMP_FULL_BYTES
    px = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (h, w, 4), dtype=np.uint8))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), px)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["frame_rgba8.npy", "frame_rgba8_pixels.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64_000_000
    val, idx = (np.load(tmp_path / "a" / f) for f in files)
    assert val.dtype == np.float32 and idx.dtype == np.float64
    assert val.shape == (bench.DUMP_SAMPLE_PIXELS, 4) and idx.shape == (bench.DUMP_SAMPLE_PIXELS,)
    assert (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < h * w
    assert np.array_equal(val, px.numpy().reshape(-1, 4)[idx.astype(np.int64)].astype(np.float32))
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_reference_frame(tmp_path, digests):
    out = tmp_path / "dump"
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--settle-ms", "0",
                        "--frame-sha", "--dump-outputs", str(out)], cwd=REPO, capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "Mray/s" and d["dtype"] == "f32"
    assert d["higher_is_better"] is True and d["full"] is False
    assert d["ms_per_step"] > 0
    # value and ms_per_step are the same measurement, pixels per timed step:
    # they differ by ms_per_step's rounding to 1e-4 ms (value's to 1e-3 is far below it)
    assert d["value"] == pytest.approx(1920 * 1080 / d["ms_per_step"] / 1e3, rel=5e-5 / d["ms_per_step"] + 1e-6)
    assert not [k for k in FULL_ONLY if k in d]
    frame = np.load(out / "frame_rgba8.npy")
    assert frame.dtype == np.float32 and frame.shape == (1080, 1920, 4)
    sha = hashlib.sha256(frame.astype(np.uint8).tobytes()).hexdigest()
    # scene2 has no reflective/refractive surface: depth 3 renders the depth-0 image
    assert sha == d["frame_rgba8_sha256"] == digests["scene2_1920x1080_d0_rgba8_sha256"]
