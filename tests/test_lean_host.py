"""The lean tile record's host helpers (csrc/rt_tile.h) in a stand-alone
program built with AddressSanitizer and UBSan (no GPU)."""
from __future__ import annotations

import os
import subprocess

from conftest import REPO


def test_lean_record_helpers_under_asan_ubsan(tmp_path):
    """lean_pack / lean_unpack round trips of every field, the lean rule
    against its plain restatement, the launch record's lights by value for 0
    to past kTinyClassLights lights, the size asserts: what
    tools/lean/lean_check.cpp writes out."""
    exe = tmp_path / "lean_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I", os.path.join(REPO, "ray-tracing-gpu_amd", "csrc"),
                    os.path.join(REPO, "tools", "lean", "lean_check.cpp"), "-o", str(exe)],
                   check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "lean_check: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
