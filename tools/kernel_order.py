#!/usr/bin/env python
"""Do the kernels of one build of librt_amd.so keep their place in another's?

    python tools/kernel_order.py OLD/librt_amd.so NEW/librt_amd.so [--new-prefix rt_refine_kernel,rt_edge_]

Takes the gfx950 code object out of each library (objcopy of .hip_fatbin, then
clang-offload-bundler), lists its kernels by address (llvm-readelf) and checks
that every kernel of OLD is in NEW with the same size and in the same order,
and that the kernels NEW adds all lie behind the last kernel of OLD.  DESIGN.md
records why the order matters; a change that adds kernels runs this on its
build and its parent's and commits the JSON line.  No GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/lib/llvm/bin")


def kernels(lib: str):
    """[(address, size, mangled name)] of the gfx950 code object, by address."""
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "co.o")
        subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
        text = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", co], check=True, capture_output=True,
                              text=True).stdout
    seen, out = set(), []
    for line in text.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC" and not f[7].endswith(".kd") and f[7] not in seen:
            seen.add(f[7])
            out.append((int(f[1], 16), int(f[2]), f[7]))
    return sorted(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    args = ap.parse_args()
    old, new = kernels(args.old), kernels(args.new)
    old_names = {k[2] for k in old}
    kept = [k for k in new if k[2] in old_names]
    added = [k for k in new if k[2] not in old_names]
    same_order = [k[2] for k in kept] == [k[2] for k in old]
    same_sizes = [(k[1], k[2]) for k in kept] == [(k[1], k[2]) for k in old]
    behind = bool(kept) and all(k[0] > kept[-1][0] for k in added)
    stems = sorted({re.sub(r"^_ZN2rt\d+", "", k[2]).split("I")[0] for k in added})
    print(json.dumps({"old_kernels": len(old), "new_kernels": len(new), "added": len(added), "added_stems": stems,
                      "old_kernels_same_order": same_order, "old_kernels_same_sizes": same_sizes,
                      "added_all_behind_the_last_old_kernel": behind,
                      "text_start_old": hex(old[0][0]), "text_start_new": hex(new[0][0])}))
    return 0 if same_order and same_sizes and behind else 1


if __name__ == "__main__":
    sys.exit(main())
