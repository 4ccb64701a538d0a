"""Whole small frames of the hard scenes (tests/hard_scenes.py) from
oracle/_ref, the reference's own code (see make_golden.py): coincident
surfaces, the launch-camera kernels' stress geometry, odd quadrics, materials
that both reflect and refract, and scenes scaled by powers of two.  Run in the
build container:

    make -C oracle ref && python tests/golden/make_hard_golden.py

Output: tests/golden/hard.npz (data only) — per frame of
hard_scenes.GOLDEN_FRAMES its float32 RGB (h, w, 3), bottom row first like
m_InfoPixel, under hard_scenes.golden_key(...), and the SHA-256 of its .dat
text under "sha256_" + that key, so a generator that drifts fails before any
pixel is compared.  The archive is written with fixed member dates and in
sorted order: the same inputs give the same bytes."""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import hard_scenes  # noqa: E402
from make_golden import Ref, load_ref  # noqa: E402
from make_wf_golden import write_npz  # noqa: E402


def main():
    L = load_ref()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for case in hard_scenes.GOLDEN_FRAMES:
            family, seed, ntri, scale, w, h, d = case
            key = hard_scenes.golden_key(*case)
            text = hard_scenes.hard_dat(family, seed, ntri, scale)
            path = os.path.join(tmp, key + ".dat")
            with open(path, "w") as f:
                f.write(text)
            out["sha256_" + key] = np.array(hard_scenes.text_sha(text))
            out[key] = Ref(L, path, w, h, d).window(0, h, 0, w)
            print(key, flush=True)
    assert len(out) == 2 * len(hard_scenes.GOLDEN_FRAMES), "two frames share a key"
    write_npz(os.path.join(HERE, "hard.npz"), out)
    print("wrote", len(hard_scenes.GOLDEN_FRAMES), "frames")


if __name__ == "__main__":
    main()
