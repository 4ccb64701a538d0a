"""Whole small frames of the wavefront test scenes (tests/wf_scenes.py) from
oracle/_ref, the reference's own code with the commented reflect/refract block
re-enabled (see make_golden.py): the refracting mesh's 2-child nodes, the
inside/out IOR flips, a deep reflection chain, and bounce rays onto a plane
and quadrics.  Run in the build container:

    make -C oracle ref && python tests/golden/make_wf_golden.py

Output: tests/golden/wf_small.npz (data only) — per frame of
wf_scenes.GOLDEN_FRAMES its float32 RGB (h, w, 3), bottom row first like
m_InfoPixel, under wf_{family}_{ntri}_{w}x{h}_d{depth}; per scene the SHA-256
of its .dat text under sha256_{family}_{ntri}, so a generator that drifts
fails before any pixel is compared.  The archive is written with fixed member
dates and in sorted order: the same inputs give the same bytes.

The reference harness has no setter for the energy floor, so frames with
another min_energy than the reference's 0.01 are not here."""
from __future__ import annotations

import io
import os
import sys
import tempfile
import time
import zipfile
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden  # noqa: E402  (puts the package on sys.path)
import wf_scenes  # noqa: E402

ROWS = 4  # rows per job


def render(job):
    path, w, h, d, r0 = job
    ref = make_golden.Ref(make_golden.load_ref(), path, w, h, d)
    return ref.window(r0, min(h, r0 + ROWS), 0, w)


def write_npz(path, arrays):
    """np.load-compatible, and the same bytes for the same arrays."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    t0 = time.time()
    out = {}
    with tempfile.TemporaryDirectory() as tmp, Pool(min(16, os.cpu_count() or 1)) as pool:
        for family, ntri, w, h, d in wf_scenes.GOLDEN_FRAMES:
            text = wf_scenes.wf_dat(family, ntri)
            path = os.path.join(tmp, f"{family}_{ntri}.dat")
            with open(path, "w") as f:
                f.write(text)
            out[wf_scenes.sha_key(family, ntri)] = np.array(wf_scenes.text_sha(text))
            parts = pool.map(render, [(path, w, h, d, r0) for r0 in range(0, h, ROWS)], chunksize=1)
            out[wf_scenes.golden_key(family, ntri, w, h, d)] = np.concatenate(parts, 0)
            print(family, ntri, d, f"{time.time() - t0:.1f} s", flush=True)
    write_npz(os.path.join(HERE, "wf_small.npz"), out)
    print(f"wrote {len(out)} arrays in {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()
