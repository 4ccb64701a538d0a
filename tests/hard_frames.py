"""The oracle's view of the hard scenes (tests/hard_scenes.py), for
test_hard_scenes.py and test_gpu_hard_scenes.py: scene files, frames with
their bounce tree by depth, and primary-hit planes, each made once."""
from __future__ import annotations

import ctypes

import numpy as np

import aov_ref
import hard_scenes as hs

LEVELS = 16  # bounce levels counted apart (the deepest frame here has 9)


class Want:
    """The oracle's frame and its bounce tree by depth."""

    def __init__(self, img, rays, parents):
        self.img, self.rays, self.parents = img, rays, parents

    @property
    def deepest(self) -> int:
        """The deepest level with rays."""
        return int(np.nonzero(self.rays)[0].max())


class Frames:
    """Scene files, oracle frames (conftest.Oracle) and oracle AOVs, each made once."""

    def __init__(self, oracle, folder):
        self.o, self.dir, self.files, self.frames, self.aovs = oracle, folder, {}, {}, {}
        L = oracle.L
        L.oracle_level_counts.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        L.oracle_set_camera.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_float] * 4 + \
                                       [ctypes.c_int, ctypes.c_int]

    def text(self, name: str, text: str) -> str:
        """The file of a scene text."""
        if name not in self.files:
            self.files[name] = str(self.dir / f"{name}.dat")
            with open(self.files[name], "w") as f:
                f.write(text)
        return self.files[name]

    def path(self, family, seed, ntri=None, scale=1.0) -> str:
        name = hs.golden_key(family, seed, ntri, scale, 0, 0, 0)
        if name not in self.files:
            self.text(name, hs.hard_dat(family, seed, ntri, scale))
        return self.files[name]

    def want(self, path, w, h, depth, frame=None, rows=None) -> Want:
        """frame: an rt_frame whose camera replaces the file's; rows: a slab."""
        cam = None if frame is None else (tuple(frame.cam_pos), tuple(frame.orient), frame.half_w, frame.half_h)
        k = (path, w, h, depth, cam, rows)
        if k not in self.frames:
            L = self.o.L
            rc, p = self.o.load(path, w, h, depth)
            assert rc == 0, (path, rc, L.oracle_error(p))
            if frame is not None:
                pos, orient = np.array(frame.cam_pos[:], np.float32), np.array(frame.orient[:], np.float32)
                assert L.oracle_set_camera(p, pos.ctypes.data, orient.ctypes.data, frame.half_w, frame.half_h,
                                           frame.inv_w, frame.inv_h, w, h) == 0
            r0, r1 = rows or (0, h)
            img = np.zeros((r1 - r0, w, 3), np.float32)
            L.oracle_render_window(p, r0, r1, 0, w, img.ctypes.data, 8)
            rays, parents = np.zeros(LEVELS, np.uint64), np.zeros(LEVELS, np.uint64)
            assert L.oracle_level_counts(p, rays.ctypes.data, parents.ctypes.data, LEVELS) == 0
            L.oracle_free(p)
            self.frames[k] = Want(img, rays.astype(np.int64), parents.astype(np.int64))
        return self.frames[k]

    def aov(self, path, w, h) -> dict:
        """The primary-hit planes (aov_ref.oracle_aov) of the file's camera."""
        if (path, w, h) not in self.aovs:
            self.aovs[(path, w, h)] = aov_ref.oracle_aov(self.o, path, w, h)
        return self.aovs[(path, w, h)]
