"""The expected image of a supersampled render (include/rt.h rt_render_ss*),
in numpy from a REFERENCE image of the sample grid — a committed oracle/_ref
fixture or liboracle.so, never the code under test: per channel the
sequential float32 sum over the s x s samples (sample row j outer, bottom row
first; i inner), starting as the first sample, then one float32 division."""
from __future__ import annotations

import numpy as np


def box(a: np.ndarray, s: int) -> np.ndarray:
    a = np.ascontiguousarray(a, np.float32)
    assert a.shape[0] % s == 0 and a.shape[1] % s == 0
    acc = None
    for j in range(s):
        for i in range(s):
            t = a[j::s, i::s]
            acc = t.copy() if acc is None else acc + t
    assert acc.dtype == np.float32
    return acc / np.float32(s * s)
