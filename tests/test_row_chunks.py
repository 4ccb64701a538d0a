"""The row chunks a render enqueues (csrc/rt_chunks.h row_chunk_step, through
rt_debug_row_chunks: no device).  A frame that renders correctly in another
number of chunks would pass every image test, so the numbers are pinned here:
the values below follow by hand from the chunk formulas (a chunk per
RT_OPT_HOST_CHUNK_MB of host output, at most 8, multiples of 16 rows; the
fewest supersampling chunks of at most 224 MiB of samples, multiples of 16 s
sample rows)."""
from __future__ import annotations

import ctypes

import pytest

import rt_amd

MB = 8.0  # RT_OPT_HOST_CHUNK_MB's default
TINY_MB = 64 * 100 * 12 / 8 / 1048576 / 1.01


def chunks(width, rows, *, band_rows=0, px_bytes=12, ss=1, wf=False, host_out=False, host_chunk_mb=MB,
           ss_chunk_rows=0.0):
    L = rt_amd.lib()
    L.rt_debug_row_chunks.argtypes = [ctypes.c_int] * 7 + [ctypes.c_double] * 2 + [ctypes.c_void_p, ctypes.c_int]
    L.rt_debug_row_chunks.restype = ctypes.c_int
    bounds = (ctypes.c_int * 64)()
    n = L.rt_debug_row_chunks(width, rows, band_rows, px_bytes, ss, int(wf), int(host_out), host_chunk_mb,
                              ss_chunk_rows, bounds, 64)
    assert n >= 1, n
    return list(bounds[: n + 1])


def sizes(bounds):
    return [b - a for a, b in zip(bounds, bounds[1:])]


CASES = [
    # host output, slab, 8 MiB chunks
    ("1080p rgba8", dict(width=1920, rows=1080, px_bytes=4, host_out=True), [1080]),
    ("4k rgba8", dict(width=3840, rows=2160, px_bytes=4, host_out=True), [720, 720, 720]),
    ("4k float", dict(width=3840, rows=2160, px_bytes=12, host_out=True), [272] * 7 + [256]),
    ("64x100 float", dict(width=64, rows=100, px_bytes=12, host_out=True, host_chunk_mb=TINY_MB), [16] * 6 + [4]),
    # supersampling, slab, sample rows
    ("ss 4k auto", dict(width=3840, rows=2160, ss=2), [2160]),
    ("ss 8k auto", dict(width=7680, rows=4320, ss=2), [2176, 2144]),
    ("ss 16 rows", dict(width=64, rows=48, ss=2, ss_chunk_rows=16.0), [32, 16]),
    ("ss 17 rows", dict(width=64, rows=48, ss=2, ss_chunk_rows=17.0), [48]),
    # one chunk
    ("band host", dict(width=3840, rows=2160, band_rows=16, px_bytes=12, host_out=True), [2160]),
    ("band ss", dict(width=7680, rows=4320, band_rows=16, ss=2, ss_chunk_rows=16.0), [4320]),
    ("wavefront ss", dict(width=7680, rows=4320, ss=2, wf=True, ss_chunk_rows=16.0), [4320]),
    ("device pointer", dict(width=3840, rows=2160, px_bytes=12, host_out=False), [2160]),
]


@pytest.mark.parametrize("name,kw,want", CASES, ids=[c[0] for c in CASES])
def test_row_chunks(name, kw, want):
    b = chunks(**kw)
    assert sizes(b) == want
    # the chunks partition [0, rows)
    assert b[0] == 0 and b[-1] == kw["rows"] and all(x < y for x, y in zip(b, b[1:]))
    s = kw.get("ss", 1)
    if kw.get("host_out"):
        assert len(b) - 1 <= 8  # one event per host chunk
    # every chunk but the last starts and ends on a multiple of 16 (s) rows
    assert all(x % (16 * s) == 0 for x in b[:-1])
