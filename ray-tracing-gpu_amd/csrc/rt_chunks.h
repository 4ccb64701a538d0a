// rt_chunks.h — the row chunks of a frame (rt_kernels.hip launch).  Plain host
// C++ with no HIP in it: the library, rt_debug_row_chunks and
// tools/chunks/row_chunks_check.cpp compile the same function.
#ifndef RT_AMD_RT_CHUNKS_H
#define RT_AMD_RT_CHUNKS_H

#include <algorithm>
#include <cmath>
#include <cstddef>

namespace rt {

// Rows per chunk of a frame of `rows` packed rows (sample rows when ss > 1);
// `rows` itself: one chunk.  A band set (band_rows != 0) and a wavefront
// frame (wf) are always one chunk.
//
// Supersampled slabs (ss > 1): sample rows per chunk — ss_chunk_rows
// (RT_OPT_SS_CHUNK_ROWS) output rows, a multiple of 16, times ss; so every
// chunk starts on a multiple of 16 ss sample rows of the slab: the 8-row
// tiles of the camera buffer stay aligned.  Auto (0): the fewest equal chunks
// whose float samples stay within 224 MiB each — under the 256 MiB Infinity
// Cache, so the resolve still finds them there.  Measured
// (tools/ssaa_probe.py): every chunk more costs 12 us (C2) to
// 50 us (C3) of drained GPU at 3840 x 2160 samples, where one chunk (95 MiB)
// is fastest; at 7680 x 4320 (380 MiB) two chunks beat one by 1.4% and four
// lose 2.4%.
//
// Synchronous renders into host memory (host_out): a big slab goes in up to 8
// row chunks (multiples of 16 rows), chunk i's copy overlapping chunk i + 1's
// kernel (the same pixels: every pixel is independent, and the chunks keep
// the unchunked launch's 8-row wave rows).  A chunk per host_chunk_mb
// (RT_OPT_HOST_CHUNK_MB, 8 MiB) of the px_bytes-per-pixel output: each copy
// has a fixed cost of tens of us: a 1080p RGBA8 frame is one copy, 4K four
// chunks -10%, 7680 x 4320 eight chunks -30% (tools/host_chunks.py).
inline int row_chunk_step(int width, int rows, int band_rows, int px_bytes, int ss, bool wf, bool host_out,
                          double host_chunk_mb, double ss_chunk_rows)
{
    if (rows <= 0 || wf || band_rows != 0) return rows;
    if (ss > 1) {
        const double row_bytes = (double)width * 12.0;
        double ch = ss_chunk_rows;
        if (ch == 0) {
            const double n = std::ceil(row_bytes * rows / (224.0 * 1048576.0));
            if (n <= 1) return rows;
            ch = std::ceil((double)(rows / ss) / n);
        }
        ch = std::max(16.0, std::ceil(ch / 16.0) * 16.0);
        return (int)std::min((double)rows, ch * ss);
    }
    const double chunk = host_chunk_mb * 1048576.0;
    if (!host_out || !(chunk > 0)) return rows;
    const size_t out_bytes = (size_t)rows * (size_t)width * (size_t)px_bytes;
    const int nch = (int)std::min(8.0, std::floor((double)out_bytes / chunk));
    if (nch <= 1) return rows;
    return std::min(rows, ((rows + nch - 1) / nch + 15) / 16 * 16);
}

}  // namespace rt
#endif  // RT_AMD_RT_CHUNKS_H
