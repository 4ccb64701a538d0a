// row_chunks_check.cpp — a stand-alone host program over the row-chunk
// function (csrc/rt_chunks.h row_chunk_step), for a sanitizer build:
//
//   g++ -std=c++17 -fsanitize=address,undefined -I ray-tracing-gpu_amd/csrc
//       tools/chunks/row_chunks_check.cpp -o row_chunks_check && ./row_chunks_check
//
// The table of tests/test_row_chunks.py, then a sweep of small widths, rows
// and options; every result's chunks are written into a heap array of exactly
// the 8 events a context holds (host chunks) and checked: they partition
// [0, rows), every chunk but the last starts and ends on a multiple of 16
// rows (16 s sample rows when supersampled), band sets and wavefronts are one
// chunk.  Prints "row_chunks_check: ok", exit 0; else exit 1.
#include <cstdio>
#include <memory>

#include "rt_chunks.h"

static long checked = 0;

// the chunks of one case; want: the expected step (0: only the properties)
static bool check(int width, int rows, int band_rows, int px_bytes, int ss, bool wf, bool host_out, double mb,
                  double ss_rows, int want)
{
    const int step = rt::row_chunk_step(width, rows, band_rows, px_bytes, ss, wf, host_out, mb, ss_rows);
    bool ok = step > 0 && step <= rows && (want == 0 || step == want);
    if (ok && (wf || band_rows != 0 || (ss == 1 && !host_out))) ok = step == rows;
    if (ok && step < rows) {
        ok = step % (16 * ss) == 0;
        const int n = (rows + step - 1) / step;
        if (ss == 1) {
            ok = ok && n <= 8;
            std::unique_ptr<int[]> ev(new int[8]);  // one slot per chunk event
            int covered = 0;
            for (int i = 0, r0 = 0; ok && r0 < rows; r0 += step, ++i) {
                ev[i] = std::min(rows, r0 + step) - r0;
                covered += ev[i];
            }
            ok = ok && covered == rows;
        }
    }
    if (!ok)
        std::printf("row_chunks_check: width %d rows %d band %d px %d ss %d wf %d host %d mb %g ss_rows %g: step %d\n", width,
                    rows, band_rows, px_bytes, ss, (int)wf, (int)host_out, mb, ss_rows, step);
    ++checked;
    return ok;
}

int main()
{
    bool ok = true;
    // host output, slab, 8 MiB chunks
    ok &= check(1920, 1080, 0, 4, 1, false, true, 8.0, 0.0, 1080);
    ok &= check(3840, 2160, 0, 4, 1, false, true, 8.0, 0.0, 720);
    ok &= check(3840, 2160, 0, 12, 1, false, true, 8.0, 0.0, 272);
    ok &= check(64, 100, 0, 12, 1, false, true, 64.0 * 100 * 12 / 8 / 1048576 / 1.01, 0.0, 16);
    // supersampling, slab, sample rows
    ok &= check(3840, 2160, 0, 12, 2, false, false, 8.0, 0.0, 2160);
    ok &= check(7680, 4320, 0, 12, 2, false, false, 8.0, 0.0, 2176);
    ok &= check(64, 48, 0, 12, 2, false, false, 8.0, 16.0, 32);
    ok &= check(64, 48, 0, 12, 2, false, false, 8.0, 17.0, 48);
    // one chunk: band sets, a supersampled wavefront, a device-pointer output
    ok &= check(3840, 2160, 16, 12, 1, false, true, 8.0, 0.0, 2160);
    ok &= check(7680, 4320, 32, 12, 2, false, false, 8.0, 16.0, 4320);
    ok &= check(7680, 4320, 0, 12, 2, true, false, 8.0, 16.0, 4320);
    ok &= check(3840, 2160, 0, 12, 1, false, false, 8.0, 0.0, 2160);
    // the sweep
    const double mbs[] = {0.0, 1e-9, 1e-5, 1e-4, 1e-3, 0.01, 8.0, 1e300};
    const double ssr[] = {0.0, 1.0, 15.0, 16.0, 17.0, 48.0, 1e9, 1e300};
    for (int width = 1; width <= 70; width += 23)
        for (int rows = 1; rows <= 400; rows += (rows < 70 ? 1 : 37))
            for (int band = 0; band <= 16; band += 16)
                for (int px = 4; px <= 12; px += 8)
                    for (int wf = 0; wf < 2; ++wf)
                        for (int host = 0; host < 2; ++host) {
                            for (double mb : mbs) ok &= check(width, rows, band, px, 1, wf, host, mb, 0.0, 0);
                            for (int ss = 2; ss <= 8; ++ss) {
                                if (rows % ss || width % ss) continue;
                                for (double r : ssr) ok &= check(width, rows, band, 12, ss, wf, false, 8.0, r, 0);
                            }
                        }
    if (!ok) return 1;
    std::printf("row_chunks_check: ok (%ld cases)\n", checked);
    return 0;
}
