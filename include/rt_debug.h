/*
 * rt_debug.h — diagnostic exports of librt_amd.so (not part of the drop-in
 * boundary, include/rt.h).
 *
 * The reference has no counterpart: these read back what the acceleration
 * structures cost (bench.py reports them beside the headline number) and
 * self-test the wave primitives the culling relies on.  They never change an
 * image and no product path depends on them; the ABI version of rt.h does not
 * cover them.  Every function returns 0 or a negative RT_E_* code (rt.h).
 */
#ifndef RT_AMD_RT_DEBUG_H
#define RT_AMD_RT_DEBUG_H

#include "rt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Light buffer of the uploaded scene: out[0] built (0/1), out[1] entries,
 * out[2] build ms; then per light j (while 3 + 3j + 2 < n): cells per face
 * edge, uncullable-pair list length, coverage distance dcov. */
int rt_debug_lb_info(rt_ctx*, double* out, int n);

/* Camera buffer of the last build: out[0] current (0/1), out[1] entries,
 * out[2] device ms of the last synchronous build's kernels, out[3] tiles, out[4] inline
 * records (0/1), out[5] host wall ms of the build's enqueue; out[6..9]
 * binning counters: candidate (triangle, tile) pairs tested, lists longer
 * than 256, the longest of them, the entry capacity; out[10] 1 when the
 * candidate pairs passed 2^32 - 1 (no pair tested, every tile flagged to the
 * per-wave path). */
int rt_debug_cb_info(rt_ctx*, double* out, int n);

/* The current camera buffer checked against brute force (every tile with
 * a list against every triangle; synchronous): out[0] tiles whose list is
 * not exactly the triangles passing the camera wave test (or mis-keyed),
 * out[1] passing pairs, out[2] tiles with a list. */
int rt_debug_cb_verify(rt_ctx*, unsigned long long* out3);

/* The last rt_upload_scene's host wall time by part (ms): out[0] records +
 * device copies, out[1] cone / cluster prepasses, out[2] light buffer,
 * out[3] total, out[4..8] the light-buffer build's phases, out[9] (n >= 10) light
 * 0's first light buffer's resolution R (6 R^2 cells; 0 without one). */
int rt_debug_upload_info(rt_ctx*, double* out, int n);

/* The builds' device prefix sum on host counts (n >= 1), in place like its
 * callers: out (n + 1 words) = the exclusive prefixes then the total, both
 * mod 2^32; *total = the 64-bit total. */
int rt_debug_scan(int device, const unsigned* in, unsigned n, unsigned* out, unsigned long long* total);

/* ABI 7: the bounce-ray BVH of the uploaded scene (rt_bvh.h): out[0] built
 * (0/1), out[1] inner nodes, out[2] leaves, out[3] depth (deepest leaf's
 * inner-node path), out[4] host build ms. */
int rt_debug_bvh_info(rt_ctx*, double* out, int n);

/* The last wavefront frame's queue counts (round 6; synchronous): per level
 * L = 0 .. 8, out[3 L] its rays (L >= 1), out[3 L + 1] its parents (nodes
 * that spawned children), out[3 L + 2] its walks finished by the straggler
 * launch.  RT_E_STATE before any wavefront frame. */
int rt_debug_wf_counts(rt_ctx*, unsigned* out, int n);

/* The host BVH build alone, no device (round 6): n triangles of 12 floats
 * (p0, e1, e2, normal); out3 = {depth, inner nodes, leaves}.  The depth is
 * at most 24 (the walk's stack) for every input; RT_E_UNSUPPORTED above
 * 4 x 2^24 triangles (bounce rays then test every triangle). */
int rt_debug_bvh_build(const float* tri12, long long n, int* out3);

/* Bounce-ray closest hits of n arbitrary rays (rays: O.xyz D.xyz per ray),
 * each through the BVH and through every triangle (planes and quadrics
 * too, both ways; synchronous): out_idx / out_t (2 per ray) = [BVH, brute
 * force] winners (file index or -1, t); tally2 = the BVH walk's triangle
 * tests and inner nodes visited, summed.  RT_E_STATE without a BVH. */
int rt_debug_bvh_rays(rt_ctx*, const float* rays, int n, int* out_idx, float* out_t, unsigned long long* tally2);

/* The same rays walked by the wavefront's straggler path — the budgeted
 * serial walk stopped after one step, then the wave-cooperative walk (one
 * wave per ray, a shared LDS stack) — winners into out_idx / out_t (one per
 * ray); compare with rt_debug_bvh_rays' brute force.  RT_E_STATE without a
 * BVH. */
int rt_debug_bvh_rays_wave(rt_ctx*, const float* rays, int n, int* out_idx, float* out_t);

/* Run the wave-primitive self-test (wave min / max / sum, wave cones) over
 * `blocks` workgroups on `device`; *failures = lanes that disagreed. */
int rt_debug_selftest(int device, int blocks, unsigned* failures);

/* The supersampling resolve alone (csrc/rt_resolve.h, tools/ssaa_probe.py):
 * rows_out rows of width / s pixels from the s rows_out x width float RGB
 * samples at samples_dev, enqueued on hip_stream; device pointers, either
 * output may be NULL; s in 2..8 dividing width. */
int rt_debug_resolve(rt_ctx*, const float* samples_dev, int width, int s, int rows_out, float* rgb_dev,
                     unsigned* rgba_dev, void* hip_stream);

/* The phases of the last synchronous rt_render_adaptive on the context
 * (tools/adaptive_probe.py): ms3[0] the base frame and its AOV pass, ms3[1]
 * classify + scan + scatter, ms3[2] the refine kernel (hipEvents on the
 * call's stream); *flagged the flagged output pixels.  Either may be NULL. */
int rt_debug_adaptive_phases(rt_ctx*, float* ms3, unsigned long long* flagged);

/* The launch-camera light records' occupied-direction bounds (RT_OPT_LB_REGION;
 * synchronous): per light j (while 6 j + 5 < n) out[6 j ..] = [a.x, a.y, a.z,
 * cosB, cells of the light's first buffer that hold an entry, violations].  A
 * violation is such a cell whose cone (the directions the lookup can map to
 * it) is not inside the stored float cone [a, cosB] with the test's rounding
 * allowance, counted by one device thread per cell; cosB = -2: the light
 * always looks, 2: never.  RT_E_STATE where the uploaded scene has no such
 * records (not a launch-camera scene). */
int rt_debug_lb_region(rt_ctx*, double* out, int n);

/* Light `light`'s first light buffer's cell offsets read back (synchronous):
 * n = 6 R^2 + 1 words (R: rt_debug_lb_info), cell c's entries are
 * [out[c], out[c + 1]).  RT_E_STATE without a light buffer. */
int rt_debug_lb_offsets(rt_ctx*, int light, unsigned* out, int n);

/* That bound's host builder alone, no device: off = one buffer's cell offsets
 * (6 R^2 + 1 rising words; cell c holds an entry when off[c + 1] > off[c];
 * c = (face R + j) R + i); out5 = [a.x, a.y, a.z, cosB, cells that hold an
 * entry]. */
int rt_debug_lb_region_build(const unsigned* off, int R, double* out5);

/* The row chunks a render enqueues, no device: a frame of `rows` packed rows
 * (sample rows when ss > 1) of `width` pixels, px_bytes of output per pixel;
 * wf: it renders as a wavefront; host_out: a synchronous render into host
 * memory; the options RT_OPT_HOST_CHUNK_MB and RT_OPT_SS_CHUNK_ROWS.  Writes
 * the n + 1 boundaries bounds[0] = 0 < ... < bounds[n] = rows (cap: the
 * array's length) and returns n, or RT_E_ARG. */
int rt_debug_row_chunks(int width, int rows, int band_rows, int px_bytes, int ss, int wf, int host_out,
                        double host_chunk_mb, double ss_chunk_rows, int* bounds, int cap);

/* The tile words a tiny-scene (launch-camera) render stored for hip_stream
 * (NULL: the synchronous renders' stream) read back (synchronous): the first
 * n words, tile = tile_row * ceil(width / 8) + tile_col over the full frame's
 * 8 x 8 tiles.  Bits 0-19: the tile's triangle mask; bits 20 + 2 l and
 * 21 + 2 l: light l's class for l < 6 (0 run the light's shadow pass, 1 lit,
 * 2 dark).  RT_E_STATE where the stream holds no stored words of n tiles. */
int rt_debug_tiny_words(rt_ctx*, void* hip_stream, unsigned* out, int n);

/* The second word stored beside each of those, the tile facts (0: nothing
 * known).  Bits 0-2: how the tile's one surface is found (1 launch-record
 * plane slot, 2 kept triangle, 3 by the full search, 4 every lane missed);
 * bits 3-7: that slot or triangle position; bits 8 + 2 l and 9 + 2 l, l < 6:
 * light l's pass changed no lane's colour / every shaded lane faces light l;
 * bits 20-31: the surface's file index + 1 (0 unknown).  Same arguments and
 * errors as rt_debug_tiny_words. */
int rt_debug_tiny_facts(rt_ctx*, void* hip_stream, unsigned* out, int n);

/* The lean records stored beside them, 16 dwords per tile into
 * out[16 * n_tiles]: [0] the word, [1] the facts — on a lean tile with kind 5
 * (for 1, a plane slot) or 6 (for 2, a kept triangle) —, then as floats
 * [2-4] the plane slot's normal and [5] its n . camera + cst (a plane tile),
 * [6-8] the hit normal, [9-11] the colour, [12-15] Ka Kd Ks shininess; zeros
 * from [2] on where the tile is not lean.  Same errors as rt_debug_tiny_words. */
int rt_debug_tiny_lean(rt_ctx*, void* hip_stream, unsigned* out, int n_tiles);

#ifdef RT_PROF
/* Only in a library built with -DRT_PROF (tools/prof_sections.py,
 * tools/prof_tiles.py): per-section shader-clock totals and event counts
 * of the last renders (read and clear), and a per-tile record buffer. */
int rt_debug_prof(unsigned long long* out8);
int rt_debug_prof_events(unsigned long long* out8);
int rt_debug_prof_tiles(unsigned* dev, int ntiles);
#endif

#ifdef __cplusplus
}
#endif
#endif /* RT_AMD_RT_DEBUG_H */
