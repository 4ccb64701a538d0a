// rt_kernels.hip — the hot path on gfx950 (MI355X) and the device half of the
// C ABI (include/rt.h).
//
// What runs here replaces, per pixel, the reference's CPU loop
// (Scene.cpp:1538-1561) -> ObtenirCouleur (:1705) -> ObtenirCouleurSurIntersection
// (:1740, plus the commented reflect/refract block :1779-1823 when
// max_bounces > 0) -> ObtenirFiltreDeSurface (:1842), and the primitive tests
// CTriangle/CPlan/CQuadrique::Intersection (Triangle.cpp:127, Plan.cpp:128,
// Quadrique.cpp:160).  It is NOT a translation of shaders/rayTracing.glsl.
//
// Execution model:
//  * one wave64 = one 8x8 pixel tile, lane l -> (l&7, l>>3); one wave per
//    workgroup;
//  * the surface list is walked in FILE ORDER by every lane of the wave in
//    lockstep, so the surface index, its type switch and its 64-byte record are
//    wave-uniform: records arrive through the scalar data cache (s_load) into
//    SGPRs and feed the VALU directly — no per-lane gather, no LDS round trip;
//  * closest hit keeps (t, index) only; the hit normal is rebuilt once for the
//    winner (bit-identical: same expressions, same inputs);
//  * shadow rays multiply the transmittance filter in file order and leave the
//    surface loop as soon as every active lane's filter is exactly +0 (only
//    when the host proved all filter factors are non-negative and finite, so
//    the skipped factors could not have changed a single bit);
//  * bounces (depth > 0) run as an explicit per-lane DFS with a compile-time
//    sized frame stack instead of recursion, folding each node's colour
//    bottom-up in the reference's order: ((local + C_refl*Kr) + C_refr*Kt);
//  * no FMA contraction, IEEE f32 division and sqrt.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cassert>
#include <chrono>
#include <cstdlib>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rt.h"
#include "../../include/rt_debug.h"
#include "rt_chunks.h"
#include "rt_cpu.hpp"
#include "rt_scan.h"
#include "rt_shade.h"
#include "rt_bvh.h"
#include "rt_rays.h"
#include "rt_filter.h"
#include "rt_wavefront.h"
#include "rt_resolve.h"
#include "rt_scenehost.h"  // scene_host_build, lb_plan; RT_BVH_MIN_TRIANGLES

#pragma clang fp contract(off)

namespace rt {

// One pixel's colour.  MAXD = compile-time bounce-stack capacity (0 = no
// bounces: the reference as shipped).
// A pushed node: its colour so far, its surface, and which child runs:
// 0 reflected (no refraction to follow), 2 reflected (the refracted ray is
// waiting in Refr), 1 refracted.  5 dwords; the 8-dword Refr is written only
// by nodes that spawn both children.
struct Frame {
    Color acc;
    int surf, stage;
};
struct Refr {
    Vec3 P, D;
    float rior, energy;
};

// kWf0 (MAXD 0, the wavefront's level 0, rt_wavefront.h): a hit
// that spawns children writes a node record and its child rays instead of
// its colour (deferred: rt_wf_fold writes the pixel).
// kRayQuery (rt_shaderays.h): O, D are the caller's, not a camera ray's —
// the first search is a bounce ray's (tile is unused); nothing else differs.
template <int MAXD, int LB, int WAVE>
__device__ Color radiance(const SceneDev& S, const FrameDev& F, Vec3 O, Vec3 D, Counters& cnt, bool live, int tile,
                          unsigned pix, bool& deferred, unsigned chunk)
{
    const Color bg{F.bg[0], F.bg[1], F.bg[2]};
    if constexpr (MAXD == 0) {
        float t;
        RT_MARK(cnt, 0);
        int idx;
        if constexpr (!is_ray_query(WAVE))
            idx = closest_hit_primary<camera_ray_bits(WAVE)>(S, O, D, t, cnt, tile);
        else if constexpr (has_bvh(WAVE))  // kRayQuery: the caller's ray, searched like a bounce ray
            idx = closest_hit_bvh(S, O, D, t, cnt);
        else
            idx = closest_hit<false>(S, O, D, t, cnt);
        RT_MARK(cnt, 1);
        // Lanes that miss (or lie outside the frame) stay in step through the
        // shading so the wave stays whole for wave-level shadow culling.
        const bool hit = idx >= 0;
        if (!__any(hit & live)) return bg;
        const int sidx = hit ? idx : 0;
        // A tile usually sees one surface: then its normal and material
        // records come by scalar (broadcast) loads instead of a per-lane gather.
        const int s0 = __builtin_amdgcn_readfirstlane(sidx);
        Vec3 N;
        Mat m;
        if (__all(sidx == s0)) {
            N = hit_normal(S, s0, O, D, t);
            m = load_mat(S, s0);
        } else {
            N = hit_normal(S, sidx, O, D, t);
            m = load_mat(S, sidx);
        }
        const Vec3 P = O + t * D;
        const Color c = shade_local<LB, WAVE>(S, m, P, N, D, cnt, hit & live);
        if constexpr (is_wf0(WAVE))
            deferred = wf_children(F, 0, hit & live, m, P, N, D, 1.0f, 1.0f, c, pix, chunk, sidx);
        return hit ? c : bg;
    } else if constexpr (is_chain(WAVE)) {
        // Reflect-only scenes (no Kt can pass the gate: the host's kt_max <= 0
        // with min_energy >= 0): every node has at most one child, the
        // reflected ray, and its colour is acc + C_child * Kr (Scene.cpp:1787).
        // The chain's (acc, Kr) pairs live in registers — a shift stack with
        // compile-time indices, top at [0] — instead of the DFS's scratch
        // frames; the fold runs bottom-up in the same order.
        Color accs[MAXD];
        float krs[MAXD];
#pragma unroll
        for (int k = 0; k < MAXD; ++k) {
            accs[k] = Color{0.f, 0.f, 0.f};
            krs[k] = 0.f;
        }
        int d = 0;  // nodes on the chain (pushed)
        float energy = 1.0f;
        Color ret = bg;
        for (int lv = 0;; ++lv) {
            float t;
            int idx;
            if (!is_ray_query(WAVE) && lv == 0)
                idx = closest_hit_primary<camera_ray_bits(WAVE)>(S, O, D, t, cnt, tile);
            else if constexpr (has_bvh(WAVE))  // bounce rays through the BVH (rt_bvh.h)
                idx = closest_hit_bvh(S, O, D, t, cnt);
            else
                idx = closest_hit<false>(S, O, D, t, cnt);
            ret = bg;
            if (idx < 0) break;
            const Vec3 N = hit_normal(S, idx, O, D, t);
            const Mat m = load_mat(S, idx);
            const Vec3 P = O + t * D;
            const Color acc = shade_local<LB, WAVE>(S, m, P, N, D, cnt);
            // Scene.cpp:1779-1781 gate; bounces == lv
            const float er = m.kr * energy;
            const bool doR = er > F.min_energy && lv < F.max_bounces && lv < MAXD;
            if (!doR) {
                ret = acc;
                break;
            }
#pragma unroll
            for (int k = MAXD - 1; k > 0; --k) {
                accs[k] = accs[k - 1];
                krs[k] = krs[k - 1];
            }
            accs[0] = acc;
            krs[0] = m.kr;
            ++d;
            ++cnt.bounce;
            O = P;
            D = reflect(D, N);  // Scene.cpp:1782-1788
            energy = er;
        }
#pragma unroll
        for (int k = 0; k < MAXD; ++k) {
            if (k < d) {
                Color a = accs[k];
                a += ret * krs[k];  // Scene.cpp:1787
                ret = a;
            }
        }
        return ret;
    } else {
        Frame stk[MAXD];
        Refr rf[MAXD];
        int sp = 0;
        float rior = 1.0f, energy = 1.0f;
        Color ret{0.f, 0.f, 0.f};
        bool trace = true, camera_ray = !is_ray_query(WAVE);  // kRayQuery: no ray of the tree is a camera ray
        for (;;) {
            if (trace) {
                float t;
                int idx;
                if (camera_ray)
                    idx = closest_hit_primary<camera_ray_bits(WAVE)>(S, O, D, t, cnt, tile);
                else if constexpr (has_bvh(WAVE))  // bounce rays through the BVH (rt_bvh.h)
                    idx = closest_hit_bvh(S, O, D, t, cnt);
                else
                    idx = closest_hit<false>(S, O, D, t, cnt);
                camera_ray = false;
                ret = bg;
                if (idx >= 0) {
                    const Vec3 N = hit_normal(S, idx, O, D, t);
                    const Mat m = load_mat(S, idx);
                    const Vec3 P = O + t * D;
                    const Color acc = shade_local<LB, WAVE>(S, m, P, N, D, cnt);
                    // Scene.cpp:1779-1781 / :1790-1792 gates; bounces == sp
                    const float er = m.kr * energy;
                    const float et = m.kt * energy;
                    const bool can = sp < F.max_bounces && sp < MAXD;
                    const bool doR = er > F.min_energy && can;
                    const bool doT = et > F.min_energy && can;
                    if (doR || doT) {
                        Frame& fr = stk[sp];
                        fr.acc = acc;
                        fr.surf = idx;
                        ++cnt.bounce;
                        // The refracted ray (Scene.cpp:1793-1822), from this
                        // node's incoming ray — the same values whether it
                        // is traced now or after the reflected subtree.
                        Vec3 Dt = D;
                        float rior_t = rior;
                        if (doT) {
                            Vec3 n = N;
                            float ratio;
                            if (rior == m.ior) {  // Scene.cpp:1797-1803 inside -> out
                                rior_t = F.scene_ior;
                                ratio = m.ior / F.scene_ior;
                                n = -n;
                            } else {
                                rior_t = m.ior;
                                ratio = F.scene_ior / m.ior;
                            }
                            Dt = refract(D, n, ratio);
                        }
                        O = P;
                        if (doR) {  // Scene.cpp:1782-1788: IOR left at CRayon's default 0
                            fr.stage = doT ? 2 : 0;
                            if (doT) rf[sp] = Refr{P, Dt, rior_t, et};
                            D = reflect(D, N);
                            rior = 0.0f;
                            energy = er;
                        } else {
                            fr.stage = 1;
                            D = Dt;
                            rior = rior_t;
                            energy = et;
                        }
                        ++sp;
                        continue;
                    }
                    ret = acc;
                }
                trace = false;
            }
            if (sp == 0) return ret;
            Frame& fr = stk[sp - 1];
            const Mat m = load_mat(S, fr.surf);
            if (fr.stage != 1) {
                fr.acc += ret * m.kr;  // Scene.cpp:1787
                if (fr.stage == 2) {   // the refracted child (Scene.cpp:1790)
                    fr.stage = 1;
                    ++cnt.bounce;
                    const Refr r = rf[sp - 1];
                    O = r.P;
                    D = r.D;
                    rior = r.rior;
                    energy = r.energy;
                    trace = true;
                    continue;
                }
                ret = fr.acc;
                --sp;
            } else {
                fr.acc += ret * m.kt;  // Scene.cpp:1822
                ret = fr.acc;
                --sp;
            }
        }
    }
}

// Occupancy floor (waves per SIMD) for the depth-0 kernels: 7 (<= 72
// VGPRs, no spills) — C2 -4% against the unconstrained 5 waves, 6 waves
// +1-3% and 8 waves +40% (spills) at C2/C4.  The big-list kernels (is_big_list_cam:
// C3, C5) ran at 8 in round 1 (-3/-4% against 7) while spilling 9-10 VGPRs
// (44 B/lane of scratch: 1.4 GB of writes per C5 frame, tools/calib); with
// the LDS walks and an unpipelined global walk they fit 72 VGPRs with no
// scratch at 7 waves, as fast as 8 waves with spills (C3 -0.4%, C5 +0.5%)
// and 0.57 GB fewer bytes written per C5 frame.
#ifndef RT_WAVES_PER_EU
#define RT_WAVES_PER_EU 7
#endif
#ifndef RT_WAVES_PER_EU_BIG
#define RT_WAVES_PER_EU_BIG 7
#endif
// The launch-camera kernel that computes its tile masks (kMaskCompute) is
// held to 64 VGPRs, 8 waves/SIMD (A/B, moving C2 camera: -2.3% against 7;
// the mask-reading kernel fits 58 VGPRs anyway, and asked for 8 measured
// +2.4% static).  Its mask planes are loaded at the top of the kernel (A/B:
// -2.7% against loading them where the mask is computed).
#ifndef RT_WAVES_PER_EU_TINY
#define RT_WAVES_PER_EU_TINY 8
#endif
constexpr int waves_per_eu(int maxd, int wave)
{
    return maxd != 0 ? 1
                     : (computes_mask(wave) ? RT_WAVES_PER_EU_TINY
                                            : (is_big_list_cam(wave) ? RT_WAVES_PER_EU_BIG : RT_WAVES_PER_EU));
}
// One 8 x 8 tile (the body of both trace kernels below).
// COUNT: also tally the exact tests executed (the RT_FLAG_STATS launch); in
// the timed kernels the tallies are dead and compile away.
template <int MAXD, int LB, int WAVE, bool COUNT>
__device__ __forceinline__ void trace_tile(const SceneDev& S, const FrameDev& F, unsigned* __restrict__ rgba,
                                           float* __restrict__ rgbf, StatsDev* __restrict__ stats, int bx, int by)
{
    const int lane = threadIdx.x & 63;
    // XCD-aware block order: the dispatcher deals workgroups round-robin over
    // the 8 XCDs (each with its own L2), so workgroup w runs on XCD w % 8 as
    // that XCD's (w / 8)-th; give every XCD one contiguous run of blocks in
    // row-major order, so neighbouring tiles — which read the same cells,
    // tile lists and records — share an L2.  A bijection for any grid size.
    const int tile_x = bx;  // 8-pixel column of the wave's tile
    const int px = tile_x * 8 + (lane & 7);
    const int ly0 = by * 8;  // the wave's first output row
    const int ly = ly0 + (lane >> 3);
    // frame row of output row r: the slab, or band (r / band_rows) of this
    // rank's cyclic set (a wave's 8 rows never straddle a band: 16 | band_rows)
    int py0 = F.row_begin + ly0, rend = F.row_end;
    if (F.band_rows > 0) {
        py0 = ((ly0 / F.band_rows) * F.band_count + F.band_index) * F.band_rows + ly0 % F.band_rows;
        rend = F.height;
    }
    if (py0 >= rend) return;  // the whole wave lies past the frame (wave-uniform)
    const int py = py0 + (lane >> 3);
    const bool valid = px < F.width && py < rend;

    Counters cnt;
#ifdef RT_PROF
    cnt.last = __builtin_amdgcn_s_memtime();
#endif
    Color c{0.f, 0.f, 0.f};
    // Without bounces every lane runs (lanes outside the frame on a clamped
    // pixel, result dropped) so edge waves stay whole for wave-level culling.
    if (MAXD == 0 || valid) {
        const int pxc = px < F.width ? px : F.width - 1;
        const int pyc = py < rend ? py : rend - 1;
        const Vec3 D = camera_dir(F, pxc, pyc);
        const Vec3 O = make3(F.cam[0], F.cam[1], F.cam[2]);
        cnt.primary = valid ? 1u : 0u;
        // camera-buffer tile: this wave's 8 rows must be one tile row of the
        // full frame (the lists and boxes hold for its lanes' clamped pixels,
        // a superset of the wave's)
        int tile = -1;
        if (has_cam_buf(WAVE) && S.cb_tiles_x > 0 && (py0 & 7) == 0) {
            tile = (py0 >> 3) * S.cb_tiles_x + tile_x;
            if (S.cb_flag[tile]) tile = -1;
        }
        const size_t o = (size_t)ly * F.width + px;
        bool deferred = false;
        c = radiance<MAXD, LB, WAVE>(S, F, O, D, cnt, valid, tile, (unsigned)o, deferred,
                                     (unsigned)(by * F.tiles_x + bx));
        if (valid & !deferred) {
            if (rgbf) {
                rgbf[3 * o] = c.r;
                rgbf[3 * o + 1] = c.g;
                rgbf[3 * o + 2] = c.b;
            }
            // Nontemporal (streaming) stores in the small-list kernels: the
            // frame's lines leave each XCD's L2 during the kernel instead of
            // in the release at its end (A/B, same images: C2 -1 to -2%, C4
            // -2%, C1 +1%).  Not in the big-list kernels: at C5 they write
            // each 128-B line out twice (WRITE_SIZE 134 -> 268 MB per frame:
            // 32-B tile rows evicted before the neighbouring tiles fill the
            // line) for -0.5%.
            if (rgba) {
                const unsigned px8 = unorm8(c.r) | (unorm8(c.g) << 8) | (unorm8(c.b) << 16) | 0xFF000000u;
                if constexpr (!is_clustered(WAVE)) __builtin_nontemporal_store(px8, rgba + o);
                else rgba[o] = px8;
            }
        }
    }
    tile_prof_flush(cnt);
    // Only the COUNT variant (the RT_FLAG_STATS launch, pick_kernel) tallies:
    // in the timed kernels every counter is dead code.
    if (COUNT && (F.flags & RT_FLAG_STATS)) tile_tally(cnt, stats, false);
}

// One wave per workgroup: one 8 x 8 tile each, so a CU takes a new tile as
// soon as any wave slot frees instead of four at once (A/B against 2 x 2
// tiles per workgroup: C3 -3.1%, C5 -4.5%, C4 -3.7%, scene7 -3.4%, scene9
// -1.4%, C2 -0.8%; declaring 64 threads: C5 -1.1%).
// XCD-aware block order: the dispatcher deals workgroups round-robin over
// the 8 XCDs (each with its own L2), so workgroup w runs on XCD w % 8 as
// that XCD's (w / 8)-th.  Big-list kernels (RT_OPT_XCD_DEAL, F.xcd_mode):
//  1: chunks of K consecutive blocks of a tile row go to one XCD, when the
//     grid divides evenly (C5 -1.4% against K = 4; C3's 240 x 135 tiles do
//     not divide: hardware order) — horizontal neighbours share an L2;
//  2: column stripes of xcd_w tiles, stripe s on XCD s % 8 (one stripe per
//     XCD by default, RT_OPT_XCD_STRIPE): XCD x walks its stripes' tiles row
//     by row, so a tile's horizontal AND vertical neighbours — which read
//     the same light-buffer cells, tile lists and records — share its L2,
//     while at any moment all XCDs work on the same frame rows (whole-region
//     runs per XCD were 1.8x slower on C3: the mesh rows piled onto a few
//     XCDs);
//  3: 4 x 2 super-tiles dealt round-robin over the XCDs;
//  0: hardware order.
// Modes 2 and 3 launch a padded grid (xcd_grid); its blocks past the frame's
// tiles return at once.  The small-list kernels: hardware order (C2 -2.5%
// against K = 4; the remap's code alone costs it).
template <int WAVE>
__device__ __forceinline__ bool tile_of_block(const FrameDev& F, int& bx, int& by)
{
    bx = (int)blockIdx.x;
    by = (int)blockIdx.y;
    constexpr unsigned K = is_clustered(WAVE) ? RT_XCD_CHUNK_BIG : RT_XCD_CHUNK_SMALL;
    if constexpr (is_clustered(WAVE)) {
        const unsigned w = blockIdx.y * gridDim.x + blockIdx.x;
        const unsigned x = w % kXcds, i = w / kXcds;
        if (F.xcd_mode == 2) {
            const unsigned sw = (unsigned)F.xcd_w, m = (unsigned)F.xcd_m, j = i % m;
            bx = (int)((j / sw) * (kXcds * sw) + x * sw + j % sw);
            by = (int)(i / m);
            return bx < F.tiles_x && by < F.tiles_y;
        }
        if (F.xcd_mode == 3) {
            const unsigned st = (i / 8u) * kXcds + x, p = i % 8u, gx = (unsigned)F.xcd_w;
            bx = (int)((st % gx) * 4u + p % 4u);
            by = (int)((st / gx) * 2u + p / 4u);
            return bx < F.tiles_x && by < F.tiles_y;
        }
        if (F.xcd_mode == 0) return true;
    }
    if constexpr (K > 0) {
        const unsigned nb = gridDim.x * gridDim.y, w = blockIdx.y * gridDim.x + blockIdx.x;
        const unsigned x = w % kXcds, i = w / kXcds;
        const unsigned lw = ((i / K) * kXcds + x) * K + i % K;
        if (lw < nb && (nb % (kXcds * K)) == 0) {
            bx = (int)(lw % gridDim.x);
            by = (int)(lw / gridDim.x);
        }
    }
    return true;
}

template <int MAXD, int LB, int WAVE, bool COUNT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(waves_per_eu(MAXD, WAVE)))) void rt_trace_kernel(
    const SceneDev S, const FrameDev F, unsigned* __restrict__ rgba, float* __restrict__ rgbf,
    StatsDev* __restrict__ stats)
{
    int bx, by;
    if (!tile_of_block<WAVE>(F, bx, by)) return;
    trace_tile<MAXD, LB, WAVE, COUNT>(S, F, rgba, rgbf, stats, bx, by);
}

// Passes the (32-bit, wave-uniform) values through scalar registers at this
// point of the program: their loads from the kernel-argument segment are
// issued above it, together, and waited for once, instead of where control
// flow first uses each.  Not volatile and without a memory clobber: an
// opaque move, no memory effect (a volatile one would bar every later
// wave-uniform load from the scalar cache).
#define RT_PIN4(a, b, c, d) asm("" : "+s"(a), "+s"(b), "+s"(c), "+s"(d))

// rt_trace_tiny's pixel store, for its lean path (the general path keeps its
// own copy of these lines: its instances' code is to stay what it was
// measured as).
__device__ __forceinline__ void tiny_store_px(float* rgbf, unsigned* rgba, size_t o, const Color c)
{
    if (rgbf) {
        rgbf[3 * o] = c.r;
        rgbf[3 * o + 1] = c.g;
        rgbf[3 * o + 2] = c.b;
    }
    // nontemporal (streaming) stores, as every small-list kernel (trace_tile)
    if (rgba)
        __builtin_nontemporal_store(unorm8(c.r) | (unorm8(c.g) << 8) | (unorm8(c.b) << 16) | 0xFF000000u, rgba + o);
}

// Tiny scenes (kTiny): one 8 x 8 tile of a depth-0 frame whose
// wave-uniform inputs all come with the launch (rt_cull.h TinyLaunch, one
// by-value argument read from the kernel-argument segment by scalar loads).
// trace_tile's frame geometry, radiance<0>'s hit and store, with the
// dependent scalar round trips of a tile cut to: the header, the tile's mask
// (issued straight behind it, in flight under the ray set-up), one per kept
// triangle, the hit's normal and material, and per light its record, its
// cell's offsets and one per entry.
// kMaskCompute: the wave computes the tile's mask; kMaskStore: and stores it.
template <int MAXD, int LB, int WAVE, bool COUNT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(waves_per_eu(MAXD, WAVE)))) void rt_trace_tiny(
    const TinyLaunch L)
{
    static_assert(MAXD == 0 && LB == 1 && (WAVE & kTinyRead) == kTinyRead,
                  "the launch-camera kernels are depth-0, light-buffer");
    const TinyHead& H = L.h;
    // ---- the header's camera / frame / mask / plane part, under one wait
    FrameDev F{};
    F.cam[0] = H.cam[0], F.cam[1] = H.cam[1], F.cam[2] = H.cam[2];
    F.width = H.width;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        F.orient[4 * i] = H.orient[3 * i];
        F.orient[4 * i + 1] = H.orient[3 * i + 1];
        F.orient[4 * i + 2] = H.orient[3 * i + 2];
    }
    F.half_w = H.half_w, F.half_h = H.half_h, F.inv_w = H.inv_w, F.inv_h = H.inv_h;
    F.bg[0] = H.bg[0], F.bg[1] = H.bg[1], F.bg[2] = H.bg[2];
    F.height = H.height;
    F.row_begin = H.row_begin, F.row_end = H.row_end;
    F.band_rows = H.band_rows, F.band_count = H.band_count, F.band_index = H.band_index;
    int tn = H.n, masked = H.masked, tiles_x = H.tiles_x;
    TileRec* const mask = H.mask;
    TinyPlanes PL;
#pragma unroll
    for (int k = 0; k < kTinyPlanes; ++k) {
        PL.a[k] = H.plane[k];
        PL.num[k] = H.pnum[k];
        PL.idx[k] = H.pidx[k];
    }
    int n_plane = H.n_plane;
    unsigned tm = H.tm_all;  // no masks: every listed triangle
    // the instance that reads the tile facts (rt_cull.h tile_facts_pack): the
    // reading frames, not a counted one (its counters are the general kernels')
    constexpr bool FACTS = !computes_mask(WAVE) && !COUNT && RT_TILE_FACTS != 0;
    // the lean record (rt_tile.h LeanRec, RT_TILE_LEAN): the storing instances
    // write it, the FACTS instance reads it in place of the TileRec and takes
    // a lean tile down a path of its own (below, behind the ray set-up)
    constexpr bool LEAN_WR = stores_mask(WAVE) && (RT_TILE_LEAN & 1) != 0;
    constexpr bool LEAN_RD = FACTS && (RT_TILE_LEAN & 2) != 0;
    constexpr bool LEAN_BV = LEAN_RD && (RT_TILE_LEAN & 4) != 0;
    // its records as 16-dword vectors in the global address space: the
    // pointer's halves pass through scalar registers with the header's first
    // batch (the first pin: one wait for all of it), and a pointer rebuilt
    // from them needs the address space named to be read by a scalar load
    typedef unsigned LeanWords __attribute__((ext_vector_type(16)));
    typedef const __attribute__((address_space(1))) LeanWords* LeanPtr;
#if (RT_TILE_LEAN & 4) != 0
    [[maybe_unused]] const float (*const lean_lv)[kLeanLightFloats] = L.lights;
#else
    [[maybe_unused]] const float (*const lean_lv)[kLeanLightFloats] = nullptr;
#endif
    [[maybe_unused]] LeanPtr lean = nullptr;
    [[maybe_unused]] int lean_nl = 0;
    if constexpr (LEAN_RD) {
        lean_nl = H.n_lights;
        unsigned lo = (unsigned)(size_t)H.lean, hi = (unsigned)((size_t)H.lean >> 32);
        RT_PIN4(lo, hi, lean_nl, tiles_x);
        lean = (LeanPtr)((size_t)lo | (size_t)hi << 32);
    }
    RT_PIN4(F.cam[0], F.cam[1], F.cam[2], F.width);
#pragma unroll
    for (int i = 0; i < 4; ++i) RT_PIN4(F.orient[4 * i], F.orient[4 * i + 1], F.orient[4 * i + 2], F.half_w);
    RT_PIN4(F.half_h, F.inv_w, F.inv_h, F.height);
    RT_PIN4(F.row_begin, F.row_end, F.band_rows, F.band_count);
    RT_PIN4(F.band_index, tn, masked, tiles_x);
    // (the lean reader's instance leaves the planes to its general path: they
    // are loaded where that path begins, and held by no lean tile)
    if constexpr (!LEAN_RD) {
        RT_PIN4(n_plane, F.bg[0], F.bg[1], F.bg[2]);
#pragma unroll
        for (int k = 0; k < kTinyPlanes; ++k) {
            RT_PIN4(PL.a[k].x, PL.a[k].y, PL.a[k].z, PL.a[k].w);
            RT_PIN4(PL.num[k], PL.idx[k], tm, masked);
        }
    }

    constexpr bool AHEAD = FACTS && (RT_TILE_FACTS & 32) != 0;
    int nl0 = 0;
    if constexpr (AHEAD) {
        nl0 = H.n_lights;
        RT_PIN4(nl0, tn, masked, tiles_x);
    }

    const int lane = threadIdx.x & 63;
    const int bx = (int)blockIdx.x, by = (int)blockIdx.y;  // hardware order (tile_of_block: small lists)
    const int px = bx * 8 + (lane & 7);
    const int ly0 = by * 8;  // the wave's first output row
    const int ly = ly0 + (lane >> 3);
    int py0 = F.row_begin + ly0, rend = F.row_end;
    if (F.band_rows > 0) {
        py0 = ((ly0 / F.band_rows) * F.band_count + F.band_index) * F.band_rows + ly0 % F.band_rows;
        rend = F.height;
    }
    if (py0 >= rend) return;  // the whole wave lies past the frame (wave-uniform)
    // the launch records' tile: this wave's 8 rows must be one tile row of
    // the full frame (the masks hold for its lanes' clamped pixels)
    const int tile = (py0 & 7) == 0 ? (py0 >> 3) * tiles_x + bx : -1;
    const bool tiled = masked && tile >= 0;
    unsigned fx = 0;  // the tile facts (0: none)
    [[maybe_unused]] LeanRec lr{};  // the tile's lean record (LEAN_RD; facts 0: not lean)
    if constexpr (!computes_mask(WAVE))
        if (tiled) {  // wave-uniform (scalar) load, waited for at the hit
            if constexpr (LEAN_RD) {
                const LeanWords q = lean[tile];  // the TileRec's two words come with it
                static_assert(sizeof(LeanWords) == sizeof(LeanRec), "one record, one load");
                lr.word = q[0], lr.facts = q[1];
                lr.pn[0] = __uint_as_float(q[2]), lr.pn[1] = __uint_as_float(q[3]), lr.pn[2] = __uint_as_float(q[4]);
                lr.pnum = __uint_as_float(q[5]);
                lr.nrm[0] = __uint_as_float(q[6]), lr.nrm[1] = __uint_as_float(q[7]), lr.nrm[2] = __uint_as_float(q[8]);
                lr.color[0] = __uint_as_float(q[9]), lr.color[1] = __uint_as_float(q[10]);
                lr.color[2] = __uint_as_float(q[11]);
                lr.ka = __uint_as_float(q[12]), lr.kd = __uint_as_float(q[13]), lr.ks = __uint_as_float(q[14]);
                lr.shin = __uint_as_float(q[15]);
            } else if constexpr (FACTS) {
                const TileRec w = mask[tile];
                tm = w.word, fx = w.facts;
            } else {
                tm = mask[tile].word;
            }
        }
    // (RT_TILE_FACTS 32) the first light's hot half with the tile's record:
    // it depends on nothing the kernel computes
    float4 la0 = make_float4(0.f, 0.f, 0.f, 0.f), la1 = la0;
    if constexpr (AHEAD)
        if (nl0 > 0) la0 = H.lrec[0], la1 = H.lrec[1];
    TinyLane tl;
    if constexpr (computes_mask(WAVE)) tl = tiny_lane_load(tn, L.rec);  // the mask's records, in flight under set-up
    const int py = py0 + (lane >> 3);
    const bool valid = px < F.width && py < rend;

    Counters cnt;
#ifdef RT_PROF
    cnt.last = __builtin_amdgcn_s_memtime();
#endif
    // every lane runs (lanes outside the frame on a clamped pixel, result
    // dropped) so edge waves stay whole
    const int pxc = px < F.width ? px : F.width - 1;
    const int pyc = py < rend ? py : rend - 1;
    const Vec3 D = camera_dir_tiny(F, pxc, pyc);
    const Vec3 O = make3(F.cam[0], F.cam[1], F.cam[2]);
    cnt.primary = valid ? 1u : 0u;
    // ---- a lean tile (rt_tile.h): one known surface, a class for every light.
    // The general path's functions on the general path's operands, in its
    // order — the record's plane, normal and material are the values it
    // loads for the facts' surface — with no scene pointer read: the
    // record's wait is the last one that hangs on the tile (a triangle
    // tile's camera record comes from the launch record; the lights from the
    // light records, or with RT_TILE_LEAN 4 from the launch record too).
    if constexpr (LEAN_RD) {
        // the record's first use stands behind the ray set-up: tied to D, or
        // the compiler lifts the word's shift to the load and waits there
        asm("" : "+s"(lr.word), "+s"(lr.facts) : "v"(D.x), "v"(D.y), "v"(D.z));
        if (tiled) tm = lr.word, fx = lr.facts;
        const unsigned lk = tile_facts_kind(lr.facts);
        if (lean_kind(lk)) {
            float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;  // the first light, in flight under the hit
            if (lean_nl > 0) lean_light_load<LEAN_BV>(H.lrec, lean_lv, 0, a0, a1);
            float tl_ = -1.0f;
            if (lk == kFactLeanPlane) {
                tl_ = -lr.pnum / dot(make3(lr.pn[0], lr.pn[1], lr.pn[2]), D);
            } else {
                int ti = -1;
                const float4* r = L.rec + 8 * tile_facts_slot(lr.facts) + 4;
                camera_tri<true>(r[0], r[1], r[2], r[3], D, tl_, ti, cnt);
            }
            const Mat m{{lr.color[0], lr.color[1], lr.color[2]}, lr.ka, lr.kd, lr.ks, lr.shin, 0.f, 0.f, 0.f};
            const Vec3 N = make3(lr.nrm[0], lr.nrm[1], lr.nrm[2]);
            const Vec3 P = O + tl_ * D;
            const unsigned lc = lean_classes(lr.word >> kTinyClassShift, tile_facts_lights(lr.facts));
            const Color cl = shade_lean_tiny<LEAN_BV>(H.lrec, lean_lv, lean_nl, m, P, N, D, valid, lc, a0, a1);
            if (valid) tiny_store_px(H.rgbf, H.rgba, (size_t)ly * F.width + px, cl);
            tile_prof_flush(cnt);
            return;
        }
    }
    unsigned tmask = 0;
    if constexpr (computes_mask(WAVE)) {
        tmask = tiny_tile_mask(tn, tl, D);
        if (tiled) tm = tmask;
    }
    // ---- the scene part of the header (one contiguous block)
    SceneDev S{};
    S.geom = H.geom, S.mat = H.mat;
    S.plane = H.planes, S.quad = H.quad, S.translucent = H.translucent;
    S.lb_off = H.lb_off, S.lb_ent = H.lb_ent, S.lb_dcap = H.lb_dcap, S.cone_light = H.cone_light, S.tri = H.tri;
    S.n_lights = H.n_lights, S.n_tri = H.n_tri, S.n_tri_opaque = H.n_tri_opaque;
    S.n_plane = n_plane, S.n_plane_opaque = H.n_plane_opaque;
    S.n_quad = H.n_quad, S.n_quad_opaque = H.n_quad_opaque, S.n_translucent = H.n_translucent;
    S.shadow_split = H.shadow_split;

    const Color bg{F.bg[0], F.bg[1], F.bg[2]};
    Color c = bg;
    float t;
    RT_MARK(cnt, 0);
    // the word's light classes (rt_cull.h kTinyClassShift): read with the
    // stored word, gathered by the storing frame, neither by a camera's first
    // frame.  A counted render runs every pass (its counters are the general
    // kernels'); a wave without a tile has tm_all's zero bits there.
    constexpr int CLS = stores_mask(WAVE) ? 2 : (!computes_mask(WAVE) && !COUNT) ? 1 : 0;
    unsigned cls = 0;
    if constexpr (!computes_mask(WAVE)) {
        if constexpr (CLS == 1) cls = tm >> kTinyClassShift;
        tm &= (1u << kTinyClassShift) - 1u;
    }
    unsigned lf = 0;  // the lights' facts (rt_cull.h kFactLightShift), two bits each
    [[maybe_unused]] Mat lean_m{};  // LEAN_WR: the shaded surface's material and normal
    [[maybe_unused]] Vec3 lean_n = make3(0.f, 0.f, 0.f);
    if constexpr (!FACTS) {
        const int idx = closest_hit_camera_tiny(S, PL, L.rec, tm, O, D, t, cnt);
        RT_MARK(cnt, 1);
        // Lanes that miss (or lie outside the frame) stay in step through the
        // shading so the wave stays whole.
        const bool hit = idx >= 0;
        if constexpr (CLS == 2) {
            // the storing frame: what the search found, for the later frames
            const int f0 = __builtin_amdgcn_readfirstlane(idx);
            if (!__any(hit)) {
                fx = tile_facts_pack(kFactMiss, 0, 0, 0);
            } else if (__all(hit & (idx == f0)) && tile_facts_surf_field(f0) != 0) {
                unsigned k = kFactSearch, sl = 0;
#pragma unroll
                for (int q = 0; q < kTinyPlanes; ++q)
                    if (q < S.n_plane && PL.idx[q] == f0) k = kFactPlane, sl = (unsigned)q;
                for (unsigned mm = tm; mm && k == kFactSearch;) {
                    const int j = (int)__builtin_ctz(mm);
                    mm &= mm - 1u;
                    if (__float_as_int(L.rec[8 * j + 7].y) == f0) k = kFactTri, sl = (unsigned)j;
                }
                fx = tile_facts_pack(k, sl, 0, tile_facts_surf_field(f0));
            }
        }
        if (__any(hit & valid)) {
            const int sidx = hit ? idx : 0;
            // A tile usually sees one surface: then its normal and material
            // records come by scalar (broadcast) loads instead of a per-lane gather.
            const int s0 = __builtin_amdgcn_readfirstlane(sidx);
            Vec3 N;
            Mat m;
            if (__all(sidx == s0)) {
                m = load_mat(S, s0);
                N = hit_normal(S, s0, O, D, t);
            } else {
                m = load_mat(S, sidx);
                N = hit_normal(S, sidx, O, D, t);
            }
            const Vec3 P = O + t * D;
            const Color cl = shade_local_tiny<CLS>(S, PL, H.lrec, m, P, N, D, cnt, hit & valid, cls, lf, la0, la1);
            c = hit ? cl : bg;
            if constexpr (LEAN_WR) lean_m = m, lean_n = N;
        }
    } else {
        // The reading frames, with the tile facts (all wave-uniform).  A tile
        // that shows one known surface takes its material and normal by
        // scalar loads issued here, in flight under the search (2), and tests
        // only the primitive the storing frame found it by: the same function
        // on the same operands, so the same t, and by determinism every lane
        // hits it (4).  A tile every lane missed keeps the background (1).
        static_assert(kTinyPlanes == 2, "the plane slot is picked by one select");
        const unsigned kind = tile_facts_kind(fx), slot = tile_facts_slot(fx);
        const int s0 = (int)tile_facts_surf(fx) - 1;
        lf = tile_facts_lights(fx);
        if constexpr ((RT_TILE_FACTS & 8) != 0) {
            // a no-op pass: class 3, both bits of the light's class
            static_assert(kTinyClassLights == 6, "0x555: the no-op bit of each light");
            const unsigned np = lf & 0x555u;
            cls |= np | np << 1;
        }
        const bool miss = (RT_TILE_FACTS & 1) != 0 && kind == kFactMiss;
        const bool known =
            (RT_TILE_FACTS & 6) != 0 && s0 >= 0 && (kind == kFactPlane || kind == kFactTri || kind == kFactSearch);
        Mat m{};
        Vec3 N = make3(0.f, 0.f, 0.f);
        bool have_n = false;
        if constexpr ((RT_TILE_FACTS & 2) != 0) {
            if (known) {
                m = load_mat(S, s0);
                const float4* g = S.geom + 4 * s0;
                if (kind == kFactPlane) {
                    const float4 a = g[0];
                    N = make3(a.y, a.z, a.w);
                    have_n = true;
                } else if (kind == kFactTri) {
                    const float4 c2 = g[2], d2 = g[3];
                    N = make3(c2.z, c2.w, d2.x);
                    have_n = true;
                }
            }
        }
        int idx = -1;
        t = -1.0f;
        bool hit = false, lit = false;
        if ((RT_TILE_FACTS & 4) != 0 && known && kind != kFactSearch) {
            if (kind == kFactPlane) {
                // closest_hit_camera_tiny's plane slot, alone
                const float4 a = slot ? PL.a[1] : PL.a[0];
                const float num = slot ? PL.num[1] : PL.num[0];
                t = -num / dot(make3(a.x, a.y, a.z), D);
            } else {
                const float4* r = L.rec + 8 * slot + 4;
                camera_tri<true>(r[0], r[1], r[2], r[3], D, t, idx, cnt);
            }
            hit = lit = true;
        } else if (!miss) {
            idx = closest_hit_camera_tiny(S, PL, L.rec, tm, O, D, t, cnt);
            hit = idx >= 0;
            lit = __any(hit & valid);
        }
        RT_MARK(cnt, 1);
        if (lit) {
            if (known) {
                if constexpr ((RT_TILE_FACTS & 2) == 0) m = load_mat(S, s0);
                if (!have_n) N = hit_normal(S, s0, O, D, t);
            } else {
                const int sidx = hit ? idx : 0;
                const int b0 = __builtin_amdgcn_readfirstlane(sidx);
                if (__all(sidx == b0)) {
                    m = load_mat(S, b0);
                    N = hit_normal(S, b0, O, D, t);
                } else {
                    m = load_mat(S, sidx);
                    N = hit_normal(S, sidx, O, D, t);
                }
            }
            const Vec3 P = O + t * D;
            const Color cl = shade_local_tiny<CLS>(S, PL, H.lrec, m, P, N, D, cnt, hit & valid, cls, lf, la0, la1);
            c = hit ? cl : bg;
        }
    }
    if (valid) {
        const size_t o = (size_t)ly * F.width + px;
        float* const rgbf = H.rgbf;
        unsigned* const rgba = H.rgba;
        if (rgbf) {
            rgbf[3 * o] = c.r;
            rgbf[3 * o + 1] = c.g;
            rgbf[3 * o + 2] = c.b;
        }
        // nontemporal (streaming) stores, as every small-list kernel (trace_tile)
        if (rgba)
            __builtin_nontemporal_store(unorm8(c.r) | (unorm8(c.g) << 8) | (unorm8(c.b) << 16) | 0xFF000000u, rgba + o);
    }
    // the tile's mask for its camera's later frames on this stream
    // (kMaskStore), stored last: at the top of the kernel the store's
    // completion held up the loads behind it (A/B: C2 -2.8%, C4 -2.5%).
    // Above the mask's 20 bits, the light classes the shading gathered (0
    // where the tile was not shaded); beside the word, the tile facts.
    if constexpr (stores_mask(WAVE))
        if (lane == 0 && tiled) mask[tile] = TileRec{tmask | cls << kTinyClassShift, fx | lf << kFactLightShift};
    // and its lean record (rt_tile.h): on a tile of one plane or triangle
    // every lane hit that surface, so lane 0 holds the wave's material and
    // normal (uniform loads), and the tile was shaded (lane 0 is in the frame)
    if constexpr (LEAN_WR)
        if (lane == 0 && tiled) {
            LeanFields f{};
            f.word = tmask | cls << kTinyClassShift, f.facts = fx | lf << kFactLightShift;
            f.lean = lean_tile(f.word, f.facts, S.n_lights, S.n_translucent, true);
            if (tile_facts_kind(fx) == kFactPlane) {  // (a triangle tile's slot is no plane's)
                const unsigned slot = tile_facts_slot(fx);
                const float4 a = slot ? PL.a[1] : PL.a[0];
                f.pn[0] = a.x, f.pn[1] = a.y, f.pn[2] = a.z;
                f.pnum = slot ? PL.num[1] : PL.num[0];
            }
            f.nrm[0] = lean_n.x, f.nrm[1] = lean_n.y, f.nrm[2] = lean_n.z;
            f.color[0] = lean_m.color.r, f.color[1] = lean_m.color.g, f.color[2] = lean_m.color.b;
            f.ka = lean_m.ka, f.kd = lean_m.kd, f.ks = lean_m.ks, f.shin = lean_m.shin;
            H.lean[tile] = lean_pack(f);
        }
    tile_prof_flush(cnt);
    if (COUNT && (H.flags & RT_FLAG_STATS)) tile_tally(cnt, H.stats, true);  // (every lane runs)
}

// Self-test of the wave primitives the culling relies on (rt_debug_selftest):
// wave_min / wave_max / wave_sum_u64 against plain loops over the same lane
// values, and wave_cone's cos W as a lower bound of every live lane's cosine.
__global__ void rt_selftest_kernel(unsigned seed, unsigned* __restrict__ fails)
{
    const int lane = (int)(threadIdx.x & 63);
    __shared__ float vals[256];
    __shared__ unsigned long long uv[256];
    unsigned h = (seed * 0x9E3779B9u) ^ (blockIdx.x * 0x85EBCA6Bu) ^ (threadIdx.x * 0xC2B2AE35u);
    h ^= h >> 16;
    h *= 0x7FEB352Du;
    h ^= h >> 15;
    const float x = (float)(h & 0xFFFFFF) / 16777216.0f * 2.0f - 1.0f;
    const unsigned long long u = (unsigned long long)(h >> 8) * 977ull;
    vals[threadIdx.x] = x;
    uv[threadIdx.x] = u;
    __syncthreads();
    const float mn = wave_min(x), mx = wave_max(x);
    const unsigned long long su = wave_sum_u64(u);
    const int base = (int)(threadIdx.x & ~63u);
    float rmn = vals[base], rmx = vals[base];
    unsigned long long rsu = 0;
    for (int i = 0; i < 64; ++i) {
        rmn = fminf(rmn, vals[base + i]);
        rmx = fmaxf(rmx, vals[base + i]);
        rsu += uv[base + i];
    }
    // a random cone of directions: every live lane's cosine to the axis >= cos W
    const float th = 0.05f * (float)((h >> 4) & 255) / 255.0f;
    const float ph = 6.2831853f * (float)((h >> 12) & 1023) / 1024.0f;
    const Vec3 d = make3(sinf(th) * cosf(ph), sinf(th) * sinf(ph), cosf(th));
    const bool live = ((h >> 20) & 3) != 0;
    const WaveCone wc = wave_cone(d, live);
    bool bad = (mn != rmn) | (mx != rmx) | (su != rsu);
    if (wc.ok && live) bad |= dot(d, wc.w) < wc.cosW;
    if (bad) atomicAdd(fails, 1u);
    (void)lane;
}

// Bounce-ray closest hits of arbitrary rays (rt_debug_bvh_rays): lane i
// takes ray i (O, D: 6 floats) through the BVH and through every triangle;
// out_idx / out_t get both winners (file index, t) as [bvh, brute].
__global__ __launch_bounds__(64) void rt_bvh_rays_kernel(const SceneDev S, const float* __restrict__ rays, int n,
                                                           int* __restrict__ out_idx, float* __restrict__ out_t,
                                                           unsigned long long* __restrict__ tally)
{
    const int i = (int)(blockIdx.x * 64 + threadIdx.x);
    if (i >= n) return;
    const float* r = rays + 6 * (size_t)i;
    const Vec3 O = make3(r[0], r[1], r[2]), D = make3(r[3], r[4], r[5]);
    Counters cnt;
    float tb, tf;
    const int ib = closest_hit_bvh(S, O, D, tb, cnt);
    const unsigned tests = cnt.btri, nodes = cnt.bnode;
    const int jf = closest_hit<false>(S, O, D, tf, cnt);
    out_idx[2 * i] = ib;
    out_idx[2 * i + 1] = jf;
    out_t[2 * i] = tb;
    out_t[2 * i + 1] = tf;
    atomicAdd(&tally[0], (unsigned long long)tests);
    atomicAdd(&tally[1], (unsigned long long)nodes);
}

// The wave-cooperative walk (rt_debug_bvh_rays_wave): one ray per wave, its
// planes and quadrics and first BVH step by the budgeted serial walk (budget
// 1: every ray straggles), the rest by bvh_walk_wave — as the wavefront's
// straggler kernel finishes a walk.
__global__ __launch_bounds__(64) void rt_bvh_wave_kernel(const SceneDev S, const float* __restrict__ rays, int n,
                                                           int* __restrict__ out_idx, float* __restrict__ out_t)
{
    extern __shared__ float4 rt_lds_dyn[];
    int* const base = reinterpret_cast<int*>(rt_lds_dyn);
    const int i = (int)blockIdx.x;
    if (i >= n) return;
    const float* r = rays + 6 * (size_t)i;
    const Vec3 O = make3(r[0], r[1], r[2]), D = make3(r[3], r[4], r[5]);
    Counters cnt;
    float bt = -1.0f;
    int bi = -1;
    bool str = false;
    if ((threadIdx.x & 63) == 0) {
        bi = closest_hit_bvh<kWfStragCap * sizeof(int), 1>(S, O, D, bt, cnt, &str);
    }
    bt = readlanef(bt, 0);
    bi = __builtin_amdgcn_readlane(bi, 0);
    str = __builtin_amdgcn_readlane((int)str, 0) != 0;
    if (str) bvh_walk_wave(S, O, D, bt, bi, base, kWfStragCap, cnt);
    if ((threadIdx.x & 63) == 0) {
        out_idx[i] = bi;
        out_t[i] = bt;
    }
}

}  // namespace rt

#include "rt_aov.h"  // rt_aov_kernel (needs tile_of_block above)
#include "rt_shaderays.h"  // rt_shade_rays_kernel (needs radiance and waves_per_eu above)
#include "rt_adaptive.h"  // rt_edge_classify_kernel, rt_refine_kernel (need radiance and camera_dir above)

// ===================================================================== host
using namespace rt;

// Frames of rt_render_sequence_async in flight at once (one stream and one
// camera slot each): a frame's camera prepasses and trace kernel overlap the
// previous frames' (measured: 1 vs 4 streams, tools/overlap_probe.py; 2
// streams gain nothing on MI355X, 3-4 do).
#ifndef RT_SEQ_STREAMS
#define RT_SEQ_STREAMS 4
#endif
constexpr int kSeqSlots = RT_SEQ_STREAMS;
constexpr int kCbWordSets = 16;  // camera buffers per context: 1 + sequence slots (spare sets)

struct rt_ctx;
// A buffer that the context's streams share, one user at a time: a user on
// another stream than the last one's waits for that one's event (enter), and
// leaves its own behind (leave); after a host sync nobody is pending (done).
struct Turn {
    hipEvent_t ev = nullptr;  // after the last user (made by the first leave)
    hipStream_t last = nullptr;
    bool pending = false;
    int enter(rt_ctx* c, hipStream_t st);
    int leave(rt_ctx* c, hipStream_t st);
    void done() { pending = false; }
};

struct rt_ctx : SceneCounts {  // (the uploaded scene's counts: rt_scenehost.h)
    int device = 0;
    // CPU backend (rt_create_cpu): no HIP object is ever made for it
    bool cpu = false;
    int cpu_threads = 0;
    void* cpu_scene = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float4* d_geom = nullptr;
    float4* d_mat = nullptr;
    float4* d_lights = nullptr;
    float4* d_tri = nullptr;
    float4* d_plane = nullptr;
    float4* d_quad = nullptr;
    int* d_translucent = nullptr;
    float4* d_trisph = nullptr;
    float4* d_cone_light = nullptr;
    float4* d_trinrm = nullptr;
    float4* d_tricoef = nullptr;
    float4* d_clu_light = nullptr;
    int n_clu = 0;
    // A camera buffer (rt_cambuf.h): per-tile lists for the camera of key,
    // built on the stream that needs it; the entry array's capacity comes
    // from the totals of earlier builds, read back without a host sync
    // (h_tot after ev_tot), and grows when a build needed more.
    struct CamBuf {
        float4* tcone = nullptr;
        unsigned* off = nullptr;
        unsigned* cur = nullptr;
        unsigned* flag = nullptr;
        int4* box = nullptr;        // n_tri triangle screen boxes
        unsigned* tcnt = nullptr;   // n_tri + 1 box sizes -> pair offsets
        unsigned long long* rmask = nullptr;  // pass mask per run of 64 candidate pairs
        size_t rcap = 0;            // runs rmask holds
        size_t observed_pairs = 0;  // largest candidate-pair count read back
        size_t built_cap = 0, built_rcap = 0;  // capacities of the last build (for its read-back)
        int* lng = nullptr;
        int* mid = nullptr;
        unsigned* stat = nullptr;
        void* scan = nullptr;
        int2* ent = nullptr;
        float4* rec = nullptr;      // inline records (RT_OPT_CB_INLINE_MAX_MB)
        size_t cap = 0, rec_cap = 0, scan_words = 0;
        int nt_alloc = 0, big_alloc = 0;
        unsigned long long* h_tot = nullptr;  // pinned: [total][stat words 0..7 as 4 u64]
        hipEvent_t ev_tot = nullptr, ev0 = nullptr, ev1 = nullptr;
        bool tot_pending = false;   // h_tot written by an enqueued copy not yet seen
        size_t observed = 0;        // largest total read back
        size_t entries = 0;         // last total read back
        unsigned hstat[8] = {};     // last stat words read back
        bool inline_rec = false;    // rec holds the current records
        int tiles_x = 0, ntiles = 0;
        float key[30] = {};
        bool valid = false;
        // a captured render references off / flag / ent / rec: the next
        // build writes fresh arrays (the captured ones are retired intact,
        // the capture-time lists that a replay reads)
        bool pinned = false;
        double host_ms = 0.0, build_ms = 0.0;
        bool timed = false;
    };
    // What one camera owns on the device: its records (cam_alloc: camera-ray
    // triangle values, cone records, and the cluster records of a big list
    // or the union records of a small one — the camera's, then one per
    // light), its camera buffer, and the camera position the records were
    // last computed for (camera_prepass; tricam_all: tricam holds every
    // triangle for it).
    struct CamState {
        float4 *tricam = nullptr, *cone_cam = nullptr, *clu_cam = nullptr, *uni = nullptr;
        CamBuf cb;
        float key[3] = {0.f, 0.f, 0.f};
        bool valid = false, tricam_all = false;
    };
    CamState cam;  // the camera of every entry point but the sequence's
    // the last async frame's camera (cb_key_of): a repeat builds the sorted lists
    float last_async_key[30] = {};
    bool last_async_valid = false;
    // The cameras of rt_render_sequence_async: frame i of a sequence uses
    // slot i % kSeqSlots on internal stream i % kSeqSlots, so up to
    // kSeqSlots consecutive frames (different cameras) are in flight at
    // once.  A slot's records are computed for every frame: its key, valid
    // and tricam_all stay unset.
    CamState seq[kSeqSlots];
    hipStream_t seq_streams[kSeqSlots] = {};
    hipEvent_t seq_fork = nullptr, seq_join[kSeqSlots] = {};
    int n_cu = 0;
    std::vector<void*> deferred;  // replaced buffers an enqueued render may read: freed at the next host sync
    void* d_scan = nullptr;     // u64 scratch of the light-buffer build scans
    size_t scan_words = 0;
    unsigned long long* h_word = nullptr;  // pinned: totals read back by the builds
    unsigned long long* h_cbwords = nullptr;  // pinned: kCbWordSets x 8 words, one set per camera buffer
    int n_cbwords = 0;
    // light buffer (shadow cells), rt_lb_build
    unsigned* d_lb_off = nullptr;
    float4* d_lb_ent = nullptr;
    float4* d_lb_dcap = nullptr;
    float4* d_lb_meta = nullptr;
    // the launch-camera kernels' per-light records (rt_shade.h kLightRec) and
    // the host copies they and the launch record are made from
    // (two sets of n_lights records: with each light's occupied-direction
    // bound, then with "always look" for RT_OPT_LB_REGION 0)
    float4* d_lrec = nullptr;
    std::vector<float4> h_lrec;  // the first set (rt_debug_lb_region)
    std::vector<float4> h_lb_meta;
    std::vector<float> h_plane;  // plane[]: [n cst] [file index 0 0 0] per plane
    bool lb_ready = false;
    int lb_levels = 0;  // buffers per light: slot = level * n_lights + light
    int lb_r0 = 0;      // light 0's first buffer's resolution (cells per face edge)
    size_t lb_entries = 0;
    double lb_build_ms = 0.0;
    // Tiny scenes (<= kTinyMax triangles, depth 0, light buffer): the camera
    // records are computed on the host per camera and passed with the launch
    // (rt_cull.h TinyCam) — host copies of the triangle records for that.
    std::vector<float4> h_tri, h_sph, h_nrm, h_coef;
    TinyCam tiny{};
    float tiny_key[30] = {};
    bool tiny_valid = false;
    bool opt_launch_camera = true;  // RT_OPT_LAUNCH_CAMERA
    struct MaskBuf {
        hipStream_t stream = nullptr;
        TileRec* d = nullptr;  // one record per tile: the word and the tile facts (rt_cull.h)
        LeanRec* lean = nullptr;  // behind them in the same allocation: one lean record per tile (rt_tile.h)
        size_t cap = 0;
        float key[30] = {};   // the camera whose masks d holds (valid)
        bool valid = false;
        float pend[30] = {};  // the camera of the stream's last computing frame (pend_valid)
        bool pend_valid = false;
        // after the kernel that stored d (a reader on a stream that only
        // shares this one's handle — a destroyed stream's successor — waits)
        hipEvent_t ev = nullptr;
        bool ev_set = false;
        unsigned long long used = 0;  // last use (LRU eviction)
    };
    std::vector<MaskBuf> tiny_masks;  // per stream, at most kMaskBufs
    unsigned long long mask_clock = 0;
    StatsDev* d_stats = nullptr;
    void* d_scratch = nullptr;  // staging for host outputs
    size_t scratch_bytes = 0;
    // Ordering of the per-camera device state across streams (rt.h, ABI 4):
    // the streams that received rt_render_async work since the last host
    // sync of the context, and the stream + event of the last write of the
    // per-camera state not yet host-synced (an async camera prepass).
    std::vector<hipStream_t> async_streams;
    hipEvent_t ev_fence = nullptr, ev_state = nullptr;
    // synchronous renders into host memory: the slab in row chunks, each
    // copied over PCIe on copy_stream while the next one renders
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_chunk[8] = {};
    hipStream_t state_stream = nullptr;
    bool state_pending = false;
    bool captured = false;                // a render was captured into a hipGraph
    std::vector<void*> retired;           // buffers a captured render may reference
    // Options (rt_set_option; rt.h RT_OPT_*)
    int opt_light_buffer = 1;
    int opt_camera_buffer = 1;  // 0 off, 1 auto, 2 async builds for every frame
    bool opt_union = true;
    double opt_lb_scale = 0.0;
    double opt_dcov_near = 0.0;
    double opt_cb_inline_mb = 0.0;
    double opt_host_chunk_mb = 8.0;
    double opt_cb_capacity = 0.0;  // camera-buffer entries; 0 = automatic
    std::vector<double> far_ladder;       // big lists' far light buffers
    double upload_parts_ms[4] = {0, 0, 0, 0};  // copy+records, prepasses, light buffer, total
    double lb_parts_ms[5] = {0, 0, 0, 0, 0};    // lb_build phases (rt_debug_upload_info out[4..8])
    // bounce-ray BVH (rt_bvh.h, built at upload for scenes that can bounce)
    float4* d_bvh_node = nullptr;
    float4* d_bvh_tri = nullptr;
    // per surface: its coherence-sort bin (WfDev::skey; triangles in the
    // BVH's leaf order, two per bin), and the bins per branch
    unsigned* d_skey = nullptr;
    unsigned nbin_half = 0;
    int bvh_inner = 0, bvh_leaves = 0, bvh_depth = 0;
    double bvh_build_ms = 0.0;
    bool opt_bvh = true;        // RT_OPT_BVH
    bool opt_ray_bvh = false;   // RT_OPT_RAY_BVH: the BVH also for scenes without bounce rays (ray queries)
    // Wavefront bounce queues (rt_wavefront.h), grown on demand; one set per
    // context: a wavefront frame on another stream than the last one's waits
    // for that frame (turn) before it reuses them.
    struct WfBuf {
        void* mem = nullptr;      // one allocation: counters, then every level's arrays
        size_t bytes = 0;
        size_t px = 0;            // pixel capacity (level-0 nodes)
        size_t cap[kWfMaxLevels + 1] = {};   // ray slots per level (level 0: pixels)
        size_t pcap[kWfMaxLevels + 1] = {};  // parent-list slots per level
        WfDev dev{};
        // coherence sort (WfDev::kin): bins of `kcap` ray slots, sorted
        // slots, the bin counts / positions (hcap words) and their scan's
        // scratch
        unsigned *kin = nullptr, *kout = nullptr, *kout2 = nullptr, *hist = nullptr;
        unsigned long long* bsum = nullptr;
        size_t kcap = 0, hcap = 0;
        int sort = 0;  // this frame's RT_OPT_WF_SORT: bit 0 parent sort, bit 1 hit sort (bit 2: by light cell)
        Turn turn;                // a wavefront frame at a time
        hipStream_t st2 = nullptr;               // RT_OPT_WF_OVERLAP: the stragglers' stream
        hipEvent_t ev_t = nullptr, ev_s = nullptr;  // fork (after the trace) / join (after the stragglers' shading)
    } wf;
    // Supersampled renders (rt_render_ss*): the float sample intermediate,
    // one per context, grown on demand: a call on another stream than the
    // last one's waits for that call's resolve (turn) before it overwrites it.
    struct SsBuf {
        float* mem = nullptr;
        size_t bytes = 0;
        Turn turn;  // left after a call's last resolve
    } ss;
    // Adaptive supersampling (rt_render_adaptive*): the base frame's planes
    // with their halo rows (rgb, id, n), the flag words, their offsets, the
    // list of flagged pixels and the scan's scratch — one allocation per
    // context, grown on demand and shared by its streams like ss (turn: left
    // after a call's refine kernel).  ev: the synchronous call's timing —
    // before the base pass, after it, after classify + scan, after refine.
    struct AdBuf {
        void* mem = nullptr;
        size_t bytes = 0;
        Turn turn;
        hipEvent_t ev[4] = {};
        float phase_ms[3] = {};  // the last synchronous call's (rt_debug_adaptive_phases)
        const unsigned* total = nullptr;  // the last call's flagged count on the device (the scan's total)
        unsigned long long flagged = 0;   // read back by the synchronous call, for rt_stats
    } ad;
    double opt_ss_chunk_rows = 0.0;  // RT_OPT_SS_CHUNK_ROWS (0 = auto)
    int opt_wavefront = 1;      // RT_OPT_WAVEFRONT
    int opt_wf_sort = 1;        // RT_OPT_WF_SORT
    bool opt_wf_overlap = true; // RT_OPT_WF_OVERLAP
    int opt_xcd_deal = 1;       // RT_OPT_XCD_DEAL
    int opt_xcd_stripe = 0;     // RT_OPT_XCD_STRIPE
    bool opt_lb_unroll = true;  // RT_OPT_LB_UNROLL
    bool opt_lb_region = true;  // RT_OPT_LB_REGION
    bool uploaded = false;
    rt_stats last{};
    std::string err;
};

static void cb_free(rt_ctx::CamBuf& B);

#define RT_EXPORT extern "C" __attribute__((visibility("default")))

static int hip_fail(rt_ctx* c, hipError_t e, const char* what)
{
    c->err = std::string(what) + ": " + hipGetErrorString(e);
    return RT_E_HIP;
}
#define HIP_TRY(c, call)                                   \
    do {                                                   \
        hipError_t e_ = (call);                            \
        if (e_ != hipSuccess) return hip_fail(c, e_, #call); \
    } while (0)

int Turn::enter(rt_ctx* c, hipStream_t st)
{
    if (pending && last != st) HIP_TRY(c, hipStreamWaitEvent(st, ev, 0));
    return RT_OK;
}
int Turn::leave(rt_ctx* c, hipStream_t st)
{
    if (!ev) HIP_TRY(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIP_TRY(c, hipEventRecord(ev, st));
    last = st;
    pending = true;
    return RT_OK;
}

// Every camera state of the context: its own, then the sequence slots'.
static std::array<rt_ctx::CamState*, 1 + kSeqSlots> cam_states(rt_ctx* c)
{
    std::array<rt_ctx::CamState*, 1 + kSeqSlots> a{&c->cam};
    for (int j = 0; j < kSeqSlots; ++j) a[1 + j] = &c->seq[j];
    return a;
}

RT_EXPORT const char* rt_last_error(rt_ctx* c) { return c ? c->err.c_str() : "null context"; }

RT_EXPORT int rt_create(int32_t dev, rt_ctx** out)
{
    if (!out) return RT_E_ARG;
    *out = nullptr;
    rt_ctx* c = new rt_ctx();
    c->device = dev;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0 || dev < 0 || dev >= ndev) {
        *out = c;
        c->err = "no usable HIP device";
        return RT_E_HIP;
    }
    *out = c;
    HIP_TRY(c, hipSetDevice(dev));
    HIP_TRY(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIP_TRY(c, hipEventCreate(&c->ev0));
    HIP_TRY(c, hipEventCreate(&c->ev1));
    HIP_TRY(c, hipEventCreateWithFlags(&c->ev_fence, hipEventDisableTiming));
    HIP_TRY(c, hipEventCreateWithFlags(&c->ev_state, hipEventDisableTiming));
    HIP_TRY(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    for (hipEvent_t& e : c->ev_chunk) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIP_TRY(c, hipHostMalloc((void**)&c->h_word, 2 * sizeof(unsigned long long), hipHostMallocDefault));
    HIP_TRY(c, hipHostMalloc((void**)&c->h_cbwords, kCbWordSets * 8 * sizeof(unsigned long long), hipHostMallocDefault));
    HIP_TRY(c, hipMalloc(&c->d_stats, kStatSlots * sizeof(StatsDev)));
    HIP_TRY(c, hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, dev));
    c->far_ladder = {2.5, 6.0, 16.0, 64.0};
    return RT_OK;
}

// Free now, or — once a render was captured into a hipGraph — keep until
// rt_upload_scene / rt_destroy (a replay may still reference it).
static void release(rt_ctx* c, void* p)
{
    if (!p) return;
    if (c->captured)
        c->retired.push_back(p);
    else
        hipFree(p);
}

static void free_retired(rt_ctx* c)
{
    for (void* p : c->retired) hipFree(p);
    c->retired.clear();
    c->captured = false;
}

// ---- ordering of the per-camera state across streams (rt.h, ABI 4)
// Make stream w wait for everything already enqueued on the streams that
// received async renders (they may read the state w is about to rewrite).
static int fence_async(rt_ctx* c, hipStream_t w)
{
    for (hipStream_t s : c->async_streams) {
        if (s == w) continue;
        HIP_TRY(c, hipEventRecord(c->ev_fence, s));
        HIP_TRY(c, hipStreamWaitEvent(w, c->ev_fence, 0));
    }
    return RT_OK;
}

// A reader on stream r of state written on another stream and not yet
// host-synced waits for that write.
static int wait_state(rt_ctx* c, hipStream_t r)
{
    if (c->state_pending && c->state_stream != r) HIP_TRY(c, hipStreamWaitEvent(r, c->ev_state, 0));
    return RT_OK;
}

static void note_async(rt_ctx* c, hipStream_t s)
{
    if (std::find(c->async_streams.begin(), c->async_streams.end(), s) == c->async_streams.end())
        c->async_streams.push_back(s);
}

// The closing step of an entry point that enqueued on a caller's stream st.
// In a capture the graph may reference the context's buffers from now on
// (release, free_later) and pins the camera buffer it walks (`used`, or
// null; cb_build); else uploads, fences and rt_destroy sync st.
static void enqueued(rt_ctx* c, hipStream_t st, bool capturing, rt_ctx::CamBuf* used)
{
    if (capturing) {
        c->captured = true;
        if (used) used->pinned = true;
    } else {
        note_async(c, st);
    }
}

// Buffers replaced while renders that read them may still have been in
// flight (free_later): after a host sync of everything nothing reads them.
// The internal sequence streams are joined into the caller's stream, which
// is one of the synced async streams.
static void free_deferred(rt_ctx* c)
{
    for (void* p : c->deferred) hipFree(p);
    c->deferred.clear();
}

// The context after a host sync of everything it enqueued: no async render,
// state write, wavefront frame or resolve is in flight any more.
static void settled(rt_ctx* c)
{
    c->async_streams.clear();
    c->state_pending = false;
    c->state_stream = nullptr;
    c->wf.turn.done();
    c->ss.turn.done();
    c->ad.turn.done();
    free_deferred(c);
}

// Host sync of everything the context enqueued.
static int sync_all(rt_ctx* c)
{
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->copy_stream) HIP_TRY(c, hipStreamSynchronize(c->copy_stream));
    for (hipStream_t s : c->async_streams) HIP_TRY(c, hipStreamSynchronize(s));
    settled(c);
    return RT_OK;
}

// Device scratch for the build scans (u64 words), grown on demand.
static int ensure_scan(rt_ctx* c, size_t words)
{
    if (c->scan_words >= words) return RT_OK;
    release(c, c->d_scan);
    c->d_scan = nullptr;
    c->scan_words = 0;
    HIP_TRY(c, hipMalloc(&c->d_scan, words * sizeof(unsigned long long)));
    c->scan_words = words;
    return RT_OK;
}

RT_EXPORT int rt_sync(rt_ctx* c)
{
    if (!c) return RT_E_ARG;
    if (c->cpu) return RT_OK;  // CPU renders are synchronous
    if (!c->stream) return RT_E_STATE;
    HIP_TRY(c, hipSetDevice(c->device));
    return sync_all(c);
}

RT_EXPORT int rt_set_option(rt_ctx* c, int32_t opt, double v)
{
    if (!c || !(v == v)) return RT_E_ARG;
    switch (opt) {
    case RT_OPT_LIGHT_BUFFER:
        if (v != 0 && v != 1 && v != 2) return RT_E_ARG;
        c->opt_light_buffer = (int)v;
        return RT_OK;
    case RT_OPT_CAMERA_BUFFER:
        if (v != 0 && v != 1 && v != 2) return RT_E_ARG;
        if ((int)v != c->opt_camera_buffer) c->cam.cb.valid = false;
        c->opt_camera_buffer = (int)v;
        return RT_OK;
    case RT_OPT_UNION_PRETEST: c->opt_union = v != 0; return RT_OK;
    case RT_OPT_LB_SCALE:
        if (v < 0 || v > 1e6) return RT_E_ARG;
        c->opt_lb_scale = v;
        return RT_OK;
    case RT_OPT_DCOV_NEAR:
        if (v < 0 || (v > 0 && v < 1.0) || v > 1e6) return RT_E_ARG;
        c->opt_dcov_near = v;
        return RT_OK;
    case RT_OPT_CB_INLINE_MAX_MB:
        if (v < 0) return RT_E_ARG;
        // the layout is chosen at a camera-buffer build: rebuild at the next render
        if (v != c->opt_cb_inline_mb) c->cam.cb.valid = false;
        c->opt_cb_inline_mb = v;
        return RT_OK;
    case RT_OPT_HOST_CHUNK_MB:
        if (v < 0) return RT_E_ARG;
        c->opt_host_chunk_mb = v;
        return RT_OK;
    case RT_OPT_LAUNCH_CAMERA: c->opt_launch_camera = v != 0; return RT_OK;
    case RT_OPT_BVH: c->opt_bvh = v != 0; return RT_OK;
    case RT_OPT_RAY_BVH: c->opt_ray_bvh = v != 0; return RT_OK;
    case RT_OPT_WAVEFRONT: c->opt_wavefront = v != 0; return RT_OK;
    case RT_OPT_WF_SORT:
        if (v < 0 || v > 7 || v != std::floor(v)) return RT_E_ARG;
        c->opt_wf_sort = (int)v;
        return RT_OK;
    case RT_OPT_WF_OVERLAP: c->opt_wf_overlap = v != 0; return RT_OK;
    case RT_OPT_XCD_DEAL:
        if (v != 0 && v != 1 && v != 2 && v != 3) return RT_E_ARG;
        c->opt_xcd_deal = (int)v;
        return RT_OK;
    case RT_OPT_LB_UNROLL: c->opt_lb_unroll = v != 0; return RT_OK;
    case RT_OPT_LB_REGION: c->opt_lb_region = v != 0; return RT_OK;
    case RT_OPT_XCD_STRIPE:
        if (v < 0 || v > 4096 || v != std::floor(v)) return RT_E_ARG;
        c->opt_xcd_stripe = (int)v;
        return RT_OK;
    case RT_OPT_SS_CHUNK_ROWS:
        if (v < 0 || v > 1e9 || v != std::floor(v)) return RT_E_ARG;
        c->opt_ss_chunk_rows = v;
        return RT_OK;
    case RT_OPT_CB_CAPACITY:
        if (v < 0 || v > 4e9 || v != std::floor(v)) return RT_E_ARG;
        if (v != c->opt_cb_capacity) c->cam.cb.valid = false;
        c->opt_cb_capacity = v;
        return RT_OK;
    default: return RT_E_ARG;
    }
}

RT_EXPORT int rt_get_option(rt_ctx* c, int32_t opt, double* v)
{
    if (!c || !v) return RT_E_ARG;
    switch (opt) {
    case RT_OPT_LIGHT_BUFFER: *v = c->opt_light_buffer; return RT_OK;
    case RT_OPT_CAMERA_BUFFER: *v = c->opt_camera_buffer; return RT_OK;
    case RT_OPT_UNION_PRETEST: *v = c->opt_union ? 1 : 0; return RT_OK;
    case RT_OPT_LB_SCALE: *v = c->opt_lb_scale; return RT_OK;
    case RT_OPT_DCOV_NEAR: *v = c->opt_dcov_near; return RT_OK;
    case RT_OPT_CB_INLINE_MAX_MB: *v = c->opt_cb_inline_mb; return RT_OK;
    case RT_OPT_HOST_CHUNK_MB: *v = c->opt_host_chunk_mb; return RT_OK;
    case RT_OPT_CB_CAPACITY: *v = c->opt_cb_capacity; return RT_OK;
    case RT_OPT_LAUNCH_CAMERA: *v = c->opt_launch_camera ? 1 : 0; return RT_OK;
    case RT_OPT_BVH: *v = c->opt_bvh ? 1 : 0; return RT_OK;
    case RT_OPT_RAY_BVH: *v = c->opt_ray_bvh ? 1 : 0; return RT_OK;
    case RT_OPT_WAVEFRONT: *v = c->opt_wavefront; return RT_OK;
    case RT_OPT_WF_SORT: *v = c->opt_wf_sort; return RT_OK;
    case RT_OPT_WF_OVERLAP: *v = c->opt_wf_overlap ? 1 : 0; return RT_OK;
    case RT_OPT_XCD_DEAL: *v = c->opt_xcd_deal; return RT_OK;
    case RT_OPT_XCD_STRIPE: *v = c->opt_xcd_stripe; return RT_OK;
    case RT_OPT_LB_UNROLL: *v = c->opt_lb_unroll ? 1 : 0; return RT_OK;
    case RT_OPT_LB_REGION: *v = c->opt_lb_region ? 1 : 0; return RT_OK;
    case RT_OPT_SS_CHUNK_ROWS: *v = c->opt_ss_chunk_rows; return RT_OK;
    default: return RT_E_ARG;
    }
}

RT_EXPORT int rt_set_far_ladder(rt_ctx* c, const double* f, int32_t n)
{
    if (!c || n > 8) return RT_E_ARG;
    if (n < 0) {
        if (f) return RT_E_ARG;
        c->far_ladder = {2.5, 6.0, 16.0, 64.0};
        return RT_OK;
    }
    if (n > 0 && !f) return RT_E_ARG;
    for (int i = 0; i < n; ++i)
        if (!(f[i] >= 1.0 && f[i] <= 1e6) || (i > 0 && !(f[i] > f[i - 1]))) return RT_E_ARG;
    c->far_ladder.assign(f, f + n);
    return RT_OK;
}

RT_EXPORT int rt_create_cpu(int32_t threads, rt_ctx** out)
{
    if (!out) return RT_E_ARG;
    rt_ctx* c = new rt_ctx();
    c->cpu = true;
    c->cpu_threads = threads;
    *out = c;
    return RT_OK;
}

// The HIP entry points refuse a CPU context (and the CPU ones a HIP context
// without a host scene): the backend is the caller's explicit choice.
static int not_cpu(rt_ctx* c)
{
    c->err = "a CPU context (rt_create_cpu) renders with rt_cpu_render / rt_cpu_render_float";
    return RT_E_STATE;
}

template <class... P>
static void free_all(P*&... p)
{
    ((hipFree(p), p = nullptr), ...);
}

// The light buffer: dropped with the scene, and by a build that turns out
// too large (lb_build: the scene then runs without it).
static void lb_drop(rt_ctx* c)
{
    free_all(c->d_lb_off, c->d_lb_ent, c->d_lb_dcap, c->d_lb_meta);
    c->h_lb_meta.clear();
    c->lb_ready = false;
    c->lb_levels = c->lb_r0 = 0;
    c->lb_entries = 0;
}

// Everything an upload makes: the scene's device buffers, the host copies and
// the per-scene counts and flags.  The one place that lists them: an upload
// drops the previous scene with it (a failed one leaves its pieces for the
// next), rt_destroy the last.  Nothing may be in flight (sync_all).  The
// camera buffers stay (reallocated on demand): they are only marked stale.
static void scene_drop(rt_ctx* c)
{
    c->uploaded = false;
    free_all(c->d_geom, c->d_mat, c->d_lights, c->d_tri, c->d_plane, c->d_quad, c->d_translucent, c->d_trisph,
             c->d_cone_light, c->d_trinrm, c->d_tricoef, c->d_clu_light, c->d_lrec, c->d_bvh_node, c->d_bvh_tri,
             c->d_skey);
    lb_drop(c);
    c->lb_build_ms = 0.0;
    for (rt_ctx::CamState* q : cam_states(c)) {  // the per-camera records
        free_all(q->tricam, q->cone_cam, q->clu_cam, q->uni);
        q->cb.valid = q->valid = false;
    }
    for (auto* h : {&c->h_lrec, &c->h_tri, &c->h_sph, &c->h_nrm, &c->h_coef}) h->clear();
    c->h_plane.clear();
    c->n_clu = 0;
    c->nbin_half = 0;
    c->bvh_inner = c->bvh_leaves = c->bvh_depth = 0;
    c->bvh_build_ms = 0.0;
    c->tiny_valid = false;
    for (auto& q : c->tiny_masks) q.valid = q.pend_valid = false;  // the old scene's triangles
    static_cast<SceneCounts&>(*c) = SceneCounts{};
}

RT_EXPORT void rt_destroy(rt_ctx* c)
{
    if (!c) return;
    if (c->cpu) {
        cpu_free(c->cpu_scene);
        delete c;
        return;
    }
    if (c->stream) {
        (void)hipSetDevice(c->device);
        (void)sync_all(c);
    }
    free_retired(c);
    scene_drop(c);
    hipFree(c->wf.mem);
    hipFree(c->wf.kin);
    hipFree(c->wf.kout);
    hipFree(c->wf.kout2);
    hipFree(c->wf.hist);
    hipFree(c->wf.bsum);
    hipFree(c->ss.mem);
    if (c->ss.turn.ev) hipEventDestroy(c->ss.turn.ev);
    hipFree(c->ad.mem);
    if (c->ad.turn.ev) hipEventDestroy(c->ad.turn.ev);
    for (hipEvent_t e : c->ad.ev)
        if (e) hipEventDestroy(e);
    if (c->wf.turn.ev) hipEventDestroy(c->wf.turn.ev);
    if (c->wf.ev_t) hipEventDestroy(c->wf.ev_t);
    if (c->wf.ev_s) hipEventDestroy(c->wf.ev_s);
    if (c->wf.st2) hipStreamDestroy(c->wf.st2);
    for (auto& q : c->tiny_masks) {
        hipFree(q.d);
        if (q.ev) hipEventDestroy(q.ev);
    }
    for (rt_ctx::CamState* q : cam_states(c)) cb_free(q->cb);
    hipFree(c->d_stats);
    hipFree(c->d_scratch);
    if (c->ev0) hipEventDestroy(c->ev0);
    if (c->ev1) hipEventDestroy(c->ev1);
    if (c->ev_fence) hipEventDestroy(c->ev_fence);
    if (c->ev_state) hipEventDestroy(c->ev_state);
    for (hipEvent_t e : c->ev_chunk)
        if (e) hipEventDestroy(e);
    if (c->copy_stream) hipStreamDestroy(c->copy_stream);
    for (int j = 0; j < kSeqSlots; ++j) {
        if (c->seq_streams[j]) hipStreamDestroy(c->seq_streams[j]);
        if (c->seq_join[j]) hipEventDestroy(c->seq_join[j]);
    }
    if (c->seq_fork) hipEventDestroy(c->seq_fork);
    if (c->h_word) hipHostFree(c->h_word);
    if (c->h_cbwords) hipHostFree(c->h_cbwords);
    hipFree(c->d_scan);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
}


// 256 camera records = 16 KB, the scalar data cache.
static constexpr int kTricamMaxTriangles = 256;
#ifndef RT_EDGE_MAX_TRIANGLES
#define RT_EDGE_MAX_TRIANGLES 0x7fffffff  // every list size (SceneDev::use_edges)
#endif
static constexpr int kEdgeMaxTriangles = RT_EDGE_MAX_TRIANGLES;

// Light buffer of every light (shadow_opaque_lb, lb_cone): resolution from
// the median angular radius of the light's triangle cones (cell half-width
// ~ that radius), nearest-first cell lists built on the device in two
// levels (supercells of 16 x 16 cells, then cells), offsets by host scans.
// Shadow-ray culling covers rays up to dcov = F x the light's farthest
// triangle (the prepass sizes each pair's margin for it; lanes beyond take
// the next level, or the per-lane loop over every triangle).  Big lists: a
// ladder of buffers per light, F = 1.25 then far buffers at 2.5, 6, 16 and
// 64 — each level's cones only as wide as its distance needs (A/B: 1.5 / 4 /
// 16 / 64 against one buffer at 3 plus one at 64: C3 -10%, C5 -8.5%; this
// ladder against that one: C3 -2%, C5 -5%; a single buffer at 2
// without far levels was 120x slower: lanes beyond fell into the per-lane
// loop over 50k triangles; one buffer at 16 or 64 widens every cone: C3
// 2.3x / 8.8x slower).  Small lists (<= 1,024 triangles, no clusters, one
// level): F = RT_DCOV_FACTOR_SMALL — far ground-plane points then stay
// in the buffer (A/B against 4: 16 / 32 / 64 / 256 = C2 -8 / -10 / -11 /
// +1%, C4 -8 / -8 / -6 / +5%; C1 and the bounce scenes flat; re-tuned at the
// end of round 2: 24 against 32 C2 -2.5%, C4 -2.4%, 20 and 28 worse).
// RT_OPT_DCOV_NEAR and rt_set_far_ladder override the big-list ladder at
// upload (tests, A/B).
#ifndef RT_DCOV_FACTOR
#define RT_DCOV_FACTOR 1.25
#endif
#ifndef RT_DCOV_FACTOR_SMALL
#define RT_DCOV_FACTOR_SMALL 24.0
#endif
// Slots: one buffer per entry of `cones` (a light's cone records, built for
// the distance dcov[j]): the lights, then (big lists) their far buffers.

// Device temporaries of one build: freed when the scope ends, on every path
// out of it.
struct DevScope {
    void* p[8] = {};
    int n = 0;
    DevScope() = default;
    DevScope(const DevScope&) = delete;
    ~DevScope()
    {
        for (int i = 0; i < n; ++i) hipFree(p[i]);
    }
    template <class T>
    hipError_t alloc(T** out, size_t bytes)
    {
        assert(n < 8);
        const hipError_t e = hipMalloc((void**)out, bytes);
        if (e == hipSuccess) p[n++] = *out;
        return e;
    }
};

// lb_build's phases (rt_ctx::lb_parts_ms): mark(i) ends phase i.
struct LbClock {
    rt_ctx* c;
    std::chrono::steady_clock::time_point tp = std::chrono::steady_clock::now();
    void mark(int i)
    {
        const auto now = std::chrono::steady_clock::now();
        c->lb_parts_ms[i] = std::chrono::duration<double, std::milli>(now - tp).count();
        tp = now;
    }
};

constexpr int kLbTooLarge = 1;  // lb_level, lb_lists: no error, but the lists do not fit 32-bit indices

// One level of lists for every slot: launch(j, false) adds slot j's counts
// to off[] (`words` zeroed words), ONE scan turns them into offsets, the total
// comes back (a host sync; it ends phase `part` if >= 0), alloc(total) makes
// the lists and launch(j, true) fills them.  kLbTooLarge: total > max_total.
template <class Launch, class Alloc>
static int lb_level(rt_ctx* c, LbClock& clk, int part, int nl, unsigned* off, size_t words,
                    unsigned long long max_total, unsigned long long* total, Launch launch, Alloc alloc)
{
    hipStream_t st = c->stream;
    for (int j = 0; j < nl; ++j)
        if (int rc = launch(j, false)) return rc;
    unsigned long long* tot = nullptr;
    HIP_TRY(c, scan_u32(off, (unsigned)words, off, (unsigned long long*)c->d_scan, st, &tot));
    HIP_TRY(c, hipMemcpyAsync(c->h_word, tot, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    *total = *c->h_word;
    if (part >= 0) clk.mark(part);
    if (*total > max_total) return kLbTooLarge;
    if (int rc = alloc(*total)) return rc;
    for (int j = 0; j < nl; ++j)
        if (int rc = launch(j, true)) return rc;
    return RT_OK;
}

// The slots' lists and records on the device (lb_build below, which owns the
// temporaries T): the plan, then three levels of lists — the hyper level of
// the big slots, the supercells, the cells — and the dcap lists.
static int lb_lists(rt_ctx* c, int ntr, int n_opaque, const std::vector<const float4*>& cones,
                    const std::vector<double>& dcov, LbClock& clk, DevScope& T)
{
    hipStream_t st = c->stream;
    const int nl = (int)cones.size();
    // cells of ~1/4 the median cone radius: best of 1-8 on C3 and C5; and
    // no coarser than 128 cells per face edge (small scenes: C2 -3.3%, C4
    // -2.5% against their 16-48, flat from 192 to 512).  An explicit
    // RT_OPT_LB_SCALE (A/B, the stress tests' coarse cells) sets R alone.
    // Big lists (the ladder): 1/6 of the median cone radius since the LDS
    // walks (round 2: C3 -4.5%, C5 -1.4% against 1/4, whose lists were
    // twice as long; 22 M -> 47 M entries and +24 ms of build at upload; 5
    // and 8 measured worse); small lists keep 4 (flat at C1/C2/C4).
    const bool scale_set = c->opt_lb_scale > 0.0;
    const double scale = scale_set ? c->opt_lb_scale : (ntr > kClusterMinTriangles ? 6.0 : 4.0);
    const int r_min = scale_set ? kLbGroup : RT_LB_RMIN;
    // 1. the cone records of every slot (c0, c1 per triangle): one sync; the
    // plan (rt_scenehost.h)
    std::vector<float> h((size_t)nl * ntr * 8);
    for (int j = 0; j < nl; ++j)
        HIP_TRY(c, hipMemcpyAsync(h.data() + (size_t)j * ntr * 8, cones[j], (size_t)ntr * 2 * sizeof(float4),
                                  hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    clk.mark(0);
    LbPlan P;
    lb_plan(h.data(), nl, ntr, n_opaque, dcov.data(), scale, r_min, P);
    clk.mark(1);
    // 2. device arrays
    int *d_perm = nullptr, *d_slists = nullptr, *d_hlists = nullptr;
    unsigned *d_soff = nullptr, *d_hoff = nullptr;
    const size_t np = P.perm.size() + P.dperm.size();
    HIP_TRY(c, T.alloc(&d_perm, std::max<size_t>(np, 1) * sizeof(int)));
    if (!P.perm.empty())
        HIP_TRY(c, hipMemcpyAsync(d_perm, P.perm.data(), P.perm.size() * sizeof(int), hipMemcpyHostToDevice, st));
    if (!P.dperm.empty())
        HIP_TRY(c, hipMemcpyAsync(d_perm + P.perm.size(), P.dperm.data(), P.dperm.size() * sizeof(int),
                                  hipMemcpyHostToDevice, st));
    HIP_TRY(c, T.alloc(&d_soff, P.sob * sizeof(unsigned) + sizeof(unsigned)));
    HIP_TRY(c, hipMalloc(&c->d_lb_off, P.ob * sizeof(unsigned) + sizeof(unsigned)));
    if (int rc = ensure_scan(c, scan_scratch(std::max(std::max(P.sob, P.ob), P.hob)))) return rc;
    HIP_TRY(c, hipMemsetAsync(d_soff, 0, P.sob * sizeof(unsigned), st));
    HIP_TRY(c, hipMemsetAsync(c->d_lb_off, 0, P.ob * sizeof(unsigned), st));
    // a level's index lists, a temporary
    auto ints = [&](int** lists) {
        return [&T, c, lists](unsigned long long n) -> int {
            HIP_TRY(c, T.alloc(lists, std::max<size_t>(n, 1) * sizeof(int)));
            return RT_OK;
        };
    };
    unsigned long long total = 0;
    // 2a. the hyper level of the big slots: blocks of kLbHyper x kLbHyper supercells
    if (P.hob > 0) {
        HIP_TRY(c, T.alloc(&d_hoff, P.hob * sizeof(unsigned) + sizeof(unsigned)));
        HIP_TRY(c, hipMemsetAsync(d_hoff, 0, P.hob * sizeof(unsigned), st));
        auto hyper = [&](int j, bool fill) -> int {
            const LbSlot& b = P.slots[j];
            if (!b.nhyp) return RT_OK;
            unsigned* const o = d_hoff + b.hob;
            hipLaunchKernelGGL(rt_lb_super, dim3(b.nhyp), dim3(256), 0, st, cones[j], ntr, d_perm + b.perm0,
                               (int)b.nperm, b.R, (float)dcov[j], fill ? o : nullptr, fill ? nullptr : o,
                               fill ? d_hlists : nullptr, kLbGroup * kLbHyper, b.Gp, 2e-3, nullptr, nullptr, 1, 1);
            HIP_TRY(c, hipGetLastError());
            return RT_OK;
        };
        if (int rc = lb_level(c, clk, -1, nl, d_hoff, P.hob, 0xFFFFFFF0ull, &total, hyper, ints(&d_hlists))) return rc;
    }
    // 2b. supercells, each from its hyper block's list where the slot has one
    auto super = [&](int j, bool fill) -> int {
        const LbSlot& b = P.slots[j];
        unsigned* const o = d_soff + b.sob;
        hipLaunchKernelGGL(rt_lb_super, dim3(b.nsup), dim3(256), 0, st, cones[j], ntr, d_perm + b.perm0, (int)b.nperm,
                           b.R, (float)dcov[j], fill ? o : nullptr, fill ? nullptr : o, fill ? d_slists : nullptr,
                           kLbGroup, b.R / kLbGroup, 1e-3, b.nhyp ? d_hoff + b.hob : nullptr, d_hlists, kLbHyper, b.Gp);
        HIP_TRY(c, hipGetLastError());
        return RT_OK;
    };
    if (int rc = lb_level(c, clk, 2, nl, d_soff, P.sob, 0xFFFFFFF0ull, &total, super, ints(&d_slists))) return rc;
    // 3. cell lists (offsets: the slots' lb_off) and, with each slot's fill,
    // its dcap list
    auto cells = [&](int j, bool fill) -> int {
        const LbSlot& b = P.slots[j];
        unsigned* const o = c->d_lb_off + b.ob;
        hipLaunchKernelGGL(rt_lb_cells, dim3(b.nsup), dim3(256), 0, st, cones[j], ntr, c->d_tri, b.R, (float)dcov[j],
                           d_soff + b.sob, d_slists, fill ? o : nullptr, fill ? nullptr : o,
                           fill ? (float*)c->d_lb_ent : nullptr);
        HIP_TRY(c, hipGetLastError());
        if (fill && b.ndperm) {
            hipLaunchKernelGGL(rt_lb_dcap, dim3((unsigned)((b.ndperm + 255) / 256)), dim3(256), 0, st, cones[j], c->d_tri,
                               d_perm + P.perm.size() + b.dperm0, (int)b.ndperm,
                               (float*)c->d_lb_dcap + kLbEntF * b.dperm0);
            HIP_TRY(c, hipGetLastError());
        }
        return RT_OK;
    };
    auto buffers = [&](unsigned long long n) -> int {
        HIP_TRY(c, hipMalloc(&c->d_lb_ent, std::max<size_t>(n, 1) * kLbEntF * sizeof(float)));
        HIP_TRY(c, hipMalloc(&c->d_lb_dcap, std::max<size_t>(P.dperm.size(), 1) * kLbEntF * sizeof(float)));
        HIP_TRY(c, hipMalloc(&c->d_lb_meta, std::max(nl, 1) * 2 * sizeof(float4)));
        return RT_OK;
    };
    // (entry indices are 32-bit: four words per entry)
    if (int rc = lb_level(c, clk, 3, nl, c->d_lb_off, P.ob, 0xFFFFFFF0ull / 4 - 1, &total, cells, buffers)) return rc;
    // 4. per slot [off base, dcap base, n dcap, R] [dcov 0 0 0]
    std::vector<float4> meta((size_t)std::max(nl, 1) * 2);
    for (int j = 0; j < nl; ++j) {
        const LbSlot& b = P.slots[j];
        const unsigned words[4] = {(unsigned)b.ob, (unsigned)b.dperm0, (unsigned)b.ndperm, (unsigned)b.R};
        std::memcpy(&meta[2 * j], words, sizeof words);
        meta[2 * j + 1] = make_float4((float)dcov[j], 0.f, 0.f, 0.f);
    }
    HIP_TRY(c, hipMemcpyAsync(c->d_lb_meta, meta.data(), meta.size() * sizeof(float4), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipStreamSynchronize(st));  // meta (host) outlives the copy; the temporaries are freed by the caller
    c->h_lb_meta = meta;  // (light_records_build makes the light records from it)
    clk.mark(4);
    c->lb_r0 = nl > 0 ? P.slots[0].R : 0;
    c->lb_ready = true;
    c->lb_entries = total;
    return RT_OK;
}

static int lb_build(rt_ctx* c, int ntr, int n_opaque, const std::vector<const float4*>& cones,
                    const std::vector<double>& dcov)
{
    const auto t0 = std::chrono::steady_clock::now();
    int rc;
    {
        DevScope T;
        LbClock clk{c};
        rc = lb_lists(c, ntr, n_opaque, cones, dcov, clk, T);
        if (rc != RT_OK) (void)hipStreamSynchronize(c->stream);  // nothing reads the temporaries any more
    }
    c->lb_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc != kLbTooLarge) return rc;
    lb_drop(c);  // too large: run without it
    return RT_OK;
}

// The occupied-direction bound [a.x a.y a.z cosB] of one light buffer
// (rt_lightbuf.h) from its cell offsets (6 R^2 + 1 words), in double: the
// axis a is the mean of the centre directions of the cells that hold an
// entry, rounded to float; B the largest angle(a, w) + W over those cells,
// grown by 1e-9 (relative and absolute: the check's libm is another one).
// Only the cells whose centre lies within two cell radii of the farthest
// centre from a can set B (a cell's W is at most the face-centre cell's),
// so only their cones are computed: a buffer with thousands of such cells
// costs a square root per cell, not four atan2.  Returns the number of cells
// that hold an entry.
static unsigned lb_region_build(const unsigned* off, int R, float* out4)
{
    out4[0] = out4[1] = out4[2] = 0.0f;
    out4[3] = -2.0f;
    const int n = 6 * R * R;
    auto centre = [R](int c, double* w) {
        lb_face_dir(c / (R * R), (2.0 * (c % R) + 1.0) / R - 1.0, (2.0 * (c / R % R) + 1.0) / R - 1.0, w);
    };
    double sum[3] = {0.0, 0.0, 0.0}, w[3];
    unsigned cnt = 0;
    for (int c = 0; c < n; ++c) {
        if (!(off[c + 1] > off[c])) continue;
        centre(c, w);
        sum[0] += w[0], sum[1] += w[1], sum[2] += w[2];
        ++cnt;
    }
    if (cnt == 0) {
        out4[3] = 2.0f;
        return 0;
    }
    const double len = std::sqrt(sum[0] * sum[0] + sum[1] * sum[1] + sum[2] * sum[2]);
    if (!(len > 0.25 * cnt)) return cnt;  // directions all around the light: no usable axis, always look
    const float af[3] = {(float)(sum[0] / len), (float)(sum[1] / len), (float)(sum[2] / len)};
    const double a[3] = {(double)af[0], (double)af[1], (double)af[2]};
    const double an = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    double dmin = 1.0;  // the farthest centre from a, as a cosine
    for (int c = 0; c < n; ++c) {
        if (!(off[c + 1] > off[c])) continue;
        centre(c, w);
        dmin = std::min(dmin, (a[0] * w[0] + a[1] * w[1] + a[2] * w[2]) / an);
    }
    const double far = std::acos(std::max(-1.0, dmin));
    if (!(far < 1.0)) return cnt;
    const double wmax = lb_cone_d(0, R / 2, R / 2 + 1, R / 2, R / 2 + 1, R, 0.0, w);
    const double dscreen = std::cos(std::max(0.0, far - 2.0 * wmax)) + 1e-12;
    double B = 0.0;
    for (int c = 0; c < n; ++c) {
        if (!(off[c + 1] > off[c])) continue;
        centre(c, w);
        if ((a[0] * w[0] + a[1] * w[1] + a[2] * w[2]) / an > dscreen) continue;
        const double W = lb_cone_d(c / (R * R), c % R, c % R + 1, c / R % R, c / R % R + 1, R, 0.0, w);
        B = std::max(B, lb_region_need(a, w, W));
    }
    B = B * (1.0 + 1e-9) + 1e-9;
    if (!(B < 1.0)) return cnt;
    const double cw = lb_region_cos(B);
    float cf = (float)cw;
    if ((double)cf > cw) cf = std::nextafterf(cf, -INFINITY);
    out4[0] = af[0], out4[1] = af[1], out4[2] = af[2], out4[3] = cf;
    return cnt;
}

// ---- rt_upload_scene's stages, in the order it runs them
static double ms_since(std::chrono::steady_clock::time_point t)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

// A host array in a device buffer of its own.
template <class P, class T>
static hipError_t up(P** dst, const std::vector<T>& v)
{
    const hipError_t e = hipMalloc((void**)dst, v.size() * sizeof(T));
    if (e != hipSuccess) return e;
    return hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

// A slot's first lb_meta record (a light record's third): the base of its
// cell offsets in lb_off and its resolution R.
static void lb_meta_words(const float4& m, unsigned& obase, int& R)
{
    std::memcpy(&obase, &m.x, 4);
    std::memcpy(&R, &m.w, 4);
}

// The per-kind lists and per-triangle records, the buffer of the lights'
// cone records, and the tiny scenes' host copies.
static int upload_records(rt_ctx* c, const SceneHost& H)
{
    const size_t ntr = H.ntr;
    HIP_TRY(c, up(&c->d_tri, H.tri));
    HIP_TRY(c, up(&c->d_plane, H.pla));
    HIP_TRY(c, up(&c->d_quad, H.qua));
    HIP_TRY(c, up(&c->d_translucent, H.translucent));
    HIP_TRY(c, up(&c->d_trisph, H.sph));
    HIP_TRY(c, up(&c->d_trinrm, H.nrm));
    HIP_TRY(c, up(&c->d_tricoef, H.coef));
    HIP_TRY(c, hipMalloc((void**)&c->d_cone_light, std::max<size_t>(ntr * H.n_lights, 1) * kConeRec * sizeof(float4)));
    c->h_plane = H.pla;
    if (ntr <= (size_t)kTinyMax) {  // the launch-camera path's host records
        auto f4 = [](const std::vector<float>& v, size_t n) {
            std::vector<float4> o(n);
            std::memcpy(o.data(), v.data(), n * sizeof(float4));
            return o;
        };
        c->h_tri = f4(H.tri, 3 * ntr);
        c->h_sph = f4(H.sph, ntr);
        c->h_nrm = f4(H.nrm, ntr);
        c->h_coef = f4(H.coef, ntr);
    }
    return RT_OK;
}

static int upload_bvh(rt_ctx* c, const SceneHost& H)
{
    c->bvh_build_ms = H.bvh_build_ms;
    if (!H.has_bvh) return RT_OK;
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(c, up(&c->d_bvh_node, H.bvh.nodes));
    HIP_TRY(c, up(&c->d_bvh_tri, H.bvh.tris));
    HIP_TRY(c, up(&c->d_skey, H.skey));
    c->nbin_half = H.nbin_half;
    c->bvh_inner = H.bvh.inner;
    c->bvh_leaves = H.bvh.leaves;
    c->bvh_depth = H.bvh.depth;
    c->bvh_build_ms += ms_since(t0);
    return RT_OK;
}

// Light j's cone records for shadow rays up to `distance` from it.
static int launch_light_cones(rt_ctx* c, const SceneHost& H, int j, float distance, float4* out)
{
    const float* l = &H.lig[8 * (size_t)j];
    hipLaunchKernelGGL(rt_cone_prepass, dim3((unsigned)((H.ntr + 255) / 256)), dim3(256), 0, c->stream, c->d_tri,
                       c->d_trisph, c->d_trinrm, c->d_tricoef, (int)H.ntr, l[0], l[1], l[2], 0, distance, out,
                       (float4*)nullptr);
    HIP_TRY(c, hipGetLastError());
    return RT_OK;
}

// Shadow rays are culled up to this factor of a light's farthest triangle.
// RT_OPT_DCOV_NEAR overrides the big lists' (tests: force lanes into the far
// buffers and beyond them).
static double dcov_factor(const rt_ctx* c, const SceneHost& H)
{
    if (H.ntr <= (size_t)kClusterMinTriangles) return RT_DCOV_FACTOR_SMALL;
    return c->opt_dcov_near > 0.0 ? c->opt_dcov_near : RT_DCOV_FACTOR;
}

// One camera's record buffers for scene H (c->n_clu is set): every
// triangle's camera record (the camera-buffer walk reads them) and cone
// records, and the cluster records of a big list or the union records of a
// small one.
static int cam_alloc(rt_ctx* c, rt_ctx::CamState& q, const SceneHost& H)
{
    HIP_TRY(c, hipMalloc((void**)&q.tricam, H.ntr * 4 * sizeof(float4)));
    HIP_TRY(c, hipMalloc((void**)&q.cone_cam, H.ntr * kConeRec * sizeof(float4)));
    if (c->n_clu > 0)
        HIP_TRY(c, hipMalloc((void**)&q.clu_cam, (size_t)c->n_clu * 4 * sizeof(float4)));
    else
        HIP_TRY(c, hipMalloc((void**)&q.uni, (size_t)(H.n_lights + 1) * 2 * sizeof(float4)));
    return RT_OK;
}

// The lights' prepasses: every light's cone records for its distance
// dcov[j], then the cluster records of a big list or the union records of a
// small one ([camera (filled when the camera is set)] [light 0] ...), whose
// light part is computed once and copied to the sequence slots.  The camera
// states' buffers are allocated here (the list's kind decides which).
static int light_prepasses(rt_ctx* c, const SceneHost& H, std::vector<double>& dcov)
{
    hipStream_t st = c->stream;
    const size_t ntr = H.ntr;
    const int nl = H.n_lights, n_tri_o = H.n_tri_opaque;
    const double dfac = dcov_factor(c, H);
    dcov.assign((size_t)nl, 0.0);
    for (int j = 0; j < nl; ++j) {
        const float d = (float)(dfac * H.far[(size_t)j]);
        if (int rc = launch_light_cones(c, H, j, d, c->d_cone_light + kConeRec * ntr * j)) return rc;
        dcov[(size_t)j] = (double)d;
    }
    c->n_clu = ntr > (size_t)kClusterMinTriangles ? (int)((ntr + 63) / 64) : 0;
    for (rt_ctx::CamState* q : cam_states(c))
        if (int rc = cam_alloc(c, *q, H)) return rc;
    if (c->n_clu > 0) {
        HIP_TRY(c, hipMalloc((void**)&c->d_clu_light, std::max<size_t>((size_t)c->n_clu * nl, 1) * 2 * sizeof(float4)));
        for (int j = 0; j < nl; ++j) {
            hipLaunchKernelGGL(rt_cluster_prepass, dim3(cluster_blocks(c->n_clu)), dim3(256), 0, st,
                               c->d_cone_light + kConeRec * ntr * j, (int)ntr, c->n_clu,
                               c->d_clu_light + 2 * (size_t)c->n_clu * j, 64);
            HIP_TRY(c, hipGetLastError());
        }
        return RT_OK;
    }
    float4* const uni = c->cam.uni;
    for (int j = 0; j < nl && n_tri_o > 0; ++j) {
        hipLaunchKernelGGL(rt_cluster_prepass, dim3(1), dim3(64), 0, st, c->d_cone_light + kConeRec * ntr * j, n_tri_o,
                           1, uni + 2 * (1 + (size_t)j), n_tri_o);  // one wave
        HIP_TRY(c, hipGetLastError());
    }
    if (n_tri_o == 0) {  // no opaque triangle: nothing for shadow rays to walk ("never" record)
        std::vector<float4> nev((size_t)nl * 2);
        for (int j = 0; j < nl; ++j) {
            nev[2 * j] = make_float4(0.f, 0.f, 0.f, 2.0f);
            nev[2 * j + 1] = make_float4(INFINITY, 0.f, INFINITY, 0.f);
        }
        if (nl) HIP_TRY(c, hipMemcpyAsync(uni + 2, nev.data(), nev.size() * sizeof(float4), hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipStreamSynchronize(st));  // nev outlives the copy
    }
    for (auto& q : c->seq)
        HIP_TRY(c, hipMemcpyAsync(q.uni, uni, (size_t)(nl + 1) * 2 * sizeof(float4), hipMemcpyDeviceToDevice, st));
    return RT_OK;
}

// The light buffers, built only where launch() will use them.  Big lists: a
// ladder of far buffers per light after the near one, level v's cone records
// built for far_ladder[v] x the farthest triangle, for the lanes beyond the
// level before (else the per-lane loop over every triangle): slots
// level * n_lights + light.
static int lb_ladder(rt_ctx* c, const SceneHost& H, const std::vector<double>& near_dcov)
{
    const size_t ntr = H.ntr;
    const int nl = H.n_lights, lbm = c->opt_light_buffer;
    const bool big = ntr > (size_t)kClusterMinTriangles;
    if (!(nl > 0 && H.n_tri_opaque > 0 && H.shadow_split && (lbm == 1 || (lbm == 2 && big)))) return RT_OK;
    std::vector<const float4*> cones;
    for (int j = 0; j < nl; ++j) cones.push_back(c->d_cone_light + kConeRec * ntr * j);
    std::vector<double> dcov = near_dcov;
    DevScope T;
    float4* d_cone_far = nullptr;
    const double dfac = dcov_factor(c, H);
    const size_t nlev = big ? c->far_ladder.size() : 0;
    if (nlev > 0) HIP_TRY(c, T.alloc(&d_cone_far, nlev * ntr * nl * kConeRec * sizeof(float4)));
    for (size_t v = 0; v < nlev; ++v)
        for (int j = 0; j < nl; ++j) {
            const double dfar = near_dcov[(size_t)j] / dfac * c->far_ladder[v];
            float4* out = d_cone_far + kConeRec * ntr * (v * nl + j);
            if (int rc = launch_light_cones(c, H, j, (float)dfar, out)) return rc;
            cones.push_back(out);
            dcov.push_back((double)(float)dfar);
        }
    if (int rc = lb_build(c, (int)ntr, H.n_tri_opaque, cones, dcov)) return rc;
    c->lb_levels = c->lb_ready ? 1 + (int)nlev : 0;
    return RT_OK;
}

// The surface, material and light records in file order (what shading reads).
static int upload_surfaces(rt_ctx* c, const SceneHost& H)
{
    HIP_TRY(c, up(&c->d_geom, H.geom));
    HIP_TRY(c, up(&c->d_mat, H.mat));
    HIP_TRY(c, up(&c->d_lights, H.lig));
    return RT_OK;
}

// The launch-camera kernels' light records (rt_shade.h), tiny scenes with a
// light buffer: per light its lights[] pair, its first buffer's lb_meta pair
// and that buffer's occupied-direction bound (lb_region_build, from the
// buffers' cell offsets read back once) in 64 bytes,
// [x y z I] [r g b dcov] [off base, dcap base, n dcap, R] [a.x a.y a.z cosB];
// then the same records with [0 0 0 -2] ("always look", RT_OPT_LB_REGION 0).
static int light_records_build(rt_ctx* c, const SceneHost& H)
{
    const int nl = H.n_lights;
    if (!(c->lb_ready && H.ntr <= (size_t)kTinyMax && c->h_lb_meta.size() >= 2 * (size_t)nl)) return RT_OK;
    // the lights' first buffers' offsets (consecutive slices of lb_off): one copy
    std::vector<unsigned> off, obase((size_t)nl);
    std::vector<int> R((size_t)nl);
    size_t lo = SIZE_MAX, hi = 0;
    for (int j = 0; j < nl; ++j) {
        lb_meta_words(c->h_lb_meta[2 * j], obase[j], R[j]);
        if (R[j] <= 0) continue;
        lo = std::min(lo, (size_t)obase[j]);
        hi = std::max(hi, (size_t)obase[j] + 6 * (size_t)R[j] * R[j] + 1);
    }
    if (hi > lo) {
        off.resize(hi - lo);
        HIP_TRY(c, hipMemcpy(off.data(), c->d_lb_off + lo, off.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    }
    std::vector<float4> lr((size_t)kLightRec * nl * 2);
    for (int j = 0; j < nl; ++j) {
        const float* l = &H.lig[8 * (size_t)j];
        lr[kLightRec * j] = make_float4(l[0], l[1], l[2], l[3]);
        lr[kLightRec * j + 1] = make_float4(l[4], l[5], l[6], c->h_lb_meta[2 * j + 1].x);
        lr[kLightRec * j + 2] = c->h_lb_meta[2 * j];
        float rg[4] = {0.f, 0.f, 0.f, -2.0f};
        if (R[j] > 0) lb_region_build(off.data() + (obase[j] - lo), R[j], rg);
        lr[kLightRec * j + 3] = make_float4(rg[0], rg[1], rg[2], rg[3]);
        for (int q = 0; q < 3; ++q) lr[kLightRec * (nl + j) + q] = lr[kLightRec * j + q];
        lr[kLightRec * (nl + j) + 3] = make_float4(0.f, 0.f, 0.f, -2.0f);
    }
    c->h_lrec.assign(lr.begin(), lr.begin() + (size_t)kLightRec * nl);
    HIP_TRY(c, up(&c->d_lrec, lr));
    return RT_OK;
}

static int cpu_upload_scene(rt_ctx* c, const rt_scene_flat* s)
{
    c->uploaded = false;
    const int rc = cpu_upload(&c->cpu_scene, s);
    if (rc) {
        c->err = "unknown surface type";
        return rc;
    }
    c->n_surf = s->n_surfaces;
    c->n_lights = s->n_lights;
    c->uploaded = true;
    return RT_OK;
}

RT_EXPORT int rt_upload_scene(rt_ctx* c, const rt_scene_flat* s)
{
    if (!c || !s || s->n_surfaces < 0 || s->n_lights < 0) return RT_E_ARG;
    if (s->n_surfaces > 0 && (!s->type || !s->geom || !s->material)) return RT_E_ARG;
    if (s->n_lights > 0 && !s->lights) return RT_E_ARG;
    if (c->cpu) return cpu_upload_scene(c, s);
    if (!c->stream) return RT_E_STATE;
    HIP_TRY(c, hipSetDevice(c->device));
    // nothing in flight may still read the buffers replaced below
    if (int rc = sync_all(c)) return rc;
    free_retired(c);
    const auto tu0 = std::chrono::steady_clock::now();
    SceneHost H;
    if (!scene_host_build(s, H, c->err, c->opt_ray_bvh)) return RT_E_ARG;  // (the context is as it was)
    scene_drop(c);
    if (int rc = upload_records(c, H)) return rc;
    if (int rc = upload_bvh(c, H)) return rc;
    c->upload_parts_ms[0] = ms_since(tu0);
    const auto tp0 = std::chrono::steady_clock::now();
    std::vector<double> dcov;  // per light: its (first) buffer's distance
    if (int rc = light_prepasses(c, H, dcov)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->upload_parts_ms[1] = ms_since(tp0);
    const auto tl0 = std::chrono::steady_clock::now();
    if (int rc = lb_ladder(c, H, dcov)) return rc;
    c->upload_parts_ms[2] = ms_since(tl0);
    if (int rc = upload_surfaces(c, H)) return rc;
    if (int rc = light_records_build(c, H)) return rc;
    static_cast<SceneCounts&>(*c) = H;  // publish the counts
    c->uploaded = true;
    c->upload_parts_ms[3] = ms_since(tu0);
    return RT_OK;
}

// Deepest bounce level any pixel can reach: a child exists only while
// K * energy > min_energy (Scene.cpp:1780,1791); energies are products of
// factors <= k_max and float rounding is monotone, so iterating with k_max
// bounds every path.
static int reachable_depth(const rt_ctx* c, const rt_frame* f)
{
    // With a negative threshold the energy argument below does not hold.
    if (!(f->min_energy >= 0.0f)) return f->max_bounces;
    int levels = 0;
    float e = 1.0f;
    while (levels < f->max_bounces) {
        const float child = c->k_max * e;
        if (!(child > f->min_energy)) break;
        e = child;
        ++levels;
        if (levels > 4096) break;
    }
    return levels;
}

// The kernel of a frame (pick_kernel): its function (nullptr: none compiled),
// its variant — bounce-stack capacity, lights per shadow pass, flags —, its
// dynamic LDS per workgroup, and its name (rt_stats.kernel).
struct KernelPick {
    const void* k = nullptr;
    Variant v;
    unsigned lds = 0;
    const KernelName* name = nullptr;
};
// One compiled variant in a kernel table: rt_variant.h's lists are expanded
// into these tables and nowhere else.  Which kernel counts (COUNT, the
// RT_FLAG_STATS launch) differs by table, each keeping the order its kernels
// have in the code object:
//   kTinyKernels             k[count]: k[0] timed, k[1] counted;
//   kWfShadeKernels<STRAG>   k[!count]: k[0] counted, k[1] timed;
//   kWf0Kernels<COUNT>, kFrameKernels<COUNT>   COUNT is the table's parameter, k[0];
//   kAovKernels              k[0] (AOV frames take no RT_FLAG_STATS).
// A row looked up for a variant that select_variant returned exists, except
// for a depth above the compiled stacks (pick_kernel):
// tools/variant/variant_check.cpp walks the facts the host can form and
// checks every selection against the lists.
template <int N>
struct KernelRow {
    Variant v;
    const void* k[N];
    KernelName name;
};
template <int N, size_t ROWS>
static const KernelRow<N>* find_row(const KernelRow<N> (&table)[ROWS], const Variant& v)
{
    for (const KernelRow<N>& r : table)
        if (r.v == v) return &r;
    return nullptr;
}

// Launch shape of a trace kernel over `rows` output rows: one 8 x 8 tile per
// workgroup, the kernel's dynamic LDS (the big-list kernels' staging
// windows, the BVH kernels' traversal stacks).
static void trace_dims(int width, int rows, dim3& grid, dim3& block)
{
    grid = dim3((width + 7) / 8, (rows + 7) / 8);
    block = dim3(64);
}

// The launch-camera kernels (tiny scenes: camera buffer replaced by the
// launch's records, light-buffer shadows, one light per pass), one per
// tile-mask mode (tiny_masks); k[COUNT].
#define RT_V(M, L, F)                                                                                           \
    {{M, L, F},                                                                                                 \
     {(const void*)&rt_trace_tiny<M, L, F, false>, (const void*)&rt_trace_tiny<M, L, F, true>},                 \
     kernel_name("rt_trace_tiny", M, L, F)},
static const KernelRow<2> kTinyKernels[] = {RT_TINY_VARIANTS};
#undef RT_V

// The launch grid over `rows` output rows and the frame's tile-dealing fields
// (tile_of_block); big: a big-list kernel (is_clustered), whose RT_OPT_XCD_DEAL
// modes other than 1 launch padded grids.
static void trace_grid(const rt_ctx* c, bool big, FrameDev& F, int width, int rows, dim3& grid, dim3& block)
{
    trace_dims(width, rows, grid, block);
    F.tiles_x = (int)grid.x;
    F.tiles_y = (int)grid.y;
    F.xcd_mode = 1;
    F.xcd_w = 0;
    F.xcd_m = 0;
    if (big && c->opt_xcd_deal != 1) {
        // the big-list kernels' padded grids (tile_of_block)
        F.xcd_mode = c->opt_xcd_deal;
        if (c->opt_xcd_deal == 2) {
            const unsigned sw = c->opt_xcd_stripe > 0 ? (unsigned)c->opt_xcd_stripe : (grid.x + kXcds - 1) / kXcds;
            F.xcd_w = (int)sw;
            F.xcd_m = (int)((grid.x + kXcds * sw - 1) / (kXcds * sw) * sw);
            grid = dim3(kXcds * (unsigned)F.xcd_m, grid.y);
        } else if (c->opt_xcd_deal == 3) {
            const unsigned gx = (grid.x + 3) / 4, gy = (grid.y + 1) / 2;
            const unsigned nst = (gx * gy + kXcds - 1) / kXcds * kXcds;  // super-tiles, a multiple of 8
            F.xcd_w = (int)gx;
            grid = dim3(8, nst);
        }
    }
}

// One trace launch of kernel kp over `rows` output rows (T: its records, when
// it is a launch-camera kernel).
static int launch_trace(rt_ctx* c, const KernelPick& kp, const TinyCam* T, SceneDev& S, FrameDev& F, int width,
                        int rows, unsigned* oa, float* ob, StatsDev* stats, hipStream_t st)
{
    dim3 grid, block;
    trace_grid(c, is_clustered(kp.v.flags), F, width, rows, grid, block);
    void* args[] = {&S, &F, &oa, &ob, &stats};
    TinyLaunch Lr;
    if (T) {
        // the launch record (rt_cull.h TinyLaunch): the frame's, the scene's
        // and the camera records' wave-uniform values, the one argument
        tiny_head_fill(Lr.h, F, S, *T, c->h_plane.data(),
                       c->d_lrec + (c->opt_lb_region ? 0 : kLightRec * S.n_lights), oa, ob, stats);
        std::memcpy(Lr.rec, T->rec, sizeof Lr.rec);
#if (RT_TILE_LEAN & 4) != 0
        // (both sets of light records have the same hot halves)
        lean_lights_fill(Lr.lights, reinterpret_cast<const float*>(c->h_lrec.data()),
                         c->h_lrec.size() == (size_t)kLightRec * S.n_lights ? S.n_lights : 0);
#endif
        args[0] = &Lr;
    }
    HIP_TRY(c, hipLaunchKernel(kp.k, grid, block, args, kp.lds, st));
    return RT_OK;
}

// Output rows of a launch: the slab, or this rank's band set.
static int frame_rows(const rt_frame* f)
{
    if (f->band_rows != 0) return std::max(0, (int)rt_band_rows(f->height, f->band_rows, f->band_count, f->band_index));
    return f->row_end - f->row_begin;
}

static void cb_key_of(const rt_frame* f, float* key)
{
    std::memcpy(key, f->cam_pos, 3 * sizeof(float));
    std::memcpy(key + 3, f->orient, 16 * sizeof(float));
    key[19] = f->half_w;
    key[20] = f->half_h;
    key[21] = f->inv_w;
    key[22] = f->inv_h;
    std::memcpy(key + 23, &f->width, sizeof(int));
    std::memcpy(key + 24, &f->height, sizeof(int));
    // the rows whose tiles have lists (a rank's slab or band set)
    const int32_t rows[5] = {f->band_rows ? 0 : f->row_begin, f->band_rows ? 0 : f->row_end, f->band_rows,
                             f->band_rows ? f->band_count : 0, f->band_rows ? f->band_index : 0};
    std::memcpy(key + 25, rows, sizeof rows);
}

static void frame_dev(const rt_frame* f, FrameDev& F)
{
    std::memcpy(F.cam, f->cam_pos, sizeof F.cam);
    std::memcpy(F.orient, f->orient, sizeof F.orient);
    F.half_w = f->half_w;
    F.half_h = f->half_h;
    F.inv_w = f->inv_w;
    F.inv_h = f->inv_h;
    std::memcpy(F.bg, f->background, sizeof F.bg);
    F.width = f->width;
    F.height = f->height;
    F.row_begin = f->row_begin;
    F.row_end = f->row_end;
    F.max_bounces = f->max_bounces;
    F.min_energy = f->min_energy;
    F.scene_ior = f->scene_ior;
    F.flags = f->flags;
    F.band_rows = f->band_rows;
    F.band_count = f->band_count;
    F.band_index = f->band_index;
    F.wf = WfDev{};
}

// Does frame f need the per-camera prepasses (the camera position moved
// from the one cam's records are for)?  A camera already prepared without
// every tricam record — a bounce frame of a big scene — is prepared again
// for the camera buffer.
static bool camera_needs_prepass(const rt_ctx* c, const rt_ctx::CamState& cam, const rt_frame* f, bool all_tricam)
{
    return c->n_tri > 0 && !(cam.valid && std::memcmp(cam.key, f->cam_pos, sizeof cam.key) == 0 &&
                             (!all_tricam || cam.tricam_all));
}

// The per-camera records of camera position cp into cam's buffers:
// camera-ray triangle values, camera cone records, union / cluster records.
static int camera_records(rt_ctx* c, rt_ctx::CamState& cam, const float* cp, hipStream_t st, bool all_tricam)
{
    float4* const cone_cam = cam.cone_cam;
    float4* tc = (all_tricam || c->n_tri <= kTricamMaxTriangles) ? cam.tricam : nullptr;
    if (cam.uni && c->n_clu == 0 && c->n_tri <= kCameraSmallMax) {  // small lists: one launch
        hipLaunchKernelGGL(rt_camera_small, dim3(1), dim3(256), 0, st, c->d_tri, c->d_trisph, c->d_trinrm,
                           c->d_tricoef, c->n_tri, cp[0], cp[1], cp[2], cone_cam, tc, cam.uni);
        HIP_TRY(c, hipGetLastError());
        return RT_OK;
    }
    hipLaunchKernelGGL(rt_cone_prepass, dim3((c->n_tri + 255) / 256), dim3(256), 0, st, c->d_tri, c->d_trisph,
                       c->d_trinrm, c->d_tricoef, c->n_tri, cp[0], cp[1], cp[2], 1, 0.0f, cone_cam, tc);
    HIP_TRY(c, hipGetLastError());
    if (cam.uni) {
        hipLaunchKernelGGL(rt_cluster_prepass, dim3(1), dim3(64), 0, st, cone_cam, c->n_tri, 1, cam.uni, c->n_tri);  // one wave
        HIP_TRY(c, hipGetLastError());
    }
    if (c->n_clu > 0) {
        float4* tmp = cam.clu_cam + 2 * (size_t)c->n_clu;  // second half: unsorted
        hipLaunchKernelGGL(rt_cluster_prepass, dim3(cluster_blocks(c->n_clu)), dim3(256), 0, st, cone_cam,
                           c->n_tri, c->n_clu, tmp, 64);
        HIP_TRY(c, hipGetLastError());
        hipLaunchKernelGGL(rt_cluster_sort, dim3(cluster_blocks(c->n_clu)), dim3(256), 0, st, tmp,
                           c->n_clu, cam.clu_cam);
        HIP_TRY(c, hipGetLastError());
    }
    return RT_OK;
}

// Per-camera prepasses (when the camera position moved) into cam, whose
// camera buffer they make stale.
static int camera_prepass(rt_ctx* c, rt_ctx::CamState& cam, const rt_frame* f, hipStream_t st, bool all_tricam)
{
    if (!camera_needs_prepass(c, cam, f, all_tricam)) return RT_OK;
    if (int rc = camera_records(c, cam, f->cam_pos, st, all_tricam)) return rc;
    std::memcpy(cam.key, f->cam_pos, sizeof cam.key);
    cam.valid = true;
    cam.tricam_all = all_tricam || c->n_tri <= kTricamMaxTriangles;
    cam.cb.valid = false;
    return RT_OK;
}

// The kernels' view of the scene, its camera-dependent fields from cam
// (cbuf: the launch walks cam's camera buffer).
static SceneDev scene_dev(const rt_ctx* c, const rt_ctx::CamState& cam, bool lbuf, bool cbuf)
{
    const int use_tricam = c->n_tri > 0 && c->n_tri <= kTricamMaxTriangles;
    return SceneDev{c->d_geom, c->d_mat, c->d_lights, c->d_tri, c->d_plane, c->d_quad, c->d_translucent, cam.tricam,
                    use_tricam, c->n_tri <= kEdgeMaxTriangles, cam.cone_cam, c->d_cone_light, cam.clu_cam,
                    c->d_clu_light, c->n_clu, c->n_surf, c->n_lights, c->n_tri, c->n_plane, c->n_quad,
                    c->n_tri_opaque, c->n_plane_opaque, c->n_quad_opaque, c->n_translucent, c->shadow_split,
                    lbuf ? c->lb_levels : 0, c->d_lb_off, c->d_lb_ent, c->d_lb_dcap, c->d_lb_meta,
                    (cam.uni && c->opt_union) ? cam.uni : nullptr,
                    cam.cb.off, cam.cb.ent, cam.cb.flag, cbuf ? cam.cb.tiles_x : 0,
                    cam.cb.inline_rec ? cam.cb.rec : nullptr, c->d_bvh_node, c->d_bvh_tri};
}

// The light buffer serves this context's shadow rays (RT_OPT_LIGHT_BUFFER).
static bool lbuf_on(const rt_ctx* c)
{
    const int mode = c->opt_light_buffer;
    return c->lb_ready && (mode == 1 || (mode == 2 && c->n_tri > kClusterMinTriangles));
}
// Bounce rays walk the BVH (rt_bvh.h) in the frame's kernel (the BVH kernels
// take their shadow rays through the light buffer).  k_max > 0: the scene can
// bounce — a BVH built for ray queries alone (RT_OPT_RAY_BVH) belongs to a
// scene whose frames never had one, whatever depth they ask for (a negative
// min_energy makes every depth reachable), and must not move them to the BVH
// kernels.
static bool bvh_on(const rt_ctx* c, int depth, bool lbuf)
{
    return depth > 0 && c->d_bvh_node && c->k_max > 0.0f && c->opt_bvh && lbuf && c->n_tri > 0;
}
// No refracted ray can pass its gate (Scene.cpp:1791: Kt * energy >
// min_energy with every Kt <= 0 and min_energy >= 0): the bounce tree of
// every pixel is a chain of reflections.
static bool reflect_chain(const rt_ctx* c, const rt_frame* f) { return !(c->kt_max > 0.0f) && f->min_energy >= 0.0f; }
// The frame's camera rays may walk a camera buffer: the depth-0 kernels and
// the BVH kernels.
static bool cam_lists(const rt_ctx* c, int depth, bool lbuf) { return depth == 0 || bvh_on(c, depth, lbuf); }

#include "rt_camhost.h"

// Make the per-camera state cam current for frame f, ordered on stream st
// (cam is the context's own: state_pending, ev_state and last_async_key
// order and remember that one): the camera prepass when the camera moved, and the camera buffer when the
// frame's kernel uses one and it is not current.  sync_path: a synchronous
// call on c->stream (fenced behind every async render at its start).
// Async (round 3: the camera buffer too, no host sync): a write fences st
// behind the other streams' renders and marks the state as written on st;
// otherwise st waits for a pending write made on another stream.
// Capturing: nothing may be written (an unprepared camera is RT_E_STATE; a
// prepared camera whose buffer is not current renders without it).
static int prepare_state(rt_ctx* c, rt_ctx::CamState& cam, const rt_frame* f, hipStream_t st, bool sync_path,
                         bool capturing, bool cb_want)
{
    if (capturing && c->state_pending && c->state_stream != st) {
        // a wait on an event recorded outside the capture cannot be captured
        c->err = "hipGraph capture: the camera state was written by an async render on another stream "
                 "(rt_sync or a synchronous render first)";
        return RT_E_STATE;
    }
    if (!sync_path && !capturing) {
        if (int rc = wait_state(c, st)) return rc;
    }
    if (!capturing) cb_harvest(cam.cb);
    const bool need_prep = camera_needs_prepass(c, cam, f, cb_want);
    // The camera buffer is built by a synchronous render, by an async frame
    // repeating the previous async frame's camera (round 4: a static camera
    // rendered async gets its lists at its second frame), and by a new
    // camera's async frame where the build pays (cb_async_pays).
    float key[30];
    cb_key_of(f, key);
    const bool repeat = !sync_path && c->last_async_valid && std::memcmp(key, c->last_async_key, sizeof key) == 0;
    if (!sync_path) {
        std::memcpy(c->last_async_key, key, sizeof key);
        c->last_async_valid = true;
    }
    const bool current = cb_matches(cam.cb, f) && !need_prep;
    const bool need_cb = cb_want && !current && (sync_path || repeat || cb_async_pays(c, f));
    if (capturing) {
        if (need_prep) {
            c->err = "hipGraph capture: the frame's camera is not prepared (rt_render or rt_prepare_camera first)";
            return RT_E_STATE;
        }
        return RT_OK;
    }
    if (!need_prep && !need_cb) return RT_OK;
    if (!sync_path) {
        if (int rc = fence_async(c, st)) return rc;
    }
    if (need_prep) {
        if (int rc = camera_prepass(c, cam, f, st, cb_want)) return rc;
    }
    if (need_cb) {
        const SceneDev S = scene_dev(c, cam, false, false);
        if (int rc = cb_build(c, cam.cb, f, S, st, sync_path, false, true)) return rc;
    }
    if (!sync_path) {
        HIP_TRY(c, hipEventRecord(c->ev_state, st));
        c->state_stream = st;
        c->state_pending = true;
    }
    return RT_OK;
}

// ---- wavefront bounce levels (rt_wavefront.h)
// Children one node can spawn (the gates compare K * energy > min_energy,
// Scene.cpp:1780,1791): with min_energy >= 0 a reflected ray needs some
// Kr > 0 and a refracted one some Kt > 0; a negative (or NaN) threshold is
// passed by K = 0 too, so every node may spawn both.
static int wf_branch(const rt_ctx* c, const rt_frame* f)
{
    if (!(f->min_energy >= 0.0f)) return 2;
    return (c->kr_max > 0.0f ? 1 : 0) + (c->kt_max > 0.0f ? 1 : 0);
}

#ifndef RT_WF_TRACE_WAVES
// trace launch: workgroups (one wave each) per CU.  Fewer than the 32 that
// fit (59 VGPRs, depth x 256 B of LDS) run faster: c3r 3.447 / 3.359 / 3.355
// / 3.338 ms at 32 / 24 / 20 / 16, c5r 21.23 / 21.16 / 21.26 / 21.59
// (profiles/r05/sorder/ab_trace_waves.log)
#define RT_WF_TRACE_WAVES 24
#endif
// Steps a lane's walk may take in the trace launch before the straggler
// launch finishes it with a whole wave.  Small levels (under
// RT_WF_BUDGET_SPLIT ray slots, ~2 rays per lane) are dominated by the trace
// launch's tail of long walks and hand off early; big ones (tens of rays
// per lane) hide that tail and keep more walks on the lanes.  Measured
// (profiles/r05/sorder/ab_budget.log): c3r (2.1 M slots) 2.944 / 2.973 /
// 2.983 ms at 128 / 112 / 160; c5r (33 M) 19.17 / 18.97 / 18.97 at 256 /
// 320 / 384.
#ifndef RT_WF_BUDGET_SMALL
#define RT_WF_BUDGET_SMALL 128
#endif
#ifndef RT_WF_BUDGET_BIG
#define RT_WF_BUDGET_BIG 320
#endif
#ifndef RT_WF_BUDGET_SPLIT
#define RT_WF_BUDGET_SPLIT (6u << 20)
#endif
#ifndef RT_WF_STRAG_WAVES
// straggler launch: workgroups (one wave, one straggling ray at a time, its
// kWfStragCap-entry LDS stack) per CU: 4 / 8 / 16 waves of 16 / 16 / 8 KB,
// c3r 3.359 / 3.273 / 3.249 ms, c5r 21.13 / 19.80 / 19.19
// (profiles/r05/sorder/ab_straggle*.log); round 6, with the sorted levels:
// 32 waves of 4 KB against 16 of 8 KB, c3r 2.862 / 2.887, c5r 17.65 / 17.77
// (profiles/r06/knobs/)
#define RT_WF_STRAG_WAVES 32
#endif
#ifndef RT_WF_FOLD_BLOCKS
#define RT_WF_FOLD_BLOCKS 64  // fold launch: 256-thread blocks per CU (4: c5r +0.5%, profiles/r06/knobs2/)
#endif
#ifndef RT_WF_SHADE_WAVES
#define RT_WF_SHADE_WAVES 24  // shade launch: workgroups (one wave each) per CU (= its occupancy)
#endif
#ifndef RT_WF_SORT
// each level's rays sorted by their parent surface's bin (BVH leaf order)
// and branch before its trace (rt_wf_sort_*), for frames whose level-1
// queue holds at least this many ray slots (0: every wavefront frame).
// Round 5's hipcub radix sort ran over the queue's capacity (+6% at c3r,
// -6% at c5r, profiles/r05/wfsort/); the counting sort reads only the
// level's live rays.
#define RT_WF_SORT 0
#endif
#ifndef RT_WF_MAX_GB
#define RT_WF_MAX_GB 32.0
#endif
// The queues' layout for a frame of `tiles` level-0 tiles (one wave each)
// over px pixels, `levels` bounce levels, `branch` children per node at most
// (rt_layout.h WfDev): segment capacities that no wave's appends can
// overflow — segment s of level L + 1 receives the children of level L's
// chunks c = s (mod kWfSeg), at most 64 * branch each — then the bytes:
// counters; level-0 node records (32 B) per pixel and its parent list;
// per level L >= 1 the rays (32 B), colours (16 B) and, but for the deepest
// level, node records (32 B) and the parent list; the hit records (8 B),
// straggler queue (16 B) and stragglers' minima (8 B) of the largest level.
struct WfLayout {
    size_t cap[kWfMaxLevels + 1] = {}, pcap[kWfMaxLevels + 1] = {};
    unsigned seg[kWfMaxLevels + 1] = {}, pseg[kWfMaxLevels + 1] = {};
    size_t most = 0, bytes = 0;
};
static WfLayout wf_layout(size_t tiles, size_t px, int levels, int branch)
{
    WfLayout w;
    auto up = [](size_t a, size_t b) { return (a + b - 1) / b; };
    size_t chunks = tiles;
    for (int L = 0; L <= levels; ++L) {
        if (L > 0) {
            w.seg[L] = (unsigned)(up(chunks, kWfSeg) * 64 * (size_t)branch);
            w.cap[L] = (size_t)kWfSeg * w.seg[L];
            chunks = up(w.cap[L], 64);
            w.most = std::max(w.most, w.cap[L]);
        }
        if (L < levels) {
            w.pseg[L] = (unsigned)(up(chunks, kWfSeg) * 64);
            w.pcap[L] = (size_t)kWfSeg * w.pseg[L];
        }
    }
    auto a = [](size_t x) { return (x + 255) & ~(size_t)255; };
    size_t tot = a(kWfCountBytes) + a(px * 32) + a(w.pcap[0] * 4);
    for (int L = 1; L <= levels; ++L) {
        tot += a(w.cap[L] * 32) + a(w.cap[L] * 16);
        if (L < levels) tot += a(w.cap[L] * 32) + a(w.pcap[L] * 4);
    }
    w.bytes = tot + a(w.most * 8) + a(w.most * 16) + a(w.most * 8);  // hit, strag, hit2
    return w;
}

static size_t frame_tiles(const rt_frame* f, int rows) { return (size_t)((f->width + 7) / 8) * (size_t)((rows + 7) / 8); }

// Would frame f (depth `depth`, its kernel a BVH kernel) render as a
// wavefront?  RT_OPT_WAVEFRONT, at most kWfMaxLevels levels, a single
// output chunk, queues within RT_WF_MAX_GB.
static bool wf_fits(const rt_ctx* c, const rt_frame* f, int depth, int rows)
{
    if (!c->opt_wavefront || depth < 1 || depth > kWfMaxLevels || wf_branch(c, f) == 0) return false;
    const WfLayout w = wf_layout(frame_tiles(f, rows), (size_t)rows * f->width, depth, wf_branch(c, f));
    return (double)w.bytes <= RT_WF_MAX_GB * 1073741824.0;
}

// The queues for frame f (grown, never shrunk; not while capturing).
// Fills c->wf.dev.
static int wf_ensure(rt_ctx* c, const rt_frame* f, int rows, int levels, bool capturing, bool* ok)
{
    rt_ctx::WfBuf& W = c->wf;
    const size_t px = (size_t)rows * f->width;
    const WfLayout w = wf_layout(frame_tiles(f, rows), px, levels, wf_branch(c, f));
    *ok = false;
    if (w.bytes > W.bytes) {
        if (capturing) return RT_OK;  // (the frame renders by the BVH megakernel)
        free_later(c, W.mem);  // an enqueued frame may still use the old queues
        W.mem = nullptr;
        W.bytes = 0;
        HIP_TRY(c, hipMalloc(&W.mem, w.bytes));
        W.bytes = w.bytes;
    }
    char* p = (char*)W.mem;
    auto take = [&](size_t bytes) {
        char* q = p;
        p += (bytes + 255) & ~(size_t)255;
        return q;
    };
    WfDev& d = W.dev;
    d = WfDev{};
    d.count = (unsigned*)take(kWfCountBytes);
    d.node[0] = (float4*)take(px * 32);
    d.plist[0] = (unsigned*)take(w.pcap[0] * 4);
    d.pseg[0] = w.pseg[0];
    for (int L = 1; L <= levels; ++L) {
        d.ray[L] = (float4*)take(w.cap[L] * 32);
        d.res[L] = (float4*)take(w.cap[L] * 16);
        d.seg[L] = w.seg[L];
        if (L < levels) {
            d.node[L] = (float4*)take(w.cap[L] * 32);
            d.plist[L] = (unsigned*)take(w.pcap[L] * 4);
            d.pseg[L] = w.pseg[L];
        }
    }
    d.hit = (float2*)take(w.most * 8);
    d.strag = (int4*)take(w.most * 16);
    d.hit2 = (float2*)take(w.most * 8);
    d.levels = levels;
    d.kin = nullptr;
    d.kout = nullptr;
    d.skey = c->d_skey;
    d.hist = nullptr;
    d.nbin_half = c->nbin_half;
    W.sort = 0;
    if (c->d_skey && c->opt_wf_sort && levels >= 1 && w.cap[1] >= (size_t)RT_WF_SORT) {
        if (w.most > W.kcap) {
            free_later(c, W.kin);
            free_later(c, W.kout);
            free_later(c, W.kout2);
            W.kin = W.kout = W.kout2 = nullptr;
            W.kcap = 0;
            HIP_TRY(c, hipMalloc((void**)&W.kin, w.most * sizeof(unsigned)));
            HIP_TRY(c, hipMalloc((void**)&W.kout, w.most * sizeof(unsigned)));
            HIP_TRY(c, hipMalloc((void**)&W.kout2, w.most * sizeof(unsigned)));
            W.kcap = w.most;
        }
        // (the hit sort's bins: nbin_half + kWfMissBins)
        size_t bins = std::max(2 * (size_t)c->nbin_half, (size_t)c->nbin_half + kWfMissBins);
        if ((c->opt_wf_sort & 4) && c->lb_r0 > 0)  // the light-cell hit sort's bins
            bins = std::max(bins, 6 * (size_t)c->lb_r0 * (size_t)c->lb_r0 + kWfMissBins);
        if (bins + 1 > W.hcap) {
            free_later(c, W.hist);
            free_later(c, W.bsum);
            W.hist = nullptr;
            W.bsum = nullptr;
            W.hcap = 0;
            // the parent counts (hist), the hit counts, the scan's positions
            // (next): bins + 1 words each
            HIP_TRY(c, hipMalloc((void**)&W.hist, 3 * (bins + 1) * sizeof(unsigned)));
            HIP_TRY(c, hipMalloc((void**)&W.bsum, scan_scratch(bins) * sizeof(unsigned long long)));
            W.hcap = bins + 1;
        }
        W.sort = c->opt_wf_sort;
        if (W.sort & 1) d.kin = W.kin;
        d.hist = W.hist;
    }
    for (int L = 0; L <= levels; ++L) {
        W.cap[L] = L == 0 ? px : w.cap[L];
        W.pcap[L] = w.pcap[L];
    }
    W.px = px;
    *ok = true;
    return RT_OK;
}

// The shading kernels of the wavefront's bounce levels; k[0] counts
// (RT_FLAG_STATS), k[1] is the timed one.  STRAG: the stragglers' launch.
#define RT_V(M, L, F)                                                                                        \
    {{M, L, F},                                                                                              \
     {(const void*)&rt_wf_shade<F, true, STRAG>, (const void*)&rt_wf_shade<F, false, STRAG>},                \
     kernel_name("rt_wf_shade", F)},
template <bool STRAG>
static const KernelRow<2> kWfShadeKernels[] = {RT_WF_SHADE_VARIANTS};
#undef RT_V

// The bounce levels and folds of a wavefront frame, after level 0 on st:
// per level a trace launch (the BVH walk; LDS = its stack) and a shade
// launch (LDS = the light-buffer staging window), then the folds.
static int wf_levels(rt_ctx* c, const SceneDev& S, const FrameDev& F, int levels, bool count, unsigned* rgba,
                     float* rgbf, StatsDev* stats, hipStream_t st)
{
    const void* kt = count ? (const void*)&rt_wf_trace<true> : (const void*)&rt_wf_trace<false>;
    const void* kg = count ? (const void*)&rt_wf_straggle<true> : (const void*)&rt_wf_straggle<false>;
    Facts fa;
    fa.wf_shade = true;
    fa.n_tri = c->n_tri;
    fa.small = c->opt_lb_unroll && small_frame((double)c->wf.px);
    const Variant vs = select_variant(fa);
    const void* ks = find_row(kWfShadeKernels<false>, vs)->k[!count];  // (the row exists: KernelRow)
    // (RT_OPT_WF_OVERLAP: the stragglers' walks and shading on a second
    // stream, beside the level's main shade launch)
    const void* ks2 = find_row(kWfShadeKernels<true>, vs)->k[!count];
    const unsigned lds_t = (unsigned)((size_t)c->bvh_depth * 64 * sizeof(int));
    const unsigned lds_s = lds_bytes(vs.flags, 0);
    rt_ctx::WfBuf& W = c->wf;
    const bool ovl = c->opt_wf_overlap;
    if (ovl) {
        if (!W.st2) HIP_TRY(c, hipStreamCreateWithFlags(&W.st2, hipStreamNonBlocking));
        if (!W.ev_t) HIP_TRY(c, hipEventCreateWithFlags(&W.ev_t, hipEventDisableTiming));
        if (!W.ev_s) HIP_TRY(c, hipEventCreateWithFlags(&W.ev_s, hipEventDisableTiming));
    }
    for (int L = 1; L <= levels; ++L) {
        // enough waves to fill the chip; each strides over the level's queue
        const size_t waves = (W.cap[L] + 63) / 64;
        const unsigned gt = (unsigned)std::max<size_t>(1, std::min<size_t>(waves, (size_t)c->n_cu * RT_WF_TRACE_WAVES));
        const unsigned gs = (unsigned)std::max<size_t>(1, std::min<size_t>(waves, (size_t)c->n_cu * RT_WF_SHADE_WAVES));
        FrameDev Fl = F;
        Fl.wf.budget = W.cap[L] >= (size_t)RT_WF_BUDGET_SPLIT ? RT_WF_BUDGET_BIG : RT_WF_BUDGET_SMALL;
        if (!ovl) Fl.wf.hit2 = nullptr;
        const unsigned gq = (unsigned)std::max<size_t>(1, std::min<size_t>(waves, (size_t)c->n_cu * 32));
        if (W.dev.kin) {
            // the level's live rays by bin (parent surface in BVH leaf order,
            // branch): rays leaving one triangle share its normal, rays of
            // neighbouring triangles their subtree, so their walks and hits
            // stay together
            // (the counts came with the appends; the scan leaves them zero
            // for the next level's)
            const unsigned bins = 2u * c->nbin_half;
            unsigned* next = W.hist + 2 * W.hcap;
            HIP_TRY(c, scan_u32(W.hist, bins, next, W.bsum, st, nullptr, true));
            hipLaunchKernelGGL(rt_wf_sort_place<0>, dim3(gq), dim3(64), 0, st, S, F, L, (const unsigned*)nullptr, next,
                               W.kout);
            HIP_TRY(c, hipGetLastError());
            Fl.wf.kout = W.kout;
        }
        int Lv = L;
        void* args[] = {(void*)&S, (void*)&Fl, (void*)&Lv, (void*)&stats};
        HIP_TRY(c, hipLaunchKernel(kt, dim3(gt), dim3(64), args, lds_t, st));
        if (!ovl)
            HIP_TRY(c, hipLaunchKernel(kg, dim3((unsigned)c->n_cu * RT_WF_STRAG_WAVES), dim3(64), args,
                                       (unsigned)(kWfStragCap * sizeof(int)), st));
        FrameDev Fs = Fl;
        if (W.sort & 2) {
            // the level's rays by hit surface's bin for the shading (whose
            // children, appended in that order, then sit by parent bin)
            // (bit 2: by the hit point's light-buffer cell instead, wf_sort_key<2>)
            const bool cell = (W.sort & 4) != 0 && c->lb_r0 > 0;
            const unsigned hb = cell ? 6u * (unsigned)c->lb_r0 * (unsigned)c->lb_r0 + kWfMissBins
                                     : c->nbin_half + kWfMissBins;
            unsigned *hist2 = W.hist + W.hcap, *next = W.hist + 2 * W.hcap;
            // (both passes read the rays in queue order: consecutive slots,
            // coalesced hit records — the order inside a bin does not matter)
            if (cell)
                hipLaunchKernelGGL(rt_wf_hit_count<2>, dim3(gq), dim3(64), 0, st, S, F, L, (const unsigned*)nullptr,
                                   hist2);
            else
                hipLaunchKernelGGL(rt_wf_hit_count<1>, dim3(gq), dim3(64), 0, st, S, F, L, (const unsigned*)nullptr,
                                   hist2);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, scan_u32(hist2, hb, next, W.bsum, st, nullptr, true));
            if (cell)
                hipLaunchKernelGGL(rt_wf_sort_place<2>, dim3(gq), dim3(64), 0, st, S, F, L, (const unsigned*)nullptr,
                                   next, W.kout2);
            else
                hipLaunchKernelGGL(rt_wf_sort_place<1>, dim3(gq), dim3(64), 0, st, S, F, L, (const unsigned*)nullptr,
                                   next, W.kout2);
            HIP_TRY(c, hipGetLastError());
            Fs.wf.kout = W.kout2;
        }
        void* sargs[] = {(void*)&S, (void*)&Fs, (void*)&Lv, (void*)&stats};
        if (ovl) {
            // fork: the stragglers finish their walks (into hit2) and are
            // shaded on st2 while st shades the level's other rays; join
            // before the next level reads its queue
            HIP_TRY(c, hipEventRecord(W.ev_t, st));
            HIP_TRY(c, hipStreamWaitEvent(W.st2, W.ev_t, 0));
            HIP_TRY(c, hipLaunchKernel(kg, dim3((unsigned)c->n_cu * RT_WF_STRAG_WAVES), dim3(64), args,
                                       (unsigned)(kWfStragCap * sizeof(int)), W.st2));
            HIP_TRY(c, hipLaunchKernel(ks2, dim3(gs), dim3(64), sargs, lds_s, W.st2));
            HIP_TRY(c, hipEventRecord(W.ev_s, W.st2));
        }
        HIP_TRY(c, hipLaunchKernel(ks, dim3(gs), dim3(64), sargs, lds_s, st));
        if (ovl) HIP_TRY(c, hipStreamWaitEvent(st, W.ev_s, 0));
    }
    for (int L = levels - 1; L >= 0; --L) {
        const unsigned g = (unsigned)std::min<size_t>((c->wf.pcap[L] + 255) / 256, (size_t)c->n_cu * RT_WF_FOLD_BLOCKS);
        hipLaunchKernelGGL(rt_wf_fold, dim3(std::max(1u, g)), dim3(256), 0, st, F, L, rgba, rgbf);
        HIP_TRY(c, hipGetLastError());
    }
    return RT_OK;
}

// ---- supersampled renders (rt.h rt_render_ss*, rt_resolve.h)
// Output rows of (frame, s); -1 if the pair is invalid.
static int ss_rows_of(const rt_frame* f, int s)
{
    if (!f || s < 1 || s > kSsMax || !frame_ok(f)) return -1;
    if (f->width % s != 0 || f->height % s != 0) return -1;
    if (f->band_rows != 0) {
        if (f->band_rows % (16 * s) != 0) return -1;
    } else if (f->row_begin % s != 0 || f->row_end % s != 0) {
        return -1;
    }
    return frame_rows(f) / s;
}

// The sample rows a render of f writes, of its `rows` packed rows: all of a
// slab; of a band set the rows inside the frame (only the frame's last band
// can reach past it, and it is the last of its rank's packed bands).
static int ss_valid_rows(const rt_frame* f, int rows)
{
    if (f->band_rows == 0) return rows;
    int v = 0;
    for (int b = 0; b < rows / f->band_rows; ++b) {
        const long long y0 = ((long long)b * f->band_count + f->band_index) * f->band_rows;
        v += (int)std::max(0LL, std::min<long long>(f->band_rows, f->height - y0));
    }
    return v;
}

template <int S>
static const void* resolve_kernel(bool vec)
{
    return vec ? (const void*)&rt_resolve_kernel<S, true> : (const void*)&rt_resolve_kernel<S, false>;
}

// rows_out output rows of width / s pixels from their s rows_out packed
// sample rows at `samples`, on st.
static int launch_resolve(rt_ctx* c, const float* samples, int width, int s, int rows_out, float* rgb, unsigned* rgba,
                          hipStream_t st)
{
    if (rows_out <= 0) return RT_OK;
    int wo = width / s;
    const bool vec = width % 4 == 0 && ((uintptr_t)samples & 15) == 0;
    const void* k = nullptr;
    switch (s) {
    case 2: k = resolve_kernel<2>(vec); break;
    case 3: k = resolve_kernel<3>(vec); break;
    case 4: k = resolve_kernel<4>(vec); break;
    case 5: k = resolve_kernel<5>(vec); break;
    case 6: k = resolve_kernel<6>(vec); break;
    case 7: k = resolve_kernel<7>(vec); break;
    case 8: k = resolve_kernel<8>(vec); break;
    default: c->err = "no resolve kernel for this factor"; return RT_E_ARG;
    }
    const size_t lanes = (size_t)(wo / (vec ? resolve_run(s) : 1)) * (size_t)rows_out;
    void* args[] = {&samples, &width, &wo, &rows_out, &rgb, &rgba};
    HIP_TRY(c, hipLaunchKernel(k, dim3((unsigned)((lanes + 255) / 256)), dim3(256), args, 0, st));
    return RT_OK;
}

// ---- entry checks: each sets the error string and returns the code, or RT_OK
// (every entry point keeps its own order of them)
static int needs_cpu(rt_ctx* c, const char* entry)
{
    c->err = std::string(entry) + " needs a CPU context (rt_create_cpu)";
    return RT_E_STATE;
}
static int check_uploaded(rt_ctx* c, const char* what = "render")
{
    if (c->uploaded) return RT_OK;
    c->err = std::string(what) + " before rt_upload_scene";
    return RT_E_STATE;
}
static int check_frame(rt_ctx* c, const rt_frame* f)
{
    if (frame_ok(f)) return RT_OK;
    c->err = "bad rt_frame geometry";
    return RT_E_ARG;
}
// Is st being captured into a hipGraph?
static int stream_capturing(rt_ctx* c, hipStream_t st, bool* capturing)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    HIP_TRY(c, hipStreamIsCapturing(st, &cs));
    *capturing = cs != hipStreamCaptureStatusNone;
    return RT_OK;
}

// ---- the trace kernels (rt_variant.h: what a variant is, which one a frame
// takes, and the lists of the compiled ones)
// COUNT: the kernels that also tally the tests executed (the RT_FLAG_STATS
// launch).  It is the tables' parameter, and level 0 of the wavefront has a
// table of its own, because the code object holds its kernels in the order
// in which they are first named here: level 0 counted, timed, then the
// frames' counted, timed.
#define RT_V(M, L, F) \
    {{M, L, F}, {(const void*)&rt_trace_kernel<M, L, F, COUNT>}, kernel_name("rt_trace_kernel", M, L, F)},
template <bool COUNT>
static const KernelRow<1> kWf0Kernels[] = {RT_TRACE_WF0_VARIANTS};
template <bool COUNT>
static const KernelRow<1> kFrameKernels[] = {RT_TRACE_FRAME_VARIANTS};
#undef RT_V

// The facts of frame f that every colour path shares; the caller adds its own
// (small, wf0, tiny).
static Facts frame_facts(const rt_ctx* c, const rt_frame* f, int depth, bool lbuf, bool cbuf, bool bvh)
{
    Facts a;
    a.depth = depth;
    a.n_tri = c->n_tri;
    a.n_lights = c->n_lights;
    a.lbuf = lbuf;
    a.cbuf = cbuf;
    a.bvh_depth = bvh ? c->bvh_depth : 0;
    a.chain = reflect_chain(c, f);
    return a;
}

// The colour kernel of a frame: the selected variant's row (k == nullptr:
// the reachable depth exceeds the compiled stacks).
static KernelPick pick_kernel(const Facts& a, bool count)
{
    KernelPick p;
    p.v = select_variant(a);
    if (is_tiny(p.v.flags)) {
        const KernelRow<2>* r = find_row(kTinyKernels, p.v);  // (the row exists: KernelRow)
        p.k = r->k[count];
        p.name = &r->name;
        return p;
    }
    const KernelRow<1>* r = is_wf0(p.v.flags)
                                ? (count ? find_row(kWf0Kernels<true>, p.v) : find_row(kWf0Kernels<false>, p.v))
                                : (count ? find_row(kFrameKernels<true>, p.v) : find_row(kFrameKernels<false>, p.v));
    if (!r) return p;
    p.k = r->k[0];
    p.name = &r->name;
    p.lds = lds_bytes(p.v.flags, a.bvh_depth);
    return p;
}

// ---- a colour frame: plan_frame decides, launch enqueues what was decided.
// The plan of one frame: its kernel and that kernel's arguments, and its
// packed rows as chunks [r0, r0 + step) — step == rows: one chunk
// (rt_chunks.h).  A new render mode is a field here and a step of launch's
// loop, not another copy of the loop.
struct FramePlan {
    int depth, rows, step;
    int tmode;  // tiny: the tile masks, 0 read, 1 computed by the kernel, 2 computed and stored (tiny_masks)
    bool lbuf, bvh, cbuf, wf;
    bool tiny;       // the launch-camera kernel (T: its records, no device state)
    bool ss_staged;  // supersampled: the chunks render into c->ss and are resolved from there
    KernelPick kp;
    TinyCam T;
    SceneDev S;
    FrameDev F;
};

// The second half of every colour frame's plan.  The caller has decided
// P.depth, lbuf, bvh, tiny, tmode, cbuf and wf by its own rules; from them,
// the camera state the kernel reads and the caller's own fact `small`
// (Facts::small): the kernel and its arguments, P.kp, P.S and P.F.
static int plan_kernel(rt_ctx* c, const rt_frame* f, const rt_ctx::CamState& cam, bool small, FramePlan& P)
{
    Facts fa = frame_facts(c, f, P.depth, P.lbuf, P.cbuf, P.bvh);
    fa.small = small;
    fa.wf0 = P.wf;
    fa.tiny = P.tiny ? P.tmode : -1;
    P.kp = pick_kernel(fa, (f->flags & RT_FLAG_STATS) != 0);
    if (!P.kp.k) {
        c->err = "reachable bounce depth " + std::to_string(P.depth) + " exceeds the compiled stack (32)";
        return RT_E_UNSUPPORTED;
    }
    P.S = scene_dev(c, cam, P.lbuf, P.cbuf);
    frame_dev(f, P.F);
    if (P.wf) P.F.wf = c->wf.dev;
    return RT_OK;
}

// Plans frame f of the context's camera for stream st, into P (filled in
// place: TinyCam and SceneDev are large).  What the plan needs on the device
// is enqueued or allocated here: the tile masks' buffer, the per-camera
// state, the wavefront queues, the sample intermediate.  Fills c->last.
// ss > 1: a supersampled render — the samples go to c->ss, one chunk at a
// time; px_bytes, host_out: the output's bytes per pixel and whether launch
// copies it to the host (rt_chunks.h).
static int plan_frame(rt_ctx* c, const rt_frame* f, hipStream_t st, bool sync_path, bool capturing, int px_bytes,
                      bool host_out, int ss, FramePlan& P)
{
    const int depth = P.depth = reachable_depth(c, f);
    const bool lbuf = P.lbuf = lbuf_on(c);
    const bool bvh = P.bvh = bvh_on(c, depth, lbuf);
    const bool cb_want = cb_wanted(c, f, depth, lbuf);
    const int rows = P.rows = frame_rows(f);
    // tiny scenes: the camera records travel with the launch (no device state)
    P.tmode = 0;
    P.tiny = tiny_ok(c, depth, lbuf);
    if (P.tiny) {
        P.T = tiny_prepare(c, f);
        if (rows > 0)
            if (int rc = tiny_masks(c, f, st, capturing, P.T, &P.tmode)) return rc;
    }
    if (rows > 0 && !P.tiny) {
        if (int rc = prepare_state(c, c->cam, f, st, sync_path, capturing, cb_want)) return rc;
    }
    P.cbuf = !P.tiny && cb_want && cb_matches(c->cam.cb, f);
    // Wavefront: a BVH frame's bounce levels as compacted queues (rt_wavefront.h);
    // its queues are shared by the context's streams: a frame on another
    // stream than the last wavefront frame waits for that one.  A captured
    // frame renders by the BVH megakernel instead (no shared state).
    bool wf = bvh && rows > 0 && !capturing && wf_fits(c, f, depth, rows);
    if (wf) {
        bool ok = false;
        if (int rc = wf_ensure(c, f, rows, depth, capturing, &ok)) return rc;
        wf = ok;
    }
    P.wf = wf;
    // A supersampled frame's samples: slabs that are not wavefronts in row
    // chunks (the intermediate holds one chunk), everything else whole.
    P.ss_staged = ss > 1;
    P.step = row_chunk_step(f->width, rows, f->band_rows, px_bytes, ss, wf, host_out, c->opt_host_chunk_mb,
                            c->opt_ss_chunk_rows);
    // tiny is depth 0, a wavefront BVH depth above 0; a wavefront is one
    // chunk; a supersampled call's caller copies the resolved image itself
    assert(!(P.tiny && wf) && (!wf || P.step == rows) && !(P.ss_staged && host_out));
    if (P.ss_staged && rows > 0) {
        rt_ctx::SsBuf& B = c->ss;
        const size_t need = (size_t)P.step * f->width * 12;
        if (need > B.bytes) {
            if (capturing) {
                c->err = "rt_render_ss_async in a capture: the sample intermediate is not sized (render the frame "
                         "once outside the capture)";
                return RT_E_STATE;
            }
            free_later(c, B.mem);  // an enqueued resolve may still read the old one
            B.mem = nullptr;
            B.bytes = 0;
            HIP_TRY(c, hipMalloc((void**)&B.mem, need));
            B.bytes = need;
        }
    }
    if (int rc = plan_kernel(c, f, c->cam, small_frame((double)f->width * rows) && c->opt_lb_unroll, P)) return rc;
    const KernelPick& kp = P.kp;
    c->last = rt_stats{};
    c->last.stack_depth = wf ? depth : kp.v.maxd;
    c->last.light_batch = kp.v.lb;
    static_assert(sizeof c->last.kernel >= sizeof kp.name->s, "rt_stats.kernel holds a kernel's name");
    if (wf)
        std::snprintf(c->last.kernel, sizeof c->last.kernel, "wavefront %s + %d levels", kp.name->s, depth);
    else
        std::memcpy(c->last.kernel, kp.name->s, sizeof kp.name->s);
    return RT_OK;
}

// One colour frame on st.  sync_path: rt_render / rt_render_float /
// rt_render_ss* on c->stream; else rt_render_async / rt_render_ss_async on
// the caller's stream (both build the camera buffer when it is not current).
// rgba_dev / rgb_dev take the image (ss > 1: the resolved width / ss x
// rows / ss one).  host_out (synchronous renders into host memory, ss == 1):
// the image is copied there, one copy on st, or — a slab in chunks — chunk
// i's copy on c->copy_stream overlapping chunk i + 1's kernel.
static int launch(rt_ctx* c, const rt_frame* f, unsigned* rgba_dev, float* rgb_dev, hipStream_t st, bool timed,
                  bool sync_path, void* host_out = nullptr, int ss = 1)
{
    if (!c || !f) return RT_E_ARG;
    if (int rc = check_uploaded(c)) return rc;
    if (int rc = check_frame(c, f)) return rc;
    bool capturing = false;
    if (!sync_path)
        if (int rc = stream_capturing(c, st, &capturing)) return rc;
    const size_t px_bytes = rgba_dev ? 4 : 12;
    FramePlan P;
    if (int rc = plan_frame(c, f, st, sync_path, capturing, (int)px_bytes, host_out != nullptr, ss, P)) return rc;
    const int rows = P.rows, step = P.step;
    if (rows == 0) return RT_OK;
    const bool count = (f->flags & RT_FLAG_STATS) != 0;
    if (count) HIP_TRY(c, hipMemsetAsync(c->d_stats, 0, kStatSlots * sizeof(StatsDev), st));
    if (timed) HIP_TRY(c, hipEventRecord(c->ev0, st));
    StatsDev* stats = c->d_stats;
    if (P.wf) {
        rt_ctx::WfBuf& W = c->wf;
        if (int rc = W.turn.enter(c, st)) return rc;
        HIP_TRY(c, hipMemsetAsync(W.dev.count, 0, kWfCountBytes, st));
        if (W.sort)  // the bin counts (level 1's: the level-0 kernel's appends)
            HIP_TRY(c, hipMemsetAsync(W.dev.hist, 0, 2 * W.hcap * sizeof(unsigned), st));
    }
    rt_ctx::SsBuf& B = c->ss;
    if (P.ss_staged && !capturing)
        if (int rc = B.turn.enter(c, st)) return rc;
    // every chunk's kernel first, then the copies (a copy into pageable
    // memory blocks the host; the kernels behind it keep running)
    const bool host_chunked = host_out && step < rows;
    const int wo = f->width / ss, vrows = ss_valid_rows(f, rows);
    int n = 0;
    for (int r0 = 0; r0 < rows; r0 += step, ++n) {
        const int r1 = std::min(rows, r0 + step);
        FrameDev Fc, *F = &P.F;
        if (step < rows) {
            Fc = P.F;
            Fc.row_begin = f->row_begin + r0;
            Fc.row_end = f->row_begin + r1;
            F = &Fc;
        }
        unsigned* oa = P.ss_staged ? nullptr : (rgba_dev ? rgba_dev + (size_t)r0 * f->width : nullptr);
        float* ob = P.ss_staged ? B.mem : (rgb_dev ? rgb_dev + (size_t)r0 * f->width * 3 : nullptr);
        if (int rc = launch_trace(c, P.kp, P.tiny ? &P.T : nullptr, P.S, *F, f->width, r1 - r0, oa, ob, stats, st))
            return rc;
        if (P.wf) {  // (one chunk)
            if (int rc = wf_levels(c, P.S, *F, P.depth, count, oa, ob, stats, st)) return rc;
            if (int rc = c->wf.turn.leave(c, st)) return rc;
        }
        if (P.ss_staged) {  // the chunk's rows inside the frame
            const int q0 = r0 / ss, nq = (std::max(r0, std::min(r1, vrows)) - r0) / ss;
            if (int rc = launch_resolve(c, B.mem, f->width, ss, nq, rgb_dev ? rgb_dev + (size_t)q0 * wo * 3 : nullptr,
                                        rgba_dev ? rgba_dev + (size_t)q0 * wo : nullptr, st))
                return rc;
        }
        if (host_chunked) {
            assert(n < 8);
            HIP_TRY(c, hipEventRecord(c->ev_chunk[n], st));
        }
    }
    if (P.tmode == 2)
        if (int rc = tiny_masks_stored(c, st)) return rc;
    if (P.ss_staged && !capturing)
        if (int rc = B.turn.leave(c, st)) return rc;
    const char* src = (const char*)(rgba_dev ? (void*)rgba_dev : (void*)rgb_dev);
    if (host_chunked) {
        if (timed) HIP_TRY(c, hipEventRecord(c->ev1, st));
        timed = false;  // ev1: after the last kernel, before the copies
        for (int i = 0; i < n; ++i) {
            const int r0 = i * step, r1 = std::min(rows, r0 + step);
            const size_t off = (size_t)r0 * f->width * px_bytes;
            HIP_TRY(c, hipStreamWaitEvent(c->copy_stream, c->ev_chunk[i], 0));
            HIP_TRY(c, hipMemcpyAsync((char*)host_out + off, src + off, (size_t)(r1 - r0) * f->width * px_bytes,
                                      hipMemcpyDeviceToHost, c->copy_stream));
        }
    } else if (host_out) {
        HIP_TRY(c, hipMemcpyAsync(host_out, src, (size_t)rows * f->width * px_bytes, hipMemcpyDeviceToHost, st));
    }
    if (timed) HIP_TRY(c, hipEventRecord(c->ev1, st));
    if (!sync_path) enqueued(c, st, capturing, P.cbuf ? &c->cam.cb : nullptr);
    return RT_OK;
}

static int finish_sync(rt_ctx* c, const rt_frame* f, hipStream_t st, bool timed)
{
    HIP_TRY(c, hipStreamSynchronize(st));
    HIP_TRY(c, hipStreamSynchronize(c->copy_stream));
    // c->stream waited for every async render enqueued before this call
    // (fence_async), so none is in flight any more
    settled(c);
    if (timed) {
        float ms = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
        c->last.kernel_ms = ms;
    }
    if (f->flags & RT_FLAG_STATS) {
        std::vector<StatsDev> slots(kStatSlots);
        HIP_TRY(c, hipMemcpy(slots.data(), c->d_stats, kStatSlots * sizeof(StatsDev), hipMemcpyDeviceToHost));
        StatsDev h{};
        for (const StatsDev& q : slots) {
            h.primary += q.primary;
            h.bounce += q.bounce;
            h.shadow += q.shadow;
            h.skipped += q.skipped;
            h.tri += q.tri;
            h.pla += q.pla;
            h.qua += q.qua;
            h.btri += q.btri;
            h.bnode += q.bnode;
        }
        c->last.primary_rays = h.primary;
        c->last.bounce_rays = h.bounce;
        c->last.shadow_rays = h.shadow;
        c->last.shadow_tests_skipped = h.skipped;
        c->last.triangle_tests = h.tri;
        c->last.plane_tests = h.pla;
        c->last.quadric_tests = h.qua;
        c->last.bounce_triangle_tests = h.btri;
        c->last.bvh_nodes_visited = h.bnode;
    }
    return RT_OK;
}

static bool is_device_ptr(const void* p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

static int ensure_scratch(rt_ctx* c, size_t bytes)
{
    if (c->scratch_bytes >= bytes) return RT_OK;
    release(c, c->d_scratch);
    c->d_scratch = nullptr;
    c->scratch_bytes = 0;
    HIP_TRY(c, hipMalloc(&c->d_scratch, bytes));
    c->scratch_bytes = bytes;
    return RT_OK;
}

// The start of every synchronous call on c->stream: each state write and
// render of the call comes after the async renders already enqueued on other
// streams.
static int sync_begin(rt_ctx* c)
{
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = fence_async(c, c->stream)) return rc;
    return wait_state(c, c->stream);
}

// The output planes (at most 3) of a synchronous render: a device pointer is
// written in place, a host pointer through its part of the context's scratch
// and copied back after the launch.
struct SyncOut {
    void *user[3] = {}, *target[3] = {};
    bool host[3] = {};
    size_t off[3] = {}, need = 0;
    int n = 0;
    // plane p (may be null: not requested), `reserve` bytes of scratch if it is a host plane
    int add(void* p, size_t reserve)
    {
        user[n] = p;
        host[n] = p && !is_device_ptr(p);
        if (host[n]) {
            off[n] = need;
            need += reserve;
        }
        return n++;
    }
    // the device pointers to launch into
    int place(rt_ctx* c)
    {
        if (need)
            if (int rc = ensure_scratch(c, need)) return rc;
        for (int i = 0; i < n; ++i) target[i] = host[i] ? (void*)((char*)c->d_scratch + off[i]) : user[i];
        return RT_OK;
    }
    // after the launch: the bytes written to host plane i, to the caller
    int copy_back(rt_ctx* c, int i, size_t bytes) const
    {
        if (host[i] && bytes) HIP_TRY(c, hipMemcpyAsync(user[i], target[i], bytes, hipMemcpyDeviceToHost, c->stream));
        return RT_OK;
    }
};

static int render_sync(rt_ctx* c, const rt_frame* f, void* out, bool as_float)
{
    if (!c || !f || !out) return RT_E_ARG;
    if (c->cpu) return not_cpu(c);
    if (int rc = sync_begin(c)) return rc;
    const size_t px = (size_t)f->width * (size_t)std::max(0, frame_rows(f));
    const size_t bytes = px * (as_float ? 12 : 4);
    SyncOut o;
    o.add(out, std::max<size_t>(bytes, 16));
    if (int rc = o.place(c)) return rc;
    // (launch copies: a big slab goes to the host in chunks)
    if (int rc = launch(c, f, as_float ? nullptr : (unsigned*)o.target[0], as_float ? (float*)o.target[0] : nullptr,
                        c->stream, true, true, (o.host[0] && bytes) ? out : nullptr))
        return rc;
    return finish_sync(c, f, c->stream, true);
}

RT_EXPORT int rt_render(rt_ctx* c, const rt_frame* f, uint8_t* rgba8_out) { return render_sync(c, f, rgba8_out, false); }

RT_EXPORT int rt_render_float(rt_ctx* c, const rt_frame* f, float* rgb_out) { return render_sync(c, f, rgb_out, true); }

RT_EXPORT int rt_render_async(rt_ctx* c, const rt_frame* f, uint8_t* rgba8_dev, float* rgb_dev, void* stream)
{
    if (!c || !f) return RT_E_ARG;
    if (c->cpu) return not_cpu(c);
    HIP_TRY(c, hipSetDevice(c->device));
    return launch(c, f, (unsigned*)rgba8_dev, rgb_dev, (hipStream_t)stream, false, false);
}

// A camera path: frame i with the camera state of slot i % kSeqSlots on
// internal stream i % nstreams, forked from and joined back into the
// caller's stream.  The frames' plans are made here, not by plan_frame: its
// first half is about the context's one camera (tiny_prepare's cache,
// prepare_state's ordering of c->cam across the caller's streams, the
// wavefront queues), and a path of new cameras wants none of that.  The
// second half (plan_kernel) is shared.  What a sequence frame does
// differently from the same frame through rt_render_async:
//  * its camera records are computed for every frame, into its slot, with
//    every tricam record exactly when the frame builds a camera buffer; the
//    slot keeps no camera key (CamState::valid stays false);
//  * TinyCam is built into the plan (tiny_build), not through c->tiny's
//    cache; the tile masks are per internal stream (tiny_masks);
//  * the camera buffer is built only where cb_async_pays says so (no
//    "repeated camera" rule), inside a capture only into arrays already
//    sized, never sized exactly first and never with inline records (so
//    SceneDev::cb_rec is null: CamBuf::inline_rec stays false);
//  * it never runs as a wavefront (a bounce frame takes the BVH megakernel)
//    and sets neither Facts::wf0 nor Facts::small.  The missing `small` is
//    an inconsistency nobody measured: a big-list frame under 4 Mpx runs the
//    kernel without kLbPair here and the kLbPair one through rt_render_async
//    (rt_variant.h).  Left as it is for a change that measures it;
//  * c->last is not written (no stats of a sequence), c->cam and
//    last_async_key are not touched;
//  * the call is fenced behind the context's other async work once, at its
//    start, not per frame, and every frame is checked before any is enqueued.
RT_EXPORT int rt_render_sequence_async(rt_ctx* c, const rt_frame* frames, int32_t n, uint8_t* rgba8_dev,
                                       size_t rgba8_stride, float* rgb_dev, size_t rgb_stride, void* stream)
{
    if (!c || (n > 0 && !frames) || n < 0) return RT_E_ARG;
    if (c->cpu) return not_cpu(c);
    if (int rc = check_uploaded(c)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    bool capturing = false;
    if (int rc = stream_capturing(c, st, &capturing)) return rc;
    // everything is checked before anything is enqueued
    for (int i = 0; i < n; ++i) {
        const rt_frame* f = frames + i;
        if (!frame_ok(f) || (f->flags & RT_FLAG_STATS)) {
            c->err = "bad rt_frame geometry (or RT_FLAG_STATS) in a sequence";
            return RT_E_ARG;
        }
        if (select_variant(frame_facts(c, f, reachable_depth(c, f), false, false, false)).maxd < 0) {
            c->err = "reachable bounce depth exceeds the compiled stack (32)";
            return RT_E_UNSUPPORTED;
        }
    }
    const bool lbuf = lbuf_on(c);
    // The camera slots are shared by every sequence call: one on another
    // stream still in flight must finish first (a captured sequence's
    // ordering against work outside the graph is the caller's, as for any
    // captured launch).
    if (!capturing && n > 0) {
        if (int rc = fence_async(c, st)) return rc;
    }
    // Fork: the internal streams start after everything already on st.
    const int nstreams = std::min(n, kSeqSlots);
    if (nstreams > 1) {
        for (int j = 0; j < nstreams; ++j) {
            if (!c->seq_streams[j]) HIP_TRY(c, hipStreamCreateWithFlags(&c->seq_streams[j], hipStreamNonBlocking));
            if (!c->seq_join[j]) HIP_TRY(c, hipEventCreateWithFlags(&c->seq_join[j], hipEventDisableTiming));
        }
        if (!c->seq_fork) HIP_TRY(c, hipEventCreateWithFlags(&c->seq_fork, hipEventDisableTiming));
        HIP_TRY(c, hipEventRecord(c->seq_fork, st));
        for (int j = 0; j < nstreams; ++j) HIP_TRY(c, hipStreamWaitEvent(c->seq_streams[j], c->seq_fork, 0));
    }
    FramePlan P;  // (one chunk each, never supersampled: step and ss_staged stay unused)
    P.wf = false;
    for (int i = 0; i < n; ++i) {
        const rt_frame* f = frames + i;
        rt_ctx::CamState& q = c->seq[i % kSeqSlots];
        hipStream_t fs = nstreams > 1 ? c->seq_streams[i % nstreams] : st;
        const int rows = P.rows = frame_rows(f);
        if (rows == 0) continue;
        const int depth = P.depth = reachable_depth(c, f);
        P.lbuf = lbuf;
        P.bvh = bvh_on(c, depth, lbuf);
        P.tmode = 0;
        P.tiny = tiny_ok(c, depth, lbuf);
        if (P.tiny) {
            tiny_build(c, f, P.T);
            if (int rc = tiny_masks(c, f, fs, capturing, P.T, &P.tmode)) return rc;
        }
        // the slot's camera buffer (round 3, big lists as for rt_render_async):
        // built on the frame's stream like its records; inside a capture only
        // into buffers already sized (a first capture renders without it —
        // the same image)
        const int nt = ((f->width + 7) / 8) * ((f->height + 7) / 8);
        const bool cbuf = P.cbuf =
            !P.tiny && cb_wanted(c, f, depth, lbuf) && cb_async_pays(c, f) &&
            (!capturing || (q.cb.cap > 0 && q.cb.rcap > 0 && q.cb.nt_alloc >= nt && q.cb.big_alloc >= c->n_tri));
        if (c->n_tri > 0 && !P.tiny) {
            if (int rc = camera_records(c, q, f->cam_pos, fs, cbuf)) return rc;
        }
        if (cbuf) {
            const SceneDev S = scene_dev(c, q, false, false);
            if (int rc = cb_build(c, q.cb, f, S, fs, false, capturing, false)) return rc;
        }
        if (int rc = plan_kernel(c, f, q, false, P)) return rc;
        unsigned* rgba = rgba8_dev ? (unsigned*)(rgba8_dev + (size_t)i * rgba8_stride) : nullptr;
        float* rgb = rgb_dev ? (float*)((char*)rgb_dev + (size_t)i * rgb_stride) : nullptr;
        if (int rc = launch_trace(c, P.kp, P.tiny ? &P.T : nullptr, P.S, P.F, f->width, rows, rgba, rgb, c->d_stats, fs))
            return rc;
        if (P.tmode == 2)
            if (int rc = tiny_masks_stored(c, fs)) return rc;
    }
    // Join: st continues after every frame.
    if (nstreams > 1) {
        for (int j = 0; j < nstreams; ++j) {
            HIP_TRY(c, hipEventRecord(c->seq_join[j], c->seq_streams[j]));
            HIP_TRY(c, hipStreamWaitEvent(st, c->seq_join[j], 0));
        }
    }
    if (capturing || n > 0) enqueued(c, st, capturing, nullptr);  // (a slot's buffer is rebuilt in every replay)
    return RT_OK;
}

RT_EXPORT int rt_prepare_camera(rt_ctx* c, const rt_frame* f)
{
    if (!c || !f) return RT_E_ARG;
    if (c->cpu) return not_cpu(c);
    if (int rc = check_uploaded(c, "rt_prepare_camera")) return rc;
    if (int rc = check_frame(c, f)) return rc;
    if (int rc = sync_begin(c)) return rc;
    const bool cb_want = cb_wanted(c, f, reachable_depth(c, f), lbuf_on(c));
    if (int rc = prepare_state(c, c->cam, f, c->stream, true, false, cb_want)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    settled(c);
    return RT_OK;
}

static int cpu_render_sync(rt_ctx* c, const rt_frame* f, uint8_t* rgba, float* rgb)
{
    if (!c || !f || (!rgba && !rgb)) return RT_E_ARG;
    if (!c->cpu) return needs_cpu(c, "rt_cpu_render");
    if (int rc = check_uploaded(c)) return rc;
    if (int rc = check_frame(c, f)) return rc;
    c->last = rt_stats{};
    double ms = 0.0;
    unsigned long long rays2[2] = {0, 0};
    const int rc = cpu_render(c->cpu_scene, c->cpu_threads, f, frame_rows(f), rgba, rgb, &ms, rays2);
    c->last.kernel_ms = (float)ms;
    if (f->flags & RT_FLAG_STATS) {  // (the rays only: the CPU backend counts no tests)
        c->last.primary_rays = rays2[0];
        c->last.bounce_rays = rays2[1];
    }
    return rc;
}

RT_EXPORT int rt_cpu_render(rt_ctx* c, const rt_frame* f, uint8_t* rgba8_out)
{
    return cpu_render_sync(c, f, rgba8_out, nullptr);
}

RT_EXPORT int rt_cpu_render_float(rt_ctx* c, const rt_frame* f, float* rgb_out)
{
    return cpu_render_sync(c, f, nullptr, rgb_out);
}

// ---- supersampled renders (rt.h)
RT_EXPORT int32_t rt_ss_rows(const rt_frame* f, int32_t s) { return ss_rows_of(f, s); }

static int ss_check(rt_ctx* c, const rt_frame* f, int s)
{
    if (ss_rows_of(f, s) >= 0) return RT_OK;
    c->err = "bad supersampling: s in 1..8 must divide the sample frame's width, height and slab rows "
             "(band_rows: a multiple of 16 s)";
    return RT_E_ARG;
}

static int render_ss_sync(rt_ctx* c, const rt_frame* f, int s, void* out, bool as_float)
{
    if (!c || !f || !out) return RT_E_ARG;
    if (c->cpu) return not_cpu(c);
    if (int rc = ss_check(c, f, s)) return rc;
    if (s == 1) return render_sync(c, f, out, as_float);
    if (int rc = sync_begin(c)) return rc;
    const size_t px = (size_t)(f->width / s) * (size_t)ss_rows_of(f, s);
    const size_t bytes = px * (as_float ? 12 : 4);
    SyncOut o;
    o.add(out, std::max<size_t>(bytes, 16));
    if (int rc = o.place(c)) return rc;
    if (int rc = launch(c, f, as_float ? nullptr : (unsigned*)o.target[0], as_float ? (float*)o.target[0] : nullptr,
                        c->stream, true, true, nullptr, s))
        return rc;
    // (a band set's rows past the frame are not written: they are not copied either)
    const size_t wrote = (size_t)(f->width / s) * (size_t)(ss_valid_rows(f, frame_rows(f)) / s) * (as_float ? 12 : 4);
    if (int rc = o.copy_back(c, 0, wrote)) return rc;
    return finish_sync(c, f, c->stream, true);
}

RT_EXPORT int rt_render_ss(rt_ctx* c, const rt_frame* f, int32_t s, uint8_t* rgba8_out)
{
    return render_ss_sync(c, f, s, rgba8_out, false);
}

RT_EXPORT int rt_render_ss_float(rt_ctx* c, const rt_frame* f, int32_t s, float* rgb_out)
{
    return render_ss_sync(c, f, s, rgb_out, true);
}

RT_EXPORT int rt_render_ss_async(rt_ctx* c, const rt_frame* f, int32_t s, uint8_t* rgba8_dev, float* rgb_dev,
                                 void* stream)
{
    if (!c || !f) return RT_E_ARG;
    if (c->cpu) return not_cpu(c);
    if (int rc = ss_check(c, f, s)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    return launch(c, f, (unsigned*)rgba8_dev, rgb_dev, (hipStream_t)stream, false, false, nullptr, s);
}

static int cpu_render_ss_sync(rt_ctx* c, const rt_frame* f, int s, uint8_t* rgba, float* rgb)
{
    if (!c || !f || (!rgba && !rgb)) return RT_E_ARG;
    if (!c->cpu) return needs_cpu(c, "rt_cpu_render_ss");
    if (int rc = ss_check(c, f, s)) return rc;
    if (s == 1) return cpu_render_sync(c, f, rgba, rgb);
    if (int rc = check_uploaded(c)) return rc;
    c->last = rt_stats{};
    const int rows = frame_rows(f);
    std::vector<float> samples((size_t)rows * f->width * 3);
    double ms = 0.0, ms2 = 0.0;
    if (int rc = cpu_render(c->cpu_scene, c->cpu_threads, f, rows, nullptr, samples.data(), &ms)) return rc;
    cpu_resolve(samples.data(), f->width, s, ss_valid_rows(f, rows) / s, rgba, rgb, &ms2);
    c->last.kernel_ms = (float)(ms + ms2);
    return RT_OK;
}

RT_EXPORT int rt_cpu_render_ss(rt_ctx* c, const rt_frame* f, int32_t s, uint8_t* rgba8_out)
{
    return cpu_render_ss_sync(c, f, s, rgba8_out, nullptr);
}

RT_EXPORT int rt_cpu_render_ss_float(rt_ctx* c, const rt_frame* f, int32_t s, float* rgb_out)
{
    return cpu_render_ss_sync(c, f, s, nullptr, rgb_out);
}

// ---- adaptive supersampling (rt.h rt_render_adaptive*, rt_adaptive.h)
// The refine kernel for the parameters of f (defined behind the query
// kernels' table: its instances are named after every other kernel's).
static int pick_refine(rt_ctx* c, const rt_frame* f, KernelPick& p);
static const void* edge_kernel(bool scatter);  // rt_edge_classify_kernel / rt_edge_scatter_kernel (named there too)
static int launch_aov(rt_ctx* c, const rt_frame* f, const rt_aov& dev, hipStream_t st, bool sync_path);

// The checks every adaptive entry point shares (after the backend's own).
static int adaptive_check(rt_ctx* c, const rt_frame* f, const rt_adaptive* a, const rt_adaptive_out* o)
{
    if (int rc = check_uploaded(c, "rt_render_adaptive")) return rc;
    const char* why = nullptr;
    if (a->s != 2 && a->s != 4 && a->s != 8)
        why = "s is 2, 4 or 8";
    else if (f->band_rows != 0)
        why = "row bands are not supported";
    else if (ss_rows_of(f, a->s) < 0)
        why = "s must divide the sample frame's width, height, row_begin and row_end";
    else if (a->criteria == 0 || (a->criteria & ~kEdgeAll) != 0)
        why = "criteria: at least one of RT_EDGE_ID, RT_EDGE_NORMAL, RT_EDGE_COLOUR and nothing else";
    else if (!o->rgba8 && !o->rgb && !o->mask)
        why = "no output requested";
    else if (f->flags & RT_FLAG_STATS)
        why = "RT_FLAG_STATS is not accepted";
    else if ((uint64_t)(f->width / a->s) * (uint64_t)ss_rows_of(f, a->s) > (uint64_t)INT32_MAX)
        why = "more than INT32_MAX output pixels";
    if (!why) return RT_OK;
    c->err = std::string("rt_render_adaptive: ") + why;
    return RT_E_ARG;
}

// One adaptive render of sample frame f on st into device planes (each may be
// null).  sync_path: rt_render_adaptive on c->stream, timed by c->ad.ev.
//  1. the base frame B with its halo rows through launch and launch_aov,
//     unchanged, into the context's planes (the AOV pass only for RT_EDGE_ID /
//     RT_EDGE_NORMAL, its normals only for RT_EDGE_NORMAL);
//  2. rt_edge_classify_kernel: masks, flags and the base colours; scan_u32 of
//     the flags; rt_edge_scatter_kernel: the row-major list of flagged pixels;
//  3. rt_refine_kernel on a fixed grid, bounded by the scan's total on the
//     device.
static int launch_adaptive(rt_ctx* c, const rt_frame* f, const rt_adaptive* a, const KernelPick& kp, unsigned* rgba,
                           float* rgb, unsigned char* mask, hipStream_t st, bool sync_path)
{
    const int s = a->s, ls = s == 2 ? 1 : (s == 4 ? 2 : 3);
    const rt_frame B = adaptive_base(*f, s), Bh = adaptive_halo(B);
    const int W = B.width, rows = B.row_end - B.row_begin, hrows = Bh.row_end - Bh.row_begin;
    rt_ctx::AdBuf& A = c->ad;
    A.flagged = 0;
    if (rows <= 0) return RT_OK;
    const size_t n = (size_t)W * rows, hpx = (size_t)W * hrows;
    const bool want_id = (a->criteria & (kEdgeId | kEdgeNormal)) != 0, want_n = (a->criteria & kEdgeNormal) != 0;
    size_t need = 0;
    auto part = [&](size_t bytes) {
        const size_t o = need;
        need += (bytes + 255) / 256 * 256;
        return o;
    };
    const size_t o_rgb = part(hpx * 12), o_id = part(want_id ? hpx * 4 : 0), o_n = part(want_n ? hpx * 12 : 0),
                 o_flag = part(n * 4), o_off = part((n + 1) * 4), o_list = part(n * 4),
                 o_scan = part(scan_scratch(n) * sizeof(unsigned long long));
    if (need > A.bytes) {
        free_later(c, A.mem);  // an enqueued call may still use the old one
        A.mem = nullptr;
        A.bytes = 0;
        HIP_TRY(c, hipMalloc(&A.mem, need));
        A.bytes = need;
    }
    char* const m = (char*)A.mem;
    float* const p_rgb = (float*)(m + o_rgb);
    int32_t* const p_id = want_id ? (int32_t*)(m + o_id) : nullptr;
    float* const p_n = want_n ? (float*)(m + o_n) : nullptr;
    unsigned* const flag = (unsigned*)(m + o_flag);
    unsigned* const off = (unsigned*)(m + o_off);
    unsigned* const list = (unsigned*)(m + o_list);
    A.total = off + n;
    if (sync_path)
        for (hipEvent_t& e : A.ev)
            if (!e) HIP_TRY(c, hipEventCreate(&e));
    if (int rc = A.turn.enter(c, st)) return rc;
    const auto enqueue = [&]() -> int {
        if (sync_path) HIP_TRY(c, hipEventRecord(A.ev[0], st));
        if (int rc = launch(c, &Bh, nullptr, p_rgb, st, false, sync_path)) return rc;
        if (want_id)
            if (int rc = launch_aov(c, &Bh, rt_aov{nullptr, p_id, p_n}, st, sync_path)) return rc;
        if (sync_path) HIP_TRY(c, hipEventRecord(A.ev[1], st));
        const EdgePlanes P{p_rgb, p_id, p_n, W, B.height, Bh.row_begin};
        const unsigned nn = (unsigned)n, blocks = (unsigned)((n + 255) / 256);
        {
            EdgePlanes Pv = P;
            int rb = B.row_begin, crit = a->criteria;
            unsigned nv = nn;
            float cosv = a->normal_cos, delta = a->colour_delta;
            unsigned* fl = flag;
            void* args[] = {&Pv, &rb, &nv, &crit, &cosv, &delta, &fl, &rgb, &rgba, &mask};
            HIP_TRY(c, hipLaunchKernel(edge_kernel(false), dim3(blocks), dim3(256), args, 0, st));
        }
        HIP_TRY(c, scan_u32(flag, nn, off, (unsigned long long*)(m + o_scan), st, nullptr));
        {
            const unsigned *fl = flag, *of = off;
            unsigned nv = nn;
            unsigned* ls_ = list;
            void* args[] = {&fl, &of, &nv, &ls_};
            HIP_TRY(c, hipLaunchKernel(edge_kernel(true), dim3(blocks), dim3(256), args, 0, st));
        }
        if (sync_path) HIP_TRY(c, hipEventRecord(A.ev[2], st));
        if (rgb || rgba) {  // (a mask alone needs no sample)
            // (after the base passes: they may have allocated the camera state scene_dev names)
            SceneDev S = scene_dev(c, c->cam, has_light_buf(kp.v.flags), false);
            FrameDev F;
            frame_dev(f, F);
            const unsigned* lst = list;
            const unsigned* total = A.total;
            int lsv = ls, wo = W, rb = B.row_begin;
            const size_t per = (size_t)64 >> (2 * ls);
            const unsigned grid = (unsigned)std::min<size_t>(kRefineGrid, (n + per - 1) / per);
            void* args[] = {&S, &F, &lst, &total, &lsv, &wo, &rb, &rgb, &rgba};
            HIP_TRY(c, hipLaunchKernel(kp.k, dim3(grid), dim3(64), args, kp.lds, st));
        }
        if (sync_path) HIP_TRY(c, hipEventRecord(A.ev[3], st));
        return RT_OK;
    };
    // (the turn is left behind a failure too: what was enqueued before it still uses the planes)
    const int rc = enqueue(), left = A.turn.leave(c, st);
    return rc ? rc : left;
}

RT_EXPORT int rt_render_adaptive(rt_ctx* c, const rt_frame* f, const rt_adaptive* a, const rt_adaptive_out* out)
{
    if (!c || !f || !a || !out) return RT_E_ARG;
    if (c->cpu) return not_cpu(c);
    if (int rc = adaptive_check(c, f, a, out)) return rc;
    KernelPick kp;
    if (int rc = pick_refine(c, f, kp)) return rc;
    if (int rc = sync_begin(c)) return rc;
    const size_t px = (size_t)(f->width / a->s) * (size_t)ss_rows_of(f, a->s);
    // (one 256-byte aligned part of the scratch per host plane)
    SyncOut o;
    const size_t bytes[3] = {px * 4, px * 12, px};
    void* const user[3] = {out->rgba8, out->rgb, out->mask};
    for (int i = 0; i < 3; ++i) o.add(user[i], (bytes[i] + 255) / 256 * 256);
    if (int rc = o.place(c)) return rc;
    if (int rc = launch_adaptive(c, f, a, kp, (unsigned*)o.target[0], (float*)o.target[1], (unsigned char*)o.target[2],
                                 c->stream, true))
        return rc;
    for (int i = 0; i < 3; ++i)
        if (int rc = o.copy_back(c, i, bytes[i])) return rc;
    if (int rc = finish_sync(c, f, c->stream, false)) return rc;
    rt_ctx::AdBuf& A = c->ad;
    c->last = rt_stats{};
    std::memcpy(c->last.kernel, kp.name->s, sizeof kp.name->s);
    c->last.stack_depth = kp.v.maxd;
    if (px) {
        unsigned flagged = 0;  // (for the stats only: no launch was sized by it)
        HIP_TRY(c, hipMemcpy(&flagged, A.total, sizeof flagged, hipMemcpyDeviceToHost));
        A.flagged = flagged;
        float ms = 0.f;
        for (int i = 0; i < 3; ++i) {
            HIP_TRY(c, hipEventElapsedTime(&A.phase_ms[i], A.ev[i], A.ev[i + 1]));
            ms += A.phase_ms[i];
        }
        c->last.kernel_ms = ms;
    }
    // (a mask alone traces no sample)
    c->last.primary_rays = (uint64_t)px + ((out->rgba8 || out->rgb) ? (uint64_t)(a->s * a->s) * A.flagged : 0);
    return RT_OK;
}

RT_EXPORT int rt_render_adaptive_async(rt_ctx* c, const rt_frame* f, const rt_adaptive* a, const rt_adaptive_out* dev,
                                       void* stream)
{
    if (!c || !f || !a || !dev) return RT_E_ARG;
    if (c->cpu) return not_cpu(c);
    if (int rc = adaptive_check(c, f, a, dev)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    for (const void* p : {(const void*)dev->rgba8, (const void*)dev->rgb, (const void*)dev->mask})
        if (p && !is_device_ptr(p)) {
            c->err = "rt_render_adaptive_async takes device pointers";
            return RT_E_ARG;
        }
    const hipStream_t st = (hipStream_t)stream;
    bool capturing = false;
    if (int rc = stream_capturing(c, st, &capturing)) return rc;
    if (capturing) {
        c->err = "rt_render_adaptive_async: hipGraph capture is not supported";
        return RT_E_STATE;
    }
    KernelPick kp;
    if (int rc = pick_refine(c, f, kp)) return rc;
    return launch_adaptive(c, f, a, kp, (unsigned*)dev->rgba8, dev->rgb, dev->mask, st, false);
}

RT_EXPORT int rt_cpu_render_adaptive(rt_ctx* c, const rt_frame* f, const rt_adaptive* a, const rt_adaptive_out* out)
{
    if (!c || !f || !a || !out) return RT_E_ARG;
    if (!c->cpu) return needs_cpu(c, "rt_cpu_render_adaptive");
    if (int rc = adaptive_check(c, f, a, out)) return rc;
    c->last = rt_stats{};
    double ms = 0.0;
    unsigned long long flagged = 0;
    const int rc = cpu_render_adaptive(c->cpu_scene, c->cpu_threads, f, a->s, a->criteria, a->normal_cos,
                                       a->colour_delta, out->rgba8, out->rgb, out->mask, &ms, &flagged);
    c->last.kernel_ms = (float)ms;
    c->last.primary_rays = (uint64_t)(f->width / a->s) * (uint64_t)ss_rows_of(f, a->s) +
                           ((out->rgba8 || out->rgb) ? (uint64_t)(a->s * a->s) * flagged : 0);
    std::snprintf(c->last.kernel, sizeof c->last.kernel, "cpu_render_adaptive");
    return rc;
}

// ---- primary-hit AOV renders (rt.h, rt_aov.h)
#define RT_V(M, L, F) {{M, L, F}, {(const void*)&rt_aov_kernel<F>}, kernel_name("rt_aov_kernel", F)},
static const KernelRow<1> kAovKernels[] = {RT_AOV_VARIANTS};
#undef RT_V

// The checks every AOV entry point shares (after the backend's own).
static int aov_check(rt_ctx* c, const rt_frame* f, const rt_aov* o)
{
    if (int rc = check_uploaded(c)) return rc;
    if (!o->t && !o->id && !o->n) {
        c->err = "rt_render_aov: no output plane requested";
        return RT_E_ARG;
    }
    if (f->flags & RT_FLAG_STATS) {
        c->err = "rt_render_aov: RT_FLAG_STATS is not accepted";
        return RT_E_ARG;
    }
    return check_frame(c, f);
}

// One AOV frame into device planes on st.  The variant: kCullNone (no camera
// state) for the scenes whose colour frames take their camera records with
// the launch — no camera state is built or invalidated behind that kernel —
// and for scenes without triangles; else the depth-0 colour frame's culling
// (wave, or clustered above kClusterMinTriangles) with the camera state made
// current exactly as rt_render / rt_render_async do (prepare_state), the
// camera buffer where it is current (a tile whose list did not fit: the
// per-wave path).  sync_path: rt_render_aov on c->stream, timed.
static int launch_aov(rt_ctx* c, const rt_frame* f, const rt_aov& dev, hipStream_t st, bool sync_path)
{
    bool capturing = false;
    if (!sync_path)
        if (int rc = stream_capturing(c, st, &capturing)) return rc;
    const bool wave0 = c->n_tri == 0 || tiny_ok(c, 0, lbuf_on(c));
    const bool cb_want = !wave0 && cb_wanted(c, f, 0, lbuf_on(c));
    const int rows = frame_rows(f);
    if (rows > 0 && !wave0) {
        if (int rc = prepare_state(c, c->cam, f, st, sync_path, capturing, cb_want)) return rc;
    }
    const bool cbuf = cb_want && cb_matches(c->cam.cb, f);
    Facts fa;
    fa.aov = true;
    fa.n_tri = c->n_tri;
    fa.tiny = wave0 ? 0 : -1;
    fa.cbuf = cbuf;
    const Variant v = select_variant(fa);
    const KernelRow<1>* const row = find_row(kAovKernels, v);  // (the row exists: KernelRow)
    SceneDev S = scene_dev(c, c->cam, false, cbuf);
    FrameDev F;
    frame_dev(f, F);
    c->last = rt_stats{};
    std::memcpy(c->last.kernel, row->name.s, sizeof row->name.s);
    c->last.primary_rays = (uint64_t)f->width * (uint64_t)ss_valid_rows(f, rows);
    if (rows == 0) return RT_OK;
    dim3 grid, block;
    trace_grid(c, is_clustered(v.flags), F, f->width, rows, grid, block);
    float* ot = dev.t;
    int* oi = dev.id;
    float* on = dev.n;
    void* args[] = {&S, &F, &ot, &oi, &on};
    if (sync_path) HIP_TRY(c, hipEventRecord(c->ev0, st));
    HIP_TRY(c, hipLaunchKernel(row->k[0], grid, block, args, lds_bytes(v.flags, 0), st));
    if (sync_path) HIP_TRY(c, hipEventRecord(c->ev1, st));
    if (!sync_path) enqueued(c, st, capturing, cbuf ? &c->cam.cb : nullptr);
    return RT_OK;
}

RT_EXPORT int rt_render_aov(rt_ctx* c, const rt_frame* f, const rt_aov* out)
{
    if (!c || !f || !out) return RT_E_ARG;
    if (c->cpu) return not_cpu(c);
    if (int rc = aov_check(c, f, out)) return rc;
    if (int rc = sync_begin(c)) return rc;
    // (one 256-byte aligned part of the scratch per host plane)
    const int rows = std::max(0, frame_rows(f));
    const size_t px = (size_t)f->width * (size_t)rows;
    void* const user[3] = {out->t, out->id, out->n};
    SyncOut o;
    for (int i = 0; i < 3; ++i) o.add(user[i], (px * (i == 2 ? 12 : 4) + 255) / 256 * 256);
    if (int rc = o.place(c)) return rc;
    const rt_aov dev{(float*)o.target[0], (int32_t*)o.target[1], (float*)o.target[2]};
    if (int rc = launch_aov(c, f, dev, c->stream, true)) return rc;
    // (a band set's rows past the frame are not written: they are not copied either)
    const size_t wrote = (size_t)f->width * (size_t)ss_valid_rows(f, rows);
    for (int i = 0; i < 3; ++i)
        if (int rc = o.copy_back(c, i, wrote * (i == 2 ? 12 : 4))) return rc;
    return finish_sync(c, f, c->stream, rows > 0);
}

RT_EXPORT int rt_render_aov_async(rt_ctx* c, const rt_frame* f, const rt_aov* dev, void* stream)
{
    if (!c || !f || !dev) return RT_E_ARG;
    if (c->cpu) return not_cpu(c);
    if (int rc = aov_check(c, f, dev)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    return launch_aov(c, f, *dev, (hipStream_t)stream, false);
}

RT_EXPORT int rt_cpu_render_aov(rt_ctx* c, const rt_frame* f, const rt_aov* out)
{
    if (!c || !f || !out) return RT_E_ARG;
    if (!c->cpu) return needs_cpu(c, "rt_cpu_render_aov");
    if (int rc = aov_check(c, f, out)) return rc;
    c->last = rt_stats{};
    const int rows = frame_rows(f);
    double ms = 0.0;
    const int rc = cpu_render_aov(c->cpu_scene, c->cpu_threads, f, rows, out->t, out->id, out->n, &ms);
    c->last.kernel_ms = (float)ms;
    c->last.primary_rays = (uint64_t)f->width * (uint64_t)ss_valid_rows(f, rows);
    std::snprintf(c->last.kernel, sizeof c->last.kernel, "cpu_render_aov");
    return rc;
}

// ---- queries of arbitrary rays: closest hits (rt.h rt_trace_rays*, rt_rays.h),
// shadow filters of segments (rt_filter_rays*, rt_filter.h) and radiance
// (rt_shade_rays*, rt_shaderays.h).  One host path (query_check, query_sync,
// query_async, query_cpu); a QueryKind says what differs between the three,
// a Query is one call.
struct Query;
struct QueryKind {
    const char* name;   // the synchronous entry point rt_<stem>: rt_<stem>_async, rt_cpu_<stem>, cpu_<stem>
    const char* noun;   // "the <noun> count must be ..."
    const char* nulls;  // the message for a null input or output
    int out_bytes[3];   // bytes per item of each output plane (0: the query has no such plane)
    bool optional_out;  // a null plane is not requested (one at least) / every plane is required
    bool takes_frame;   // the call carries an rt_frame of parameters
    uint64_t rt_stats::*count;                // the counter of c->last that takes n
    int (*pick)(rt_ctx*, Query&);             // the kernel for the call's parameters (null: nothing to pick)
    void (*label)(rt_ctx*, const Query&);     // c->last's kernel name, and what goes with it
    int (*launch)(rt_ctx*, const Query&, const float* d_in, void* const d_out[3], hipStream_t);
    int (*cpu)(rt_ctx*, const Query&, double* ms);
};
struct Query {
    const QueryKind& k;
    const rt_frame* f;  // (takes_frame)
    const float* in;    // n x 6 floats
    int64_t n;
    void* out[3];
    KernelPick kp;      // (pick)
};

// The checks every entry point shares, in the order rt.h documents.  *go:
// there is something to do (n == 0 is RT_OK with nothing written).
static int query_check(rt_ctx* c, Query& q, bool cpu, bool* go)
{
    const QueryKind& k = q.k;
    *go = false;
    if (!c) return RT_E_ARG;
    if (c->cpu != cpu) return cpu ? needs_cpu(c, (std::string("rt_cpu_") + (k.name + 3)).c_str()) : not_cpu(c);
    if (int rc = check_uploaded(c, k.name)) return rc;
    if (k.takes_frame && !q.f) {
        c->err = std::string(k.name) + ": no rt_frame (max_bounces, min_energy, scene_ior, background)";
        return RT_E_ARG;
    }
    if (q.n < 0 || q.n > INT32_MAX) {
        c->err = std::string(k.name) + ": the " + k.noun + " count must be 0 .. INT32_MAX";
        return RT_E_ARG;
    }
    if (q.n == 0) return RT_OK;
    bool any = false, all = true;
    for (int i = 0; i < 3; ++i) {
        if (!k.out_bytes[i]) continue;
        any = any || q.out[i];
        all = all && q.out[i];
    }
    if (!q.in || !(k.optional_out ? any : all)) {
        c->err = std::string(k.name) + ": " + k.nulls;
        return RT_E_ARG;
    }
    // (a depth above the compiled stacks is refused before any pointer is classified)
    if (!cpu && k.pick)
        if (int rc = k.pick(c, q)) return rc;
    *go = true;
    return RT_OK;
}

static int query_aligned(rt_ctx* c, const Query& q, const void* p)
{
    if (((uintptr_t)p & 7u) == 0) return RT_OK;
    c->err = std::string(q.k.name) + ": device pointers must be 8-byte aligned";
    return RT_E_ARG;
}

// Host or device pointers, on c->stream, timed.  The scratch: a host input
// first, then one 256-byte aligned part per host output plane.
static int query_sync(rt_ctx* c, Query q)
{
    const QueryKind& k = q.k;
    bool go;
    if (int rc = query_check(c, q, false, &go)) return rc;
    if (!go) return RT_OK;
    if (int rc = sync_begin(c)) return rc;
    const bool in_host = !is_device_ptr(q.in);
    const size_t n = (size_t)q.n, in_bytes = n * 6 * sizeof(float);
    SyncOut o;
    if (in_host) o.need = (in_bytes + 255) / 256 * 256;
    for (int i = 0; i < 3; ++i) o.add(q.out[i], (n * k.out_bytes[i] + 255) / 256 * 256);
    if (!in_host)
        if (int rc = query_aligned(c, q, q.in)) return rc;
    for (int i = 0; i < 3; ++i)
        if (q.out[i] && !o.host[i])
            if (int rc = query_aligned(c, q, q.out[i])) return rc;
    if (int rc = o.place(c)) return rc;
    const float* d_in = q.in;
    if (in_host) {
        HIP_TRY(c, hipMemcpyAsync(c->d_scratch, q.in, in_bytes, hipMemcpyHostToDevice, c->stream));
        d_in = (const float*)c->d_scratch;
    }
    c->last = rt_stats{};
    k.label(c, q);
    c->last.*k.count = (uint64_t)q.n;
    HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
    if (int rc = k.launch(c, q, d_in, o.target, c->stream)) return rc;
    HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
    for (int i = 0; i < 3; ++i)
        if (int rc = o.copy_back(c, i, n * k.out_bytes[i])) return rc;
    static const rt_frame no_frame{};  // (no RT_FLAG_STATS: a query has no counting instances)
    return finish_sync(c, &no_frame, c->stream, true);
}

// Device pointers, enqueued on the caller's stream: one kernel and host
// bookkeeping, no state of the context (legal inside a stream capture).
static int query_async(rt_ctx* c, Query q, void* stream)
{
    bool go;
    if (int rc = query_check(c, q, false, &go)) return rc;
    if (!go) return RT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const void* const ptr[4] = {q.in, q.out[0], q.out[1], q.out[2]};
    for (const void* p : ptr) {
        if (!p) continue;
        if (!is_device_ptr(p)) {
            c->err = std::string(q.k.name) + "_async takes device pointers";
            return RT_E_ARG;
        }
        if (int rc = query_aligned(c, q, p)) return rc;
    }
    const hipStream_t st = (hipStream_t)stream;
    bool capturing = false;
    if (int rc = stream_capturing(c, st, &capturing)) return rc;
    if (int rc = q.k.launch(c, q, q.in, q.out, st)) return rc;
    // (host bookkeeping only: an upload syncs st, or keeps what a graph references)
    enqueued(c, st, capturing, nullptr);
    return RT_OK;
}

static int query_cpu(rt_ctx* c, Query q)
{
    bool go;
    if (int rc = query_check(c, q, true, &go)) return rc;
    if (!go) return RT_OK;
    c->last = rt_stats{};
    double ms = 0.0;
    const int rc = q.k.cpu(c, q, &ms);
    c->last.kernel_ms = (float)ms;
    c->last.*q.k.count = (uint64_t)q.n;
    std::snprintf(c->last.kernel, sizeof c->last.kernel, "cpu_%s", q.k.name + 3);
    return rc;
}

// -- closest hits.  The query walks the BVH whenever the scene has one
// (RT_OPT_BVH): the tree of a scene that can bounce, or RT_OPT_RAY_BVH's.
static bool rays_bvh(const rt_ctx* c) { return c->d_bvh_node && c->opt_bvh; }

// n rays into device planes on st: one kernel, no state of the context.
static int launch_rays(rt_ctx* c, const float* d_rays, int n, const rt_aov& dev, hipStream_t st)
{
    const bool bvh = rays_bvh(c);
    SceneDev S = scene_dev(c, c->cam, false, false);
    const float2* rays = reinterpret_cast<const float2*>(d_rays);
    float* ot = dev.t;
    int* oi = dev.id;
    float* on = dev.n;
    void* args[] = {&S, &rays, &n, &ot, &oi, &on};
    const void* k = bvh ? (const void*)&rt_rays_kernel<1> : (const void*)&rt_rays_kernel<0>;
    const unsigned lds = bvh ? (unsigned)rays_lds_bytes(c->bvh_depth) : 0u;
    HIP_TRY(c, hipLaunchKernel(k, dim3((unsigned)(((int64_t)n + 63) / 64)), dim3(64), args, lds, st));
    return RT_OK;
}

static const QueryKind kTraceRays = {
    "rt_trace_rays", "ray", "no rays or no output plane", {4, 4, 12}, true, false, &rt_stats::bounce_rays, nullptr,
    [](rt_ctx* c, const Query&) {
        std::snprintf(c->last.kernel, sizeof c->last.kernel, "rt_rays_kernel<%d>", rays_bvh(c) ? 1 : 0);
    },
    [](rt_ctx* c, const Query& q, const float* d_in, void* const o[3], hipStream_t st) {
        return launch_rays(c, d_in, (int)q.n, rt_aov{(float*)o[0], (int32_t*)o[1], (float*)o[2]}, st);
    },
    [](rt_ctx* c, const Query& q, double* ms) {
        return cpu_trace_rays(c->cpu_scene, c->cpu_threads, q.in, q.n, (float*)q.out[0], (int32_t*)q.out[1],
                              (float*)q.out[2], ms);
    }};

static Query trace_query(const float* rays, int64_t n, const rt_aov* o)
{
    const rt_aov none{};  // (no rt_aov at all: no plane requested)
    if (!o) o = &none;
    return Query{kTraceRays, nullptr, rays, n, {o->t, o->id, o->n}};
}

RT_EXPORT int rt_trace_rays(rt_ctx* c, const float* rays, int64_t n, const rt_aov* out)
{
    return query_sync(c, trace_query(rays, n, out));
}

RT_EXPORT int rt_trace_rays_async(rt_ctx* c, const float* dev_rays, int64_t n, const rt_aov* dev, void* stream)
{
    return query_async(c, trace_query(dev_rays, n, dev), stream);
}

RT_EXPORT int rt_cpu_trace_rays(rt_ctx* c, const float* rays, int64_t n, const rt_aov* out)
{
    return query_cpu(c, trace_query(rays, n, out));
}

// -- shadow filters.  The any-hit walk needs the tree and factors that are all
// finite and >= +0 (rt_filter.h); else the file-order product.
static bool filter_bvh_on(const rt_ctx* c) { return rays_bvh(c) && c->shadow_split; }

// n segments into dev_out on st: one kernel, no state of the context.
static int launch_filter(rt_ctx* c, const float* d_segs, int n, float* d_out, hipStream_t st)
{
    const bool bvh = filter_bvh_on(c);
    SceneDev S = scene_dev(c, c->cam, false, false);
    const float2* segs = reinterpret_cast<const float2*>(d_segs);
    int depth = c->bvh_depth;
    void* args[] = {&S, &segs, &n, &d_out, &depth};
    const void* k = bvh ? (const void*)&rt_filter_kernel<1> : (const void*)&rt_filter_kernel<0>;
    const unsigned lds = bvh ? (unsigned)filter_lds_bytes(c->bvh_depth) : 0u;
    HIP_TRY(c, hipLaunchKernel(k, dim3((unsigned)(((int64_t)n + 63) / 64)), dim3(64), args, lds, st));
    return RT_OK;
}

static const QueryKind kFilterRays = {
    "rt_filter_rays", "segment", "no segments or no output", {12, 0, 0}, false, false, &rt_stats::shadow_rays, nullptr,
    [](rt_ctx* c, const Query&) {
        std::snprintf(c->last.kernel, sizeof c->last.kernel, "rt_filter_kernel<%d>", filter_bvh_on(c) ? 1 : 0);
    },
    [](rt_ctx* c, const Query& q, const float* d_in, void* const o[3], hipStream_t st) {
        return launch_filter(c, d_in, (int)q.n, (float*)o[0], st);
    },
    [](rt_ctx* c, const Query& q, double* ms) {
        return cpu_filter_rays(c->cpu_scene, c->cpu_threads, q.in, q.n, (float*)q.out[0], ms);
    }};

RT_EXPORT int rt_filter_rays(rt_ctx* c, const float* segs, int64_t n, float* filter)
{
    return query_sync(c, Query{kFilterRays, nullptr, segs, n, {filter}});
}

RT_EXPORT int rt_filter_rays_async(rt_ctx* c, const float* dev_segs, int64_t n, float* dev_filter, void* stream)
{
    return query_async(c, Query{kFilterRays, nullptr, dev_segs, n, {dev_filter}}, stream);
}

RT_EXPORT int rt_cpu_filter_rays(rt_ctx* c, const float* segs, int64_t n, float* filter)
{
    return query_cpu(c, Query{kFilterRays, nullptr, segs, n, {filter}});
}

// -- radiance
#define RT_V(M, L, F) \
    {{M, L, F}, {(const void*)&rt_shade_rays_kernel<M, L, F>}, kernel_name("rt_shade_rays_kernel", M, L, F)},
static const KernelRow<1> kShadeRaysKernels[] = {RT_SHADE_RAYS_VARIANTS};
#undef RT_V

// The query's kernel for the parameters of f: select_query_variant's row
// (k == nullptr: the reachable depth exceeds the compiled stacks).
template <size_t ROWS>
static int pick_query_row(rt_ctx* c, const rt_frame* f, const KernelRow<1> (&table)[ROWS], KernelPick& p)
{
    QueryFacts q;
    q.depth = reachable_depth(c, f);
    q.n_tri = c->n_tri;
    q.lbuf = lbuf_on(c);
    q.bvh = rays_bvh(c);
    p = KernelPick{};
    p.v = select_query_variant(q);
    if (const KernelRow<1>* r = find_row(table, p.v)) {
        p.k = r->k[0];
        p.name = &r->name;
        p.lds = lds_bytes(p.v.flags, c->bvh_depth);
        return RT_OK;
    }
    c->err = "reachable bounce depth " + std::to_string(q.depth) + " exceeds the compiled stack (32)";
    return RT_E_UNSUPPORTED;
}
static int pick_shade_rays(rt_ctx* c, const rt_frame* f, KernelPick& p)
{
    return pick_query_row(c, f, kShadeRaysKernels, p);
}

// The refine kernels of the adaptive renders (rt_adaptive.h): the query's
// variants, selected the same way; s is a launch argument.  Named here, behind
// every other table, so that the code object keeps the other kernels' order.
#define RT_V(M, L, F) {{M, L, F}, {(const void*)&rt_refine_kernel<M, L, F>}, kernel_name("rt_refine_kernel", M, L, F)},
static const KernelRow<1> kRefineKernels[] = {RT_SHADE_RAYS_VARIANTS};
#undef RT_V
static int pick_refine(rt_ctx* c, const rt_frame* f, KernelPick& p) { return pick_query_row(c, f, kRefineKernels, p); }
static const void* edge_kernel(bool scatter)
{
    return scatter ? (const void*)&rt_edge_scatter_kernel<0> : (const void*)&rt_edge_classify_kernel<0>;
}

// n rays into d_rgb on st: one kernel, no state of the context besides the
// uploaded scene (light buffer and BVH included).  c->cam may never have been
// prepared: its fields are then null, and no query instance reads them
// (rt_shaderays.h).
static int launch_shade_rays(rt_ctx* c, const KernelPick& kp, const rt_frame* f, const float* d_rays, int n,
                             float* d_rgb, hipStream_t st)
{
    SceneDev S = scene_dev(c, c->cam, has_light_buf(kp.v.flags), false);
    FrameDev F{};  // what radiance reads outside kWf0, and nothing of the camera
    std::memcpy(F.bg, f->background, sizeof F.bg);
    F.max_bounces = f->max_bounces;
    F.min_energy = f->min_energy;
    F.scene_ior = f->scene_ior;
    const float2* rays = reinterpret_cast<const float2*>(d_rays);
    void* args[] = {&S, &F, &rays, &n, &d_rgb};
    HIP_TRY(c, hipLaunchKernel(kp.k, dim3((unsigned)(((int64_t)n + 63) / 64)), dim3(64), args, kp.lds, st));
    return RT_OK;
}

// (RT_FLAG_STATS in f->flags is ignored)
static const QueryKind kShadeRays = {
    "rt_shade_rays", "ray", "no rays or no output", {12, 0, 0}, false, true, &rt_stats::primary_rays,
    [](rt_ctx* c, Query& q) { return pick_shade_rays(c, q.f, q.kp); },
    [](rt_ctx* c, const Query& q) {
        std::memcpy(c->last.kernel, q.kp.name->s, sizeof q.kp.name->s);
        c->last.stack_depth = q.kp.v.maxd;
        c->last.light_batch = q.kp.v.lb;
    },
    [](rt_ctx* c, const Query& q, const float* d_in, void* const o[3], hipStream_t st) {
        return launch_shade_rays(c, q.kp, q.f, d_in, (int)q.n, (float*)o[0], st);
    },
    [](rt_ctx* c, const Query& q, double* ms) {
        return cpu_shade_rays(c->cpu_scene, c->cpu_threads, q.f, q.in, q.n, (float*)q.out[0], ms);
    }};

RT_EXPORT int rt_shade_rays(rt_ctx* c, const rt_frame* f, const float* rays, int64_t n, float* rgb)
{
    return query_sync(c, Query{kShadeRays, f, rays, n, {rgb}});
}

RT_EXPORT int rt_shade_rays_async(rt_ctx* c, const rt_frame* f, const float* dev_rays, int64_t n, float* dev_rgb,
                                  void* stream)
{
    return query_async(c, Query{kShadeRays, f, dev_rays, n, {dev_rgb}}, stream);
}

RT_EXPORT int rt_cpu_shade_rays(rt_ctx* c, const rt_frame* f, const float* rays, int64_t n, float* rgb)
{
    return query_cpu(c, Query{kShadeRays, f, rays, n, {rgb}});
}

// Diagnostic (include/rt_debug.h): the resolve kernel alone.
RT_EXPORT int rt_debug_resolve(rt_ctx* c, const float* samples, int width, int s, int rows_out, float* rgb,
                               unsigned* rgba, void* stream)
{
    if (!c || !samples || (!rgb && !rgba) || s < 2 || s > kSsMax || width <= 0 || width % s != 0 || rows_out < 0)
        return RT_E_ARG;
    if (c->cpu) return not_cpu(c);
    HIP_TRY(c, hipSetDevice(c->device));
    return launch_resolve(c, samples, width, s, rows_out, rgb, rgba, (hipStream_t)stream);
}

// Diagnostic (include/rt_debug.h): the last synchronous adaptive render's phases.
RT_EXPORT int rt_debug_adaptive_phases(rt_ctx* c, float* ms3, unsigned long long* flagged)
{
    if (!c) return RT_E_ARG;
    if (ms3) std::memcpy(ms3, c->ad.phase_ms, sizeof c->ad.phase_ms);
    if (flagged) *flagged = c->ad.flagged;
    return RT_OK;
}

RT_EXPORT int rt_last_stats(rt_ctx* c, rt_stats* out)
{
    if (!c || !out) return RT_E_ARG;
    *out = c->last;
    return RT_OK;
}

#ifdef RT_PROF
// Diagnostic builds only (include/rt_debug.h, RT_PROF): read and clear the per-section
// shader-clock totals (summed over waves).
extern "C" __attribute__((visibility("default"))) int rt_debug_prof(unsigned long long* out8)
{
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(rt::rt_prof_acc), 8 * sizeof(unsigned long long)) != hipSuccess)
        return RT_E_HIP;
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(rt::rt_prof_acc), z, sizeof z) != hipSuccess) return RT_E_HIP;
    return RT_OK;
}
// Per-tile records of the next renders (device buffer of 16 x u32 per 8x8
// tile, tile = tile_row * (2 * grid.x) + tile_col); NULL turns it off.
extern "C" __attribute__((visibility("default"))) int rt_debug_prof_tiles(unsigned* dev, int ntiles)
{
    if (hipMemcpyToSymbol(HIP_SYMBOL(rt::rt_prof_tiles), &dev, sizeof dev) != hipSuccess) return RT_E_HIP;
    if (hipMemcpyToSymbol(HIP_SYMBOL(rt::rt_prof_ntiles), &ntiles, sizeof ntiles) != hipSuccess) return RT_E_HIP;
    return RT_OK;
}
// Same for the wave-uniform event counts (summed over waves).
extern "C" __attribute__((visibility("default"))) int rt_debug_prof_events(unsigned long long* out8)
{
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(rt::rt_prof_ev), 8 * sizeof(unsigned long long)) != hipSuccess)
        return RT_E_HIP;
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(rt::rt_prof_ev), z, sizeof z) != hipSuccess) return RT_E_HIP;
    return RT_OK;
}
#endif

// Diagnostic (include/rt_debug.h): light-buffer summary of the uploaded
// scene: out[0] = built (0/1), out[1] = entries, out[2] = build ms,
// then per light (up to (n - 3) / 3): R, dcap-list length, dcov.
RT_EXPORT int rt_debug_lb_info(rt_ctx* c, double* out, int n)
{
    if (!c || !out || n < 3) return RT_E_ARG;
    out[0] = c->lb_ready ? 1.0 : 0.0;
    out[1] = (double)c->lb_entries;
    out[2] = c->lb_build_ms;
    if (!c->lb_ready) return RT_OK;
    std::vector<float4> meta((size_t)c->n_lights * 2);
    HIP_TRY(c, hipMemcpy(meta.data(), c->d_lb_meta, meta.size() * sizeof(float4), hipMemcpyDeviceToHost));
    for (int j = 0; j < c->n_lights && 3 + 3 * j + 2 < n; ++j) {
        int R;
        unsigned obase, nd;
        lb_meta_words(meta[2 * j], obase, R);
        std::memcpy(&nd, &meta[2 * j].z, 4);
        out[3 + 3 * j] = R;
        out[4 + 3 * j] = nd;
        out[5 + 3 * j] = meta[2 * j + 1].x;
    }
    return RT_OK;
}

// Diagnostic (include/rt_debug.h): the launch-camera light records'
// occupied-direction bounds, per light [a.x a.y a.z cosB, cells that hold an
// entry, cells whose cone is outside the stored bound] (rt_lb_region_check).
RT_EXPORT int rt_debug_lb_region(rt_ctx* c, double* out, int n)
{
    if (!c || !out || n < 6) return RT_E_ARG;
    if (c->cpu) return not_cpu(c);
    const int nl = c->n_lights;
    if (!c->uploaded || !c->lb_ready || !c->d_lrec || c->h_lrec.size() != (size_t)kLightRec * nl) {
        c->err = "no launch-camera light records";
        return RT_E_STATE;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    unsigned* d_cnt = nullptr;
    HIP_TRY(c, hipMalloc(&d_cnt, 2 * sizeof(unsigned) * (size_t)nl));
    hipError_t e = hipMemsetAsync(d_cnt, 0, 2 * sizeof(unsigned) * (size_t)nl, c->stream);
    for (int j = 0; j < nl && e == hipSuccess; ++j) {
        unsigned obase;
        int R;
        lb_meta_words(c->h_lrec[kLightRec * j + 2], obase, R);
        if (R <= 0) continue;
        hipLaunchKernelGGL(rt_lb_region_check, dim3((unsigned)((6 * R * R + 255) / 256)), dim3(256), 0, c->stream,
                           c->d_lb_off + obase, R, c->h_lrec[kLightRec * j + 3], d_cnt + 2 * j);
        e = hipGetLastError();
    }
    std::vector<unsigned> cnt(2 * (size_t)nl);
    if (e == hipSuccess) e = hipMemcpyAsync(cnt.data(), d_cnt, cnt.size() * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    hipFree(d_cnt);
    HIP_TRY(c, e);
    for (int j = 0; j < nl && 6 * j + 5 < n; ++j) {
        const float4 rg = c->h_lrec[kLightRec * j + 3];
        out[6 * j] = rg.x, out[6 * j + 1] = rg.y, out[6 * j + 2] = rg.z, out[6 * j + 3] = rg.w;
        out[6 * j + 4] = cnt[2 * j], out[6 * j + 5] = cnt[2 * j + 1];
    }
    return RT_OK;
}

// Diagnostic (include/rt_debug.h): light `light`'s first buffer's cell
// offsets (6 R^2 + 1 words, R from rt_debug_lb_info) read back into out.
RT_EXPORT int rt_debug_lb_offsets(rt_ctx* c, int light, unsigned* out, int n)
{
    if (!c || !out || light < 0) return RT_E_ARG;
    if (c->cpu) return not_cpu(c);
    if (!c->uploaded || !c->lb_ready || light >= c->n_lights || c->h_lb_meta.size() < 2 * (size_t)c->n_lights) {
        c->err = "no light buffer";
        return RT_E_STATE;
    }
    unsigned obase;
    int R;
    lb_meta_words(c->h_lb_meta[2 * (size_t)light], obase, R);
    if (R <= 0 || n != 6 * R * R + 1) return RT_E_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpy(out, c->d_lb_off + obase, (size_t)n * sizeof(unsigned), hipMemcpyDeviceToHost));
    return RT_OK;
}

// The bound's host builder alone, no device (rt_debug.h): off = the cell
// offsets of one buffer (6 R^2 + 1 rising words); out5 = [a.x a.y a.z cosB,
// cells that hold an entry].
RT_EXPORT int rt_debug_lb_region_build(const unsigned* off, int R, double* out5)
{
    if (!off || !out5 || R <= 0 || R > 1024) return RT_E_ARG;
    float rg[4];
    out5[4] = lb_region_build(off, R, rg);
    for (int q = 0; q < 4; ++q) out5[q] = rg[q];
    return RT_OK;
}

// The row chunks of a frame, no device (rt_debug.h, rt_chunks.h).
RT_EXPORT int rt_debug_row_chunks(int width, int rows, int band_rows, int px_bytes, int ss, int wf, int host_out,
                                  double host_chunk_mb, double ss_chunk_rows, int* bounds, int cap)
{
    if (!bounds || width <= 0 || rows <= 0 || px_bytes <= 0 || ss < 1) return RT_E_ARG;
    const int step = row_chunk_step(width, rows, band_rows, px_bytes, ss, wf != 0, host_out != 0, host_chunk_mb,
                                    ss_chunk_rows);
    if (step <= 0) return RT_E_ARG;
    const int n = (rows + step - 1) / step;
    if (cap < n + 1) return RT_E_ARG;
    for (int i = 0; i <= n; ++i) bounds[i] = std::min(rows, i * step);
    return n;
}

// Diagnostic (include/rt_debug.h): camera-buffer summary: out[0] = current
// (0/1), out[1] = entries, out[2] = the last synchronous build's device ms
// (its kernels, first to last; async builds are not timed), out[3] = tiles,
// out[4] = inline records (0/1), out[5] = the build's host wall time up to
// its last enqueue (ms); out[6..9] = candidate pairs, lists longer than
// 256, the longest of them, the entry capacity.
RT_EXPORT int rt_debug_cb_info(rt_ctx* c, double* out, int n)
{
    if (!c || !out || n < 4) return RT_E_ARG;
    if (c->cpu) return not_cpu(c);
    rt_ctx::CamBuf& B = c->cam.cb;
    if (B.timed) {
        float ms = 0.f;
        HIP_TRY(c, hipEventSynchronize(B.ev1));
        HIP_TRY(c, hipEventElapsedTime(&ms, B.ev0, B.ev1));
        B.build_ms = ms;
        B.timed = false;
    }
    if (B.tot_pending) {
        HIP_TRY(c, hipEventSynchronize(B.ev_tot));
        cb_harvest(B);
    }
    out[0] = B.valid ? 1.0 : 0.0;
    out[1] = (double)B.entries;
    out[2] = B.build_ms;
    out[3] = (double)B.ntiles;
    if (n > 4) out[4] = B.inline_rec ? 1.0 : 0.0;
    if (n > 5) out[5] = B.host_ms;
    // binning counters: candidate (triangle, tile) pairs tested, lists
    // sorted in LDS (longer than 256), the longest of them, the capacity
    if (n > 6) out[6] = B.hstat[1];
    if (n > 7) out[7] = B.hstat[3];
    if (n > 8) out[8] = B.hstat[4];
    if (n > 9) out[9] = (double)B.cap;
    if (n > 10) out[10] = B.hstat[6];  // 1: candidate pairs past 2^32 - 1 (every tile flagged)
    return RT_OK;
}

// Diagnostic (include/rt_debug.h): the current camera buffer against brute
// force (rt_cb_verify): out[0] = tiles whose list is not exactly the
// passing triangles (or mis-keyed), out[1] = passing pairs, out[2] = tiles
// with a list.  Synchronous.
RT_EXPORT int rt_debug_cb_verify(rt_ctx* c, unsigned long long* out)
{
    if (!c || !out) return RT_E_ARG;
    if (c->cpu) return not_cpu(c);
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = sync_all(c)) return rc;
    rt_ctx::CamBuf& B = c->cam.cb;
    if (!B.valid) {
        c->err = "no current camera buffer";
        return RT_E_STATE;
    }
    unsigned* d = nullptr;
    HIP_TRY(c, hipMalloc((void**)&d, 2 * sizeof(unsigned)));
    int rc = RT_OK;
    if (hipMemset(d, 0, 2 * sizeof(unsigned)) != hipSuccess) rc = RT_E_HIP;
    CbDev D{};
    D.tcone = B.tcone;
    D.off = B.off;
    D.cur = B.cur;
    D.flag = B.flag;
    D.ent = B.ent;
    D.cap = (unsigned)B.cap;
    D.tiles_x = B.tiles_x;
    D.tiles_y = B.ntiles / std::max(1, B.tiles_x);
    const SceneDev S = scene_dev(c, c->cam, false, true);
    unsigned h[2] = {0, 0};
    std::vector<unsigned> flags((size_t)B.ntiles);
    if (rc == RT_OK) {
        hipLaunchKernelGGL(rt_cb_verify, dim3((unsigned)((B.ntiles + 3) / 4)), dim3(256), 0, c->stream, S, D, d);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess ||
            hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(flags.data(), B.flag, flags.size() * sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess)
            rc = RT_E_HIP;
    }
    hipFree(d);
    out[0] = h[0];
    out[1] = h[1];
    out[2] = (unsigned long long)std::count(flags.begin(), flags.end(), 0u);
    return rc;
}

// Diagnostic (include/rt_debug.h): the tile words (rt_cull.h: mask and light
// classes) a launch-camera render stored for `stream` (tiny_masks; NULL: the
// synchronous renders' stream), the first n of them.  Synchronous.
// what: 0 the words, 1 the facts, 2 the lean records (16 dwords per tile).
static int tiny_records_read(rt_ctx* c, void* stream, unsigned* out, int n, int what)
{
    if (!c || !out || n < 0) return RT_E_ARG;
    if (c->cpu) return not_cpu(c);
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = sync_all(c)) return rc;
    const hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    for (const auto& q : c->tiny_masks)
        if (q.stream == st && q.valid && q.d && (size_t)n <= q.cap) {
            if (what == 2) {
                if (!q.lean) break;
                HIP_TRY(c, hipMemcpy(out, q.lean, (size_t)n * sizeof(LeanRec), hipMemcpyDeviceToHost));
                return RT_OK;
            }
            std::vector<TileRec> h((size_t)n);
            HIP_TRY(c, hipMemcpy(h.data(), q.d, (size_t)n * sizeof(TileRec), hipMemcpyDeviceToHost));
            for (int i = 0; i < n; ++i) out[i] = what ? h[(size_t)i].facts : h[(size_t)i].word;
            return RT_OK;
        }
    c->err = "no stored tile words of that size for the stream";
    return RT_E_STATE;
}
RT_EXPORT int rt_debug_tiny_words(rt_ctx* c, void* stream, unsigned* out, int n)
{
    return tiny_records_read(c, stream, out, n, 0);
}
// Diagnostic (include/rt_debug.h): the same records' second word, the tile
// facts (rt_cull.h tile_facts_pack).
RT_EXPORT int rt_debug_tiny_facts(rt_ctx* c, void* stream, unsigned* out, int n)
{
    return tiny_records_read(c, stream, out, n, 1);
}
// Diagnostic (include/rt_debug.h): the lean records stored beside them
// (rt_tile.h LeanRec), 16 dwords per tile into out[16 * n_tiles].
RT_EXPORT int rt_debug_tiny_lean(rt_ctx* c, void* stream, unsigned* out, int n_tiles)
{
    return tiny_records_read(c, stream, out, n_tiles, 2);
}

// Diagnostic (include/rt_debug.h): the last rt_upload_scene's host wall
// time by part (ms): out[0] records + device copies, out[1] cone / cluster
// prepasses, out[2] light buffer (incl. its far ladder), out[3] total.
RT_EXPORT int rt_debug_upload_info(rt_ctx* c, double* out, int n)
{
    if (!c || !out || n < 4) return RT_E_ARG;
    for (int i = 0; i < 4; ++i) out[i] = c->upload_parts_ms[i];
    // light-buffer build phases: cone records to the host, host preparation,
    // supercell counts + scan, supercell lists + cell counts + scan, entries
    for (int i = 0; i < 5 && 4 + i < n; ++i) out[4 + i] = c->lb_parts_ms[i];
    if (n > 9) out[9] = c->lb_r0;  // light 0's first buffer: cells per face edge (0: none)
    return RT_OK;
}

// Diagnostic (include/rt_debug.h): scan_u32 (the builds' device prefix sum)
// of host counts, in place like its callers: out[0..n) the exclusive
// prefixes mod 2^32, out[n] the total mod 2^32, *total the 64-bit total.
RT_EXPORT int rt_debug_scan(int device, const unsigned* in, unsigned n, unsigned* out, unsigned long long* total)
{
    if (!in || !out || !total || n == 0) return RT_E_ARG;
    if (hipSetDevice(device) != hipSuccess) return RT_E_HIP;
    unsigned* d = nullptr;
    unsigned long long* bs = nullptr;
    int rc = RT_OK;
    if (hipMalloc(&d, ((size_t)n + 1) * sizeof(unsigned)) != hipSuccess ||
        hipMalloc(&bs, scan_scratch(n) * sizeof(unsigned long long)) != hipSuccess)
        rc = RT_E_HIP;
    unsigned long long* tot = nullptr;
    if (rc == RT_OK && (hipMemcpy(d, in, (size_t)n * sizeof(unsigned), hipMemcpyHostToDevice) != hipSuccess ||
                        scan_u32(d, n, d, bs, 0, &tot) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
                        hipMemcpy(out, d, ((size_t)n + 1) * sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess ||
                        hipMemcpy(total, tot, sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess))
        rc = RT_E_HIP;
    hipFree(d);
    hipFree(bs);
    return rc;
}

// Diagnostic (include/rt_debug.h): run rt_selftest_kernel over `blocks`
// workgroups; *failures = lanes whose wave reduction or wave cone was wrong.
RT_EXPORT int rt_debug_bvh_info(rt_ctx* c, double* out, int n)
{
    if (!c || !out || n <= 0) return RT_E_ARG;
    const double v[5] = {c->d_bvh_node ? 1.0 : 0.0, (double)c->bvh_inner, (double)c->bvh_leaves, (double)c->bvh_depth,
                         c->bvh_build_ms};
    for (int i = 0; i < n; ++i) out[i] = i < 5 ? v[i] : 0.0;
    return RT_OK;
}

// Diagnostic (include/rt_debug.h): the last wavefront frame's queue counts,
// per level L = 0 .. kWfMaxLevels: out[3 L] rays of level L (L >= 1), out[3 L
// + 1] parents of level L, out[3 L + 2] straggling walks of level L.
RT_EXPORT int rt_debug_wf_counts(rt_ctx* c, unsigned* out, int n)
{
    if (!c || !out || n <= 0) return RT_E_ARG;
    if (c->cpu) return not_cpu(c);
    if (!c->wf.mem) {
        c->err = "no wavefront frame rendered";
        return RT_E_STATE;
    }
    if (int rc = sync_all(c)) return rc;
    std::vector<unsigned> w(kWfCountBytes / 4);
    HIP_TRY(c, hipMemcpy(w.data(), c->wf.dev.count, kWfCountBytes, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
        const int L = i / 3, k = i % 3;
        unsigned v = 0;
        if (L <= kWfMaxLevels) {
            if (k == 2) {
                v = w[wf_strag(L)];
            } else {
                for (int s = 0; s < kWfSeg; ++s) v += w[k == 0 ? wf_rays(L, s) : wf_pars(L, s)];
            }
        }
        out[i] = v;
    }
    return RT_OK;
}

// Diagnostic (include/rt_debug.h): the host BVH build alone (no device) over
// n triangles of 12 floats (p0, e1, e2, normal: the upload's tri[] records);
// out3 = {depth, inner nodes, leaves}.  RT_E_UNSUPPORTED past kBvhMaxTriangles.
RT_EXPORT int rt_debug_bvh_build(const float* tri12, long long n, int* out3)
{
    if (!tri12 || !out3 || n <= kBvhLeafMax) return RT_E_ARG;
    if ((size_t)n > kBvhMaxTriangles) return RT_E_UNSUPPORTED;
    std::vector<float> tri(tri12, tri12 + 12 * (size_t)n);
    BvhBuilt B;
    bvh_build(tri, (size_t)n, B);
    out3[0] = B.depth;
    out3[1] = B.inner;
    out3[2] = B.leaves;
    return RT_OK;
}

RT_EXPORT int rt_debug_bvh_rays(rt_ctx* c, const float* rays, int n, int* out_idx, float* out_t,
                                unsigned long long* tally2)
{
    if (!c || !rays || n < 0 || !out_idx || !out_t || !tally2) return RT_E_ARG;
    if (c->cpu) return not_cpu(c);
    if (!c->uploaded || !c->d_bvh_node) {
        c->err = "no bounce-ray BVH (scene without reflective/refractive surfaces or < 64 triangles)";
        return RT_E_STATE;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = sync_all(c)) return rc;
    if (n == 0) return RT_OK;
    float* d_rays = nullptr;
    int* d_idx = nullptr;
    float* d_t = nullptr;
    unsigned long long* d_tally = nullptr;
    int rc = RT_OK;
    auto chk = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && rc == RT_OK) rc = hip_fail(c, e, what);
        return rc == RT_OK;
    };
    if (chk(hipMalloc(&d_rays, (size_t)n * 6 * sizeof(float)), "hipMalloc") &&
        chk(hipMalloc(&d_idx, (size_t)n * 2 * sizeof(int)), "hipMalloc") &&
        chk(hipMalloc(&d_t, (size_t)n * 2 * sizeof(float)), "hipMalloc") &&
        chk(hipMalloc(&d_tally, 2 * sizeof(unsigned long long)), "hipMalloc") &&
        chk(hipMemcpy(d_rays, rays, (size_t)n * 6 * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy") &&
        chk(hipMemset(d_tally, 0, 2 * sizeof(unsigned long long)), "hipMemset")) {
        const SceneDev S = scene_dev(c, c->cam, false, false);
        hipLaunchKernelGGL(rt_bvh_rays_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64),
                           (unsigned)(kLdsWaveBytes + kBvhLdsBytes), c->stream, S, d_rays, n, d_idx, d_t, d_tally);
        if (chk(hipGetLastError(), "rt_bvh_rays_kernel") && chk(hipStreamSynchronize(c->stream), "sync") &&
            chk(hipMemcpy(out_idx, d_idx, (size_t)n * 2 * sizeof(int), hipMemcpyDeviceToHost), "hipMemcpy") &&
            chk(hipMemcpy(out_t, d_t, (size_t)n * 2 * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy"))
            chk(hipMemcpy(tally2, d_tally, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost), "hipMemcpy");
    }
    hipFree(d_rays);
    hipFree(d_idx);
    hipFree(d_t);
    hipFree(d_tally);
    return rc;
}

RT_EXPORT int rt_debug_bvh_rays_wave(rt_ctx* c, const float* rays, int n, int* out_idx, float* out_t)
{
    if (!c || !rays || n < 0 || !out_idx || !out_t) return RT_E_ARG;
    if (c->cpu) return not_cpu(c);
    if (!c->uploaded || !c->d_bvh_node) {
        c->err = "no bounce-ray BVH";
        return RT_E_STATE;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = sync_all(c)) return rc;
    if (n == 0) return RT_OK;
    float* d_rays = nullptr;
    int* d_idx = nullptr;
    float* d_t = nullptr;
    int rc = RT_OK;
    auto chk = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && rc == RT_OK) rc = hip_fail(c, e, what);
        return rc == RT_OK;
    };
    if (chk(hipMalloc(&d_rays, (size_t)n * 6 * sizeof(float)), "hipMalloc") &&
        chk(hipMalloc(&d_idx, (size_t)n * sizeof(int)), "hipMalloc") &&
        chk(hipMalloc(&d_t, (size_t)n * sizeof(float)), "hipMalloc") &&
        chk(hipMemcpy(d_rays, rays, (size_t)n * 6 * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy")) {
        const SceneDev S = scene_dev(c, c->cam, false, false);
        // the shared stack, then lane 0's serial stack (one step: a row)
        const unsigned lds = (unsigned)(kWfStragCap * sizeof(int) + 64 * sizeof(int) * (size_t)c->bvh_depth);
        hipLaunchKernelGGL(rt_bvh_wave_kernel, dim3((unsigned)n), dim3(64), lds, c->stream, S, d_rays, n, d_idx, d_t);
        if (chk(hipGetLastError(), "rt_bvh_wave_kernel") && chk(hipStreamSynchronize(c->stream), "sync") &&
            chk(hipMemcpy(out_idx, d_idx, (size_t)n * sizeof(int), hipMemcpyDeviceToHost), "hipMemcpy"))
            chk(hipMemcpy(out_t, d_t, (size_t)n * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy");
    }
    hipFree(d_rays);
    hipFree(d_idx);
    hipFree(d_t);
    return rc;
}

RT_EXPORT int rt_debug_selftest(int device, int blocks, unsigned* failures)
{
    if (!failures || blocks <= 0) return RT_E_ARG;
    if (hipSetDevice(device) != hipSuccess) return RT_E_HIP;
    unsigned* d = nullptr;
    if (hipMalloc(&d, sizeof(unsigned)) != hipSuccess) return RT_E_HIP;
    int rc = RT_OK;
    if (hipMemset(d, 0, sizeof(unsigned)) != hipSuccess) rc = RT_E_HIP;
    if (rc == RT_OK) {
        hipLaunchKernelGGL(rt_selftest_kernel, dim3((unsigned)blocks), dim3(256), 0, 0, 12345u, d);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(failures, d, sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess)
            rc = RT_E_HIP;
    }
    hipFree(d);
    return rc;
}

