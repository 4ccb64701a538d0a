// rt_aov.h — the primary-hit AOV pass (include/rt.h rt_render_aov*): per
// pixel the closest surface of the camera ray — its distance t, its file
// index and its normal — and nothing else: no shading, no shadow rays.
//
// The hit is the colour kernels' own: closest_hit_primary<WAVE> (rt_cull.h)
// with the camera state their depth-0 frame would use, and hit_normal
// (rt_shade.h), so an AOV is the colour image's primary hit by construction.
// Part of the device code of rt_kernels.hip, included behind tile_of_block
// (the big-list variants deal their tiles to the XCDs as the colour kernels
// do); built with the same exactness flags.
#ifndef RT_AMD_RT_AOV_H
#define RT_AMD_RT_AOV_H

#include "rt_shade.h"

#pragma clang fp contract(off)

namespace rt {

// Store policy: plain stores in every variant, by measurement (MI355X,
// tools/aov_probe.py, profiles/r09/aov/): streaming (nontemporal) stores —
// trace_tile's choice for RGBA8 in the small-list kernels — lose here, where
// a lane writes 12 B of a 3-float plane: scene2 1920 x 1080 all planes
// 0.0154 -> 0.0315 ms (WAVE 9) and 0.0291 -> 0.0319 ms (WAVE 0), the 50k
// heightfield at 7680 x 4320 0.347 -> 0.518 ms (partial lines leave the L2
// before the neighbouring lanes' words fill them); id alone: no difference.
// -DRT_AOV_NT=1 builds the streaming stores again (A/B).
#ifndef RT_AOV_NT
#define RT_AOV_NT 0
#endif
template <typename T>
__device__ __forceinline__ void aov_store(T v, T* p)
{
    if constexpr (RT_AOV_NT != 0) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// One wave per 8 x 8 tile: trace_tile's frame geometry (slab / band row
// mapping, lanes outside the frame on a clamped pixel so that edge waves stay
// whole for the wave-level culling; their result is dropped).
// WAVE (rt_variant.h), the culling and the camera buffer only:
//   kCullNone: no per-camera state, every surface per lane
//     (closest_hit<false>: closest_hit_primary<kCullNone> would read the
//     camera's cone records, which do not exist for the scenes that render
//     here — the launch-camera scenes and those without triangles; culling
//     never changes a winner, so the hit is the same);
//   kCullWave: wave culling, without / with kCamBuf (labels 1 / 9);
//   kCullClustered: clustered two-level culling, without / with kCamBuf
//     (labels 2 / 10; the dynamic LDS window of the colour kernels' staged
//     walks).
// out_t / out_id / out_n: planar (1, 1, 3 values per pixel), each may be null.
template <int WAVE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(
    is_clustered(WAVE) ? RT_WAVES_PER_EU_BIG : RT_WAVES_PER_EU))) void rt_aov_kernel(const SceneDev S, const FrameDev F,
                                                                              float* __restrict__ out_t,
                                                                              int* __restrict__ out_id,
                                                                              float* __restrict__ out_n)
{
    static_assert((WAVE & ~(kCullMask | kCamBuf)) == 0 && cull_mode(WAVE) <= kCullClustered &&
                      (culls_by_wave(WAVE) || !has_cam_buf(WAVE)),
                  "rt_aov_kernel variants");
    int bx, by;
    if (!tile_of_block<WAVE>(F, bx, by)) return;
    const int lane = threadIdx.x & 63;
    const int px = bx * 8 + (lane & 7);
    const int ly0 = by * 8;  // the wave's first output row
    const int ly = ly0 + (lane >> 3);
    int py0 = F.row_begin + ly0, rend = F.row_end;
    if (F.band_rows > 0) {
        py0 = ((ly0 / F.band_rows) * F.band_count + F.band_index) * F.band_rows + ly0 % F.band_rows;
        rend = F.height;
    }
    if (py0 >= rend) return;  // the whole wave lies past the frame (wave-uniform)
    const int py = py0 + (lane >> 3);
    const bool valid = px < F.width && py < rend;
    const int pxc = px < F.width ? px : F.width - 1;
    const int pyc = py < rend ? py : rend - 1;
    const Vec3 D = camera_dir(F, pxc, pyc);
    const Vec3 O = make3(F.cam[0], F.cam[1], F.cam[2]);

    Counters cnt;  // the hit routines' tallies: dead here
    float t;
    int idx;
    if constexpr (cull_mode(WAVE) == kCullNone) {
        idx = closest_hit<false>(S, O, D, t, cnt);
    } else {
        // the camera-buffer tile, as in trace_tile
        int tile = -1;
        if (has_cam_buf(WAVE) && S.cb_tiles_x > 0 && (py0 & 7) == 0) {
            tile = (py0 >> 3) * S.cb_tiles_x + bx;
            if (S.cb_flag[tile]) tile = -1;
        }
        idx = closest_hit_primary<WAVE>(S, O, D, t, cnt, tile);
    }
    const bool hit = idx >= 0;
    // The reference's empty CIntersection for a miss: distance -1, normal 0.
    Vec3 N = make3(0.f, 0.f, 0.f);
    if (out_n && __any(hit & valid)) {
        // A tile usually sees one surface: its normal record then comes by
        // scalar (broadcast) loads, as in radiance<0>.
        const int sidx = hit ? idx : 0;
        const int s0 = __builtin_amdgcn_readfirstlane(sidx);
        Vec3 n;
        if (__all(sidx == s0)) n = hit_normal(S, s0, O, D, t);
        else n = hit_normal(S, sidx, O, D, t);
        if (hit) N = n;
    }
    if (!valid) return;
    const size_t o = (size_t)ly * F.width + px;
    if (out_t) aov_store(hit ? t : -1.0f, out_t + o);
    if (out_id) aov_store(hit ? idx : -1, out_id + o);
    if (out_n) {
        aov_store(N.x, out_n + 3 * o);
        aov_store(N.y, out_n + 3 * o + 1);
        aov_store(N.z, out_n + 3 * o + 2);
    }
}

}  // namespace rt
#endif  // RT_AMD_RT_AOV_H
