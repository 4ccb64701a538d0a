// rt_rays.h — closest-hit queries of arbitrary rays (include/rt.h
// rt_trace_rays*): per ray what CScene::ObtenirCouleur's search
// (Scene.cpp:1705-1715) holds when it leaves its loop — the winner's
// distance, file index and normal — for an origin and a direction the caller
// chooses.  No camera, no shading, no state of the context.
//
// The hit is the bounce rays' own: closest_hit<false> (every surface) or
// closest_hit_bvh (rt_bvh.h: planes and quadrics one by one, the triangles
// through the exact BVH; a ray that is not finite or not of unit length walks
// every triangle there, which is what keeps a direction "as given" exact), and
// hit_normal (rt_shade.h) — the values rt_aov_kernel writes for a camera ray.
// Part of the device code of rt_kernels.hip, included behind rt_bvh.h; built
// with the same exactness flags.
#ifndef RT_AMD_RT_RAYS_H
#define RT_AMD_RT_RAYS_H

#include "rt_bvh.h"
#include "rt_shade.h"

#pragma clang fp contract(off)

namespace rt {

// The serial walk's budget (steps: inner nodes + leaves; the wavefront's two
// values are 128 and 320) and the finishing walk's shared LDS stack (entries;
// bvh_walk_wave needs it comfortably above the tree's depth + 96).
// RT_RAYS_BUDGET 0: no budget, no finishing loop, no shared stack.
#ifndef RT_RAYS_BUDGET
#define RT_RAYS_BUDGET 128
#endif
#ifndef RT_RAYS_CAP
#define RT_RAYS_CAP 1024
#endif
constexpr int kRaysBudget = RT_RAYS_BUDGET;
constexpr int kRaysCap = RT_RAYS_CAP;
static_assert(kRaysBudget >= 0 && kRaysCap >= kBvhStack + 96 + 32 && kRaysCap % 4 == 0, "rt_rays_kernel's LDS carve");
// The shared stack lies in front of the per-lane stacks (rt_bvh_wave_kernel's carve).
constexpr size_t kRaysWin = kRaysBudget > 0 ? (size_t)kRaysCap * sizeof(int) : 0;
// Dynamic LDS of one workgroup (one wave) of rt_rays_kernel<1> for a tree of `depth`.
constexpr size_t rays_lds_bytes(int depth) { return kRaysWin + (size_t)depth * 64 * sizeof(int); }

// One ray per lane, one wave per workgroup (bvh_stack indexes by lane only).
// rays: n records [O.xyz D.xyz], read as three 8-byte words per lane — a wave
// reads 1,536 contiguous bytes.  Lanes past n in the last wave take ray n - 1
// and drop their result: waves stay whole for the cooperative walk.
// BVH 0: every surface.  BVH 1: the budgeted serial walk, then the wave
// finishes its stragglers itself, one at a time, lowest lane first — the ray
// and its partial minimum are broadcast, bvh_walk_wave runs with all 64 lanes
// over the shared stack, and the result goes back to the ray's lane.  No
// queue, no atomics, no second launch: the kernel touches its arguments only.
// out_t / out_id / out_n: planar (1, 1, 3 values per ray), each may be null;
// plain stores (rt_aov.h's measurement).
template <int BVH>
__global__ __launch_bounds__(64) void rt_rays_kernel(const SceneDev S, const float2* __restrict__ rays, int n,
                                                       float* __restrict__ out_t, int* __restrict__ out_id,
                                                       float* __restrict__ out_n)
{
    const int lane = (int)(threadIdx.x & 63);
    const size_t i = (size_t)blockIdx.x * 64 + (size_t)lane;
    const bool valid = i < (size_t)n;
    const float2* const r = rays + 3 * (valid ? i : (size_t)n - 1);
    const float2 w0 = r[0], w1 = r[1], w2 = r[2];
    const Vec3 O = make3(w0.x, w0.y, w1.x), D = make3(w1.y, w2.x, w2.y);

    Counters cnt;  // the hit routines' tallies: dead here
    float t;
    int idx;
    if constexpr (BVH == 0) {
        idx = closest_hit<false>(S, O, D, t, cnt);
    } else if constexpr (kRaysBudget == 0) {
        idx = closest_hit_bvh<0, 0>(S, O, D, t, cnt);
    } else {
        bool str = false;
        idx = closest_hit_bvh<kRaysWin, kRaysBudget>(S, O, D, t, cnt, &str);
        // the wave is whole again: its per-lane stacks are dead, a straggler
        // starts over from the root under its partial minimum
        extern __shared__ float4 rt_lds_dyn[];
        int* const shared = reinterpret_cast<int*>(rt_lds_dyn);
        for (unsigned long long m = __ballot(str); m != 0; m &= m - 1) {
            const int l = (int)__builtin_ctzll(m);
            const Vec3 o = make3(readlanef(O.x, l), readlanef(O.y, l), readlanef(O.z, l));
            const Vec3 d = make3(readlanef(D.x, l), readlanef(D.y, l), readlanef(D.z, l));
            float bt = readlanef(t, l);
            int bi = __builtin_amdgcn_readlane(idx, l);
            bvh_walk_wave(S, o, d, bt, bi, shared, kRaysCap, cnt);
            if (lane == l) {
                t = bt;
                idx = bi;
            }
        }
    }
    const bool hit = idx >= 0;
    // The reference's empty CIntersection for a miss: distance -1, normal 0.
    Vec3 N = make3(0.f, 0.f, 0.f);
    if (out_n && __any(hit & valid)) {
        // coherent rays usually see one surface: its record then comes by
        // scalar loads, as in rt_aov_kernel
        const int sidx = hit ? idx : 0;
        const int s0 = __builtin_amdgcn_readfirstlane(sidx);
        Vec3 nn;
        if (__all(sidx == s0)) nn = hit_normal(S, s0, O, D, t);
        else nn = hit_normal(S, sidx, O, D, t);
        if (hit) N = nn;
    }
    if (!valid) return;
    if (out_t) out_t[i] = hit ? t : -1.0f;
    if (out_id) out_id[i] = hit ? idx : -1;
    if (out_n) {
        out_n[3 * i] = N.x;
        out_n[3 * i + 1] = N.y;
        out_n[3 * i + 2] = N.z;
    }
}

}  // namespace rt
#endif  // RT_AMD_RT_RAYS_H
