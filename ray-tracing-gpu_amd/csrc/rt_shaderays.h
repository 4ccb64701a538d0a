// rt_shaderays.h — radiance queries of arbitrary rays (include/rt.h
// rt_shade_rays*): per ray the colour CScene::ObtenirCouleur
// (Scene.cpp:1705-1826, with the reflect / refract block re-enabled below
// max_bounces) returns for a CRayon of the caller's origin and direction,
// energy 1, 0 bounces, IOR 1 — the state the pixel loop gives a camera ray.
// No camera: the third piece beside rt_rays.h (the search) and rt_filter.h
// (the shadow filter).
//
// The colour is radiance<MAXD, LB, FLAGS>'s own (rt_kernels.hip), the frames'
// routine, with kRayQuery in its variant word: the first ray is then searched
// like every bounce ray — closest_hit<false>, or closest_hit_bvh with kBvh —
// instead of through the camera's culling state; shade_local, the bounce DFS
// and the fold are the frames' code, unchanged.  Of SceneDev the kernel reads
// the uploaded scene only (surfaces, lights, light buffer, BVH): the one
// per-camera field shade_local can reach, S.uni (the union records of the
// small-list wave culling without a light buffer), is read behind
// `cull_mode == kCullWave && S.uni` — no query instance has kCullWave without
// kLightBuf, and a context that never rendered hands a null S.uni anyway.  Of
// FrameDev radiance reads bg, min_energy, max_bounces and scene_ior, and
// nothing else outside kWf0.
// Part of the device code of rt_kernels.hip, included behind radiance and
// waves_per_eu; built with the same exactness flags.
#ifndef RT_AMD_RT_SHADERAYS_H
#define RT_AMD_RT_SHADERAYS_H

#pragma clang fp contract(off)

namespace rt {

// One ray per lane, one wave per workgroup (the BVH's per-lane stacks and the
// big lists' staging window index by lane only).  rays: n records
// [O.xyz D.xyz], read as three 8-byte words per lane, as in rt_rays_kernel;
// rgb: 3 floats per ray.  The last wave's lanes past n: without bounces they
// take ray n - 1 with live = false and drop their result, so the wave stays
// whole for the wave-level shadow culling; with bounces only valid lanes run,
// as in trace_tile.  D is used as given (not normalised).
template <int MAXD, int LB, int FLAGS>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(waves_per_eu(MAXD, FLAGS)))) void rt_shade_rays_kernel(
    const SceneDev S, const FrameDev F, const float2* __restrict__ rays, int n, float* __restrict__ rgb)
{
    static_assert(is_ray_query(FLAGS) && !has_cam_buf(FLAGS) && !is_tiny(FLAGS) && !is_wf0(FLAGS), "a query variant");
    const int lane = (int)(threadIdx.x & 63);
    const size_t i = (size_t)blockIdx.x * 64 + (size_t)lane;
    const bool valid = i < (size_t)n;
    if (MAXD == 0 || valid) {
        const float2* const r = rays + 3 * (valid ? i : (size_t)n - 1);
        const float2 w0 = r[0], w1 = r[1], w2 = r[2];
        const Vec3 O = make3(w0.x, w0.y, w1.x), D = make3(w1.y, w2.x, w2.y);
        Counters cnt;  // radiance's tallies: dead here (no counting instances)
        bool deferred = false;
        const Color c = radiance<MAXD, LB, FLAGS>(S, F, O, D, cnt, valid, -1, 0u, deferred, 0u);
        if (valid) {
            rgb[3 * i] = c.r;
            rgb[3 * i + 1] = c.g;
            rgb[3 * i + 2] = c.b;
        }
    }
}

}  // namespace rt
#endif  // RT_AMD_RT_SHADERAYS_H
