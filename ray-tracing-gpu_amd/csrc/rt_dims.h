// rt_dims.h — the sizes that the device code (rt_bvh.h, rt_lightbuf.h,
// rt_cull.h) and the plain host headers (rt_bvhhost.h, rt_scenehost.h,
// rt_variant.h) both need.  No HIP in it: the stand-alone host checks
// compile it too.
#ifndef RT_AMD_RT_DIMS_H
#define RT_AMD_RT_DIMS_H

#include <cstddef>

namespace rt {

// Levels of the bounce-ray BVH's per-lane traversal stack (rt_bvh.h): the
// host enables the BVH only for trees of depth <= kBvhStack.
constexpr int kBvhStack = 24;
constexpr int kLbGroup = 16;  // cells per supercell edge (two-level build)

// two-level (clustered) culling above this many triangles
constexpr int kClusterMinTriangles = 1024;

// Per-wave LDS windows (dynamic LDS, one per wave): the light-buffer walk's
// staged entries (rt_shade.h lb_walk_lds: kLbLdsCap entries of a, b,
// c per wave) and the camera-list walk's staged records (a, b:
// kLbLdsCap / 2 records of 64 B per wave).  The two walks never overlap in a
// wave.
#ifndef RT_LB_LDS_CAP
#define RT_LB_LDS_CAP 64
#endif
constexpr int kLbLdsCap = RT_LB_LDS_CAP;  // entries per wave window
// The wave's window in the launch's dynamic LDS (kLdsWaveBytes per wave of
// the workgroup, rt_variant.h lds_bytes): a[cap], b[cap] float4, c[cap] float2.
constexpr size_t kLdsWaveBytes = (size_t)kLbLdsCap * 40;

}  // namespace rt
#endif  // RT_AMD_RT_DIMS_H
