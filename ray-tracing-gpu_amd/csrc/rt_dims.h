// rt_dims.h — the two sizes that the device code (rt_bvh.h, rt_lightbuf.h)
// and the plain host headers (rt_bvhhost.h, rt_scenehost.h) both need.  No
// HIP in it: the stand-alone host checks compile it too.
#ifndef RT_AMD_RT_DIMS_H
#define RT_AMD_RT_DIMS_H

namespace rt {

// Levels of the bounce-ray BVH's per-lane traversal stack (rt_bvh.h): the
// host enables the BVH only for trees of depth <= kBvhStack.
constexpr int kBvhStack = 24;
constexpr int kLbGroup = 16;  // cells per supercell edge (two-level build)

}  // namespace rt
#endif  // RT_AMD_RT_DIMS_H
