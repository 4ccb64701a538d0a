// rt_variant.h — the trace kernels' variant word: what the bits of the
// kernels' `int WAVE` template argument mean, which variant a frame takes
// (select_variant), how much dynamic LDS it needs (lds_bytes), and the list
// of every variant the build instantiates.  Plain C++17 with no HIP in it: the device
// code reads the predicates, the host half of rt_kernels.hip the selection
// and the lists, and tools/variant/variant_check.cpp checks one against the
// other.
//
// The word stays an int and the bits keep their values: the kernels' names
// (rt_stats.kernel, the label tests, tools/check_kernel_label.py,
// tools/trace_seq.py, the committed rocprof summaries) spell it in decimal.
#ifndef RT_AMD_RT_VARIANT_H
#define RT_AMD_RT_VARIANT_H

#include "rt_dims.h"

// Lights per shadow pass of the depth-0 kernels that cull by wave and do not
// use the light buffer (tools/ab_variants.py, MI355X): 1 — with the camera
// buffer and the union pre-test, C2 -5.3% and C4 -6.9% against 2; 3 is 50%
// slower.  Without triangles nothing is culled: light batches of 3.  Bounce
// kernels: per-lane culling, one light per pass (LB 3 regressed scene7 by 4%).
#ifndef RT_WAVE_LB
#define RT_WAVE_LB 1
#endif

namespace rt {

// ---- the bits
// Bits 0-1 are one field, the culling of camera and shadow rays (rt_cull.h
// closest_hit_primary, rt_shade.h shade_local):
constexpr int kCullMask = 3;
constexpr int kCullNone = 0;       // per lane
constexpr int kCullWave = 1;       // wave-level
constexpr int kCullClustered = 2;  // wave-level, two-level: the "big list" kernels (above kClusterMinTriangles);
                                   // they stage their walks in the wave's LDS window and deal tiles to the XCDs
                                   // (rt_kernels.hip tile_of_block)
// The flags:
constexpr int kLightBuf = 4;  // shadow rays through the light buffer, one light per pass (rt_lightbuf.h)
constexpr int kCamBuf = 8;    // camera rays walk the camera buffer's tile lists (rt_cambuf.h); a no-op in a
                              // launch whose S.cb_tiles_x is 0
constexpr int kRayQuery = 16;  // the first ray is the caller's, not a camera ray: it is searched like a bounce ray
                               // (rt_shaderays.h; closest_hit<false> or, with kBvh, closest_hit_bvh)
constexpr int kTiny = 32;          // the camera records come with the launch (tiny scenes, rt_trace_tiny;
                                   // rt_cull.h TinyLaunch)
constexpr int kMaskCompute = 64;   // ... and the wave computes its tile's mask instead of reading it
constexpr int kMaskStore = 128;    // ... and stores it, for its camera's later frames on the stream
constexpr int kBvh = 256;          // bounce rays through the BVH (rt_bvh.h); traversal stacks in LDS behind the window
constexpr int kWf0 = 512;          // level 0 of a wavefront frame (rt_wavefront.h): a hit that spawns children
                                   // writes a node record and its child rays instead of its colour
constexpr int kChain = 1024;       // reflect-only scenes: the bounce chain in registers instead of the DFS stack
constexpr int kLbPair = 2048;      // the light buffer's per-lane lists two entries per round (rt_shade.h lb_slot)

constexpr int cull_mode(int w) { return w & kCullMask; }
constexpr bool culls_by_wave(int w) { return cull_mode(w) != kCullNone; }
constexpr bool is_clustered(int w) { return cull_mode(w) == kCullClustered; }
constexpr bool has_light_buf(int w) { return (w & kLightBuf) != 0; }
constexpr bool has_cam_buf(int w) { return (w & kCamBuf) != 0; }
constexpr bool is_ray_query(int w) { return (w & kRayQuery) != 0; }
constexpr bool is_tiny(int w) { return (w & kTiny) != 0; }
constexpr bool computes_mask(int w) { return (w & kMaskCompute) != 0; }
constexpr bool stores_mask(int w) { return (w & kMaskStore) != 0; }
constexpr bool has_bvh(int w) { return (w & kBvh) != 0; }
constexpr bool is_wf0(int w) { return (w & kWf0) != 0; }
constexpr bool is_chain(int w) { return (w & kChain) != 0; }
constexpr bool has_lb_pair(int w) { return (w & kLbPair) != 0; }

// What a camera ray's closest hit depends on (radiance hands
// closest_hit_primary this part of its word, so that kernels which differ
// only in their shading share one instance of it).
constexpr int kCameraRayBits = kCullMask | kCamBuf | kTiny | kMaskCompute;
constexpr int camera_ray_bits(int w) { return w & kCameraRayBits; }

// The occupancy classes of the depth-0 kernels (rt_kernels.hip waves_per_eu).
// "Big" there means clustered with the light buffer AND the camera buffer:
// the same kernel without the camera buffer (kBigList alone) takes
// RT_WAVES_PER_EU, while rt_aov.h gives every clustered kernel
// RT_WAVES_PER_EU_BIG.  Both macros are 7, so nothing observable depends on
// the difference; it is recorded here and not resolved.
constexpr int kSmallList = kCullWave | kLightBuf;
constexpr int kBigList = kCullClustered | kLightBuf;
constexpr bool is_big_list_cam(int w) { return (w & (kCullMask | kLightBuf | kCamBuf)) == (kBigList | kCamBuf); }

// The composites that tests, tools and profiles spell:
constexpr int kTinyRead = kTiny | kSmallList;
constexpr int kTinyCompute = kTinyRead | kMaskCompute;
constexpr int kTinyStore = kTinyCompute | kMaskStore;
constexpr int kBvhSmall = kBvh | kCamBuf | kSmallList;  // the depth-0 kernels' camera and shadow paths
constexpr int kBvhBig = kBvh | kCamBuf | kBigList;
static_assert(kCameraRayBits == 107 && (kCullMask | kLightBuf | kCamBuf) == 15 && (kBigList | kCamBuf) == 14, "");
static_assert(kSmallList == 5 && (kSmallList | kCamBuf) == 13 && kBigList == 6, "");
static_assert((kBigList | kLbPair) == 2054 && (kBigList | kCamBuf | kLbPair) == 2062, "");
static_assert((kSmallList | kWf0) == 517 && (kSmallList | kCamBuf | kWf0) == 525, "");
static_assert((kBigList | kWf0) == 518 && (kBigList | kCamBuf | kWf0) == 526, "");
static_assert((kBigList | kLbPair | kWf0) == 2566 && (kBigList | kCamBuf | kLbPair | kWf0) == 2574, "");
static_assert(kTinyRead == 37 && kTinyCompute == 101 && kTinyStore == 229, "");
static_assert(kBvhSmall == 269 && kBvhBig == 270 && (kBvhSmall | kChain) == 1293 && (kBvhBig | kChain) == 1294, "");
static_assert((kCullWave | kCamBuf) == 9 && (kCullClustered | kCamBuf) == 10, "");
static_assert(kRayQuery == 16 && (kRayQuery | kSmallList) == 21 && (kRayQuery | kBigList) == 22, "");
static_assert((kRayQuery | kBvh | kSmallList) == 277 && (kRayQuery | kBvh | kBigList) == 278, "");

// ---- the instantiated variants: (MAXD, LB, flags) of every kernel the
// build compiles, one list per kernel template, each entry through RT_V.
// rt_kernels.hip expands them into its kernel tables and nowhere else.
// The order of the entries — and level 0 of the wavefront in a list of its
// own — is the order of the kernels in the code object: reordering a list
// reorders the image.
//
// Compiled bounce-stack capacities.  The host picks the smallest one that
// covers the bounce depth the scene can actually reach.
#define RT_STACK_DEPTHS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(8) X(12) X(16) X(20) X(32)

// rt_trace_kernel<MAXD, LB, flags, COUNT>, level 0 of a wavefront frame
#define RT_TRACE_WF0_VARIANTS                                                     \
    RT_V(0, 1, kBigList | kCamBuf | kLbPair | kWf0) RT_V(0, 1, kBigList | kLbPair | kWf0) \
    RT_V(0, 1, kBigList | kCamBuf | kWf0) RT_V(0, 1, kBigList | kWf0)             \
    RT_V(0, 1, kSmallList | kCamBuf | kWf0) RT_V(0, 1, kSmallList | kWf0)
// rt_trace_kernel, whole frames.  (A depth above 0 never takes the BVH
// entries of depth 0; they are compiled all the same.)
#define RT_TRACE_BVH_AT(N) \
    RT_V(N, 1, kBvhBig | kChain) RT_V(N, 1, kBvhSmall | kChain) RT_V(N, 1, kBvhBig) RT_V(N, 1, kBvhSmall)
#define RT_TRACE_PLAIN_AT(N) RT_V(N, 1, kChain) RT_V(N, 1, kCullNone)
#define RT_TRACE_FRAME_VARIANTS                                                                 \
    RT_V(0, 1, kBigList | kCamBuf | kLbPair) RT_V(0, 1, kBigList | kLbPair)                     \
    RT_V(0, 1, kBigList | kCamBuf) RT_V(0, 1, kBigList)                                         \
    RT_V(0, 1, kSmallList | kCamBuf) RT_V(0, 1, kSmallList)                                     \
    RT_V(0, RT_WAVE_LB, kCullClustered | kCamBuf) RT_V(0, RT_WAVE_LB, kCullClustered)           \
    RT_V(0, RT_WAVE_LB, kCullWave | kCamBuf) RT_V(0, RT_WAVE_LB, kCullWave)                     \
    RT_V(0, 3, kCullNone)                                                                       \
    RT_STACK_DEPTHS(RT_TRACE_BVH_AT) RT_STACK_DEPTHS(RT_TRACE_PLAIN_AT)
// rt_trace_tiny<MAXD, LB, flags, COUNT>, by tile-mask mode
#define RT_TINY_VARIANTS RT_V(0, 1, kTinyRead) RT_V(0, 1, kTinyCompute) RT_V(0, 1, kTinyStore)
// rt_wf_shade<flags, COUNT, STRAG>
#define RT_WF_SHADE_VARIANTS RT_V(0, 1, kBigList | kLbPair) RT_V(0, 1, kBigList) RT_V(0, 1, kSmallList)
// rt_aov_kernel<flags>
#define RT_AOV_VARIANTS                                                                       \
    RT_V(0, 1, kCullWave) RT_V(0, 1, kCullWave | kCamBuf) RT_V(0, 1, kCullClustered)          \
    RT_V(0, 1, kCullClustered | kCamBuf) RT_V(0, 1, kCullNone)
// rt_shade_rays_kernel<MAXD, LB, flags> (rt_shaderays.h), radiance queries of
// the caller's own rays.  A thinner depth list than the frames' bounds the
// build time; the host takes the smallest entry that covers the reachable
// depth (select_query_variant).  Plain: every surface per ray, per-lane
// shadows.  Lit (depth 0 only): triangles with the light buffer.  BVH (every
// depth): the first ray walks the tree like the others.  No kChain (the DFS
// gives the same bits), no kLbPair, no kCamBuf (there is no camera).
#define RT_QUERY_DEPTHS(X) X(0) X(1) X(2) X(3) X(5) X(8) X(16) X(32)
#define RT_SHADE_RAYS_AT(N) \
    RT_V(N, 1, kRayQuery | kBvh | kBigList) RT_V(N, 1, kRayQuery | kBvh | kSmallList) RT_V(N, 1, kRayQuery)
#define RT_SHADE_RAYS_VARIANTS                                             \
    RT_V(0, 1, kRayQuery | kBigList) RT_V(0, 1, kRayQuery | kSmallList) \
    RT_QUERY_DEPTHS(RT_SHADE_RAYS_AT)

// ---- the selection
struct Variant {
    int maxd = -1;  // bounce-stack capacity; -1: none compiled (a depth above 32)
    int lb = 1;     // lights per shadow pass
    int flags = 0;
};
constexpr bool operator==(const Variant& a, const Variant& b)
{
    return a.maxd == b.maxd && a.lb == b.lb && a.flags == b.flags;
}

// What the choice of a kernel depends on.
struct Facts {
    int depth = 0;  // deepest bounce level a pixel can reach
    int n_tri = 0, n_lights = 1;
    bool lbuf = false;  // shadow rays through the light buffer
    bool cbuf = false;  // the camera buffer is current for the frame
    int bvh_depth = 0;  // the BVH's depth where bounce rays walk it, else 0
    bool chain = false;  // no refracted ray can pass its gate: every bounce tree is a chain of reflections
    // small: under kSmallFramePx of output rows — the big-list kernels walk
    // the light buffer's per-lane lists two entries per round (kLbPair: their
    // 8 x 8 tiles see more cells there than the staged walk takes; C3 -6%,
    // and no gain at C5 for the registers it holds, profiles/r06/lbwalk/)
    bool small = false;
    bool wf0 = false;       // level 0 of a wavefront frame (a BVH frame: light buffer on, triangles)
    bool wf_shade = false;  // rt_wf_shade, the wavefront's bounce levels
    int tiny = -1;          // the launch-camera kernel's tile-mask mode (0 read, 1 compute, 2 compute and store), or -1
    bool aov = false;       // rt_aov_kernel
};

// Frames of fewer output pixels are "small" (Facts::small); the camera
// buffer of an async frame pays from as many (rt_camhost.h cb_async_pays).
constexpr double kSmallFramePx = 4e6;
constexpr bool small_frame(double px) { return px < kSmallFramePx; }

constexpr Variant select_variant(const Facts& f)
{
    const bool big = f.n_tri > kClusterMinTriangles;
    const int cull = big ? kCullClustered : kCullWave;
    const int cam = f.cbuf ? kCamBuf : 0;
    if (f.aov)  // no camera state for the launch-camera scenes and without triangles
        return f.tiny >= 0 || f.n_tri == 0 ? Variant{0, 1, kCullNone} : Variant{0, 1, cull | cam};
    if (f.tiny >= 0)
        return Variant{0, 1, kTinyRead | (f.tiny >= 1 ? kMaskCompute : 0) | (f.tiny >= 2 ? kMaskStore : 0)};
    // depth 0 with triangles and the light buffer
    const int lit = big ? kBigList | (f.small ? kLbPair : 0) : kSmallList;
    if (f.wf_shade) return Variant{0, 1, lit};
    if (f.wf0) return Variant{0, 1, lit | cam | kWf0};
    if (f.depth == 0 && f.n_tri > 0) return f.lbuf ? Variant{0, 1, lit | cam} : Variant{0, RT_WAVE_LB, cull | cam};
    if (f.depth == 0 && f.n_lights > 1) return Variant{0, 3, kCullNone};
    int flags = f.chain ? kChain : 0;
    if (f.bvh_depth > 0 && f.lbuf && f.n_tri > 0) flags |= big ? kBvhBig : kBvhSmall;
#define RT_DEPTH(N) \
    if (f.depth <= N) return Variant{N, 1, flags};
    RT_STACK_DEPTHS(RT_DEPTH)
#undef RT_DEPTH
    return Variant{};
}

// What the choice of a radiance query's kernel depends on (rt.h
// rt_shade_rays): no camera, no frame size.
struct QueryFacts {
    int depth = 0;      // deepest bounce level a ray can reach
    int n_tri = 0;
    bool lbuf = false;  // shadow rays through the light buffer
    bool bvh = false;   // the scene has the tree and ray queries walk it (RT_OPT_BVH, RT_OPT_RAY_BVH)
};
constexpr Variant select_query_variant(const QueryFacts& f)
{
    int flags = kRayQuery;
    if (f.lbuf && f.n_tri > 0) {
        const int lit = f.n_tri > kClusterMinTriangles ? kBigList : kSmallList;
        if (f.bvh) flags |= kBvh | lit;
        else if (f.depth == 0) flags |= lit;
    }
#define RT_DEPTH(N) \
    if (f.depth <= N) return Variant{N, 1, flags};
    RT_QUERY_DEPTHS(RT_DEPTH)
#undef RT_DEPTH
    return Variant{};
}

// Dynamic LDS per workgroup (one wave) of a variant: the staging window of
// the big-list and BVH kernels, and behind it the BVH kernels' traversal
// stacks (bvh_depth levels of 64 lanes).
constexpr unsigned lds_bytes(int flags, int bvh_depth)
{
    return (unsigned)((is_clustered(flags) || has_bvh(flags) ? kLdsWaveBytes : 0) +
                      (has_bvh(flags) ? (size_t)bvh_depth * 64 * sizeof(int) : 0));
}

// ---- a kernel's name as rt_stats.kernel spells it: stem<a,b,c> in decimal
// (numbers below 0 are left out).  It is here, and constexpr, so that the
// kernel tables hold every name ready-made — no frame formats one — and the
// host check can compare the spelling with printf's.
struct KernelName {
    char s[48] = {};
};
constexpr KernelName kernel_name(const char* stem, int a, int b = -1, int c = -1)
{
    KernelName n;
    int p = 0;
    while (*stem) n.s[p++] = *stem++;
    const int v[3] = {a, b, c};
    for (int i = 0; i < 3 && v[i] >= 0; ++i) {
        n.s[p++] = i ? ',' : '<';
        int d = 1;
        while (v[i] / d >= 10) d *= 10;
        for (; d > 0; d /= 10) n.s[p++] = (char)('0' + v[i] / d % 10);
    }
    n.s[p] = '>';
    return n;
}

}  // namespace rt
#endif  // RT_AMD_RT_VARIANT_H
