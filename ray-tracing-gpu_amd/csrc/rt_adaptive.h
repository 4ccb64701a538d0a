// rt_adaptive.h — adaptive supersampling (include/rt.h rt_render_adaptive*):
// the edge classification, written once for both backends, and the HIP kernels
// that classify a base frame and refine its flagged pixels.
//
// Definition (DESIGN.md "Adaptive supersampling").  B is the plain frame at
// W x H of the sample frame at s W x s H (s in 2, 4, 8: its pixels are the
// sample lattice S[s y][s x], bit for bit).  Pixel p is flagged when, for one
// of its 4-neighbours q inside the WHOLE frame and one requested criterion,
//   RT_EDGE_ID      I(p) != I(q)
//   RT_EDGE_NORMAL  exactly one of I(p), I(q) is a miss, or both hit and
//                   ((Np.x Nq.x + Np.y Nq.y) + Np.z Nq.z) < normal_cos
//   RT_EDGE_COLOUR  fabsf(C(p).c - C(q).c) > colour_delta in some channel
// (C the float colour of B, I / N its primary-hit id and normal; a NaN
// compares false).  An unflagged pixel keeps C(p); a flagged one becomes
// resolve_px (rt_resolve.h) of its s x s samples, each the frames' own
// radiance of the sample frame's camera ray.
#ifndef RT_AMD_RT_ADAPTIVE_H
#define RT_AMD_RT_ADAPTIVE_H

#include "rt_math.h"
#include "rt_resolve.h"

#pragma clang fp contract(off)

namespace rt {

constexpr int kEdgeId = 1, kEdgeNormal = 2, kEdgeColour = 4;  // rt.h RT_EDGE_*
constexpr int kEdgeAll = kEdgeId | kEdgeNormal | kEdgeColour;

// The base frame's planes as the classification reads them: packed rows of
// `width` pixels, plane row 0 = frame row `row0` (the slab's first row, or
// the halo row below it).  rgb: 3 floats per pixel; id: the primary hit's file
// index (-1: a miss); n: its normal, 3 floats.  id is read for RT_EDGE_ID and
// RT_EDGE_NORMAL, n for RT_EDGE_NORMAL, rgb for RT_EDGE_COLOUR only.
struct EdgePlanes {
    const float* rgb;
    const int* id;
    const float* n;
    int width, height;  // the whole base frame
    int row0;
};

// The criteria that separate pixel p from its neighbour q (indices into the planes).
RT_HD int edge_pair(const EdgePlanes& P, size_t p, size_t q, int criteria, float normal_cos, float colour_delta)
{
    int m = 0;
    if (criteria & (kEdgeId | kEdgeNormal)) {
        const int ip = P.id[p], iq = P.id[q];
        if ((criteria & kEdgeId) && ip != iq) m |= kEdgeId;
        if (criteria & kEdgeNormal) {
            if ((ip < 0) != (iq < 0)) {
                m |= kEdgeNormal;
            } else if (ip >= 0) {
                const float* a = P.n + 3 * p;
                const float* b = P.n + 3 * q;
                if (((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) < normal_cos) m |= kEdgeNormal;
            }
        }
    }
    if (criteria & kEdgeColour) {
        const float* a = P.rgb + 3 * p;
        const float* b = P.rgb + 3 * q;
        if (fabsf(a[0] - b[0]) > colour_delta || fabsf(a[1] - b[1]) > colour_delta ||
            fabsf(a[2] - b[2]) > colour_delta)
            m |= kEdgeColour;
    }
    return m;
}

// mask(p) of pixel (x, y) of the base frame: the OR over its 4-neighbours
// inside the frame.  The planes must hold rows y - 1 .. y + 1 (those inside).
RT_HD int edge_mask(const EdgePlanes& P, int x, int y, int criteria, float normal_cos, float colour_delta)
{
    const size_t w = (size_t)P.width, p = (size_t)(y - P.row0) * w + (size_t)x;
    int m = 0;
    if (x > 0) m |= edge_pair(P, p, p - 1, criteria, normal_cos, colour_delta);
    if (x + 1 < P.width) m |= edge_pair(P, p, p + 1, criteria, normal_cos, colour_delta);
    if (y > 0) m |= edge_pair(P, p, p - w, criteria, normal_cos, colour_delta);
    if (y + 1 < P.height) m |= edge_pair(P, p, p + w, criteria, normal_cos, colour_delta);
    return m;
}

// The kernels: part of the device code of rt_kernels.hip, which includes this
// file behind rt_shaderays.h (radiance, camera_dir, waves_per_eu above it).
#if (defined(__HIPCC__) || defined(__HIP__)) && defined(RT_AMD_RT_SHADERAYS_H)

// One lane per output pixel t of the slab (rows x width, packed; output row 0
// = frame row `row_begin`): the mask byte, the 0 / 1 flag word the scan turns
// into list offsets, and the pixel's base colour into the outputs (a flagged
// pixel's are overwritten by rt_refine_kernel, behind this kernel on the
// stream).  rgb / rgba / mask may be null.
// (This kernel and the next are templates only to be emitted where the host
// code first names them, behind every other kernel of the code object, whose
// order and addresses they leave alone: LAST has no other meaning.)
template <int LAST>
__global__ __launch_bounds__(256) void rt_edge_classify_kernel(const EdgePlanes P, int row_begin, unsigned n,
                                                               int criteria, float normal_cos, float colour_delta,
                                                               unsigned* __restrict__ flag, float* __restrict__ rgb,
                                                               unsigned* __restrict__ rgba,
                                                               unsigned char* __restrict__ mask)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int q = (int)(t / (size_t)P.width), x = (int)(t % (size_t)P.width), y = row_begin + q;
    const int m = edge_mask(P, x, y, criteria, normal_cos, colour_delta);
    flag[t] = m != 0 ? 1u : 0u;
    if (mask) mask[t] = (unsigned char)m;
    const float* c = P.rgb + 3 * ((size_t)(y - P.row0) * (size_t)P.width + (size_t)x);
    const Color C{c[0], c[1], c[2]};
    if (rgb) {
        rgb[3 * t] = C.r;
        rgb[3 * t + 1] = C.g;
        rgb[3 * t + 2] = C.b;
    }
    if (rgba) rgba[t] = resolve_rgba8(C);
}

// The flags' exclusive scan (rt_scan.h: off[t], off[n] = the total) -> the
// row-major list of flagged pixel indices: no atomics, a deterministic order.
template <int LAST>
__global__ __launch_bounds__(256) void rt_edge_scatter_kernel(const unsigned* __restrict__ flag,
                                                              const unsigned* __restrict__ off, unsigned n,
                                                              unsigned* __restrict__ list)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n && flag[t]) list[off[t]] = (unsigned)t;
}

// The refine pass: s x s samples of every flagged pixel, resolved in LDS.
// One wave per workgroup, as for the query kernels; a wave owns 64 / s^2
// flagged pixels of the list at a time: lane l traces sample l % s^2 of pixel
// slot l / s^2, sample k = j s + i being sample-frame pixel (s x + i, s y + j)
// — rt_render_ss's order.  The ray is camera_dir of the SAMPLE frame F, the
// colour radiance<MAXD, 1, FLAGS> with kRayQuery exactly as
// rt_shade_rays_kernel calls it.  The colours go to a 768-byte tile, per pixel
// s rows of 3 s floats, and the first lane of each pixel runs resolve_px on
// its part and overwrites the pixel's outputs.  Tails as in the query kernel:
// without bounces the lanes past the list take its last pixel with live =
// false, so the wave stays whole; with bounces only valid lanes run.
// The grid is fixed (at most kRefineGrid workgroups, each striding over the
// groups of pixels); *total, the scan's device-resident count of flagged
// pixels, bounds the loop, so no count is read back to size a launch.
//   ls       : log2 s (1, 2, 3)
//   wo       : the output's width; row_begin: the frame row of output row 0
//   list     : flagged pixels, indices into the packed output
constexpr int kRefineGrid = 2048;
template <int MAXD, int LB, int FLAGS>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(waves_per_eu(MAXD, FLAGS)))) void rt_refine_kernel(
    const SceneDev S, const FrameDev F, const unsigned* __restrict__ list, const unsigned* __restrict__ total, int ls,
    int wo, int row_begin, float* __restrict__ rgb, unsigned* __restrict__ rgba)
{
    static_assert(is_ray_query(FLAGS) && !has_cam_buf(FLAGS) && !is_tiny(FLAGS) && !is_wf0(FLAGS), "a query variant");
    __shared__ float tile[64 * 3];
    const int lane = (int)(threadIdx.x & 63);
    const int s = 1 << ls, per = 64 >> (2 * ls);
    const int slot = lane >> (2 * ls), smp = lane & ((1 << (2 * ls)) - 1);
    const int i = smp & (s - 1), j = smp >> ls;
    const unsigned count = __builtin_amdgcn_readfirstlane(*total);
    const unsigned groups = (count + (unsigned)per - 1u) / (unsigned)per;
    const Vec3 O = make3(F.cam[0], F.cam[1], F.cam[2]);
    for (unsigned g = blockIdx.x; g < groups; g += gridDim.x) {
        const unsigned idx = g * (unsigned)per + (unsigned)slot;
        const bool valid = idx < count;
        unsigned pix = 0;
        if (MAXD == 0 || valid) {
            pix = list[valid ? idx : count - 1u];
            const int x = (int)(pix % (unsigned)wo), y = row_begin + (int)(pix / (unsigned)wo);
            const Vec3 D = camera_dir(F, s * x + i, s * y + j);
            Counters cnt;  // radiance's tallies: dead here (no counting instances)
            bool deferred = false;
            const Color c = radiance<MAXD, LB, FLAGS>(S, F, O, D, cnt, valid, -1, 0u, deferred, 0u);
            tile[3 * lane] = c.r;
            tile[3 * lane + 1] = c.g;
            tile[3 * lane + 2] = c.b;
        }
        __syncthreads();
        if (valid && smp == 0) {
            const Color c = resolve_px(tile + 3 * (slot << (2 * ls)), (size_t)(3 * s), s);
            if (rgb) {
                rgb[3 * (size_t)pix] = c.r;
                rgb[3 * (size_t)pix + 1] = c.g;
                rgb[3 * (size_t)pix + 2] = c.b;
            }
            if (rgba) rgba[pix] = resolve_rgba8(c);
        }
        __syncthreads();  // (the tile is rewritten by the next group)
    }
}

#endif  // HIP

}  // namespace rt

#endif  // RT_AMD_RT_ADAPTIVE_H
