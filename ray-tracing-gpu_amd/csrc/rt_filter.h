// rt_filter.h — shadow-filter (occlusion) queries of arbitrary segments
// (include/rt.h rt_filter_rays*): per segment P -> P + L what
// CScene::ObtenirFiltreDeSurface (Scene.cpp:1842-1861) returns for the
// unnormalised vector L — the product, in file order, of colour x Kt over
// every surface whose hit lies strictly between EPSILON and |L|.  No light,
// no camera, no state of the context.
//
// rt_filter_kernel<0> is shadow_filter's (rt_shade.h) two bodies without the
// per-light cones: the file-order product over every surface, or — when
// S.shadow_split — an any-hit pass over the opaque surfaces and the file-order
// product over the translucent list.
//
// rt_filter_kernel<1> (shadow_split scenes with the BVH of rt_bvh.h) tests the
// planes and quadrics one by one and sends the triangles through a segment
// any-hit walk of the BVH.  Why it returns <0>'s bits:
//  * Boxes.  rt_bvh.h proves that a triangle hit REPORTED at t~ by a finite
//    ray of unit length has its point O + t~ D inside the box grown by alpha sb,
//    so the widened slab interval [t0, t1] of bvh_box contains t~.  A hit that
//    counts here has EPS < t~ < dist; a box with t1 < EPS or t0 > dist (bvh_box
//    with have = true, bt = dist; t0 > t1: the ray misses the grown box) holds
//    no counted hit, and skipping it removes no factor.  Segments that are not
//    finite or not of unit length after the division (|D|^2 outside
//    [0.98, 1.02]: an under- or overflowing dist) test every triangle instead.
//  * Early exit.  shadow_split means every factor is finite and >= +0 (no
//    negative zero), so the running product is never negative, NaN or inf,
//    and one opaque factor (+0, +0, +0) makes it exactly (+0, +0, +0) whatever
//    is multiplied before or after it: a lane may stop at its first opaque hit.
//  * Sorting.  float multiplication is not associative, so the translucent
//    factors must be multiplied in file order.  Every triangle lies in exactly
//    one leaf and a leaf is visited at most once (each node is pushed or
//    entered once), so the walk finds each translucent hit once, in tree
//    order; their file indices — with those of the translucent planes and
//    quadrics that hit — are put in ascending order before the factors
//    (geometry record words 13..15, the values shadow_hit_record multiplies)
//    are multiplied.  A lane that finds more than kFilterList hits drops its
//    list and runs <0>'s file-order loop over S.translucent: the same
//    tests, the same order, the same bits.
// How a leaf triangle is known to be translucent: word 10 of its bvh_tri
// record ([2].z, int 1; 0: opaque), written by scene_host_bvh and read by no
// other kernel.
// No step budget and no wave-finish pass: an occluded walk ends early by
// construction, and rt_rays_kernel's budget measured 3.1 times slower than
// none on the triangle soup.
// Part of the device code of rt_kernels.hip, included behind rt_bvh.h; built
// with the same exactness flags.
#ifndef RT_AMD_RT_FILTER_H
#define RT_AMD_RT_FILTER_H

#include "rt_bvh.h"
#include "rt_shade.h"

#pragma clang fp contract(off)

namespace rt {

// Translucent hits a lane of <1> remembers (file indices) before it falls
// back to the file-order loop.
constexpr int kFilterList = 8;
// Dynamic LDS of one workgroup (one wave) of rt_filter_kernel<1> for a tree of
// `depth`: the per-lane stacks (entry i of lane l at word 64 i + l), then the
// per-lane lists in the same lane-contiguous rows.
constexpr size_t filter_lds_bytes(int depth) { return (size_t)(depth + kFilterList) * 64 * sizeof(int); }

// Scene.cpp:1842-1861 over every surface (shadow_filter without a light).
__device__ __forceinline__ Color filter_all(const SceneDev& S, const Vec3 P, const Vec3 D, float dist, Counters& cnt)
{
    Color F{1.0f, 1.0f, 1.0f};
    if (!S.shadow_split) {
        for (int i = 0; i < S.n_surf; ++i) {
            Color fc;
            if (shadow_hit_record(S.geom + 4 * i, P, D, dist, fc, cnt)) F *= fc;
        }
        return F;
    }
    // Opaque surfaces, any hit: each lane tests on its own, the wave leaves
    // once every lane is occluded.
    bool occluded = false;
    for (int k = 0; k < S.n_plane_opaque; ++k) {
        if (!__any(!occluded)) break;
        const float4 a = S.plane[2 * k];
        float t;
        const bool ok = hit_plane(make_float4(0.f, a.x, a.y, a.z), make_float4(a.w, 0.f, 0.f, 0.f), P, D, t);
        occluded |= ok & (t > kEps) & (t < dist);
    }
    for (int k = 0; k < S.n_quad_opaque; ++k) {
        if (!__any(!occluded)) break;
        const float4* r = S.quad + 3 * k;
        const float4 a = r[0], b = r[1], c = r[2];
        float t;
        const bool ok = hit_quadric(make_float4(0.f, a.x, a.y, a.z), make_float4(a.w, b.x, b.y, b.z),
                                    make_float4(b.w, c.x, c.y, 0.f), P, D, t);
        occluded |= ok & (t > kEps) & (t < dist);
    }
    for (int k = 0; k < S.n_tri_opaque; ++k) {
        if (!__any(!occluded)) break;
        const TriRec tr = load_tri(S, k);
        float t;
        const bool ok = hit_triangle(make_float4(0.f, tr.p0.x, tr.p0.y, tr.p0.z),
                                     make_float4(tr.e1.x, tr.e1.y, tr.e1.z, tr.e2.x),
                                     make_float4(tr.e2.y, tr.e2.z, 0.f, 0.f), P, D, t);
        occluded |= ok & (t > kEps) & (t < dist);
    }
    if (__any(!occluded)) {  // translucent surfaces, file order
        for (int j = 0; j < S.n_translucent; ++j) {
            Color fc;
            if (shadow_hit_record(S.geom + 4 * S.translucent[j], P, D, dist, fc, cnt)) F *= fc;
        }
    }
    return occluded ? Color{0.0f, 0.0f, 0.0f} : F;
}

// The same value for a shadow_split scene with the BVH (the header's proof).
// steps: inner nodes + leaves this lane's walk took (tools/filter_probe.py, an RT_FILTER_STEPS build).
__device__ __forceinline__ Color filter_bvh(const SceneDev& S, const Vec3 P, const Vec3 D, float dist, int depth,
                                            Counters& cnt, int& steps)
{
    extern __shared__ float4 rt_lds_dyn[];
    const int lane = (int)(threadIdx.x & 63);
    int* const stk = reinterpret_cast<int*>(rt_lds_dyn) + lane;
    int* const lst = stk + 64 * depth;
    bool occluded = false, overflow = false;
    int nl = 0;  // entries of lst
    auto remember = [&](bool hit, int idx) {
        if (hit & !overflow) {
            if (nl < kFilterList) lst[64 * nl++] = idx;
            else overflow = true;
        }
    };
    for (int k = 0; k < S.n_plane; ++k) {
        if (!__any(!occluded)) break;
        const float4 a = S.plane[2 * k], b = S.plane[2 * k + 1];
        float t;
        const bool ok = hit_plane(make_float4(0.f, a.x, a.y, a.z), make_float4(a.w, 0.f, 0.f, 0.f), P, D, t);
        const bool hit = ok & (t > kEps) & (t < dist);
        if (k < S.n_plane_opaque) occluded |= hit;
        else remember(hit, __float_as_int(b.x));
    }
    for (int k = 0; k < S.n_quad; ++k) {
        if (!__any(!occluded)) break;
        const float4* r = S.quad + 3 * k;
        const float4 a = r[0], b = r[1], c = r[2];
        float t;
        const bool ok = hit_quadric(make_float4(0.f, a.x, a.y, a.z), make_float4(a.w, b.x, b.y, b.z),
                                    make_float4(b.w, c.x, c.y, 0.f), P, D, t);
        const bool hit = ok & (t > kEps) & (t < dist);
        if (k < S.n_quad_opaque) occluded |= hit;
        else remember(hit, __float_as_int(c.z));
    }
    const float dd = dot(D, D);
    const bool walk = finite3(P) & finite3(D) & (dd >= 0.98f) & (dd <= 1.02f);  // closest_hit_bvh's condition
    if (__any(!walk & !occluded)) {
        // every opaque triangle (the box bound assumes a finite, unit ray);
        // the translucent ones through the file-order loop below
        bool mine = !walk & !occluded;
        for (int k = 0; k < S.n_tri_opaque; ++k) {
            if (!__any(mine)) break;
            const TriRec tr = load_tri(S, k);
            float t;
            const bool ok = hit_triangle(make_float4(0.f, tr.p0.x, tr.p0.y, tr.p0.z),
                                         make_float4(tr.e1.x, tr.e1.y, tr.e1.z, tr.e2.x),
                                         make_float4(tr.e2.y, tr.e2.z, 0.f, 0.f), P, D, t);
            if (mine & ok & (t > kEps) & (t < dist)) {
                occluded = true;
                mine = false;
            }
        }
        if (!walk) overflow = true;
    }
    if (walk & !occluded) {
        const Vec3 inv = make3(__builtin_amdgcn_rcpf(D.x), __builtin_amdgcn_rcpf(D.y), __builtin_amdgcn_rcpf(D.z));
        // closest_hit_bvh's while-while loop; the segment's end bounds every
        // box from the first node on, and an occluded lane stops walking
        constexpr int kDone = 0x7fffffff;
        int node = 0, leaf = 0, sp = 0;
        for (;;) {
            while ((node >= 0) & (node != kDone)) {
                const float4* n = S.bvh_node + 4 * (size_t)node;
                const float4 a0 = n[0], a1 = n[1], b0 = n[2], b1 = n[3];
                ++steps;
                const int r0 = __float_as_int(a1.w), r1 = __float_as_int(b1.w);
                float t0, t1;
                const bool h0 = bvh_box(a0, a1, P, inv, true, dist, t0);
                const bool h1 = bvh_box(b0, b1, P, inv, true, dist, t1);
                if (h0 & h1) {
                    const bool near0 = !(t1 < t0);
                    stk[64 * sp] = near0 ? r1 : r0;
                    ++sp;
                    node = near0 ? r0 : r1;
                } else if (h0 | h1) {
                    node = h0 ? r0 : r1;
                } else {
                    node = sp > 0 ? stk[64 * --sp] : kDone;
                }
                if ((node < 0) & (leaf == 0)) {  // postpone the first leaf, walk on
                    leaf = node;
                    node = sp > 0 ? stk[64 * --sp] : kDone;
                }
                if (__all(leaf != 0)) break;
            }
            while (leaf != 0) {
                const unsigned enc = ~(unsigned)leaf;
                const int first = (int)(enc >> 4), count = (int)(enc & 15u) + 1;
                ++steps;
                for (int k = first; k < first + count; ++k) {
                    const float4* r = S.bvh_tri + 3 * (size_t)k;
                    const float4 a = r[0], b = r[1], c = r[2];
                    float t;
                    const bool ok = hit_triangle(make_float4(0.f, a.x, a.y, a.z), make_float4(a.w, b.x, b.y, b.z),
                                                 make_float4(b.w, c.x, 0.f, 0.f), P, D, t);
                    const bool hit = ok & (t > kEps) & (t < dist);
                    if (__float_as_int(c.z) != 0) remember(hit, __float_as_int(c.y));
                    else occluded |= hit;
                }
                leaf = 0;
                if ((node < 0) & (node != kDone)) {  // the leaf that ended the inner loop
                    leaf = node;
                    node = sp > 0 ? stk[64 * --sp] : kDone;
                }
                if (occluded) {  // done: the result is (0, 0, 0)
                    leaf = 0;
                    node = kDone;
                }
            }
            if (node == kDone) break;
        }
    }
    Color F{1.0f, 1.0f, 1.0f};
    if (!occluded & !overflow) {
        // ascending file index (insertion sort of at most kFilterList entries), then the product
        for (int i = 1; i < nl; ++i) {
            const int v = lst[64 * i];
            int j = i;
            while (j > 0 && lst[64 * (j - 1)] > v) {
                lst[64 * j] = lst[64 * (j - 1)];
                --j;
            }
            lst[64 * j] = v;
        }
        for (int i = 0; i < nl; ++i) {
            const float4 d = S.geom[4 * (size_t)lst[64 * i] + 3];
            F *= Color{d.y, d.z, d.w};
        }
    }
#ifdef RT_FILTER_STEPS
    if (overflow & walk) steps |= 1 << 30;  // (the probe's overflow share)
#endif
    if (__any(overflow & !occluded)) {  // <0>'s loop for the lanes without a list
        Color G{1.0f, 1.0f, 1.0f};
        for (int j = 0; j < S.n_translucent; ++j) {
            Color fc;
            if (shadow_hit_record(S.geom + 4 * S.translucent[j], P, D, dist, fc, cnt)) G *= fc;
        }
        if (overflow) F = G;
    }
    return occluded ? Color{0.0f, 0.0f, 0.0f} : F;
}

// One segment per lane, one wave per workgroup (the stacks index by lane).
// segs: n records [P.xyz L.xyz], read as three 8-byte words per lane.  Lanes
// past n in the last wave take segment n - 1 and drop their result.  dist and
// D as shadow_filter computes them.  out: 3 floats per segment, plain stores.
// depth: the tree's (the LDS carve of <1>; unused by <0>).
template <int BVH>
__global__ __launch_bounds__(64) void rt_filter_kernel(const SceneDev S, const float2* __restrict__ segs, int n,
                                                         float* __restrict__ out, int depth)
{
    const int lane = (int)(threadIdx.x & 63);
    const size_t i = (size_t)blockIdx.x * 64 + (size_t)lane;
    const bool valid = i < (size_t)n;
    const float2* const r = segs + 3 * (valid ? i : (size_t)n - 1);
    const float2 w0 = r[0], w1 = r[1], w2 = r[2];
    const Vec3 P = make3(w0.x, w0.y, w1.x), L = make3(w1.y, w2.x, w2.y);
    const float dist = norm(L);
    const Vec3 D = div_recip(L, dist);
    Counters cnt;  // the hit routines' tallies: dead here
    Color F;
    if constexpr (BVH == 0) F = filter_all(S, P, D, dist, cnt);
    else {
        int steps = 0;
        F = filter_bvh(S, P, D, dist, depth, cnt, steps);
#ifdef RT_FILTER_STEPS  // a measuring build (tools/filter_probe.py --steps): the walk's tallies instead of the filter
        F = Color{(float)(steps & 0xffffff), (float)(steps >> 30), 0.0f};
#endif
    }
    if (!valid) return;
    out[3 * i] = F.r;
    out[3 * i + 1] = F.g;
    out[3 * i + 2] = F.b;
}

}  // namespace rt
#endif  // RT_AMD_RT_FILTER_H
