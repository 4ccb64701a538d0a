// rt_scenehost.h — the host half of rt_upload_scene (rt_kernels.hip): what an
// upload computes from the flat scene alone (scene_host_build) and the layout
// of the light-buffer build from the cone records read back (lb_plan).  Plain
// host C++ with no HIP in it: the library and
// tools/upload/scene_host_check.cpp compile the same functions.
#ifndef RT_AMD_RT_SCENEHOST_H
#define RT_AMD_RT_SCENEHOST_H

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rt.h"
#include "rt_bvhhost.h"
#include "rt_math.h"

// Bounce rays walk the BVH (rt_bvh.h) in scenes of at least this many
// triangles (fewer: every triangle, by wave-uniform scalar loads).
#ifndef RT_BVH_MIN_TRIANGLES
#define RT_BVH_MIN_TRIANGLES 64
#endif

namespace rt {

inline bool nonneg_finite(float v) { return std::isfinite(v) && !std::signbit(v); }

// Cluster order for the two-level culling: a top-down median split of the
// centroids on the longest axis of their bounds, at multiples of 64, so
// every run of 64 consecutive triangles is a compact leaf (a Morton order
// scatters clusters of meshes with a thin, noisy axis: C3 cluster cones
// 34 mrad median, 94 at the 90th percentile vs the members' 7.6).
inline void kd_order(std::vector<size_t>& ord, const std::vector<double>& cen, size_t b, size_t e)
{
    while (e - b > 64) {
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (size_t i = b; i < e; ++i)
            for (int a = 0; a < 3; ++a) {
                lo[a] = std::min(lo[a], cen[3 * ord[i] + a]);
                hi[a] = std::max(hi[a], cen[3 * ord[i] + a]);
            }
        int ax = 0;
        for (int a = 1; a < 3; ++a)
            if (hi[a] - lo[a] > hi[ax] - lo[ax]) ax = a;
        const size_t n = e - b;
        const size_t mid = b + std::max<size_t>(64, ((n / 2 + 32) / 64) * 64);
        std::nth_element(ord.begin() + b, ord.begin() + mid, ord.begin() + e, [&](size_t x, size_t y) {
            return cen[3 * x + ax] < cen[3 * y + ax] || (cen[3 * x + ax] == cen[3 * y + ax] && x < y);
        });
        kd_order(ord, cen, b, mid);
        b = mid;
    }
}
// Reorder 12-float triangle records into clusters, the ranges [0, n_opaque)
// and [n_opaque, n) separately.
inline void cluster_order(std::vector<float>& tri, int n_opaque)
{
    const size_t n = tri.size() / 12;
    std::vector<double> cen(3 * n);
    for (size_t k = 0; k < n; ++k)
        for (int a = 0; a < 3; ++a) {
            const double v = tri[12 * k + a] + (tri[12 * k + 3 + a] + (double)tri[12 * k + 6 + a]) / 3.0;
            cen[3 * k + a] = std::isfinite(v) ? v : 0.0;
        }
    std::vector<size_t> ord(n);
    for (size_t k = 0; k < n; ++k) ord[k] = k;
    kd_order(ord, cen, 0, (size_t)n_opaque);
    kd_order(ord, cen, (size_t)n_opaque, n);
    std::vector<float> out(tri.size());
    for (size_t k = 0; k < n; ++k) std::memcpy(&out[12 * k], &tri[12 * ord[k]], 12 * sizeof(float));
    tri.swap(out);
}

// What the renders ask about the uploaded scene (rt_ctx keeps these).
struct SceneCounts {
    int n_surf = 0, n_lights = 0;
    int n_tri = 0, n_plane = 0, n_quad = 0;
    int n_tri_opaque = 0, n_plane_opaque = 0, n_quad_opaque = 0, n_translucent = 0;
    int shadow_split = 0;  // 1: every filter factor is finite and >= 0
    float k_max = 0.0f, kr_max = 0.0f, kt_max = 0.0f;  // max(Kr, Kt), max Kr, max Kt over surfaces (NaN ignored)
};

// Everything an upload derives from the flat scene on the host.  Every array
// holds at least one (zero) record, so no device buffer is empty: the counts
// say how many are real.
struct SceneHost : SceneCounts {
    // file order (rt_layout.h): 16 floats per surface, 12 per material, 8 per light
    std::vector<float> geom, mat, lig;
    // per kind, opaque surfaces first, each record with its file index:
    // 12 / 8 / 12 floats per triangle / plane / quadric
    std::vector<float> tri, pla, qua;
    std::vector<int> translucent;  // file indices with a non-zero filter factor, ascending
    // per record of tri[] (ntr = max(n_tri, 1) of them), 4 floats each, for
    // rt_cone_prepass: bounding sphere; unit normal and longest edge; the
    // rounding-bound coefficients gS, gL, rho_cap and |e1 x e2|
    size_t ntr = 0;
    std::vector<float> sph, nrm, coef;
    // the bounce-ray BVH (has_bvh) and, per surface, its coherence-sort bin
    // (WfDev::skey): a triangle at leaf position p has bin p / 2, every other
    // surface a bin of its own after them; nbin_half = the bins
    bool has_bvh = false;
    BvhBuilt bvh;
    std::vector<unsigned> skey;
    unsigned nbin_half = 0;
    double bvh_build_ms = 0.0;
    std::vector<double> far;  // per light: the distance to its farthest triangle's sphere
};

// The surface, material and light records in file order; false (and err) on
// an unknown surface type, before anything of H is written.
inline bool scene_host_records(const rt_scene_flat* s, SceneHost& H, std::string& err)
{
    const int n = s->n_surfaces, nl = s->n_lights;
    for (int i = 0; i < n; ++i)
        if (s->type[i] < RT_TRIANGLE || s->type[i] > RT_QUADRIC) {
            err = "unknown surface type";
            return false;
        }
    H = SceneHost{};
    H.n_surf = n;
    H.n_lights = nl;
    H.shadow_split = 1;
    H.geom.assign((size_t)std::max(n, 1) * 16, 0.0f);
    H.mat.assign((size_t)std::max(n, 1) * 12, 0.0f);
    H.lig.assign((size_t)std::max(nl, 1) * 8, 0.0f);
    for (int i = 0; i < n; ++i) {
        const float* g = s->geom + 12 * (size_t)i;
        const float* m = s->material + 10 * (size_t)i;
        float* o = &H.geom[16 * (size_t)i];
        const int kind = s->type[i];
        std::memcpy(&o[0], &kind, sizeof(int));
        if (kind == RT_TRIANGLE) {
            const Vec3 p0 = make3(g[0], g[1], g[2]), p1 = make3(g[3], g[4], g[5]), p2 = make3(g[6], g[7], g[8]);
            const Vec3 e1 = p1 - p0, e2 = p2 - p0;  // Triangle.cpp:135-136
            o[1] = p0.x; o[2] = p0.y; o[3] = p0.z;
            o[4] = e1.x; o[5] = e1.y; o[6] = e1.z;
            o[7] = e2.x; o[8] = e2.y; o[9] = e2.z;
            o[10] = g[9]; o[11] = g[10]; o[12] = g[11];
        } else if (kind == RT_PLANE) {
            o[1] = g[0]; o[2] = g[1]; o[3] = g[2]; o[4] = g[3];
        } else {
            o[1] = g[0]; o[2] = g[1]; o[3] = g[2];  // quad
            o[4] = g[6]; o[5] = g[7]; o[6] = g[8];  // mix
            o[7] = g[3]; o[8] = g[4]; o[9] = g[5];  // lin
            o[10] = g[9];
        }
        const Color fc = Color{m[0], m[1], m[2]} * m[8];  // colour * Kt
        o[13] = fc.r; o[14] = fc.g; o[15] = fc.b;
        if (!(nonneg_finite(fc.r) && nonneg_finite(fc.g) && nonneg_finite(fc.b))) H.shadow_split = 0;
        float* q = &H.mat[12 * (size_t)i];
        for (int k = 0; k < 10; ++k) q[k] = m[k];
        if (m[7] > H.k_max) H.k_max = m[7];
        if (m[8] > H.k_max) H.k_max = m[8];
        if (m[7] > H.kr_max) H.kr_max = m[7];
        if (m[8] > H.kt_max) H.kt_max = m[8];
    }
    for (int j = 0; j < nl; ++j) {
        const float* l = s->lights + 7 * (size_t)j;
        float* o = &H.lig[8 * (size_t)j];
        o[0] = l[0]; o[1] = l[1]; o[2] = l[2]; o[3] = l[6];
        o[4] = l[3]; o[5] = l[4]; o[6] = l[5]; o[7] = 0.0f;
    }
    return true;
}

// Per-kind arrays, opaque surfaces first (file order kept inside each class),
// then the cluster order of a big triangle list; each padded to one record.
inline void scene_host_lists(const rt_scene_flat* s, SceneHost& H)
{
    const int n = H.n_surf;
    auto opaque_at = [&](int i) {
        const float* o = &H.geom[16 * (size_t)i];
        return o[13] == 0.0f && o[14] == 0.0f && o[15] == 0.0f;
    };
    for (int pass = 0; pass < 2; ++pass) {
        for (int i = 0; i < n; ++i) {
            if (opaque_at(i) != (pass == 0)) continue;
            const float* o = &H.geom[16 * (size_t)i];
            float idx;
            std::memcpy(&idx, &i, sizeof(int));
            const int kind = s->type[i];
            if (kind == RT_TRIANGLE) {
                const float r[12] = {o[1], o[2], o[3], o[4], o[5], o[6], o[7], o[8], o[9], idx, 0.f, 0.f};
                H.tri.insert(H.tri.end(), r, r + 12);
                H.n_tri_opaque += pass == 0;
            } else if (kind == RT_PLANE) {
                const float r[8] = {o[1], o[2], o[3], o[4], idx, 0.f, 0.f, 0.f};
                H.pla.insert(H.pla.end(), r, r + 8);
                H.n_plane_opaque += pass == 0;
            } else {
                const float r[12] = {o[1], o[2], o[3], o[4], o[5], o[6], o[7], o[8], o[9], o[10], idx, 0.f};
                H.qua.insert(H.qua.end(), r, r + 12);
                H.n_quad_opaque += pass == 0;
            }
        }
    }
    for (int i = 0; i < n; ++i)
        if (!opaque_at(i)) H.translucent.push_back(i);
    // Big lists: cluster order (kd_order) inside the opaque and the
    // translucent ranges, so 64 consecutive triangles form a compact cluster
    // for the two-level culling.  The order is free: closest hit is the
    // lexicographic (t, file index) minimum and opaque shadow tests are any-hit.
    if (H.tri.size() / 12 > (size_t)kClusterMinTriangles) cluster_order(H.tri, H.n_tri_opaque);
    H.n_tri = (int)(H.tri.size() / 12);
    H.n_plane = (int)(H.pla.size() / 8);
    H.n_quad = (int)(H.qua.size() / 12);
    H.n_translucent = (int)H.translucent.size();
    H.tri.resize(std::max<size_t>(H.tri.size(), 12));
    H.pla.resize(std::max<size_t>(H.pla.size(), 8));
    H.qua.resize(std::max<size_t>(H.qua.size(), 12));
    H.translucent.resize(std::max<size_t>(H.translucent.size(), 1));
    H.ntr = H.tri.size() / 12;
}

// Per triangle (tri[] order), for rt_cone_prepass: the bounding sphere of
// the triangle the reference tests (p0, p0 + e1, p0 + e2 with the float
// edges; radius measured from the float-rounded centre), the unit normal
// and longest edge, and the rounding-bound coefficients gS, gL, rho_cap.
// rho_cap = -1: det can be too inexact at the reference's 0.01 gate
// (longest edge >~ 110) — never culled.
inline void scene_host_tri_records(SceneHost& H)
{
    const size_t ntr = H.ntr;
    H.sph.assign(ntr * 4, 0.0f);
    H.nrm.assign(ntr * 4, 0.0f);
    H.coef.assign(ntr * 4, 0.0f);
    const double eps = 0x1p-24;
    for (size_t k = 0; k < ntr; ++k) {
        const float* r = &H.tri[12 * k];
        double p[3][3];
        for (int a = 0; a < 3; ++a) {
            p[0][a] = r[a];
            p[1][a] = (double)r[a] + (double)r[3 + a];
            p[2][a] = (double)r[a] + (double)r[6 + a];
        }
        float ctr[3];
        for (int a = 0; a < 3; ++a) ctr[a] = (float)((p[0][a] + p[1][a] + p[2][a]) / 3.0);
        double rad = 0, L2 = 0;
        for (int q = 0; q < 3; ++q) {
            double d2 = 0;
            for (int a = 0; a < 3; ++a) d2 += (p[q][a] - ctr[a]) * (p[q][a] - ctr[a]);
            rad = std::max(rad, std::sqrt(d2));
            for (int w = q + 1; w < 3; ++w) {
                double l2 = 0;
                for (int a = 0; a < 3; ++a) l2 += (p[q][a] - p[w][a]) * (p[q][a] - p[w][a]);
                L2 = std::max(L2, l2);
            }
        }
        rad = rad * (1.0 + 1e-9);
        for (int a = 0; a < 3; ++a) H.sph[4 * k + a] = ctr[a];
        H.sph[4 * k + 3] = std::nextafter((float)rad, INFINITY);
        const double e1[3] = {r[3], r[4], r[5]}, e2[3] = {r[6], r[7], r[8]};
        const double nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2],
                     nz = e1[0] * e2[1] - e1[1] * e2[0];
        const double nn = std::sqrt(nx * nx + ny * ny + nz * nz);
        const double L = std::sqrt(L2) * (1.0 + 1e-9);
        const double dl = 7.0 * eps * L * L;
        const double rho_cap = dl < 0.01 ? dl / (0.01 - dl) + 3.0 * eps : INFINITY;
        const bool fine = nn > 0 && std::isfinite(nn) && rho_cap <= 0.5;
        const double kk = fine ? 1.0 / (1.0 - rho_cap) : 2.0;
        H.nrm[4 * k] = fine ? (float)(nx / nn) : 0.f;
        H.nrm[4 * k + 1] = fine ? (float)(ny / nn) : 0.f;
        H.nrm[4 * k + 2] = fine ? (float)(nz / nn) : 0.f;
        H.nrm[4 * k + 3] = std::nextafter((float)L, INFINITY);
        H.coef[4 * k] = fine ? (float)(54.0 * kk * eps * L * L / nn * 1.01) : 0.f;
        H.coef[4 * k + 1] = fine ? (float)(21.0 * kk * eps * L * L * L / nn * 1.01) : 0.f;
        H.coef[4 * k + 2] = fine ? (float)(rho_cap * 1.01) : -1.0f;
        H.coef[4 * k + 3] = fine ? (float)nn : 0.0f;  // |N| = |e1 x e2| (never-hit bound)
    }
    // per light, the farthest triangle (shadow rays are culled up to a
    // factor of it, rt_kernels.hip light_prepasses)
    H.far.assign((size_t)H.n_lights, 0.0);
    for (int j = 0; j < H.n_lights; ++j) {
        const float* l = &H.lig[8 * (size_t)j];
        double far = 0;
        for (size_t k = 0; k < ntr; ++k) {
            double d2 = 0;
            for (int a = 0; a < 3; ++a) d2 += ((double)H.sph[4 * k + a] - l[a]) * ((double)H.sph[4 * k + a] - l[a]);
            far = std::max(far, std::sqrt(d2) + H.sph[4 * k + 3]);
        }
        H.far[(size_t)j] = far;
    }
}

// The bounce-ray BVH: only a scene with a reflective or refractive surface
// has bounce rays (Scene.cpp:1779-1823 gate on Kr, Kt > 0).  A tree deeper
// than the walk's stack is dropped (bounce rays then test every triangle).
// ray_bvh (RT_OPT_RAY_BVH): also a scene that cannot bounce gets the tree, for
// rt_trace_rays — the same size limits; its frames never use it (bvh_on).
inline void scene_host_bvh(SceneHost& H, bool ray_bvh = false)
{
    if (!((H.k_max > 0.0f || ray_bvh) && H.n_tri >= RT_BVH_MIN_TRIANGLES && (size_t)H.n_tri <= kBvhMaxTriangles))
        return;
    const auto tb = std::chrono::steady_clock::now();
    bvh_build(H.tri, (size_t)H.n_tri, H.bvh);
    if (H.bvh.depth <= kBvhStack) {
        // the sort bins: triangle at leaf position p -> p / 2 (its
        // file index is the leaf record's third float4 .y), every other
        // surface a bin of its own after them
        const int n = H.n_surf;
        H.skey.assign((size_t)n, 0u);
        std::vector<char> is_tri((size_t)n, 0);
        for (int i = 0; i < H.n_tri; ++i) {
            int fi;
            std::memcpy(&fi, &H.bvh.tris[3 * (size_t)i + 2].y, sizeof fi);
            if (fi >= 0 && fi < n) {
                H.skey[(size_t)fi] = (unsigned)i >> 1;
                is_tri[(size_t)fi] = 1;
            }
        }
        unsigned nb = ((unsigned)H.n_tri + 1u) >> 1;
        for (int i = 0; i < n; ++i)
            if (!is_tri[(size_t)i]) H.skey[(size_t)i] = nb++;
        H.nbin_half = nb;
        // word 10 of a leaf record ([2].z, 0 in tri[]): int 1 for a translucent
        // triangle — rt_filter_kernel<1>'s any-hit walk alone reads it
        for (int i = 0; i < H.n_tri; ++i) {
            float4& c = H.bvh.tris[3 * (size_t)i + 2];
            int fi;
            std::memcpy(&fi, &c.y, sizeof fi);
            if (!(fi >= 0 && fi < n)) continue;
            const float* o = &H.geom[16 * (size_t)fi];
            const int translucent = !(o[13] == 0.0f && o[14] == 0.0f && o[15] == 0.0f);
            std::memcpy(&c.z, &translucent, sizeof translucent);
        }
        H.has_bvh = true;
    } else {
        H.bvh = BvhBuilt{};
    }
    H.bvh_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb).count();
}

// The host half of an upload.  false with err set ("unknown surface type"):
// H is untouched.
inline bool scene_host_build(const rt_scene_flat* s, SceneHost& H, std::string& err, bool ray_bvh = false)
{
    if (!scene_host_records(s, H, err)) return false;
    scene_host_lists(s, H);
    scene_host_bvh(H, ray_bvh);
    scene_host_tri_records(H);
    return true;
}

// ---- the light-buffer build's layout (rt_kernels.hip lb_build)
// Big slots (more than kLbHyperMin triangles) first filter their triangles
// per block of kLbHyper x kLbHyper supercells.
constexpr int kLbHyper = 4;
constexpr size_t kLbHyperMin = 4096;
// The coarsest automatic resolution (lb_lists' r_min: why 128).
#ifndef RT_LB_RMIN
#define RT_LB_RMIN 128
#endif

// Slot j's pieces in the concatenated device arrays: its triangles in
// dmin order (perm) and its dcap list (dperm); its supercell counts /
// offsets (nsup + 1 words from sob) and cell offsets (ncell + 1 words
// from ob: the slot's lb_off) — each slot's last word stays 0 as a
// count, so ONE exclusive scan over a whole array gives every slot its
// absolute offsets, the last word its end.  hob: the hyper level's counts /
// offsets of a big slot, like sob (nhyp = 0: the slot has no such level).
struct LbSlot {
    int R = 16;
    size_t perm0 = 0, nperm = 0, dperm0 = 0, ndperm = 0, sob = 0, ob = 0, hob = 0;
    unsigned nsup = 0, ncell = 0, nhyp = 0;
    int Gp = 0;
};
struct LbPlan {
    std::vector<LbSlot> slots;
    std::vector<int> perm, dperm;    // every slot's list, concatenated
    size_t sob = 0, ob = 0, hob = 0;  // words of the three offset arrays
};

// The plan for nl slots from the host copy of their cone records (slot j's
// at cones + 8 ntr j: c0, c1 per triangle) built for the distances dcov[j]:
// per slot the cell resolution R from the median cone angle (cells of
// 1 / scale of it, a multiple of kLbGroup in [r_min, 1024]), the opaque
// triangles with a usable cone nearer than dcov in dmin order, and the dcap
// list (pairs whose cull does not hold up to dcov) in dcap order.  The slots
// are independent: above 20,000 triangle-slots each runs on its own thread.
inline void lb_plan(const float* cones, int nl, int ntr, int n_opaque, const double* dcov, double scale, int r_min,
                    LbPlan& P)
{
    P = LbPlan{};
    P.slots.resize((size_t)nl);
    std::vector<std::vector<int>> perms((size_t)nl), dperms((size_t)nl);
    auto prep = [&](int j) {
        LbSlot& b = P.slots[j];
        const float* hj = cones + (size_t)j * ntr * 8;  // c0 = hj[8 k ..], c1 = hj[8 k + 4 ..]
        std::vector<double> T;
        std::vector<int>& perm = perms[j];
        std::vector<int>& dperm = dperms[j];
        for (int k = 0; k < n_opaque; ++k) {
            const float c0w = hj[8 * k + 3], c1x = hj[8 * k + 4], c1z = hj[8 * k + 6];
            if (c0w > 0.0f && c0w <= 1.0f) T.push_back(std::acos((double)c0w));
            if (c0w > 0.0f && c1x < (float)dcov[j]) perm.push_back(k);
            if (!(c1z >= (float)dcov[j])) dperm.push_back(k);
        }
        if (!T.empty()) {
            std::nth_element(T.begin(), T.begin() + T.size() / 2, T.end());
            const double med = std::max(T[T.size() / 2], 1e-4);
            b.R = (int)std::lround(scale / (kLbGroup * med)) * kLbGroup;
            b.R = std::min(1024, std::max(r_min, b.R));
        }
        auto dmin = [&](int k) { return hj[8 * k + 4]; };
        std::sort(perm.begin(), perm.end(),
                  [&](int x, int y) { return dmin(x) < dmin(y) || (dmin(x) == dmin(y) && x < y); });
        auto key = [&](int k) { const float z = hj[8 * k + 6]; return z == z ? z : -INFINITY; };
        std::sort(dperm.begin(), dperm.end(),
                  [&](int x, int y) { return key(x) < key(y) || (key(x) == key(y) && x < y); });
    };
    if (nl > 1 && (size_t)n_opaque * nl > 20000) {
        std::vector<std::thread> th;
        for (int j = 0; j < nl; ++j) th.emplace_back(prep, j);
        for (auto& t : th) t.join();
    } else {
        for (int j = 0; j < nl; ++j) prep(j);
    }
    for (int j = 0; j < nl; ++j) {
        LbSlot& b = P.slots[j];
        b.perm0 = P.perm.size();
        b.nperm = perms[j].size();
        P.perm.insert(P.perm.end(), perms[j].begin(), perms[j].end());
        b.dperm0 = P.dperm.size();
        b.ndperm = dperms[j].size();
        P.dperm.insert(P.dperm.end(), dperms[j].begin(), dperms[j].end());
        const unsigned G = (unsigned)(b.R / kLbGroup);
        b.nsup = 6u * G * G;
        b.ncell = 6u * (unsigned)b.R * (unsigned)b.R;
        b.sob = P.sob;
        P.sob += b.nsup + 1;
        b.ob = P.ob;
        P.ob += b.ncell + 1;
        if (b.nperm > kLbHyperMin) {
            b.Gp = (int)((G + kLbHyper - 1) / kLbHyper);
            b.nhyp = 6u * (unsigned)(b.Gp * b.Gp);
            b.hob = P.hob;
            P.hob += b.nhyp + 1;
        }
    }
}

}  // namespace rt
#endif  // RT_AMD_RT_SCENEHOST_H
