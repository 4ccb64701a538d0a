// scene_host_check.cpp — a stand-alone host program over the host half of
// rt_upload_scene (csrc/rt_scenehost.h: scene_host_build, lb_plan), for a
// sanitizer build (tests/test_host_scene.py):
//
//   g++ -std=c++17 -pthread -fsanitize=address,undefined -I ray-tracing-gpu_amd/csrc -I include
//       tools/upload/scene_host_check.cpp -o scene_host_check && ./scene_host_check
//
// The scenes are made here, the smallest at which each branch can go wrong:
// empty lists, one surface of each kind, the sizes around kTinyMax (20), the
// BVH's 64 triangles and the cluster order's 1,024, class ranges that are no
// multiple of 64 or empty, and values that break the arithmetic (degenerate,
// huge, NaN and infinite triangles, NaN and negative filter colours, an
// unknown surface type).  lb_plan gets synthetic cone records.  Only
// properties are asserted (no second implementation): see check_scene and
// check_plan.  Prints "scene_host_check: ok (N cases)", exit 0; else exit 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "rt_scenehost.h"

using namespace rt;

static const char* g_case = "";
#define REQUIRE(cond)                                                                   \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            std::printf("scene_host_check: %s: %s (line %d)\n", g_case, #cond, __LINE__); \
            std::exit(1);                                                               \
        }                                                                               \
    } while (0)

static const float kNaN = std::numeric_limits<float>::quiet_NaN();
static int g_cases = 0;

static unsigned g_rng = 12345u;
static float rnd()  // [0, 1)
{
    g_rng = g_rng * 1664525u + 1013904223u;
    return (float)(g_rng >> 8) / 16777216.0f;
}

struct Gen {
    std::vector<int32_t> type;
    std::vector<float> geom, mat, lights;
    void surface(int kind, const float* g, int ng, float kr, float kt, float r = 0.5f, float gr = 0.5f, float b = 0.5f)
    {
        type.push_back(kind);
        geom.insert(geom.end(), 12, 0.0f);
        std::copy(g, g + ng, geom.end() - 12);
        const float m[10] = {r, gr, b, 0.2f, 0.6f, 0.3f, 10.f, kr, kt, 1.f};
        mat.insert(mat.end(), m, m + 10);
    }
    void tri(const float* v9, float kr = 0.f, float kt = 0.f)
    {
        float g[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0.f, 0.f, 1.f};
        std::copy(v9, v9 + 9, g);
        surface(RT_TRIANGLE, g, 12, kr, kt);
    }
    // a small triangle somewhere in a 40 x 40 x 10 box
    void random_tri(float kr = 0.f, float kt = 0.f)
    {
        const float x = 40.f * rnd() - 20.f, y = 40.f * rnd() - 20.f, z = -10.f * rnd();
        const float v[9] = {x, y, z, x + 0.2f + rnd(), y + 0.3f * rnd(), z + 0.3f * rnd(),
                            x + 0.3f * rnd(), y + 0.2f + rnd(), z + 0.3f * rnd()};
        tri(v, kr, kt);
    }
    void plane(float kr = 0.f, float kt = 0.f)
    {
        const float g[4] = {0.f, 1.f, 0.f, 5.f};
        surface(RT_PLANE, g, 4, kr, kt);
    }
    void quadric(float kr = 0.f, float kt = 0.f)
    {
        const float g[10] = {1.f, 1.f, 1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, -4.f};
        surface(RT_QUADRIC, g, 10, kr, kt);
    }
    void light(float x, float y, float z)
    {
        const float l[7] = {x, y, z, 1.f, 1.f, 1.f, 1.f};
        lights.insert(lights.end(), l, l + 7);
    }
    rt_scene_flat flat() const
    {
        return rt_scene_flat{(int32_t)type.size(), (int32_t)(lights.size() / 7), type.data(), geom.data(), mat.data(),
                             lights.data()};
    }
    // n triangles, `translucent(k)` of them with Kt = 0.5, Kr = kr on all
    template <class F>
    static Gen triangles(int n, float kr, F translucent, int n_lights = 2)
    {
        Gen g;
        for (int k = 0; k < n; ++k) g.random_tri(kr, translucent(k) ? 0.5f : 0.f);
        for (int j = 0; j < n_lights; ++j) g.light(5.f + 30.f * j, 9.f, 9.f);
        return g;
    }
};
static bool none(int) { return false; }

static int bits(float f)
{
    int i;
    std::memcpy(&i, &f, 4);
    return i;
}

// One list of a kind: rec floats per record, the file index at word `iw`, the
// surface's geom words 1.. in the words before it.  A permutation of the
// kind's surfaces, the opaque ones first; file order inside each class when
// `ordered`.
static void check_list(const Gen& g, const SceneHost& H, int kind, const std::vector<float>& list, int rec, int iw,
                       int count, int count_o, bool ordered)
{
    const int n = (int)g.type.size();
    REQUIRE(list.size() == (size_t)rec * std::max(count, 1));
    std::vector<char> seen((size_t)n, 0);
    int prev = -1;
    for (int k = 0; k < count; ++k) {
        const float* r = &list[(size_t)rec * k];
        const int fi = bits(r[iw]);
        REQUIRE(fi >= 0 && fi < n && g.type[fi] == kind && !seen[fi]);
        seen[fi] = 1;
        const float* o = &H.geom[16 * (size_t)fi];
        REQUIRE(std::memcmp(r, o + 1, (size_t)iw * sizeof(float)) == 0);
        const bool is_opaque = o[13] == 0.0f && o[14] == 0.0f && o[15] == 0.0f;
        REQUIRE(is_opaque == (k < count_o));  // every run of a class's range holds that class alone
        if (k == count_o) prev = -1;
        if (ordered) REQUIRE(fi > prev);
        prev = fi;
    }
    int of_kind = 0;
    for (int i = 0; i < n; ++i) of_kind += g.type[i] == kind;
    REQUIRE(of_kind == count);
}

static void check_scene(const char* name, const Gen& g)
{
    g_case = name;
    ++g_cases;
    const rt_scene_flat s = g.flat();
    SceneHost H;
    std::string err;
    REQUIRE(scene_host_build(&s, H, err) && err.empty());
    const int n = s.n_surfaces, nl = s.n_lights;
    // the counts add up
    REQUIRE(H.n_surf == n && H.n_lights == nl);
    REQUIRE(H.n_tri + H.n_plane + H.n_quad == n);
    REQUIRE(H.n_tri_opaque <= H.n_tri && H.n_plane_opaque <= H.n_plane && H.n_quad_opaque <= H.n_quad);
    REQUIRE(H.n_translucent == n - H.n_tri_opaque - H.n_plane_opaque - H.n_quad_opaque);
    REQUIRE(H.geom.size() == 16 * (size_t)std::max(n, 1) && H.mat.size() == 12 * (size_t)std::max(n, 1));
    REQUIRE(H.lig.size() == 8 * (size_t)std::max(nl, 1));
    REQUIRE(H.ntr == (size_t)std::max(H.n_tri, 1));
    REQUIRE(H.sph.size() == 4 * H.ntr && H.nrm.size() == 4 * H.ntr && H.coef.size() == 4 * H.ntr);
    // the lists
    check_list(g, H, RT_TRIANGLE, H.tri, 12, 9, H.n_tri, H.n_tri_opaque, H.n_tri <= kClusterMinTriangles);
    check_list(g, H, RT_PLANE, H.pla, 8, 4, H.n_plane, H.n_plane_opaque, true);
    check_list(g, H, RT_QUADRIC, H.qua, 12, 10, H.n_quad, H.n_quad_opaque, true);
    // translucent: the ascending file indices with a filter factor
    REQUIRE(H.translucent.size() == (size_t)std::max(H.n_translucent, 1));
    int q = 0;
    bool split = true;
    float kmax = 0.f, krmax = 0.f, ktmax = 0.f;
    for (int i = 0; i < n; ++i) {
        const float* o = &H.geom[16 * (size_t)i];
        if (!(o[13] == 0.0f && o[14] == 0.0f && o[15] == 0.0f)) {
            REQUIRE(q < H.n_translucent && H.translucent[q] == i);
            ++q;
        }
        for (int a = 13; a < 16; ++a) split = split && std::isfinite(o[a]) && !std::signbit(o[a]);
        const float kr = g.mat[10 * (size_t)i + 7], kt = g.mat[10 * (size_t)i + 8];
        if (kr == kr) krmax = std::max(krmax, kr);
        if (kt == kt) ktmax = std::max(ktmax, kt);
    }
    kmax = std::max(krmax, ktmax);
    REQUIRE(q == H.n_translucent);
    REQUIRE((H.shadow_split != 0) == split);
    REQUIRE(H.k_max == kmax && H.kr_max == krmax && H.kt_max == ktmax);  // NaN ignored
    // per triangle: the sphere holds the vertices the record implies; a unit
    // normal, or none and "never culled"
    for (int k = 0; k < H.n_tri; ++k) {
        const float* r = &H.tri[12 * (size_t)k];
        bool finite = true;
        for (int a = 0; a < 9; ++a) finite = finite && std::isfinite(r[a]);
        const float* sp = &H.sph[4 * (size_t)k];
        for (int v = 0; v < 3 && finite; ++v) {
            double d2 = 0;
            for (int a = 0; a < 3; ++a) {
                const double x = (double)r[a] + (v ? (double)r[3 * v + a] : 0.0) - sp[a];
                d2 += x * x;
            }
            REQUIRE(std::sqrt(d2) <= sp[3]);
            for (int j = 0; j < nl; ++j) {  // and the light's far distance reaches it
                double l2 = 0;
                for (int a = 0; a < 3; ++a) {
                    const double x = (double)r[a] + (v ? (double)r[3 * v + a] : 0.0) - H.lig[8 * (size_t)j + a];
                    l2 += x * x;
                }
                REQUIRE(H.far[(size_t)j] >= std::sqrt(l2));
            }
        }
        const float* nr = &H.nrm[4 * (size_t)k];
        const float* co = &H.coef[4 * (size_t)k];
        const double len = std::sqrt((double)nr[0] * nr[0] + (double)nr[1] * nr[1] + (double)nr[2] * nr[2]);
        if (nr[0] == 0.f && nr[1] == 0.f && nr[2] == 0.f)
            REQUIRE(co[2] == -1.0f);
        else
            REQUIRE(std::fabs(len - 1.0) <= 1e-6 && co[2] >= 0.0f && finite);
        if (!finite) REQUIRE(co[2] == -1.0f);
    }
    REQUIRE(H.far.size() == (size_t)nl);
    // the BVH and the sort bins
    const bool want_bvh = kmax > 0.f && H.n_tri >= RT_BVH_MIN_TRIANGLES;
    REQUIRE(H.has_bvh == want_bvh);  // (these trees are far from kBvhStack levels deep)
    if (!H.has_bvh) {
        REQUIRE(H.skey.empty() && H.nbin_half == 0 && H.bvh.tris.empty() && H.bvh.nodes.empty());
        return;
    }
    REQUIRE(H.bvh.depth >= 1 && H.bvh.depth <= kBvhStack && H.bvh.tris.size() == 3 * (size_t)H.n_tri);
    REQUIRE(H.bvh.nodes.size() == 4 * (size_t)H.bvh.inner && H.skey.size() == (size_t)n);
    std::vector<char> in_leaf((size_t)n, 0);
    for (int p = 0; p < H.n_tri; ++p) {
        const int fi = bits(H.bvh.tris[3 * (size_t)p + 2].y);
        REQUIRE(fi >= 0 && fi < n && g.type[fi] == RT_TRIANGLE && !in_leaf[fi]);
        in_leaf[fi] = 1;
        REQUIRE(H.skey[fi] == (unsigned)p / 2);
    }
    unsigned next = ((unsigned)H.n_tri + 1) / 2;
    for (int i = 0; i < n; ++i)
        if (!in_leaf[i]) REQUIRE(H.skey[i] == next++);
    REQUIRE(H.nbin_half == next);
}

// An unknown surface type: an error, and the output struct is untouched.
static void check_unknown_type()
{
    g_case = "unknown surface type";
    ++g_cases;
    for (int bad : {RT_TRIANGLE - 1, RT_QUADRIC + 1}) {
        Gen g = Gen::triangles(3, 0.f, none);
        g.plane();
        g.type[2] = bad;
        const rt_scene_flat s = g.flat();
        SceneHost H;
        H.n_surf = 777;
        H.tri = {1.f, 2.f, 3.f};
        H.far = {4.0};
        std::string err;
        REQUIRE(!scene_host_build(&s, H, err));
        REQUIRE(err == "unknown surface type");
        REQUIRE(H.n_surf == 777 && H.n_lights == 0 && H.tri.size() == 3 && H.tri[2] == 3.f && H.far.size() == 1 && H.geom.empty());
    }
}

// ---- lb_plan
struct Cones {
    int nl, ntr;
    std::vector<float> f;  // exactly nl x ntr x 8
    Cones(int nl, int ntr) : nl(nl), ntr(ntr), f((size_t)nl * ntr * 8, 0.0f) {}
    void set(int j, int k, float c0w, float dmin, float dcap)
    {
        float* r = &f[((size_t)j * ntr + k) * 8];
        r[3] = c0w, r[4] = dmin, r[6] = dcap;
    }
    const float* rec(int j, int k) const { return &f[((size_t)j * ntr + k) * 8]; }
};

static void check_plan(const char* name, const Cones& C, int n_opaque, const std::vector<double>& dcov, double scale,
                       int r_min)
{
    g_case = name;
    ++g_cases;
    LbPlan P;
    P.sob = 99;  // (overwritten)
    lb_plan(C.f.data(), C.nl, C.ntr, n_opaque, dcov.data(), scale, r_min, P);
    REQUIRE(P.slots.size() == (size_t)C.nl);
    size_t perm0 = 0, dperm0 = 0, sob = 0, ob = 0, hob = 0;
    for (int j = 0; j < C.nl; ++j) {
        const LbSlot& b = P.slots[j];
        const float dc = (float)dcov[j];
        bool any_angle = false;
        size_t want_perm = 0, want_dperm = 0;
        std::vector<char> in_perm((size_t)C.ntr, 0), in_dperm((size_t)C.ntr, 0);
        for (int k = 0; k < n_opaque; ++k) {
            const float* r = C.rec(j, k);
            any_angle = any_angle || (r[3] > 0.f && r[3] <= 1.f);
            want_perm += in_perm[k] = r[3] > 0.f && r[4] < dc;
            want_dperm += in_dperm[k] = !(r[6] >= dc);
        }
        // R: a multiple of kLbGroup within [r_min, 1024] (no usable cone angle at all: the default 16)
        REQUIRE(b.R % kLbGroup == 0 && b.R <= 1024 && (any_angle ? b.R >= r_min : b.R == 16));
        // the slots' ranges tile their arrays
        REQUIRE(b.perm0 == perm0 && b.dperm0 == dperm0 && b.sob == sob && b.ob == ob);
        REQUIRE(b.nperm == want_perm && b.ndperm == want_dperm);
        const unsigned G = (unsigned)(b.R / kLbGroup);
        REQUIRE(b.nsup == 6 * G * G && b.ncell == 6u * b.R * b.R);
        if (b.nperm > kLbHyperMin) {
            REQUIRE(b.hob == hob && b.Gp == (int)((G + kLbHyper - 1) / kLbHyper) && b.nhyp == 6u * b.Gp * b.Gp);
            hob += b.nhyp + 1;
        } else {
            REQUIRE(b.nhyp == 0 && b.Gp == 0 && b.hob == 0);
        }
        perm0 += b.nperm, dperm0 += b.ndperm, sob += b.nsup + 1, ob += b.ncell + 1;
        REQUIRE(perm0 <= P.perm.size() && dperm0 <= P.dperm.size());
        // perm: exactly the triangles with a cone and dmin < dcov, by (dmin, index)
        for (size_t i = 0; i < b.nperm; ++i) {
            const int k = P.perm[b.perm0 + i];
            REQUIRE(k >= 0 && k < n_opaque && in_perm[k]);
            in_perm[k] = 0;  // (once)
            if (i == 0) continue;
            const int p = P.perm[b.perm0 + i - 1];
            const float a = C.rec(j, p)[4], z = C.rec(j, k)[4];
            REQUIRE(a < z || (a == z && p < k));
        }
        // dperm: by (dcap with NaN first, index)
        for (size_t i = 0; i < b.ndperm; ++i) {
            const int k = P.dperm[b.dperm0 + i];
            REQUIRE(k >= 0 && k < n_opaque && in_dperm[k]);
            in_dperm[k] = 0;
            if (i == 0) continue;
            const int p = P.dperm[b.dperm0 + i - 1];
            const float a = C.rec(j, p)[6], z = C.rec(j, k)[6];
            REQUIRE(a != a ? (z == z || p < k) : (z == z && (a < z || (a == z && p < k))));
        }
    }
    REQUIRE(perm0 == P.perm.size() && dperm0 == P.dperm.size() && sob == P.sob && ob == P.ob && hob == P.hob);
}

static void plan_cases()
{
    const float dc = 10.0f;
    {
        // every special record, twice (ties go by index); the last two are translucent (beyond n_opaque)
        Cones C(1, 20);
        const float rows[9][3] = {{0.f, 1.f, 20.f},   {1.f, 2.f, 20.f},  {1.5f, 3.f, 20.f}, {0.9f, dc, 20.f},
                                  {0.9f, 4.f, kNaN},  {0.9f, 4.f, dc},   {0.99f, 0.5f, 5.f}, {-1.f, 1.f, -5.f},
                                  {0.999f, 9.f, 7.f}};
        for (int k = 0; k < 18; ++k) C.set(0, k, rows[k % 9][0], rows[k % 9][1], rows[k % 9][2]);
        C.set(0, 18, 0.9f, 1.f, kNaN);
        C.set(0, 19, 0.9f, 1.f, kNaN);
        check_plan("plan: special records", C, 18, {dc}, 4.0, RT_LB_RMIN);
        check_plan("plan: explicit scale", C, 18, {dc}, 0.5, kLbGroup);
        check_plan("plan: scale beyond 1024 cells", C, 18, {dc}, 1e6, kLbGroup);
        check_plan("plan: no opaque triangle", C, 0, {dc}, 4.0, RT_LB_RMIN);
        check_plan("plan: one triangle", C, 1, {dc}, 4.0, RT_LB_RMIN);  // c0.w = 0: no angle, no cone
        check_plan("plan: no slot", Cones(0, 20), 18, {}, 4.0, RT_LB_RMIN);
    }
    {
        // 7,000 triangles x 3 slots: above 20,000 triangle-slots the slots run on threads; slot 0 has more
        // than kLbHyperMin triangles in reach (a hyper level), slot 2 few
        Cones C(3, 7000);
        const std::vector<double> dcov = {50.0, 8.0, 0.5};
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < 7000; ++k) {
                const float w = k % 97 == 0 ? 0.f : std::cos(0.002f + 0.02f * rnd());
                const float dmin = (float)(k % 50) * 0.25f + (k % 3 == 0 ? 0.f : rnd());
                const float dcap = k % 31 == 0 ? kNaN : (k % 7 == 0 ? 60.f * rnd() : 100.f);
                C.set(j, k, w, dmin, dcap);
            }
        check_plan("plan: 7000 x 3 slots (threads)", C, 6990, dcov, 6.0, RT_LB_RMIN);
        check_plan("plan: 7000 x 3 slots, 6666 opaque (serial)", C, 6666, dcov, 6.0, RT_LB_RMIN);
    }
}

int main()
{
    // surface and light counts
    check_scene("0 surfaces, 0 lights", Gen{});
    {
        Gen g;
        g.light(1.f, 2.f, 3.f);
        g.light(-1.f, 2.f, 3.f);
        check_scene("0 surfaces, 2 lights", g);
    }
    for (int which = 0; which < 4; ++which) {
        Gen g;
        const float v[9] = {-1.f, 0.f, -3.f, 1.f, 0.f, -3.f, 0.f, 1.f, -3.f};
        if (which == 0) g.plane();
        if (which == 1) g.quadric();
        if (which == 2) g.tri(v);
        if (which == 3) g.tri(v, 0.f, 0.5f);  // translucent: no opaque triangle
        g.light(5.f, 9.f, 9.f);
        const char* names[4] = {"one plane", "one quadric", "one opaque triangle", "one translucent triangle"};
        check_scene(names[which], g);
    }
    {
        // every kind in both classes, planes and quadrics between the triangles
        Gen g;
        for (int k = 0; k < 12; ++k) {
            g.random_tri(0.f, k % 3 == 1 ? 0.5f : 0.f);
            if (k % 4 == 0) g.plane(0.3f, k % 8 == 0 ? 0.4f : 0.f);
            if (k % 5 == 0) g.quadric(0.f, k % 10 == 0 ? 0.4f : 0.f);
        }
        g.light(5.f, 9.f, 9.f);
        check_scene("mixed kinds and classes", g);
    }
    // triangle counts: kTinyMax, the BVH's minimum (reflective or matt), the cluster order's
    check_scene("20 triangles", Gen::triangles(20, 0.f, none));
    check_scene("21 triangles", Gen::triangles(21, 0.f, none));
    for (int n : {63, 64, 65}) {
        check_scene("63-65 triangles, reflective", Gen::triangles(n, 0.5f, none));
        check_scene("63-65 triangles, matt", Gen::triangles(n, 0.f, none));
    }
    {
        Gen g = Gen::triangles(70, 0.5f, [](int k) { return k % 9 == 4; });  // other surfaces get bins of their own
        g.plane(0.5f);
        g.quadric(0.f, 0.5f);
        g.random_tri(0.5f);
        check_scene("71 triangles, a plane and a quadric, reflective", g);
    }
    for (int n : {1024, 1025, 1026}) check_scene("1024-1026 triangles", Gen::triangles(n, 0.5f, none, 1));
    check_scene("1025 triangles, 3 translucent", Gen::triangles(1025, 0.f, [](int k) { return k == 7 || k == 500 || k == 1024; }, 1));
    check_scene("1025 triangles, all translucent", Gen::triangles(1025, 0.f, [](int) { return true; }, 1));
    check_scene("1500 triangles, 700 translucent, reflective", Gen::triangles(1500, 0.5f, [](int k) { return k % 15 < 7; }, 1));
    // values
    {
        Gen g;
        const float degenerate[9] = {1.f, 1.f, 1.f, 2.f, 2.f, 2.f, 3.f, 3.f, 3.f};    // e1 x e2 = 0
        const float point[9] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
        const float long_edge[9] = {0.f, 0.f, 0.f, 200.f, 0.f, 0.f, 0.f, 1.f, 0.f};   // the rounding bound is not usable
        const float nan_vertex[9] = {0.f, 0.f, 0.f, 1.f, kNaN, 0.f, 0.f, 1.f, 0.f};
        const float inf_vertex[9] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, INFINITY, 0.f};
        const float huge[9] = {3e38f, 0.f, 0.f, -3e38f, 1.f, 0.f, 0.f, -3e38f, 0.f};  // finite vertices, infinite edges
        for (const float* v : {degenerate, point, long_edge, nan_vertex, inf_vertex, huge}) g.tri(v);
        g.random_tri();
        g.light(5.f, 9.f, 9.f);
        check_scene("degenerate, long, NaN and infinite triangles", g);
        SceneHost H;
        std::string err;
        const rt_scene_flat s = g.flat();
        REQUIRE(scene_host_build(&s, H, err));
        for (int k = 0; k < 6; ++k) REQUIRE(H.coef[4 * k + 2] == -1.0f && H.nrm[4 * k] == 0.f);
        REQUIRE(H.coef[4 * 6 + 2] >= 0.0f);
        // the same among 70 reflective ones: the BVH build sees them too
        Gen b = Gen::triangles(70, 0.5f, none);
        for (const float* v : {degenerate, nan_vertex, inf_vertex, huge}) b.tri(v, 0.5f);
        check_scene("a BVH over NaN and infinite triangles", b);
    }
    {
        Gen g = Gen::triangles(5, 0.f, none);
        const float v[9] = {-1.f, 0.f, -3.f, 1.f, 0.f, -3.f, 0.f, 1.f, -3.f};
        float gg[12] = {0};
        std::copy(v, v + 9, gg);
        g.surface(RT_TRIANGLE, gg, 12, 0.f, 0.5f, kNaN, 0.5f, 0.5f);  // a NaN filter colour
        check_scene("NaN filter colour", g);
        SceneHost H;
        std::string err;
        rt_scene_flat s = g.flat();
        REQUIRE(scene_host_build(&s, H, err) && !H.shadow_split && H.n_translucent == 1);
        Gen h = Gen::triangles(5, 0.f, none);
        h.surface(RT_TRIANGLE, gg, 12, 0.f, 0.5f, 0.5f, -0.5f, 0.5f);  // a negative one
        check_scene("negative filter colour", h);
        s = h.flat();
        REQUIRE(scene_host_build(&s, H, err) && !H.shadow_split);
        Gen k = Gen::triangles(5, 0.25f, none);
        k.surface(RT_TRIANGLE, gg, 12, kNaN, 0.f);  // Kr NaN: ignored by the maxima
        k.surface(RT_PLANE, gg, 4, 0.f, kNaN);      // Kt NaN: a NaN filter factor too
        check_scene("Kr and Kt NaN", k);
        s = k.flat();
        REQUIRE(scene_host_build(&s, H, err) && H.k_max == 0.25f && H.kr_max == 0.25f && H.kt_max == 0.f && !H.shadow_split);
    }
    check_unknown_type();
    plan_cases();
    std::printf("scene_host_check: ok (%d cases)\n", g_cases);
    return 0;
}
