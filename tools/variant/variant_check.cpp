// variant_check.cpp — a stand-alone host program over the trace kernels'
// variant word (csrc/rt_variant.h: select_variant, lds_bytes, kernel_name and
// the lists of instantiated variants), for a sanitizer build
// (tests/test_host_scene.py, test_variant_selection_under_asan_ubsan):
//
//   g++ -std=c++17 -fsanitize=address,undefined -I ray-tracing-gpu_amd/csrc
//       tools/variant/variant_check.cpp -o variant_check && ./variant_check
//
// (a) Every variant that select_variant() can return for facts the host can
//     form is in the list of its kernel template, so the host never asks for
//     a kernel the build did not instantiate; the lists hold no entry twice; and
//     kernel_name spells what printf would.
//     The same for select_query_variant() and RT_SHADE_RAYS_VARIANTS, the
//     radiance queries' kernels.
// (b) select_variant(), select_query_variant() and lds_bytes() against
//     expected results written out below, one per branch of the selection.
// Prints "variant_check: ok (N selections)", exit 0; else exit 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rt_variant.h"

using namespace rt;

#define REQUIRE(cond)                                                      \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("variant_check: %s (line %d)\n", #cond, __LINE__); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

#define RT_V(M, L, F) {M, L, F},
static const Variant kWf0List[] = {RT_TRACE_WF0_VARIANTS};
static const Variant kFrameList[] = {RT_TRACE_FRAME_VARIANTS};
static const Variant kTinyList[] = {RT_TINY_VARIANTS};
static const Variant kWfShadeList[] = {RT_WF_SHADE_VARIANTS};
static const Variant kAovList[] = {RT_AOV_VARIANTS};
static const Variant kShadeRaysList[] = {RT_SHADE_RAYS_VARIANTS};
#undef RT_V

template <size_t N>
static int count_of(const Variant (&list)[N], const Variant& v)
{
    int n = 0;
    for (const Variant& e : list) n += e == v;
    return n;
}

template <size_t N>
static void check_list(const Variant (&list)[N], const char* stem, int numbers)
{
    for (const Variant& e : list) {
        REQUIRE(count_of(list, e) == 1);
        REQUIRE(e.maxd >= 0 && e.lb >= 1 && e.flags >= 0);
        char want[64];
        if (numbers == 3) std::snprintf(want, sizeof want, "%s<%d,%d,%d>", stem, e.maxd, e.lb, e.flags);
        else std::snprintf(want, sizeof want, "%s<%d>", stem, e.flags);
        const KernelName got = numbers == 3 ? kernel_name(stem, e.maxd, e.lb, e.flags) : kernel_name(stem, e.flags);
        REQUIRE(std::strlen(want) < sizeof got.s && got.s[sizeof got.s - 1] == 0);
        REQUIRE(std::strcmp(got.s, want) == 0);
    }
}

static int g_selections = 0;

// (a) the facts the host can form.  The four kernel templates exclude one
// another (kind).  Left out, as rt_kernels.hip never forms them:
//  * a BVH depth without bounces, the light buffer and triangles (bvh_on);
//  * a current camera buffer without triangles, for a launch-camera frame,
//    or for a bounce frame that does not walk the BVH (cam_lists);
//  * a launch-camera frame (tiny mode 0..2) other than depth 0 with the
//    light buffer and 1..20 triangles (tiny_ok);
//  * level 0 of a wavefront, or its shading, of anything but a BVH frame;
//  * for the AOV kernels, anything but the triangle count, whether the
//    scene's colour frames are launch-camera ones, and the camera buffer.
static void walk()
{
    static const int tris[] = {0, 1, 20, 21, 1024, 1025};
    enum { kColour, kWf0Kind, kWfShadeKind, kAovKind };
    for (int kind = kColour; kind <= kAovKind; ++kind)
        for (int depth = 0; depth <= 33; ++depth)
            for (int n_tri : tris)
                for (int n_lights = 1; n_lights <= 2; ++n_lights)
                    for (int bits = 0; bits < 16; ++bits)
                        for (int bvh_depth = 0; bvh_depth <= 24; bvh_depth += 24)
                            for (int tiny = -1; tiny <= 2; ++tiny) {
                                Facts f;
                                f.depth = depth;
                                f.n_tri = n_tri;
                                f.n_lights = n_lights;
                                f.lbuf = (bits & 1) != 0;
                                f.cbuf = (bits & 2) != 0;
                                f.chain = (bits & 4) != 0;
                                f.small = (bits & 8) != 0;
                                f.bvh_depth = bvh_depth;
                                f.tiny = tiny;
                                f.wf0 = kind == kWf0Kind;
                                f.wf_shade = kind == kWfShadeKind;
                                f.aov = kind == kAovKind;
                                const bool bvh = bvh_depth > 0;
                                if (bvh && !(depth > 0 && f.lbuf && n_tri > 0)) continue;
                                if (f.cbuf && (n_tri == 0 || tiny >= 0 || (depth > 0 && !bvh))) continue;
                                if (tiny >= 0 && !(n_tri >= 1 && n_tri <= 20)) continue;
                                if (tiny >= 0 && kind != kAovKind && !(depth == 0 && f.lbuf)) continue;
                                if ((f.wf0 || f.wf_shade) && !(bvh && tiny < 0)) continue;
                                if (f.aov && (depth > 0 || bvh || tiny > 0)) continue;
                                const Variant v = select_variant(f);
                                ++g_selections;
                                if (f.aov) {
                                    REQUIRE(count_of(kAovList, v) == 1);
                                } else if (f.wf_shade) {
                                    REQUIRE(count_of(kWfShadeList, v) == 1);
                                } else if (f.wf0) {
                                    REQUIRE(is_wf0(v.flags) && count_of(kWf0List, v) == 1);
                                } else if (tiny >= 0) {
                                    REQUIRE(is_tiny(v.flags) && count_of(kTinyList, v) == 1);
                                } else if (depth > 32) {
                                    REQUIRE(v.maxd < 0);
                                } else {
                                    REQUIRE(v.maxd >= depth && !is_wf0(v.flags) && !is_tiny(v.flags));
                                    REQUIRE(count_of(kFrameList, v) == 1);
                                }
                                // the staging window exactly where the device code takes one
                                const unsigned lds = lds_bytes(v.flags, f.bvh_depth);
                                REQUIRE((lds >= kLdsWaveBytes) == (is_clustered(v.flags) || has_bvh(v.flags)));
                            }
}

// (a) for the radiance queries (select_query_variant): every depth, triangle
// count, light buffer and tree the host can form.  A tree without triangles
// is left out (scene_host_bvh builds none below 64).
static void walk_queries()
{
    static const int tris[] = {0, 1, 63, 64, 1024, 1025, 50000};
    for (int depth = 0; depth <= 33; ++depth)
        for (int n_tri : tris)
            for (int bits = 0; bits < 4; ++bits) {
                QueryFacts q;
                q.depth = depth;
                q.n_tri = n_tri;
                q.lbuf = (bits & 1) != 0;
                q.bvh = (bits & 2) != 0;
                if (q.bvh && n_tri < 64) continue;
                const Variant v = select_query_variant(q);
                ++g_selections;
                if (depth > 32) {
                    REQUIRE(v.maxd < 0);
                    continue;
                }
                REQUIRE(v.maxd >= depth && v.lb == 1 && count_of(kShadeRaysList, v) == 1);
                REQUIRE(is_ray_query(v.flags) && !has_cam_buf(v.flags) && !is_chain(v.flags) && !has_lb_pair(v.flags));
                REQUIRE(!is_wf0(v.flags) && !is_tiny(v.flags));
                // the smallest entry of the thinner depth list
                for (const Variant& e : kShadeRaysList) REQUIRE(!(e.flags == v.flags && e.maxd >= depth && e.maxd < v.maxd));
                // the tree only with the light buffer; the light buffer alone only without bounces
                REQUIRE(has_bvh(v.flags) == (q.bvh && q.lbuf));
                REQUIRE(has_light_buf(v.flags) == (q.lbuf && n_tri > 0 && (q.bvh || depth == 0)));
                REQUIRE(is_clustered(v.flags) == (has_light_buf(v.flags) && n_tri > 1024));
                const unsigned lds = lds_bytes(v.flags, 24);
                REQUIRE((lds >= kLdsWaveBytes) == (is_clustered(v.flags) || has_bvh(v.flags)));
            }
}

// (b) expected results, written out (not computed by the code under test)
static void expect(const Facts& f, int maxd, int lb, int flags, unsigned lds, int line)
{
    const Variant v = select_variant(f);
    if (!(v.maxd == maxd && v.lb == lb && v.flags == flags && lds_bytes(v.flags, f.bvh_depth) == lds)) {
        std::printf("variant_check: line %d: selected <%d,%d,%d> lds %u, expected <%d,%d,%d> lds %u\n", line, v.maxd,
                    v.lb, v.flags, lds_bytes(v.flags, f.bvh_depth), maxd, lb, flags, lds);
        std::exit(1);
    }
    ++g_selections;
}
#define EXPECT(f, maxd, lb, flags, lds) expect(f, maxd, lb, flags, lds, __LINE__)

static Facts facts(int depth, int n_tri, bool lbuf, bool cbuf, bool small = false)
{
    Facts f;
    f.depth = depth;
    f.n_tri = n_tri;
    f.lbuf = lbuf;
    f.cbuf = cbuf;
    f.small = small;
    return f;
}

static void literals()
{
    const unsigned win = 40u * RT_LB_LDS_CAP;  // the wave's staging window
    REQUIRE(win == kLdsWaveBytes);
    const int L = RT_WAVE_LB;
    // depth 0, light buffer on
    EXPECT(facts(0, 12, true, false), 0, 1, 5, 0);
    EXPECT(facts(0, 12, true, true), 0, 1, 13, 0);
    EXPECT(facts(0, 1024, true, false, true), 0, 1, 5, 0);  // small is ignored at or below 1,024
    EXPECT(facts(0, 1024, true, true, true), 0, 1, 13, 0);
    EXPECT(facts(0, 1025, true, false), 0, 1, 6, win);
    EXPECT(facts(0, 1025, true, true), 0, 1, 14, win);
    EXPECT(facts(0, 1025, true, false, true), 0, 1, 2054, win);
    EXPECT(facts(0, 1025, true, true, true), 0, 1, 2062, win);
    // depth 0, light buffer off
    EXPECT(facts(0, 1025, false, false), 0, L, 2, win);
    EXPECT(facts(0, 1025, false, true), 0, L, 10, win);
    EXPECT(facts(0, 12, false, false), 0, L, 1, 0);
    EXPECT(facts(0, 12, false, true), 0, L, 9, 0);
    // depth 0, no triangles
    {
        Facts f = facts(0, 0, false, false);
        f.n_lights = 2;
        EXPECT(f, 0, 3, 0, 0);
        f.n_lights = 1;
        EXPECT(f, 0, 1, 0, 0);
        f.chain = true;
        EXPECT(f, 0, 1, 1024, 0);
    }
    // depth 3 through a BVH of depth 24, light buffer on
    {
        Facts f = facts(3, 50000, true, false);
        f.bvh_depth = 24;
        const unsigned lds = win + 24u * 256u;
        f.chain = true;
        EXPECT(f, 3, 1, 1294, lds);
        f.chain = false;
        EXPECT(f, 3, 1, 270, lds);
        f.n_tri = 1024;
        f.chain = true;
        EXPECT(f, 3, 1, 1293, lds);
        f.chain = false;
        EXPECT(f, 3, 1, 269, lds);
    }
    // bounces without the BVH: the smallest compiled depth at or above the reachable one
    {
        static const int reach[][2] = {{1, 1}, {6, 8}, {9, 12}, {13, 16}, {17, 20}, {21, 32}, {32, 32}, {33, -1}};
        for (const auto& r : reach) {
            Facts f = facts(r[0], 50000, true, true);
            EXPECT(f, r[1], 1, 0, 0);
            f.chain = true;
            EXPECT(f, r[1], 1, r[1] < 0 ? 0 : 1024, 0);
        }
    }
    // level 0 of a wavefront frame
    {
        Facts f = facts(3, 1024, true, false);
        f.bvh_depth = 24;
        f.wf0 = true;
        EXPECT(f, 0, 1, 517, 0);
        f.cbuf = true;
        EXPECT(f, 0, 1, 525, 0);
        f.n_tri = 1025;
        EXPECT(f, 0, 1, 526, win);
        f.cbuf = false;
        EXPECT(f, 0, 1, 518, win);
        f.small = true;
        EXPECT(f, 0, 1, 2566, win);
        f.cbuf = true;
        EXPECT(f, 0, 1, 2574, win);
    }
    // the wavefront's shading
    {
        Facts f = facts(3, 1024, true, false);
        f.bvh_depth = 24;
        f.wf_shade = true;
        EXPECT(f, 0, 1, 5, 0);
        f.small = true;
        EXPECT(f, 0, 1, 5, 0);
        f.n_tri = 1025;
        EXPECT(f, 0, 1, 2054, win);
        f.small = false;
        EXPECT(f, 0, 1, 6, win);
    }
    // the launch-camera kernels by tile-mask mode
    {
        Facts f = facts(0, 12, true, false);
        f.tiny = 0;
        EXPECT(f, 0, 1, 37, 0);
        f.tiny = 1;
        EXPECT(f, 0, 1, 101, 0);
        f.tiny = 2;
        EXPECT(f, 0, 1, 229, 0);
    }
    // AOV
    {
        Facts f;
        f.aov = true;
        EXPECT(f, 0, 1, 0, 0);  // no triangles
        f.n_tri = 12;
        f.tiny = 0;
        EXPECT(f, 0, 1, 0, 0);  // a launch-camera scene
        f.tiny = -1;
        EXPECT(f, 0, 1, 1, 0);
        f.cbuf = true;
        EXPECT(f, 0, 1, 9, 0);
        f.n_tri = 1024;
        EXPECT(f, 0, 1, 9, 0);
        f.n_tri = 1025;
        EXPECT(f, 0, 1, 10, win);
        f.cbuf = false;
        EXPECT(f, 0, 1, 2, win);
    }
    // radiance queries: <stack, 1, flags>
    {
        auto query = [](int depth, int n_tri, bool lbuf, bool bvh) {
            QueryFacts q;
            q.depth = depth;
            q.n_tri = n_tri;
            q.lbuf = lbuf;
            q.bvh = bvh;
            return select_query_variant(q);
        };
        REQUIRE((query(0, 0, true, false) == Variant{0, 1, 16}));
        REQUIRE((query(0, 12, true, false) == Variant{0, 1, 21}));
        REQUIRE((query(0, 1025, true, false) == Variant{0, 1, 22}));
        REQUIRE((query(0, 12, false, false) == Variant{0, 1, 16}));
        REQUIRE((query(0, 1024, true, true) == Variant{0, 1, 277}));
        REQUIRE((query(0, 1025, true, true) == Variant{0, 1, 278}));
        REQUIRE((query(3, 1025, true, true) == Variant{3, 1, 278}));
        REQUIRE((query(3, 1025, false, true) == Variant{3, 1, 16}));  // no light buffer: no BVH instance
        REQUIRE((query(3, 1025, true, false) == Variant{3, 1, 16}));
        REQUIRE((query(4, 64, true, true) == Variant{5, 1, 277}));    // the thinner depth list
        REQUIRE((query(6, 0, false, false) == Variant{8, 1, 16}));
        REQUIRE((query(9, 0, false, false) == Variant{16, 1, 16}));
        REQUIRE((query(17, 0, false, false) == Variant{32, 1, 16}));
        REQUIRE(query(33, 0, false, false).maxd == -1);
        g_selections += 14;
    }
    // the frame threshold
    REQUIRE(small_frame(3999999.0) && !small_frame(4000000.0));
}

int main()
{
    check_list(kWf0List, "rt_trace_kernel", 3);
    check_list(kFrameList, "rt_trace_kernel", 3);
    check_list(kTinyList, "rt_trace_tiny", 3);
    check_list(kWfShadeList, "rt_wf_shade", 1);
    check_list(kAovList, "rt_aov_kernel", 1);
    check_list(kShadeRaysList, "rt_shade_rays_kernel", 3);
    for (const Variant& v : kShadeRaysList) REQUIRE(is_ray_query(v.flags) && count_of(kFrameList, v) == 0);
    for (const Variant& v : kFrameList) REQUIRE(!is_ray_query(v.flags));
    for (const Variant& v : kWf0List) REQUIRE(count_of(kFrameList, v) == 0 && is_wf0(v.flags));
    walk();
    walk_queries();
    literals();
    std::printf("variant_check: ok (%d selections)\n", g_selections);
    return 0;
}
