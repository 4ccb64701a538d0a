// adaptive_check.cpp — a stand-alone host program over the CPU backend's
// adaptive supersampled render (csrc/rt_cpu.cpp cpu_render_adaptive) and the
// classification both backends share (csrc/rt_adaptive.h edge_mask), for a
// sanitizer build (tests/test_adaptive_cpu.py: -fsanitize=address,undefined):
//
//   g++ -std=c++17 -fsanitize=address,undefined -ffp-contract=off -pthread -I ray-tracing-gpu_amd/csrc
//       tools/adaptive/adaptive_check.cpp ray-tracing-gpu_amd/csrc/rt_cpu.cpp -o adaptive_check && ./adaptive_check
//
// shade_check's scene (a translucent triangle, a ground plane, a mirror
// sphere) seen from (0, 0, 10).  Every array is a heap buffer of exactly the
// size the call may read or write, so a load or store past a plane's last row
// — the halo rows of a slab are the risk — is a sanitizer report:
//  * edge_mask on planes of exactly the rows a slab needs (its rows and the
//    halo rows that exist), every slab of a 6 x 5 frame, against the mask of
//    the whole frame's planes;
//  * cpu_render_adaptive for s = 2, 4, 8, every criterion set, bounce depths 0
//    and 3, one and several threads: the thread count changes no bit; slabs
//    stitch to the whole frame; colour_delta = +inf gives cpu_render of the
//    base frame and an all-zero mask, colour_delta = -1 cpu_render +
//    cpu_resolve of the sample frame; each output alone equals the three
//    together; an empty slab writes nothing.
// Prints "adaptive_check: ok", exit 0; else exit 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "rt_adaptive.h"
#include "rt_cpu.hpp"

static int fail(const char* what)
{
    std::printf("adaptive_check: %s\n", what);
    return 1;
}

// The sample frame of a W x H image with factor s: a camera at (0, 0, 10)
// looking down -z, a 45-degree vertical field of view.
static rt_frame sample_frame(int W, int H, int s, int depth)
{
    rt_frame f{};
    f.cam_pos[2] = 10.f;
    for (int i = 0; i < 4; ++i) f.orient[5 * i] = 1.f;
    f.width = W * s;
    f.height = H * s;
    f.half_h = std::tan(0.5f * 0.785398f);
    f.half_w = f.half_h * (float)W / (float)H;
    f.inv_w = 1.0f / (float)f.width;
    f.inv_h = 1.0f / (float)f.height;
    f.background[0] = 0.125f;
    f.background[1] = 0.25f;
    f.background[2] = 0.5f;
    f.row_end = f.height;
    f.max_bounces = depth;
    f.min_energy = 0.01f;
    f.scene_ior = 1.0f;
    return f;
}

struct Image {
    std::vector<uint8_t> rgba, mask;
    std::vector<float> rgb;
    unsigned long long flagged = 0;
};

// One adaptive render into buffers of exactly the output's size.
static bool render(const void* scene, int threads, const rt_frame& f, int s, int criteria, float cosv, float delta,
                   Image& im)
{
    const size_t px = (size_t)(f.width / s) * (size_t)((f.row_end - f.row_begin) / s);
    im.rgba.assign(px * 4, 7);
    im.mask.assign(px, 7);
    im.rgb.assign(px * 3, 7.f);
    double ms = -1.0;
    return rt::cpu_render_adaptive(scene, threads, &f, s, criteria, cosv, delta, px ? im.rgba.data() : nullptr,
                                   px ? im.rgb.data() : nullptr, px ? im.mask.data() : nullptr, &ms,
                                   &im.flagged) == RT_OK &&
           ms >= 0.0;
}

static bool same(const Image& a, const Image& b)
{
    return a.rgba == b.rgba && a.mask == b.mask && a.rgb.size() == b.rgb.size() &&
           std::memcmp(a.rgb.data(), b.rgb.data(), a.rgb.size() * 4) == 0;
}

int main()
{
    // ---- edge_mask on exactly sized planes
    {
        const int W = 6, H = 5;
        std::vector<float> rgb((size_t)W * H * 3), nrm((size_t)W * H * 3);
        std::vector<int> id((size_t)W * H);
        const float nan = std::numeric_limits<float>::quiet_NaN();
        for (int k = 0; k < W * H; ++k) {
            id[k] = (k % 7 == 3) ? -1 : k / 4;
            for (int c = 0; c < 3; ++c) {
                rgb[3 * k + c] = (k % 5 == 0 && c == 1) ? nan : 0.07f * (float)((k * (c + 2)) % 9);
                nrm[3 * k + c] = id[k] < 0 ? 0.f : (c == k % 3 ? 1.f : 0.f);
            }
        }
        const rt::EdgePlanes whole{rgb.data(), id.data(), nrm.data(), W, H, 0};
        for (int criteria = 1; criteria <= rt::kEdgeAll; ++criteria) {
            int any = 0;
            for (int rb = 0; rb < H; ++rb)
                for (int re = rb + 1; re <= H; ++re) {
                    const int r0 = rb > 0 ? rb - 1 : 0, r1 = re < H ? re + 1 : H;  // with the halo rows that exist
                    const std::vector<float> c(rgb.begin() + (size_t)r0 * W * 3, rgb.begin() + (size_t)r1 * W * 3);
                    const std::vector<float> n(nrm.begin() + (size_t)r0 * W * 3, nrm.begin() + (size_t)r1 * W * 3);
                    const std::vector<int> ids(id.begin() + (size_t)r0 * W, id.begin() + (size_t)r1 * W);
                    // (a plane the criteria do not read is a null pointer)
                    const rt::EdgePlanes slab{(criteria & rt::kEdgeColour) ? c.data() : nullptr,
                                              (criteria & (rt::kEdgeId | rt::kEdgeNormal)) ? ids.data() : nullptr,
                                              (criteria & rt::kEdgeNormal) ? n.data() : nullptr, W, H, r0};
                    for (int y = rb; y < re; ++y)
                        for (int x = 0; x < W; ++x) {
                            const int m = rt::edge_mask(slab, x, y, criteria, 0.9f, 0.1f);
                            if (m != rt::edge_mask(whole, x, y, criteria, 0.9f, 0.1f)) return fail("a slab's mask differs");
                            if (m & ~criteria) return fail("a bit that was not asked for");
                            any |= m;
                        }
                }
            if (any != criteria) return fail("a criterion never fired on the synthetic planes");
        }
    }

    // ---- cpu_render_adaptive
    const int32_t type[3] = {RT_TRIANGLE, RT_PLANE, RT_QUADRIC};
    float geom[36] = {0};
    const float tri[12] = {-6.f, -1.f, -3.f, 6.f, -1.f, -3.f, 0.f, 7.f, -3.f, 0.f, 0.f, 1.f};
    std::memcpy(geom, tri, sizeof tri);
    const float pla[4] = {0.f, 1.f, 0.f, 5.f};  // y = -5
    std::memcpy(geom + 12, pla, sizeof pla);
    const float qua[10] = {1.f, 1.f, 1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, -4.f};  // |p| = 2
    std::memcpy(geom + 24, qua, sizeof qua);
    const float mats[3][10] = {{0.9f, 0.4f, 0.3f, 0.2f, 0.6f, 0.3f, 10.f, 0.0f, 0.4f, 1.3f},
                               {0.2f, 0.8f, 0.2f, 0.2f, 0.7f, 0.0f, 0.f, 0.3f, 0.0f, 1.0f},
                               {0.5f, 0.5f, 0.9f, 0.1f, 0.5f, 0.5f, 20.f, 0.6f, 0.0f, 1.0f}};
    float mat[30];
    std::memcpy(mat, mats, sizeof mat);
    const float light[7] = {5.f, 9.f, 9.f, 1.f, 1.f, 1.f, 1.f};
    const rt_scene_flat flat{3, 1, type, geom, mat, light};
    void* scene = nullptr;
    if (rt::cpu_upload(&scene, &flat) != RT_OK) return fail("cpu_upload failed");

    const int W = 22, H = 13;  // odd sizes: the last chunk of flagged pixels is ragged
    const float inf = std::numeric_limits<float>::infinity();
    for (int s : {2, 4, 8})
        for (int depth : {0, 3}) {
            const rt_frame f = sample_frame(W, H, s, depth);
            const size_t px = (size_t)W * H;
            for (int criteria = 1; criteria <= rt::kEdgeAll; ++criteria) {
                Image a, b;
                if (!render(scene, 4, f, s, criteria, 0.9f, 0.1f, a)) return fail("render failed");
                if (!render(scene, 1, f, s, criteria, 0.9f, 0.1f, b)) return fail("render failed");
                if (!same(a, b)) return fail("the thread count changed a result");
                unsigned long long n = 0;
                for (uint8_t m : a.mask) {
                    if (m & ~criteria) return fail("a mask bit that was not asked for");
                    n += m != 0;
                }
                if (n != a.flagged) return fail("the flagged count is not the mask's");
                for (float v : a.rgb)
                    if (!std::isfinite(v)) return fail("a non-finite colour");
                // slabs of 1, 5 and the remaining rows stitch to the whole frame
                Image st;
                const int slabs[3][2] = {{0, 1}, {1, 6}, {6, H}};
                for (const auto& rows : slabs) {
                    rt_frame g = f;
                    g.row_begin = rows[0] * s;
                    g.row_end = rows[1] * s;
                    Image part;
                    if (!render(scene, 3, g, s, criteria, 0.9f, 0.1f, part)) return fail("slab failed");
                    st.rgba.insert(st.rgba.end(), part.rgba.begin(), part.rgba.end());
                    st.mask.insert(st.mask.end(), part.mask.begin(), part.mask.end());
                    st.rgb.insert(st.rgb.end(), part.rgb.begin(), part.rgb.end());
                }
                if (!same(a, st)) return fail("the slabs do not stitch to the whole frame");
                // each output alone
                std::vector<float> rgb(px * 3);
                std::vector<uint8_t> q(px * 4), mk(px);
                rt::cpu_render_adaptive(scene, 2, &f, s, criteria, 0.9f, 0.1f, nullptr, rgb.data(), nullptr, nullptr, nullptr);
                rt::cpu_render_adaptive(scene, 2, &f, s, criteria, 0.9f, 0.1f, q.data(), nullptr, nullptr, nullptr, nullptr);
                rt::cpu_render_adaptive(scene, 2, &f, s, criteria, 0.9f, 0.1f, nullptr, nullptr, mk.data(), nullptr, nullptr);
                if (std::memcmp(rgb.data(), a.rgb.data(), px * 12) || q != a.rgba || mk != a.mask)
                    return fail("an output alone differs");
            }
            // nothing flagged: the base frame; everything flagged: the resolved sample frame
            const rt_frame B = rt::adaptive_base(f, s);
            std::vector<float> base(px * 3), samples(px * (size_t)(s * s) * 3), boxed(px * 3);
            rt::cpu_render(scene, 4, &B, H, nullptr, base.data(), nullptr);
            rt::cpu_render(scene, 4, &f, H * s, nullptr, samples.data(), nullptr);
            rt::cpu_resolve(samples.data(), f.width, s, H, nullptr, boxed.data(), nullptr);
            Image none, every;
            if (!render(scene, 4, f, s, rt::kEdgeColour, 0.9f, inf, none)) return fail("render failed");
            if (!render(scene, 4, f, s, rt::kEdgeColour, 0.9f, -1.0f, every)) return fail("render failed");
            if (none.flagged != 0 || std::memcmp(none.rgb.data(), base.data(), px * 12)) return fail("no flag: not the base frame");
            if (every.flagged != px || std::memcmp(every.rgb.data(), boxed.data(), px * 12))
                return fail("every flag: not the supersampled frame");
            // an empty slab
            rt_frame e = f;
            e.row_begin = e.row_end = 2 * s;
            Image empty;
            if (!render(scene, 4, e, s, rt::kEdgeAll, 0.9f, 0.1f, empty) || empty.flagged != 0) return fail("empty slab");
        }
    rt::cpu_free(scene);
    std::printf("adaptive_check: ok\n");
    return 0;
}
