// shade_check.cpp — a stand-alone host program over the CPU backend's
// radiance query (csrc/rt_cpu.cpp cpu_shade_rays), for a sanitizer build
// (tests/test_shade_cpu.py: -fsanitize=address,undefined):
//
//   g++ -std=c++17 -fsanitize=address,undefined -ffp-contract=off -pthread -I ray-tracing-gpu_amd/csrc
//       tools/shade/shade_check.cpp ray-tracing-gpu_amd/csrc/rt_cpu.cpp -o shade_check && ./shade_check
//
// A translucent triangle, a ground plane and a mirror sphere (rays_check's
// geometry with bouncing materials).  Every array is a heap buffer of exactly
// the size the call may read or write (so a load or store past the last ray
// is a sanitizer report): n = 0 with null arrays, counts around the chunk of
// 256 rays (1, 255, 256, 257, 1000), one and several threads, bounce depths 0
// to 5 with the default and a negative energy threshold, and degenerate rays —
// the zero direction, NaN and inf in the origin or the direction, huge and
// tiny directions.  The values are checked against what the definition
// implies (rt.h): a miss is the frame's background exactly, finite rays give
// finite colours, depth 0 differs from depth 3 on the mirror and through the
// translucent triangle, and the thread count changes no bit.
// Prints "shade_check: ok", exit 0; else exit 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "rt_cpu.hpp"

static int fail(const char* what)
{
    std::printf("shade_check: %s\n", what);
    return 1;
}

int main()
{
    // file order: triangle 0, plane 1, sphere 2
    const int32_t type[3] = {RT_TRIANGLE, RT_PLANE, RT_QUADRIC};
    float geom[36] = {0};
    const float tri[12] = {-6.f, -1.f, -3.f, 6.f, -1.f, -3.f, 0.f, 7.f, -3.f, 0.f, 0.f, 1.f};
    std::memcpy(geom, tri, sizeof tri);
    const float pla[4] = {0.f, 1.f, 0.f, 5.f};  // y = -5
    std::memcpy(geom + 12, pla, sizeof pla);
    const float qua[10] = {1.f, 1.f, 1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, -4.f};  // |p| = 2
    std::memcpy(geom + 24, qua, sizeof qua);
    // colour, ka, kd, ks, shininess, kr, kt, ior
    const float mats[3][10] = {{0.9f, 0.4f, 0.3f, 0.2f, 0.6f, 0.3f, 10.f, 0.0f, 0.4f, 1.3f},   // translucent
                               {0.2f, 0.8f, 0.2f, 0.2f, 0.7f, 0.0f, 0.f, 0.3f, 0.0f, 1.0f},    // a dull mirror
                               {0.5f, 0.5f, 0.9f, 0.1f, 0.5f, 0.5f, 20.f, 0.6f, 0.0f, 1.0f}};  // a mirror
    float mat[30];
    std::memcpy(mat, mats, sizeof mat);
    const float light[7] = {5.f, 9.f, 9.f, 1.f, 1.f, 1.f, 1.f};
    const rt_scene_flat flat{3, 1, type, geom, mat, light};
    void* scene = nullptr;
    if (rt::cpu_upload(&scene, &flat) != RT_OK) return fail("cpu_upload failed");

    rt_frame f{};  // only max_bounces, min_energy, scene_ior and background are read
    f.background[0] = 0.125f;
    f.background[1] = 0.25f;
    f.background[2] = 0.5f;
    f.min_energy = 0.01f;
    f.scene_ior = 1.0f;

    // n = 0: nothing is read or written (null arrays)
    if (rt::cpu_shade_rays(scene, 4, &f, nullptr, 0, nullptr, nullptr) != RT_OK) return fail("n = 0 failed");

    // known answers from (0, 0, 10)
    {
        const float rays[4 * 6] = {0.f, 0.f, 10.f, 0.f, 0.f, -1.f,   // the sphere's near pole
                                   0.f, 0.f, 10.f, 0.f, 0.f, -2.f,   // the same ray, |D| = 2
                                   0.f, 0.f, 10.f, 0.f, 1.f, 0.f,    // straight up: a miss
                                   4.f, 0.f, 10.f, 0.f, 0.f, -1.f};  // beside the sphere: through the triangle
        float c0[12], c3[12];
        f.max_bounces = 0;
        if (rt::cpu_shade_rays(scene, 2, &f, rays, 4, c0, nullptr) != RT_OK) return fail("shade failed");
        f.max_bounces = 3;
        if (rt::cpu_shade_rays(scene, 2, &f, rays, 4, c3, nullptr) != RT_OK) return fail("shade failed");
        if (std::memcmp(c0 + 6, f.background, 12) || std::memcmp(c3 + 6, f.background, 12)) return fail("a miss is the background");
        for (int k = 0; k < 12; ++k)
            if (!std::isfinite(c0[k]) || !std::isfinite(c3[k])) return fail("a finite ray gave a non-finite colour");
        if (!(c0[0] > 0.f && c0[2] >= c0[0])) return fail("the sphere's ambient term is missing");
        if (!std::memcmp(c0, c3, 12)) return fail("the mirror's colour must change with the depth");
        if (!std::memcmp(c0 + 9, c3 + 9, 12)) return fail("the translucent triangle's colour must change with the depth");
    }

    // degenerate rays: no trap, no out-of-bounds access
    {
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        const float vals[] = {0.f, -0.f, nan, inf, -inf, 1e38f, 1e-38f, 1.f};
        std::vector<float> rays;
        for (float a : vals)
            for (float b : vals)
                for (int c = 0; c < 6; ++c) {
                    float r[6] = {0.5f, 0.25f, 10.f, 0.f, 0.f, -1.f};
                    r[c] = a;
                    r[(c + 3) % 6] = b;
                    rays.insert(rays.end(), r, r + 6);
                }
        const int64_t n = (int64_t)rays.size() / 6;
        for (int depth : {0, 5}) {
            std::vector<float> rgb((size_t)n * 3);
            f.max_bounces = depth;
            if (rt::cpu_shade_rays(scene, 3, &f, rays.data(), n, rgb.data(), nullptr) != RT_OK)
                return fail("degenerate rays failed");
        }
    }

    // counts around the chunk, threads, depths — each array at its exact size
    const int64_t counts[] = {1, 255, 256, 257, 1000};
    for (int64_t n : counts) {
        std::vector<float> rays((size_t)n * 6);
        for (int64_t i = 0; i < n; ++i) {
            const float a = 0.37f * (float)i, b = 0.11f * (float)i;
            float* r = &rays[6 * (size_t)i];
            r[0] = 3.f * std::sin(a);
            r[1] = 2.f * std::cos(b);
            r[2] = 10.f;
            r[3] = 0.3f * std::sin(b);
            r[4] = 0.3f * std::cos(a) - 0.2f;
            r[5] = -1.f;
        }
        for (int depth = 0; depth <= 5; ++depth)
            for (float me : {0.01f, -1.0f}) {
                f.max_bounces = depth;
                f.min_energy = me;
                std::vector<float> rgb((size_t)n * 3);
                double ms = -1.0;
                if (rt::cpu_shade_rays(scene, 4, &f, rays.data(), n, rgb.data(), &ms) != RT_OK || !(ms >= 0.0))
                    return fail("shade failed");
                for (int threads : {1, 7}) {
                    std::vector<float> r1((size_t)n * 3);
                    rt::cpu_shade_rays(scene, threads, &f, rays.data(), n, r1.data(), nullptr);
                    if (std::memcmp(r1.data(), rgb.data(), (size_t)n * 12)) return fail("the thread count changed a result");
                }
            }
        f.min_energy = 0.01f;
    }
    rt::cpu_free(scene);
    std::printf("shade_check: ok\n");
    return 0;
}
