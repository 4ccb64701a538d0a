// rays_check.cpp — a stand-alone host program over the CPU backend's ray
// query (csrc/rt_cpu.cpp cpu_trace_rays), for a sanitizer build
// (tests/test_rays_cpu.py: -fsanitize=address,undefined):
//
//   g++ -std=c++17 -fsanitize=address,undefined -ffp-contract=off -pthread -I ray-tracing-gpu_amd/csrc
//       tools/rays/rays_check.cpp ray-tracing-gpu_amd/csrc/rt_cpu.cpp -o rays_check && ./rays_check
//
// A triangle, a ground plane and a sphere (aov_check's scene).  Every array is
// a heap buffer of exactly the size the call may read or write (so a load or
// store past the last ray is a sanitizer report): n = 0 with null arrays,
// counts around the chunk of 256 rays (1, 255, 256, 257, 1000), each single
// plane and every other subset, one and several threads, and degenerate rays
// — the zero direction, NaN and inf in the origin or the direction, huge and
// tiny directions.  The values are checked against what the definition
// implies (rt.h): a miss is -1 / -1 / +0, a triangle or plane reports its
// stored normal, t is in units of |D|, a hit's t exceeds EPSILON.
// Prints "rays_check: ok", exit 0; else exit 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "rt_cpu.hpp"

static int fail(const char* what)
{
    std::printf("rays_check: %s\n", what);
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
    float mat[30];
    for (int i = 0; i < 3; ++i) {
        const float m[10] = {0.5f, 0.5f, 0.5f, 0.2f, 0.6f, 0.3f, 10.f, 0.f, 0.f, 1.f};
        std::memcpy(mat + 10 * i, m, sizeof m);
    }
    const float light[7] = {5.f, 9.f, 9.f, 1.f, 1.f, 1.f, 1.f};
    const rt_scene_flat flat{3, 1, type, geom, mat, light};
    void* scene = nullptr;
    if (rt::cpu_upload(&scene, &flat) != RT_OK) return fail("cpu_upload failed");

    // n = 0: nothing is read or written (null arrays)
    if (rt::cpu_trace_rays(scene, 4, nullptr, 0, nullptr, nullptr, nullptr, nullptr) != RT_OK) return fail("n = 0 failed");

    // known answers from (0, 0, 10)
    {
        const float rays[5 * 6] = {0.f, 0.f,  10.f, 0.f, 0.f,  -1.f,   // the sphere's near pole: t = 8
                                   0.f, 0.f,  10.f, 0.f, 0.f,  -2.f,   // the same ray, |D| = 2: t = 4
                                   4.f, 0.f,  10.f, 0.f, 0.f,  -1.f,   // beside the sphere: the triangle at z = -3, t = 13
                                   0.f, 20.f, 10.f, 0.f, -1.f, 0.f,    // straight down: the plane y = -5, t = 25
                                   0.f, 0.f,  10.f, 0.f, 1.f,  0.f};   // straight up: a miss
        float t[5], n[15];
        int32_t id[5];
        if (rt::cpu_trace_rays(scene, 2, rays, 5, t, id, n, nullptr) != RT_OK) return fail("trace failed");
        if (id[0] != 2 || t[0] != 8.f || n[0] != 0.f || n[1] != 0.f || n[2] != 1.f) return fail("sphere pole");
        if (id[1] != 2 || t[1] != 4.f || n[5] != 1.f) return fail("t is not in units of |D|");
        if (id[2] != 0 || std::fabs(t[2] - 13.f) > 1e-4f || n[6] != 0.f || n[7] != 0.f || n[8] != 1.f) return fail("triangle");
        if (id[3] != 1 || t[3] != 25.f || n[9] != 0.f || n[10] != 1.f || n[11] != 0.f) return fail("plane");
        if (id[4] != -1 || t[4] != -1.f || n[12] != 0.f || n[13] != 0.f || n[14] != 0.f || std::signbit(n[12]))
            return fail("miss encoding");
    }

    // degenerate rays: no trap, no out-of-bounds access; a hit's t is above EPSILON (never NaN)
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
        std::vector<float> t((size_t)n), nn((size_t)n * 3);
        std::vector<int32_t> id((size_t)n);
        if (rt::cpu_trace_rays(scene, 3, rays.data(), n, t.data(), id.data(), nn.data(), nullptr) != RT_OK)
            return fail("degenerate rays failed");
        for (int64_t i = 0; i < n; ++i) {
            if (id[i] < -1 || id[i] > 2) return fail("degenerate ray: bad id");
            if (id[i] >= 0 && !(t[i] > 0.01f)) return fail("degenerate ray: a hit at or below EPSILON");
            if (id[i] < 0 && (t[i] != -1.f || nn[3 * i] != 0.f || nn[3 * i + 1] != 0.f || nn[3 * i + 2] != 0.f))
                return fail("degenerate ray: bad miss encoding");
        }
    }

    // counts around the chunk, threads, subsets of planes — each array at its exact size
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
        std::vector<float> t((size_t)n), nn((size_t)n * 3);
        std::vector<int32_t> id((size_t)n);
        if (rt::cpu_trace_rays(scene, 4, rays.data(), n, t.data(), id.data(), nn.data(), nullptr) != RT_OK)
            return fail("trace failed");
        if (n == 1000) {
            long hits[3] = {0, 0, 0};
            for (int64_t i = 0; i < n; ++i)
                if (id[i] >= 0) ++hits[id[i]];
            if (!hits[0] || !hits[1] || !hits[2]) return fail("the rays must reach every surface");
        }
        for (int threads : {1, 7}) {
            std::vector<float> t1((size_t)n), n1((size_t)n * 3);
            std::vector<int32_t> id1((size_t)n);
            rt::cpu_trace_rays(scene, threads, rays.data(), n, t1.data(), id1.data(), n1.data(), nullptr);
            if (std::memcmp(t1.data(), t.data(), (size_t)n * 4) || std::memcmp(id1.data(), id.data(), (size_t)n * 4) ||
                std::memcmp(n1.data(), nn.data(), (size_t)n * 12))
                return fail("the thread count changed a result");
        }
        for (int m = 1; m < 7; ++m) {
            std::vector<float> ts(m & 1 ? (size_t)n : 0), ns(m & 4 ? (size_t)n * 3 : 0);
            std::vector<int32_t> is(m & 2 ? (size_t)n : 0);
            rt::cpu_trace_rays(scene, 3, rays.data(), n, m & 1 ? ts.data() : nullptr, m & 2 ? is.data() : nullptr,
                               m & 4 ? ns.data() : nullptr, nullptr);
            if ((m & 1 && std::memcmp(ts.data(), t.data(), (size_t)n * 4)) ||
                (m & 2 && std::memcmp(is.data(), id.data(), (size_t)n * 4)) ||
                (m & 4 && std::memcmp(ns.data(), nn.data(), (size_t)n * 12)))
                return fail("a subset of planes differs");
        }
    }
    rt::cpu_free(scene);
    std::printf("rays_check: ok\n");
    return 0;
}
