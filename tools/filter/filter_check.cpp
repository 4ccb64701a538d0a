// filter_check.cpp — a stand-alone host program over the CPU backend's
// shadow-filter query (csrc/rt_cpu.cpp cpu_filter_rays), for a sanitizer build
// (tests/test_filter_cpu.py: -fsanitize=address,undefined):
//
//   g++ -std=c++17 -fsanitize=address,undefined -ffp-contract=off -pthread -I ray-tracing-gpu_amd/csrc
//       tools/filter/filter_check.cpp ray-tracing-gpu_amd/csrc/rt_cpu.cpp -o filter_check && ./filter_check
//
// Two scenes: an opaque triangle, a ground plane and a translucent sphere
// (every factor >= 0: the any-hit path), and the same with a negative
// coefficient on the sphere (the file-order product).  Every array is a heap
// buffer of exactly the size the call may read or write: n = 0 with null
// arrays, counts around the chunk of 256 segments (1, 255, 256, 257, 1000),
// one and several threads, and degenerate segments — the zero vector, NaN and
// inf in P or L, huge and tiny L.  The values are checked against what the
// definition implies (rt.h): white past nothing, exactly +0 behind the
// triangle, the sphere's factor squared through the sphere, a segment that
// stops short is white.
// Prints "filter_check: ok", exit 0; else exit 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "rt_cpu.hpp"

static int fail(const char* what)
{
    std::printf("filter_check: %s\n", what);
    return 1;
}

static void* make_scene(float sphere_kt)
{
    // file order: triangle 0, plane 1, sphere 2
    static const int32_t type[3] = {RT_TRIANGLE, RT_PLANE, RT_QUADRIC};
    float geom[36] = {0};
    const float tri[12] = {-6.f, -1.f, -3.f, 6.f, -1.f, -3.f, 0.f, 7.f, -3.f, 0.f, 0.f, 1.f};
    std::memcpy(geom, tri, sizeof tri);
    const float pla[4] = {0.f, 1.f, 0.f, 5.f};  // y = -5
    std::memcpy(geom + 12, pla, sizeof pla);
    const float qua[10] = {1.f, 1.f, 1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, -4.f};  // |p| = 2
    std::memcpy(geom + 24, qua, sizeof qua);
    float mat[30];
    for (int i = 0; i < 3; ++i) {
        const float m[10] = {0.5f, 0.25f, 1.0f, 0.2f, 0.6f, 0.3f, 10.f, 0.f, i == 2 ? sphere_kt : 0.f, 1.f};
        std::memcpy(mat + 10 * i, m, sizeof m);
    }
    const float light[7] = {5.f, 9.f, 9.f, 1.f, 1.f, 1.f, 1.f};
    const rt_scene_flat flat{3, 1, type, geom, mat, light};
    void* scene = nullptr;
    if (rt::cpu_upload(&scene, &flat) != RT_OK) return nullptr;
    return scene;
}

static bool is3(const float* f, float r, float g, float b) { return f[0] == r && f[1] == g && f[2] == b; }

int main()
{
    for (float kt : {0.5f, -0.5f}) {
        void* scene = make_scene(kt);
        if (!scene) return fail("cpu_upload failed");

        // n = 0: nothing is read or written (null arrays)
        if (rt::cpu_filter_rays(scene, 4, nullptr, 0, nullptr, nullptr) != RT_OK) return fail("n = 0 failed");

        // known answers from (0, 0, 10)
        {
            const float segs[5 * 6] = {0.f, 0.f, 10.f, 0.f, 0.f,   -5.f,    // stops in front of the sphere: white
                                       0.f, 0.f, 10.f, 0.f, 0.f,   -10.f,   // ends inside it: one sphere hit (t = 8)
                                       0.f, 0.f, 10.f, 0.f, 0.f,   -20.f,   // through sphere and triangle
                                       4.f, 0.f, 10.f, 0.f, 0.f,   -20.f,   // beside the sphere, through the triangle
                                       0.f, 0.f, 10.f, 0.f, 100.f, 0.f};    // straight up: white
            float f[15];
            if (rt::cpu_filter_rays(scene, 2, segs, 5, f, nullptr) != RT_OK) return fail("filter failed");
            const float r = 0.5f * kt, g = 0.25f * kt, b = 1.0f * kt;
            if (!is3(f, 1.f, 1.f, 1.f)) return fail("a segment that stops short must be white");
            if (!is3(f + 3, r, g, b)) return fail("one translucent factor");
            // the triangle's factor is (0, 0, 0); the sphere's multiplies it after in file order
            if (!(f[6] == 0.f && f[7] == 0.f && f[8] == 0.f)) return fail("behind the triangle");
            if (kt > 0 && (std::signbit(f[6]) || std::signbit(f[7]) || std::signbit(f[8])))
                return fail("the opaque result must be +0");
            if (kt < 0 && !(std::signbit(f[6]) && std::signbit(f[7]) && std::signbit(f[8])))
                return fail("a negative factor after the zero gives -0 in file order");
            if (!is3(f + 9, 0.f, 0.f, 0.f)) return fail("the triangle alone");
            if (!is3(f + 12, 1.f, 1.f, 1.f)) return fail("nothing in the way");
        }

        // degenerate segments: no trap, no out-of-bounds access; every component is 1, 0, the factor or NaN
        {
            const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
            const float vals[] = {0.f, -0.f, nan, inf, -inf, 1e38f, 1e-38f, 1.f};
            std::vector<float> segs;
            for (float a : vals)
                for (float b : vals)
                    for (int c = 0; c < 6; ++c) {
                        float r[6] = {0.5f, 0.25f, 10.f, 0.f, 0.f, -20.f};
                        r[c] = a;
                        r[(c + 3) % 6] = b;
                        segs.insert(segs.end(), r, r + 6);
                    }
            const int64_t n = (int64_t)segs.size() / 6;
            std::vector<float> f((size_t)n * 3);
            if (rt::cpu_filter_rays(scene, 3, segs.data(), n, f.data(), nullptr) != RT_OK)
                return fail("degenerate segments failed");
            for (int64_t i = 0; i < n; ++i) {
                const float v = f[3 * (size_t)i];  // the red channel: 1, 0 or 0.25 (the sphere's 0.5 * Kt)
                if (!(v == 1.f || v == 0.f || v == 0.5f * kt)) return fail("degenerate segment: an impossible filter");
            }
        }

        // counts around the chunk, threads — each array at its exact size
        const int64_t counts[] = {1, 255, 256, 257, 1000};
        for (int64_t n : counts) {
            std::vector<float> segs((size_t)n * 6);
            for (int64_t i = 0; i < n; ++i) {
                const float a = 0.37f * (float)i, b = 0.11f * (float)i;
                float* r = &segs[6 * (size_t)i];
                r[0] = 3.f * std::sin(a);
                r[1] = 2.f * std::cos(b);
                r[2] = 10.f;
                r[3] = 6.f * std::sin(b);
                r[4] = 6.f * std::cos(a) - 4.f;
                r[5] = -20.f;
            }
            std::vector<float> f((size_t)n * 3);
            if (rt::cpu_filter_rays(scene, 4, segs.data(), n, f.data(), nullptr) != RT_OK) return fail("filter failed");
            if (n == 1000) {
                long white = 0, black = 0, tint = 0;
                for (int64_t i = 0; i < n; ++i) {
                    const float v = f[3 * (size_t)i];
                    ++(v == 1.f ? white : v == 0.f ? black : tint);
                }
                if (!white || !black || (kt > 0 && !tint)) return fail("the segments must give every kind of result");
            }
            for (int threads : {1, 7}) {
                std::vector<float> f1((size_t)n * 3);
                rt::cpu_filter_rays(scene, threads, segs.data(), n, f1.data(), nullptr);
                if (std::memcmp(f1.data(), f.data(), (size_t)n * 12)) return fail("the thread count changed a result");
            }
        }
        rt::cpu_free(scene);
    }
    std::printf("filter_check: ok\n");
    return 0;
}
