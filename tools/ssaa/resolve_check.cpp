// resolve_check.cpp — a stand-alone host program over the shared resolve
// function (csrc/rt_resolve.h resolve_px / resolve_rgba8), for a sanitizer
// build (tests/test_ssaa_cpu.py: -fsanitize=address,undefined):
//
//   g++ -std=c++17 -fsanitize=address,undefined -ffp-contract=off -I ray-tracing-gpu_amd/csrc
//       tools/ssaa/resolve_check.cpp -o resolve_check && ./resolve_check
//
// Every factor 1..8 over heap buffers of exactly the size the call may read
// (so a read past the last sample is a sanitizer report), checked against a
// sum written out here.  Prints "resolve_check: ok", exit 0; else exit 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rt_resolve.h"

int main()
{
    unsigned seed = 12345u;
    auto rnd = [&]() {
        seed = seed * 1664525u + 1013904223u;
        return (float)(seed >> 8) * (1.0f / 16777216.0f) * 1.5f - 0.25f;  // some samples outside [0, 1]
    };
    long checked = 0;
    for (int s = 1; s <= rt::kSsMax; ++s) {
        const int sizes[3][2] = {{1, 1}, {3, 2}, {5, 7}};
        for (const auto& wh : sizes) {
            const int wo = wh[0], ho = wh[1], w = wo * s, h = ho * s;
            std::vector<float> samples((size_t)w * h * 3);
            for (float& v : samples) v = rnd();
            const size_t pitch = (size_t)w * 3;
            for (int y = 0; y < ho; ++y) {
                for (int x = 0; x < wo; ++x) {
                    const rt::Color c = rt::resolve_px(samples.data() + (size_t)y * s * pitch + (size_t)x * s * 3, pitch, s);
                    float want[3];
                    for (int k = 0; k < 3; ++k) {
                        float acc = samples[((size_t)(y * s) * w + (size_t)x * s) * 3 + k];
                        for (int j = 0; j < s; ++j)
                            for (int i = 0; i < s; ++i)
                                if (i || j) acc = acc + samples[((size_t)(y * s + j) * w + (size_t)(x * s + i)) * 3 + k];
                        want[k] = acc / (float)(s * s);
                    }
                    if (c.r != want[0] || c.g != want[1] || c.b != want[2]) {
                        std::printf("resolve_check: s %d pixel (%d, %d) differs\n", s, x, y);
                        return 1;
                    }
                    const unsigned q = rt::resolve_rgba8(c);
                    if ((q >> 24) != 255u || (q & 255u) != rt::unorm8(want[0])) {
                        std::printf("resolve_check: s %d pixel (%d, %d) rgba8 differs\n", s, x, y);
                        return 1;
                    }
                    ++checked;
                }
            }
        }
    }
    std::printf("resolve_check: ok (%ld pixels)\n", checked);
    return 0;
}
