// lean_check.cpp — a stand-alone host program over the lean tile record's
// helpers (ray-tracing-gpu_amd/csrc/rt_tile.h): lean_pack / lean_unpack, the
// lean rule and the launch record's lights by value.  Built and run by
// tests/test_lean_host.py with the sanitizers on:
//
//   g++ -std=c++17 -fsanitize=address,undefined -I ray-tracing-gpu_amd/csrc
//       tools/lean/lean_check.cpp -o lean_check && ./lean_check
//
// Checks: a round trip of every field, lean and not (a tile that is not lean
// stores its two words and zeros; the record's facts carry a lean kind, the
// unpacked ones the TileRec's); the rule against a plain restatement over
// every kind, light count 0 .. kTinyClassLights + 2 and class pattern; the
// lights' fill for 0 .. kTinyClassLights + 2 lights (hot halves copied, the
// rest zero, nothing past the array); the size asserts (compiled in).
// Prints "lean_check: ok (N checks)", exit 0; else exit 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_tile.h"

using namespace rt;

static int g_checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++g_checks;                                                        \
        if (!(cond)) {                                                     \
            std::printf("lean_check: %s (line %d)\n", #cond, __LINE__);    \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

static_assert(sizeof(LeanRec) == 64 && alignof(LeanRec) == 64 && sizeof(LeanRec) == 16 * sizeof(unsigned),
              "16 dwords, as rt_debug_tiny_lean returns them");
static_assert(sizeof(float[kTinyClassLights][kLeanLightFloats]) == 192, "the lights by value: 192 bytes");

static bool same_bits(const float* a, const float* b, int n) { return std::memcmp(a, b, sizeof(float) * n) == 0; }

static LeanFields fields(unsigned kind, unsigned seed)
{
    LeanFields f{};
    f.word = 0xABCDEu | (seed * 0x9E3779B9u & 0xFFF00000u);
    f.facts = tile_facts_pack(kind, seed % 20, seed * 2654435761u & 0xFFF, 1 + seed % 4000);
    f.lean = true;
    float* v[] = {f.pn, &f.pnum, f.nrm, f.color, &f.ka, &f.kd, &f.ks, &f.shin};
    const int n[] = {3, 1, 3, 3, 1, 1, 1, 1};
    unsigned k = seed;
    for (int i = 0; i < 8; ++i)
        for (int j = 0; j < n[i]; ++j) {
            k = k * 1664525u + 1013904223u;
            // every bit pattern that is no NaN payload game: signs, zeros, denormals, large values
            const unsigned bits = (k & 0x80000000u) | ((k >> 3) % 0x7F800000u);
            std::memcpy(&v[i][j], &bits, 4);
        }
    f.color[1] = -0.0f;
    return f;
}

static void round_trips()
{
    for (unsigned seed = 1; seed <= 200; ++seed)
        for (unsigned kind : {kFactPlane, kFactTri}) {
            const LeanFields f = fields(kind, seed);
            const LeanRec r = lean_pack(f);
            CHECK(r.word == f.word);
            CHECK(tile_facts_kind(r.facts) == (kind == kFactPlane ? kFactLeanPlane : kFactLeanTri));
            CHECK((r.facts >> kFactKindBits) == (f.facts >> kFactKindBits));
            const LeanFields g = lean_unpack(r);
            CHECK(g.lean && g.word == f.word && g.facts == f.facts);
            CHECK(same_bits(g.pn, f.pn, 3) && same_bits(&g.pnum, &f.pnum, 1) && same_bits(g.nrm, f.nrm, 3));
            CHECK(same_bits(g.color, f.color, 3) && same_bits(&g.ka, &f.ka, 1) && same_bits(&g.kd, &f.kd, 1));
            CHECK(same_bits(&g.ks, &f.ks, 1) && same_bits(&g.shin, &f.shin, 1));
            // the record's dwords, in the order the export returns them
            unsigned w[16];
            std::memcpy(w, &r, sizeof w);
            CHECK(w[0] == r.word && w[1] == r.facts);
            CHECK(std::memcmp(&w[2], f.pn, 12) == 0 && std::memcmp(&w[5], &f.pnum, 4) == 0);
            CHECK(std::memcmp(&w[6], f.nrm, 12) == 0 && std::memcmp(&w[9], f.color, 12) == 0);
            CHECK(std::memcmp(&w[12], &f.ka, 4) == 0 && std::memcmp(&w[15], &f.shin, 4) == 0);
        }
    // not lean: the two words and zeros, whatever the other fields hold
    for (unsigned kind : {kFactNone, kFactPlane, kFactTri, kFactSearch, kFactMiss}) {
        LeanFields f = fields(kind, 7);
        f.lean = false;
        const LeanRec r = lean_pack(f);
        unsigned w[16];
        std::memcpy(w, &r, sizeof w);
        CHECK(w[0] == f.word && w[1] == f.facts);
        for (int i = 2; i < 16; ++i) CHECK(w[i] == 0);
        const LeanFields g = lean_unpack(r);
        CHECK(!g.lean && g.word == f.word && g.facts == f.facts);
    }
}

// the rule, restated light by light
static bool rule(unsigned word, unsigned facts, int n_lights, int n_translucent, bool tiled)
{
    const unsigned kind = tile_facts_kind(facts);
    if (!tiled || n_translucent != 0 || n_lights > kTinyClassLights) return false;
    if (kind != kFactPlane && kind != kFactTri) return false;
    if (tile_facts_surf(facts) == 0) return false;
    for (int li = 0; li < n_lights; ++li) {
        const unsigned cls = (word >> (kTinyClassShift + 2 * li)) & 3u;
        const unsigned noop = (tile_facts_lights(facts) >> (2 * li)) & kFactNoop;
        if (cls == 0 && !noop) return false;
    }
    return true;
}

static void rules()
{
    unsigned k = 12345u;
    for (int n_lights = 0; n_lights <= kTinyClassLights + 2; ++n_lights)
        for (unsigned kind = 0; kind <= kFactMiss; ++kind)
            for (int rep = 0; rep < 400; ++rep) {
                k = k * 1664525u + 1013904223u;
                // sparse zero classes: most lights classed, as in a frame
                unsigned cls = 0, lights = 0;
                for (int li = 0; li < kTinyClassLights; ++li) {
                    k = k * 1664525u + 1013904223u;
                    cls |= ((k >> 8) % 5 == 0 ? 0u : 1u + (k >> 16) % 2u) << (2 * li);
                    lights |= ((k >> 20) & 3u) << (2 * li);
                }
                const unsigned word = (k & 0xFFFFFu) | cls << kTinyClassShift;
                const unsigned facts = tile_facts_pack(kind, k % 20, lights, rep % 3 == 0 ? 0 : 1 + k % 100);
                for (int nt = 0; nt < 2; ++nt)
                    for (int tiled = 0; tiled < 2; ++tiled)
                        CHECK(lean_tile(word, facts, n_lights, nt, tiled != 0) == rule(word, facts, n_lights, nt, tiled != 0));
            }
    CHECK(lean_tile(0, tile_facts_pack(kFactPlane, 0, 0, 1), 0, 0, true));  // no light: nothing to class
    CHECK(lean_classes(0x000, 0x555) == 0xFFF && lean_classes(0x249, 0) == 0x249);
}

static void lights()
{
    for (int n = 0; n <= kTinyClassLights + 2; ++n) {
        // exactly n records on the heap: a read past them is the sanitizer's to see
        std::vector<float> lrec((size_t)kLightRecFloats * n);
        for (size_t i = 0; i < lrec.size(); ++i) lrec[i] = 1.0f + (float)i;
        struct {
            float before[4];
            float v[kTinyClassLights][kLeanLightFloats];
            float after[4];
        } d;
        std::memset(&d, 0x5A, sizeof d);
        lean_lights_fill(d.v, lrec.data(), n);
        for (int i = 0; i < 4; ++i) {
            unsigned b, a;
            std::memcpy(&b, &d.before[i], 4), std::memcpy(&a, &d.after[i], 4);
            CHECK(b == 0x5A5A5A5Au && a == 0x5A5A5A5Au);
        }
        for (int li = 0; li < kTinyClassLights; ++li)
            for (int j = 0; j < kLeanLightFloats; ++j)
                CHECK(d.v[li][j] == (li < n ? lrec[(size_t)kLightRecFloats * li + j] : 0.0f));
    }
}

int main()
{
    round_trips();
    rules();
    lights();
    std::printf("lean_check: ok (%d checks)\n", g_checks);
    return 0;
}
