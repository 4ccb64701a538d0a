// rt_tile.h — the per-tile records of the launch-camera (tiny-scene) kernels:
// the tile word, the tile facts, TileRec and the lean record, with their pack
// and unpack helpers.  Plain C++ without a HIP type, so that a host program
// can include it alone (tools/lean/lean_check.cpp); the device code takes it
// through rt_cull.h, whose comment on the launch-camera records explains what
// the words mean.
#ifndef RT_AMD_RT_TILE_H
#define RT_AMD_RT_TILE_H

#include <cstddef>
#include <cstring>

#if defined(__HIPCC__) || defined(__HIP__)
#define RT_TILE_HD __host__ __device__ inline
#else
#define RT_TILE_HD inline
#endif

namespace rt {

constexpr int kTinyMax = 20;
constexpr int kTinyClassShift = 20, kTinyClassLights = 6;
static_assert(kTinyMax <= 20, "the tile word's bits from 20 up are the light classes");
static_assert(kTinyMax <= kTinyClassShift && kTinyClassShift + 2 * kTinyClassLights <= 32, "the tile word is 32 bits");

// The tile's second word, the tile facts: stored beside the word above (one
// 8-byte record per tile, TileRec) by the same frame, read by the same later
// frames, exact by the same determinism.  0: nothing is known.
//   bits 0-2   kind: how the tile's one surface is found (kFact*)
//   bits 3-7   the launch record's plane slot (kFactPlane) or the kept
//              triangle's position in the camera records (kFactTri)
//   bits 8-19  per light li < kTinyClassLights two bits: 8 + 2 li no-op (the
//              pass left the colour bit-identical in every active lane),
//              9 + 2 li all gated (every active lane passed dot(Lr, N) > 0)
//   bits 20-31 surf + 1, the file index every lane's winner has (0: unknown,
//              or an index past the field)
// Kinds: every lane of the wave (clamped lanes included: each repeats a pixel
// of the tile) missed, or every lane's winner is the one surface `surf`.
constexpr unsigned kFactNone = 0, kFactPlane = 1, kFactTri = 2, kFactSearch = 3, kFactMiss = 4;
constexpr int kFactKindBits = 3, kFactSlotShift = 3, kFactSlotBits = 5, kFactLightShift = 8, kFactSurfShift = 20;
constexpr unsigned kFactSurfMax = (1u << (32 - kFactSurfShift)) - 2u;  // the largest index the field holds
constexpr unsigned kFactNoop = 1, kFactGated = 2;  // a light's two bits
static_assert(kFactMiss < (1u << kFactKindBits), "the kind's field");
static_assert(kTinyMax <= (1 << kFactSlotBits), "a kept triangle's position fits the slot field");
static_assert(kFactSlotShift == kFactKindBits && kFactLightShift == kFactSlotShift + kFactSlotBits &&
                  kFactSurfShift == kFactLightShift + 2 * kTinyClassLights && kFactSurfShift < 32,
              "the tile facts are 32 bits, fields back to back");
constexpr unsigned tile_facts_pack(unsigned kind, unsigned slot, unsigned lights, unsigned surf_plus_1)
{
    return kind | slot << kFactSlotShift | lights << kFactLightShift | surf_plus_1 << kFactSurfShift;
}
constexpr unsigned tile_facts_kind(unsigned w) { return w & ((1u << kFactKindBits) - 1u); }
constexpr unsigned tile_facts_slot(unsigned w) { return (w >> kFactSlotShift) & ((1u << kFactSlotBits) - 1u); }
constexpr unsigned tile_facts_lights(unsigned w)
{
    return (w >> kFactLightShift) & ((1u << (2 * kTinyClassLights)) - 1u);
}
constexpr unsigned tile_facts_surf(unsigned w) { return w >> kFactSurfShift; }  // surf + 1
// the field of a file index: surf + 1, 0 where it does not fit
constexpr unsigned tile_facts_surf_field(int surf)
{
    return surf >= 0 && (unsigned)surf <= kFactSurfMax ? (unsigned)surf + 1u : 0u;
}
static_assert(tile_facts_kind(tile_facts_pack(kFactMiss, 31, 0xFFF, 0xFFF)) == kFactMiss &&
                  tile_facts_slot(tile_facts_pack(kFactTri, 19, 0, 0)) == 19 &&
                  tile_facts_lights(tile_facts_pack(0, 0, 0xABC, 0)) == 0xABC &&
                  tile_facts_surf(tile_facts_pack(kFactSearch, 0, 0, 4095)) == 4095 &&
                  tile_facts_surf_field((int)kFactSurfMax) == 4095 && tile_facts_surf_field((int)kFactSurfMax + 1) == 0,
              "pack and unpack agree");
// What the reading instance does with the facts, one bit per part (a build
// option for tools/ab_variants.py; profiles/r13/tile_facts/README.md):
//   1 miss tile: store the background   2 known surface: its records loaded early
//   4 known primitive: only it is tested   8 no-op pass skipped
//   16 all-gated pass without the gate's dot product   32 the light record's
//   hot half one light ahead, its cold half inside the shadow pass's branch
//   64 only the cold half inside that branch
#ifndef RT_TILE_FACTS
#define RT_TILE_FACTS (1 | 4 | 8 | 64)
#endif
struct alignas(8) TileRec {
    unsigned word, facts;
};
static_assert(sizeof(TileRec) == 8, "one tile's record: two words, one 8-byte scalar load");

// The lean record: a second, 64-byte record per tile, stored by the same frame
// as the TileRec, in the same buffer, read by the same later frames (not the
// counted one), exact by the same determinism.  It repeats the tile's word
// and facts and, for a LEAN tile, carries every per-surface value the reading
// frame's shading takes: the reader makes one 16-dword scalar load and, on a
// lean tile, no other load that hangs on the tile.
// A tile is lean exactly when
//   - its facts' kind is kFactPlane or kFactTri (one known surface, found by
//     one known primitive),
//   - the scene has no translucent surface and at most kTinyClassLights lights,
//   - every light has a class other than 0 once a no-op pass counts as class
//     3 (lean_classes),
//   - it is a real tile of the full frame's grid with masks.
// The lean flag is the kind field of the RECORD's facts: kFactLeanPlane for
// kFactPlane, kFactLeanTri for kFactTri (two values a TileRec never holds);
// lean_unpack gives the TileRec's facts back.  Operands are stored, never
// products, so every rounding stays in the reader, in the general path's order.
constexpr unsigned kFactLeanPlane = 5, kFactLeanTri = 6;
static_assert(kFactLeanPlane > kFactMiss && kFactLeanTri > kFactMiss && kFactLeanPlane != kFactLeanTri &&
                  kFactLeanTri < (1u << kFactKindBits),
              "the lean kinds are free values of the kind's field");
struct alignas(64) LeanRec {
    unsigned word, facts;                  // TileRec's; facts with a lean kind on a lean tile
    float pn[3], pnum;                     // plane tile: the launch record's slot [n] and n . O + cst
    float nrm[3];                          // hit_normal's value (constant over a plane or a triangle)
    float color[3], ka, kd, ks, shin;      // the material fields the ambient term and add_light read
};
static_assert(sizeof(LeanRec) == 64 && alignof(LeanRec) == 64, "one tile's lean record: one 16-dword scalar load");
static_assert(offsetof(LeanRec, word) == 0 && offsetof(LeanRec, facts) == 4 && offsetof(LeanRec, pn) == 8 &&
                  offsetof(LeanRec, pnum) == 20 && offsetof(LeanRec, nrm) == 24 && offsetof(LeanRec, color) == 36 &&
                  offsetof(LeanRec, ka) == 48 && offsetof(LeanRec, kd) == 52 && offsetof(LeanRec, ks) == 56 &&
                  offsetof(LeanRec, shin) == 60,
              "the lean record's dwords, as the debug export returns them");
// What parts of the lean record are built (a build option for
// tools/ab_variants.py; profiles/r14/tile_lean/README.md):
//   1 the storing frame writes the records   2 the reading frame takes the lean
//   path (lights through the light records)   4 its lights from the launch
//   record instead (measured slower, and the longer launch record costs the
//   smallest frames 0.0002 ms: off, and then the record does not carry them)
#ifndef RT_TILE_LEAN
#define RT_TILE_LEAN (1 | 2)
#endif
static_assert((RT_TILE_LEAN & 6) == 0 || (RT_TILE_LEAN & 1) != 0, "a lean reader needs the records written");

// A tile's classes with the facts' no-op bits folded in as class 3.
constexpr unsigned lean_classes(unsigned cls, unsigned lights)
{
    static_assert(kTinyClassLights == 6, "0x555: the no-op bit of each light");
    return cls | (lights & 0x555u) | (lights & 0x555u) << 1;
}
// Has every light li < n_lights a class other than 0 in c (lean_classes)?
constexpr bool lean_all_classed(unsigned c, int n_lights)
{
    return n_lights >= 0 && n_lights <= kTinyClassLights &&
           (((c | c >> 1) & 0x555u & ((1u << 2 * n_lights) - 1u)) == (0x555u & ((1u << 2 * n_lights) - 1u)));
}
// The rule above from the tile's two words and the scene's counts (tiled: a
// real tile with masks).
constexpr bool lean_tile(unsigned word, unsigned facts, int n_lights, int n_translucent, bool tiled)
{
    return tiled && n_translucent == 0 && tile_facts_surf(facts) != 0 &&
           (tile_facts_kind(facts) == kFactPlane || tile_facts_kind(facts) == kFactTri) &&
           lean_all_classed(lean_classes(word >> kTinyClassShift, tile_facts_lights(facts)), n_lights);
}

// The record's fields, unpacked (facts: the TileRec's).
struct LeanFields {
    unsigned word, facts;
    bool lean;
    float pn[3], pnum, nrm[3], color[3], ka, kd, ks, shin;
};
constexpr unsigned lean_kind_set(unsigned facts, unsigned kind)
{
    return (facts & ~((1u << kFactKindBits) - 1u)) | kind;
}
// A tile that is not lean stores its two words and zeros.
RT_TILE_HD LeanRec lean_pack(const LeanFields& f)
{
    LeanRec r{};
    r.word = f.word, r.facts = f.facts;
    if (!f.lean) return r;
    r.facts = lean_kind_set(f.facts, tile_facts_kind(f.facts) == kFactPlane ? kFactLeanPlane : kFactLeanTri);
    for (int i = 0; i < 3; ++i) r.pn[i] = f.pn[i], r.nrm[i] = f.nrm[i], r.color[i] = f.color[i];
    r.pnum = f.pnum;
    r.ka = f.ka, r.kd = f.kd, r.ks = f.ks, r.shin = f.shin;
    return r;
}
constexpr bool lean_kind(unsigned kind) { return kind == kFactLeanPlane || kind == kFactLeanTri; }
RT_TILE_HD LeanFields lean_unpack(const LeanRec& r)
{
    LeanFields f{};
    const unsigned k = tile_facts_kind(r.facts);
    f.word = r.word;
    f.lean = lean_kind(k);
    f.facts = f.lean ? lean_kind_set(r.facts, k == kFactLeanPlane ? kFactPlane : kFactTri) : r.facts;
    for (int i = 0; i < 3; ++i) f.pn[i] = r.pn[i], f.nrm[i] = r.nrm[i], f.color[i] = r.color[i];
    f.pnum = r.pnum;
    f.ka = r.ka, f.kd = r.kd, f.ks = r.ks, f.shin = r.shin;
    return f;
}

// The lights the lean path reads, by value with the launch (TinyLaunch): the
// hot half [x y z I] [r g b dcov] of the first kTinyClassLights light-shade
// records (rt_shade.h kLightRec: 16 floats each), zeros behind the last.  A
// scene with more lights has no lean tile; its first kTinyClassLights are
// copied all the same.
constexpr int kLeanLightFloats = 8, kLightRecFloats = 16;
inline void lean_lights_fill(float (*dst)[kLeanLightFloats], const float* lrec, int n_lights)
{
    std::memset(dst, 0, sizeof(float) * kLeanLightFloats * kTinyClassLights);
    for (int li = 0; li < n_lights && li < kTinyClassLights; ++li)
        std::memcpy(dst[li], lrec + (size_t)kLightRecFloats * li, sizeof(float) * kLeanLightFloats);
}

}  // namespace rt
#endif  // RT_AMD_RT_TILE_H
