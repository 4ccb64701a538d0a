// rt_resolve.h — the supersampling resolve (include/rt.h rt_render_ss*): the
// box filter that turns an s x s sample grid into one pixel, written once for
// both backends, and the HIP kernel that streams it.
//
// Definition (DESIGN.md "Supersampled anti-aliasing"): output pixel (x, y) of
// factor s is
//     (((S[sy][sx] + S[sy][sx+1]) + ...) + S[sy+s-1][sx+s-1]) / (float)(s s)
// per channel: sample rows bottom row first, samples left to right within a
// row, a sequential float32 sum that STARTS as the first sample (no 0 +),
// then ONE IEEE division (never a multiply by a reciprocal: 1/9 is not a
// float).  No contraction (nothing here could contract, and the build's
// -ffp-contract=off holds anyway).
#ifndef RT_AMD_RT_RESOLVE_H
#define RT_AMD_RT_RESOLVE_H

#include "rt_math.h"

#pragma clang fp contract(off)

namespace rt {

constexpr int kSsMax = 8;  // largest supersampling factor

// One sample row's s samples (3 s floats at `row`) added to acc in order;
// `first`: the pixel's first sample row, whose first sample starts the sum.
RT_HD void resolve_row(Color& acc, const float* row, int s, bool first)
{
    for (int i = 0; i < s; ++i) {
        const float r = row[3 * i], g = row[3 * i + 1], b = row[3 * i + 2];
        if (first && i == 0) {
            acc = Color{r, g, b};
        } else {
            acc.r = acc.r + r;
            acc.g = acc.g + g;
            acc.b = acc.b + b;
        }
    }
}

// The sum over s s samples -> the pixel.
RT_HD Color resolve_div(Color acc, int s)
{
    const float n = (float)(s * s);
    return Color{acc.r / n, acc.g / n, acc.b / n};
}

// One output pixel from the sample frame: `px` = the pixel's bottom-left
// sample, `pitch` = floats per sample row.
RT_HD Color resolve_px(const float* px, size_t pitch, int s)
{
    Color acc{0.0f, 0.0f, 0.0f};
    for (int j = 0; j < s; ++j) resolve_row(acc, px + (size_t)j * pitch, s, j == 0);
    return resolve_div(acc, s);
}

RT_HD unsigned int resolve_rgba8(Color c)
{
    return unorm8(c.r) | (unorm8(c.g) << 8) | (unorm8(c.b) << 16) | 0xFF000000u;
}

#if defined(__HIPCC__) || defined(__HIP__)

// Output pixels per lane of the 16-byte path: the fewest whose sample-row
// segment (12 S P bytes) is a whole number of 16-byte words.
constexpr int resolve_run(int S) { return S % 4 == 0 ? 1 : (S % 2 == 0 ? 2 : 4); }

typedef float resolve_f4 __attribute__((ext_vector_type(4)));  // (the builtin loads take native vectors)

// A/B switches (DESIGN.md "Supersampled anti-aliasing" has the measurement):
// non-temporal sample loads / pixel stores.  Both measured slower than the
// plain forms on the MI355X — the samples come from the Infinity Cache, where
// the trace kernel has just left them — so both are off.
#ifndef RT_RESOLVE_NT_LOAD
#define RT_RESOLVE_NT_LOAD 0
#endif
#ifndef RT_RESOLVE_NT_STORE
#define RT_RESOLVE_NT_STORE 0
#endif

// The resolve: pure streaming, one lane = a run of P consecutive output
// pixels of one output row.  VEC: the sample frame's base and row pitch are
// 16-byte aligned (width % 4 == 0, which also makes every row a whole number
// of runs): the lane's segment of each sample row arrives as 16-byte loads.
// Otherwise P = 1 and plain dword loads.  The sample frame is read once and
// never again, the pixels are not read here at all.
//   samples : rows_out S rows of `width` samples (3 floats each), packed
//   out row q, pixel x -> rgb[(q wo + x) 3 ..], rgba[q wo + x]; wo = width / S
template <int S, bool VEC>
__global__ __launch_bounds__(256) void rt_resolve_kernel(const float* __restrict__ samples, int width, int wo,
                                                         int rows_out, float* __restrict__ rgb,
                                                         unsigned* __restrict__ rgba)
{
    constexpr int P = VEC ? resolve_run(S) : 1;
    constexpr int SEG = 3 * S * P;  // floats of one sample row this lane reads
    const int runs = wo / P;        // (VEC: wo % P == 0, see above)
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)runs * (size_t)rows_out) return;
    const int q = (int)(t / (size_t)runs);
    const int x0 = (int)(t % (size_t)runs) * P;
    const size_t pitch = (size_t)width * 3;
    const float* base = samples + (size_t)q * S * pitch + (size_t)x0 * S * 3;
    Color acc[P];
    // (the sample rows one at a time where all of them would not fit the
    // registers of a well-occupied wave: factors from 5)
    constexpr int UNR = SEG * S <= 128 ? S : 1;
#pragma unroll UNR
    for (int j = 0; j < S; ++j) {
        float seg[SEG];
        const float* row = base + (size_t)j * pitch;
        if constexpr (VEC) {
            const resolve_f4* row4 = reinterpret_cast<const resolve_f4*>(row);
#pragma unroll
            for (int k = 0; k < SEG / 4; ++k) {
#if RT_RESOLVE_NT_LOAD
                const resolve_f4 v = __builtin_nontemporal_load(row4 + k);
#else
                const resolve_f4 v = row4[k];
#endif
                seg[4 * k] = v.x, seg[4 * k + 1] = v.y, seg[4 * k + 2] = v.z, seg[4 * k + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < SEG; ++k) {
#if RT_RESOLVE_NT_LOAD
                seg[k] = __builtin_nontemporal_load(row + k);
#else
                seg[k] = row[k];
#endif
            }
        }
#pragma unroll
        for (int p = 0; p < P; ++p) resolve_row(acc[p], seg + 3 * S * p, S, j == 0);
    }
    const size_t o = (size_t)q * wo + x0;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const Color c = resolve_div(acc[p], S);
        if (rgb) {
#if RT_RESOLVE_NT_STORE
            __builtin_nontemporal_store(c.r, rgb + 3 * (o + p));
            __builtin_nontemporal_store(c.g, rgb + 3 * (o + p) + 1);
            __builtin_nontemporal_store(c.b, rgb + 3 * (o + p) + 2);
#else
            rgb[3 * (o + p)] = c.r;
            rgb[3 * (o + p) + 1] = c.g;
            rgb[3 * (o + p) + 2] = c.b;
#endif
        }
        if (rgba) {
#if RT_RESOLVE_NT_STORE
            __builtin_nontemporal_store(resolve_rgba8(c), rgba + o + p);
#else
            rgba[o + p] = resolve_rgba8(c);
#endif
        }
    }
}

#endif  // HIP

}  // namespace rt

#endif  // RT_AMD_RT_RESOLVE_H
