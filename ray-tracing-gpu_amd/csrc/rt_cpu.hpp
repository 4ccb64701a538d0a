// rt_cpu.hpp — internal interface of the CPU backend (rt_cpu.cpp) to the C
// ABI in rt_kernels.hip.  Host code only.
#ifndef RT_AMD_RT_CPU_HPP
#define RT_AMD_RT_CPU_HPP

#include "../../include/rt.h"

namespace rt {
// (Re)build the host scene from the flat post-Pretraitement scene.
int cpu_upload(void** handle, const rt_scene_flat* s);
void cpu_free(void* handle);
// Render `rows` output rows of frame f (slab or band set) on `threads` host
// threads (<= 0: all); either output may be null.  *ms = wall time; rays2
// (may be null) = the camera rays and the bounce rays traced.
int cpu_render(const void* handle, int threads, const rt_frame* f, int rows, uint8_t* rgba8, float* rgb, double* ms,
               unsigned long long* rays2 = nullptr);
// The primary-hit AOV planes of the same rows (rt.h rt_render_aov: t, file
// index, normal; a miss is -1, -1, 0); each output may be null.
int cpu_render_aov(const void* handle, int threads, const rt_frame* f, int rows, float* t, int32_t* id, float* n,
                   double* ms);
// Closest-hit queries of n arbitrary rays (rt.h rt_trace_rays: 6 floats per
// ray, O then D, the direction as given; planes of n entries, each may be
// null; a miss is -1, -1, 0): rt_rays_kernel's values bit for bit.
int cpu_trace_rays(const void* handle, int threads, const float* rays, int64_t n, float* t, int32_t* id, float* nrm,
                   double* ms);
// Shadow-filter queries of n arbitrary segments (rt.h rt_filter_rays: 6 floats
// per segment, P then the unnormalised L; 3 floats out per segment):
// rt_filter_kernel's values bit for bit.
int cpu_filter_rays(const void* handle, int threads, const float* segs, int64_t n, float* filter, double* ms);
// Radiance queries of n arbitrary rays (rt.h rt_shade_rays: 6 floats per ray,
// O then D as given; 3 floats out per ray; f carries max_bounces, min_energy,
// scene_ior and background): rt_shade_rays_kernel's values (bit for bit but
// for powf on materials with a shininess, as for a render).
int cpu_shade_rays(const void* handle, int threads, const rt_frame* f, const float* rays, int64_t n, float* rgb,
                   double* ms);
// The supersampling resolve (rt_resolve.h resolve_px, the HIP kernel's own
// arithmetic): rows_out rows of width / s pixels from their packed sample
// rows; either output may be null.  *ms = wall time.
void cpu_resolve(const float* samples, int width, int s, int rows_out, uint8_t* rgba8, float* rgb, double* ms);

// Adaptive supersampling (rt.h rt_render_adaptive*), both backends' frames.
// The base frame B of sample frame f with factor s (2, 4 or 8, dividing the
// frame and its slab): the plain frame at W x H whose pixels are the sample
// lattice S[s y][s x] — inv_w s and inv_h s are exact products of a power of
// two, and nothing else of the camera depends on the resolution.
inline rt_frame adaptive_base(const rt_frame& f, int s)
{
    rt_frame B = f;
    B.width = f.width / s;
    B.height = f.height / s;
    B.inv_w = f.inv_w * (float)s;
    B.inv_h = f.inv_h * (float)s;
    B.row_begin = f.row_begin / s;
    B.row_end = f.row_end / s;
    return B;
}
// B's slab with the halo: one more row on each side where the frame has one
// (the flag of a slab's edge row depends on the row beyond it).
inline rt_frame adaptive_halo(const rt_frame& B)
{
    rt_frame h = B;
    if (B.row_end > B.row_begin) {
        h.row_begin = B.row_begin > 0 ? B.row_begin - 1 : 0;
        h.row_end = B.row_end < B.height ? B.row_end + 1 : B.height;
    }
    return h;
}
// rt_cpu_render_adaptive: the base frame and its AOV planes through cpu_render
// / cpu_render_aov, rt_adaptive.h's edge_mask per pixel, then the flagged
// pixels' s x s samples through the pixel loop's own trace and resolve_px.
// Each output may be null.  *ms = wall time; *flagged = the flagged pixels.
int cpu_render_adaptive(const void* handle, int threads, const rt_frame* samples, int s, int criteria, float normal_cos,
                        float colour_delta, uint8_t* rgba8, float* rgb, uint8_t* mask, double* ms,
                        unsigned long long* flagged);
}  // namespace rt

#endif  // RT_AMD_RT_CPU_HPP
