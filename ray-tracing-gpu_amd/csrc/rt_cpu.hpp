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
}  // namespace rt

#endif  // RT_AMD_RT_CPU_HPP
