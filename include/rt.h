/*
 * rt.h — C ABI of the MI355X-native Whitted ray tracer (librt_amd.so).
 *
 * Drop-in boundary for the reference's per-pixel hot path.  The reference
 * (Rodyll/Ray-Tracing-GPU, /root/reference/Projet-INF8702) exposes that path
 * through the CScene singleton (Scene.h:41-70) and chooses the CPU loop or the
 * GL compute shader inside CScene::LancerRayons (Scene.cpp:672) on the global
 * CVar::g_ComputerShadersON (Var.cpp:11).  This header replaces:
 *
 *   rt_scene_*      CScene's host surface: AjusterResolution (Scene.cpp:162),
 *                   AjusterNbRebondsMax / AjusterEnergieMinimale /
 *                   AjusterIndiceRefraction (Scene.cpp:180-217),
 *                   TraiterFichierDeScene (Scene.cpp:231), Initialiser
 *                   (Scene.cpp:140: InitialiserCamera + Pretraitement) and the
 *                   LancerRayons prologue (Scene.cpp:676-679).
 *   rt_create /     CNuanceurCalculProg(path, compile) + activer()
 *   rt_destroy      (NuanceurCalculProg.cpp:57,146) and the GL context.
 *   rt_upload_scene the std140 UBO marshal "General"/"SceneData"
 *                   (Scene.cpp:697-1269) — but file-ordered, unbounded, and
 *                   without the ≤10-per-type cap.
 *   rt_render*      glDispatchCompute(W/16,H/16,1) + glMemoryBarrier
 *                   (Scene.cpp:1307-1310) and, for parity, the CPU loop
 *                   (Scene.cpp:1538-1561) whose float RGB went to
 *                   glTexImage2D(GL_RGBA8, GL_RGB, GL_FLOAT) (Scene.cpp:1562).
 *
 * Conventions: every call returns 0 on success, a negative RT_E* code on
 * failure (the library never exits; see rt_last_error / rt_scene_error).
 * Images are row-major, memory row y = pixel row PixY, row 0 = BOTTOM
 * scanline (GL texture origin, Scene.cpp:1545-1546).  Thread-safe across
 * contexts, not within one.
 */
#ifndef RT_AMD_RT_H
#define RT_AMD_RT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 8

enum {
    RT_OK = 0,
    RT_E_ARG = -1,       /* bad argument / null pointer                 */
    RT_E_IO = -2,        /* scene file cannot be opened                 */
    RT_E_PARSE = -3,     /* scene file rejected (see rt_scene_error)    */
    RT_E_STATE = -4,     /* call order violated (e.g. render before upload) */
    RT_E_HIP = -5,       /* HIP runtime error (see rt_last_error)       */
    RT_E_UNSUPPORTED = -6/* e.g. bounce depth beyond the compiled stack */
};

/* Surface kinds, file order is preserved in every array below. */
enum { RT_TRIANGLE = 0, RT_PLANE = 1, RT_QUADRIC = 2 };

/* Post-Pretraitement scene, FILE ORDER (the order of CScene::m_Surfaces).
 * geom[i*12 + …]:
 *   triangle: p0 p1 p2 (9)  normal (3)      — Triangle.h m_Pts / m_Normale
 *   plane   : normal (3) cst (1) 0…         — Plan.h m_Normale / m_Cst
 *   quadric : quad (3) lin (3) mix (3) cst  — Quadrique.h m_Quadratique /
 *                                             m_Lineaire / m_Mixte / m_Cst
 * material[i*10 + …]: r g b Ka Kd Ks shininess Kr Kt ior (ISurface.h:25-41)
 * lights[j*7 + …]   : pos(3) r g b intensity (Lumiere.h:23-27)
 * Caller owns the memory; rt_upload_scene deep-copies to the device. */
typedef struct rt_scene_flat {
    int32_t n_surfaces;
    int32_t n_lights;
    const int32_t* type;
    const float* geom;
    const float* material;
    const float* lights;
} rt_scene_flat;

/* One frame (or one row slab of it, for multi-GPU sharding). */
typedef struct rt_frame {
    float cam_pos[3];     /* CameraDeScene::Position                        */
    float orient[16];     /* CameraDeScene::Orientation, row-major m[4][4]  */
    float half_w, half_h; /* Scene.cpp:676-677                              */
    float inv_w, inv_h;   /* Scene.cpp:678-679                              */
    float background[3];  /* m_CouleurArrierePlan                           */
    int32_t width, height;
    int32_t row_begin, row_end; /* slab [row_begin,row_end) of PixY         */
    int32_t max_bounces;  /* m_NbRebondsMax (0 = the shipped executable)    */
    float min_energy;     /* m_EnergieMinRayon (0.01)                       */
    float scene_ior;      /* m_IndiceRefractionScene (1.0)                  */
    int32_t flags;        /* RT_FLAG_*                                      */
    /* ABI 3, multi-GPU load balance: band_rows > 0 (a
     * multiple of 16) renders cyclic row bands instead of the slab — global
     * bands b = band_index, band_index + band_count, ... of band_rows rows
     * each (band b = rows [b*band_rows, (b+1)*band_rows)), packed in that
     * order into the output; rows >= height are skipped and row_begin /
     * row_end are ignored.  The output then holds rt_band_rows(height,
     * band_rows, band_count, band_index) rows.  band_rows = 0: the slab.   */
    int32_t band_rows;
    int32_t band_count;
    int32_t band_index;
} rt_frame;

#define RT_FLAG_STATS 1   /* count rays / tests into rt_stats (small cost)  */

typedef struct rt_stats {
    uint64_t primary_rays;
    uint64_t bounce_rays;  /* reflected + refracted rays traced            */
    uint64_t shadow_rays;  /* rays sent to ObtenirFiltreDeSurface           */
    uint64_t shadow_tests_skipped; /* shadow tests elided by the exact
                                      all-lanes-opaque early exit           */
    float kernel_ms;       /* last render's kernel time (hipEvent)          */
    int32_t stack_depth;   /* compiled bounce-stack depth that ran          */
    int32_t light_batch;   /* lights sharing one shadow pass in that kernel */
    /* exact ray-primitive tests executed (ABI 2): a test a wave runs counts
       once per lane of the wave, culled tests not at all                    */
    uint64_t triangle_tests;
    uint64_t plane_tests;
    uint64_t quadric_tests;
    /* ABI 7: bounce rays (reflected / refracted, Scene.cpp:1779-1823): their
       exact triangle tests (part of triangle_tests; brute force: every
       triangle per ray) and the BVH inner nodes they visited (RT_OPT_BVH)  */
    uint64_t bounce_triangle_tests;
    uint64_t bvh_nodes_visited;
    char kernel[48];       /* the trace kernel that ran, e.g.
                              "rt_trace_tiny<0,1,37>"                        */
} rt_stats;

/* ------------------------------------------------------------ host scene */
typedef struct rt_scene rt_scene;

int rt_scene_create(rt_scene** out);                          /* CScene::CScene, Scene.cpp:61 */
int rt_scene_set_resolution(rt_scene*, int32_t w, int32_t h);  /* AjusterResolution, Scene.cpp:162 */
int rt_scene_set_max_bounces(rt_scene*, int32_t n);            /* AjusterNbRebondsMax, Scene.cpp:180 */
int rt_scene_set_min_energy(rt_scene*, float e);               /* AjusterEnergieMinimale, Scene.cpp:197 */
int rt_scene_set_scene_ior(rt_scene*, float ior);              /* AjusterIndiceRefraction, Scene.cpp:214 */
int rt_scene_load_file(rt_scene*, const char* path);           /* TraiterFichierDeScene, Scene.cpp:231 */
int rt_scene_prepare(rt_scene*);            /* Initialiser, Scene.cpp:140 (ONCE; not per frame) */
int rt_scene_get_flat(const rt_scene*, rt_scene_flat* out);    /* views into scene-owned arrays */
int rt_scene_get_frame(const rt_scene*, rt_frame* out);        /* full-frame rt_frame */
const char* rt_scene_error(const rt_scene*);
void rt_scene_destroy(rt_scene*);

/* --------------------------------------------------------------- device */
typedef struct rt_ctx rt_ctx;

int rt_create(int32_t hip_device, rt_ctx** out);
int rt_upload_scene(rt_ctx*, const rt_scene_flat*);
/* Synchronous.  rgba8_out: host or device pointer to
 * (row_end-row_begin)*width*4 bytes (or rt_band_rows(...) rows for bands),
 * RGBA8 = GL float->unorm8 of the RGB (clamp to [0,1], round to nearest,
 * alpha 255).  The synchronous renders also (re)build what is kept per
 * camera — the camera buffer of per-tile triangle lists — when the camera
 * (position, orientation, resolution) changed since the last build. */
int rt_render(rt_ctx*, const rt_frame*, uint8_t* rgba8_out);
/* Parity/debug: float RGB exactly as m_InfoPixel (unclamped), 3 floats/px. */
int rt_render_float(rt_ctx*, const rt_frame*, float* rgb_out);
/* Asynchronous, device pointers only, enqueued on `hip_stream` (a hipStream_t;
 * NULL = the HIP null stream, as in every HIP API).  Either output may be
 * NULL.  No host sync.  ABI 5: a new camera's per-camera state — the camera
 * buffer included, where it pays (RT_OPT_CAMERA_BUFFER) — is built on
 * `hip_stream` too; allocation happens only when that state grows (its
 * capacity follows earlier builds' totals, read back without waiting; a tile
 * whose list does not fit this time renders by the per-wave path — the same
 * image either way).
 *
 * Ordering (ABI 4).  The context keeps per-camera state on the device (camera
 * records, cone records, the camera buffer).  Every write of that state is
 * ordered after every render already enqueued on any stream that may read
 * it, and every render after the write that produced its state, with HIP
 * events — the caller needs no host sync between rt_render_async on any
 * number of streams and the synchronous calls, in any order.  A stream
 * passed here must stay alive until the next synchronous call on the context
 * (rt_render*, rt_upload_scene, rt_sync, rt_destroy) returns.
 *
 * hipGraph capture.  When `hip_stream` is capturing, the call records only
 * the trace kernel: the camera state must already be current for the frame
 * (a synchronous render, or rt_prepare_camera, of that camera first), else
 * RT_E_STATE.  A replay renders with the camera state current at replay
 * time, so it is valid while no other camera is rendered on the context; no
 * buffer a captured render references is freed before rt_upload_scene or
 * rt_destroy. */
int rt_render_async(rt_ctx*, const rt_frame*, uint8_t* rgba8_dev, float* rgb_dev, void* hip_stream);
/* ABI 4: a camera path rendered on the device — the headless analogue of
 * the reference's GLUT display loop (Main.cpp:229-250).
 * frames[0..n) (any cameras and sizes) are rendered after the work already
 * on `hip_stream`, and the work enqueued on it afterwards runs after all of
 * them; frame i's RGBA8 goes to rgba8_dev + i * rgba8_stride bytes and/or
 * its float RGB to (char*)rgb_dev + i * rgb_stride.  Frame i prepares its
 * own camera into sequence slot i % 4 (apart from the state the other
 * render calls use) and runs on the context's internal stream i % 4, forked
 * from and joined back into `hip_stream` by events, so up to four
 * consecutive frames are in flight at once; the call needs no host sync (and
 * allocates only when a slot's state grows), and a sequence captured into a hipGraph
 * (the internal streams join the capture) replays exactly whatever was
 * rendered on the context between capture and replay.  A sequence waits for
 * the context's async work on other streams (the slots are shared); a
 * captured one is ordered by its graph's position only.  Shadow rays use the
 * light buffer; camera rays the slot's own camera buffer (ABI 5: built on
 * the frame's stream; inside a capture only into a slot an earlier call
 * sized, else the per-wave culling — the same image).  RT_FLAG_STATS is not
 * accepted here. */
int rt_render_sequence_async(rt_ctx*, const rt_frame* frames, int32_t n, uint8_t* rgba8_dev, size_t rgba8_stride,
                             float* rgb_dev, size_t rgb_stride, void* hip_stream);
/* ABI 4: make the per-camera state (camera records, and the camera buffer
 * where the frame's kernel uses one) current for `frame` without rendering.
 * Synchronous, like rt_render. */
int rt_prepare_camera(rt_ctx*, const rt_frame* frame);
/* ABI 4: wait until everything enqueued through this context (any stream)
 * has finished. */
int rt_sync(rt_ctx*);

/* ABI 4: the CPU backend (the reference's CPU branch of
 * LancerRayons, Scene.cpp:1535-1563, which it chose on
 * CVar::g_ComputerShadersON, Var.cpp:11).  Explicit only: a context made by
 * rt_create_cpu (threads <= 0: all cores; no HIP call is made) takes
 * rt_upload_scene and renders with rt_cpu_render / rt_cpu_render_float into
 * host memory — the HIP path's images, bit for bit, by brute force on host
 * threads.  The HIP render entry points return RT_E_STATE on a CPU context,
 * and rt_create never returns one: a missing GPU is an error, never a switch. */
int rt_create_cpu(int32_t threads, rt_ctx** out);
int rt_cpu_render(rt_ctx*, const rt_frame*, uint8_t* rgba8_out);
int rt_cpu_render_float(rt_ctx*, const rt_frame*, float* rgb_out);

/* Supersampled anti-aliasing — an addition within ABI 8 (rt_abi_version()
 * stays 8; test for RT_HAS_SUPERSAMPLE).  `samples` describes the SAMPLE
 * grid: what rt_scene_set_resolution(s W, s H) + rt_scene_get_frame returns
 * for a W x H image, its slab (row_begin / row_end) or band fields in sample
 * rows.  The camera maps pixel px of a frame w wide to 2 px / w - 1, so the
 * s x s samples of output pixel (x, y) are exactly pixels (s x + i, s y + j)
 * of the plain frame at s W x s H.  With S that frame's float RGB, for s in
 * 1..8 and per channel
 *   out[y][x] = (((S[s y][s x] + S[s y][s x + 1]) + ...) + S[s y + s - 1][s x + s - 1]) / (float)(s s)
 * — sample rows bottom row first, left to right within a row, a sequential
 * float32 sum that starts as the first sample, then one IEEE division; RGBA8
 * is rt_render's unorm8 of that float; s = 1 is the plain render's bits.  The
 * output has width / s columns and rt_ss_rows(samples, s) rows (the sample
 * frame's rows / s), row 0 = bottom, packed by the slab / band rules (a band
 * row past the frame stays unwritten, as in rt_render).
 * RT_E_ARG, nothing enqueued: s outside 1..8; s does not divide width or
 * height, or (slabs) row_begin or row_end; band_rows > 0 not a multiple of
 * 16 s.
 * The samples are rendered by the plain render's kernels into a float
 * intermediate owned by the context and resolved on the same stream by
 * rt_resolve_kernel (csrc/rt_resolve.h).  Slab frames that do not render as
 * a wavefront are rendered and resolved in row chunks (RT_OPT_SS_CHUNK_ROWS),
 * which bounds the intermediate.  The intermediate is shared by the context's
 * streams: calls on different streams are ordered against each other by
 * events (no host sync needed), and it is allocated only when it grows.
 * Inside a hipGraph capture it cannot grow: RT_E_STATE unless an earlier
 * uncaptured call sized it (and, as for rt_render_async, the camera state is
 * current).  rt_stats of a synchronous call: kernel_ms covers trace and
 * resolve, primary_rays counts samples.  The rt_cpu_* pair is the CPU
 * backend's (same arithmetic, one shared function); each backend's calls
 * return RT_E_STATE on the other's context. */
#define RT_HAS_SUPERSAMPLE 1
int rt_render_ss(rt_ctx*, const rt_frame* samples, int32_t s, uint8_t* rgba8_out);   /* sync, host or device ptr */
int rt_render_ss_float(rt_ctx*, const rt_frame* samples, int32_t s, float* rgb_out); /* sync, host or device ptr */
int rt_render_ss_async(rt_ctx*, const rt_frame* samples, int32_t s, uint8_t* rgba8_dev, float* rgb_dev,
                       void* hip_stream);                                            /* either may be NULL */
int rt_cpu_render_ss(rt_ctx*, const rt_frame* samples, int32_t s, uint8_t* rgba8_out);
int rt_cpu_render_ss_float(rt_ctx*, const rt_frame* samples, int32_t s, float* rgb_out);
/* Output rows of a supersampled render; -1 if the (frame, s) pair is invalid. */
int32_t rt_ss_rows(const rt_frame* samples, int32_t s);

/* Primary-hit AOV renders (arbitrary output variables) — an addition within
 * ABI 8 (rt_abi_version() stays 8; test for RT_HAS_AOV).  One pass of primary
 * rays only, no shading: per pixel what CScene::ObtenirCouleur's search
 * (Scene.cpp:1705-1715) holds in `Result` when it leaves its loop.
 * Definition.  For pixel (px, py) of the frame the ray is the plain render's
 * (Scene.cpp:1543-1552).  Over the surfaces in file order, surface i with
 * distance t_i replaces the current winner when
 *   t_i > EPSILON && (t_i < t_best || t_best < 0)
 * (a tie keeps the earlier surface).  The planes, each (rows x width), planar:
 *   t   float32      the winner's ObtenirDistance()
 *   id  int32        the winner's file index (rt_scene_flat order)
 *   n   3 x float32  the winner's ObtenirNormale(): triangles and planes the
 *                    stored post-Pretraitement normal, NOT flipped towards
 *                    the ray; quadrics the normalised gradient at the hit
 *   miss: id = -1, t = -1.0f, n = (0, 0, 0) — the reference's empty
 *   CIntersection (Intersection.cpp:17-18).
 * max_bounces, min_energy, scene_ior, the background and the lights play no
 * part.  Rows, slabs and bands are packed exactly as by rt_render_float: row
 * 0 is the bottom row, and a band row past the frame stays unwritten.
 * Each plane pointer may be NULL (not all three).  rt_render_aov is
 * synchronous and takes a host or a device pointer per plane;
 * rt_render_aov_async takes device pointers and follows rt_render_async's
 * ordering and capture rules (ABI 4 / 5): per-camera state is made current
 * on `hip_stream`; inside a hipGraph capture only the AOV kernel is recorded,
 * RT_E_STATE if it needs camera state that is not current.  Scenes whose
 * colour frames take their camera records with the launch
 * (RT_OPT_LAUNCH_CAMERA) and scenes without triangles need no camera state:
 * their AOV pass never builds or invalidates any.  The other scenes run the
 * culling of their depth-0 colour frame (RT_OPT_CAMERA_BUFFER,
 * RT_OPT_CB_CAPACITY and RT_OPT_XCD_DEAL apply), so the AOV hit is the colour
 * image's primary hit by construction (rt_aov_kernel, csrc/rt_aov.h).
 * RT_E_ARG: all three planes NULL, RT_FLAG_STATS set, a bad slab / band.
 * RT_E_STATE: before rt_upload_scene, or on the other backend's context
 * (rt_cpu_render_aov is the CPU backend's: the same bits).
 * rt_last_stats after the synchronous call: kernel_ms the AOV kernel's time,
 * kernel its name and variant (e.g. "rt_aov_kernel<10>"), primary_rays the
 * pixels written, everything else 0.
 * Supersampling: an AOV render of the sample frame is the AOVs of the sample
 * grid; there is no resolve of AOVs. */
#define RT_HAS_AOV 1
typedef struct rt_aov {
    float* t;
    int32_t* id;
    float* n;
} rt_aov; /* each may be NULL, not all */
int rt_render_aov(rt_ctx*, const rt_frame*, const rt_aov* out);  /* sync; host or device ptr per plane */
int rt_render_aov_async(rt_ctx*, const rt_frame*, const rt_aov* dev, void* hip_stream); /* device ptrs */
int rt_cpu_render_aov(rt_ctx*, const rt_frame*, const rt_aov* out);                     /* CPU backend */

/* Closest-hit queries of arbitrary rays — an addition within ABI 8
 * (rt_abi_version() stays 8; test for RT_HAS_RAYS): "what does THIS ray hit",
 * as CScene::ObtenirCouleur's search (Scene.cpp:1705-1715) decides it, for
 * picking, line of sight, collision probes and a caller's own secondary rays.
 * Input.  rays: n records of 6 floats [Ox Oy Oz Dx Dy Dz] (a C-order (n, 6)
 * float32 array).  The direction is used AS GIVEN: CRayon::AjusterDirection
 * does not normalise, so t is in units of |D|.
 * Output.  `out` reuses rt_aov as planes of n entries: t (float32), id (int32,
 * the file index), n (3 x float32 per ray); each may be NULL, not all three.
 * Definition.  Over the surfaces in file order, surface i with distance t_i
 * replaces the current winner when
 *   t_i > EPSILON && (t_i < t_best || t_best < 0)
 * (a tie keeps the earlier surface); a miss is -1 / -1.0f / (0, 0, 0); the
 * normal is the winner's ObtenirNormale(): triangles and planes the stored
 * post-Pretraitement normal, quadrics the normalised gradient at the hit —
 * exactly rt_render_aov's values, so the AOV planes of a frame equal a ray
 * query of that frame's camera rays, bit for bit.
 * rt_trace_rays is synchronous; each of its four pointers is independently a
 * host or a device pointer (as in rt_render_aov).  rt_last_stats afterwards:
 * kernel ("rt_rays_kernel<0>": every surface per ray; "rt_rays_kernel<1>":
 * the triangles through the exact BVH, csrc/rt_rays.h), kernel_ms,
 * bounce_rays = n, primary_rays = 0.
 * rt_trace_rays_async takes device pointers only and enqueues one kernel on
 * `hip_stream`: it allocates nothing, builds nothing and reads or writes no
 * device state of the context besides the uploaded scene, so it needs no
 * ordering against any render and can be recorded into a hipGraph capture
 * unconditionally (a context that has never rendered included).  As for
 * rt_render_async, rt_upload_scene syncs the streams used here first, and a
 * stream must stay alive until the next synchronous call returns.
 * A query walks the BVH whenever the uploaded scene has one (at least 64
 * triangles and a reflective or refractive surface, or RT_OPT_RAY_BVH) and
 * RT_OPT_BVH is 1; else it tests every surface: the same bits either way.
 * Device pointers must be 8-byte aligned.
 * RT_OK and nothing written: n == 0.  RT_E_ARG: n < 0 or n > INT32_MAX, a NULL
 * rays / out, all three planes NULL, a misaligned device pointer, a host
 * pointer given to rt_trace_rays_async.  RT_E_STATE: before rt_upload_scene,
 * or on the other backend's context (rt_cpu_trace_rays is the CPU backend's:
 * host pointers, the same bits). */
#define RT_HAS_RAYS 1
int rt_trace_rays(rt_ctx*, const float* rays, int64_t n, const rt_aov* out);            /* sync; host or device ptrs */
int rt_trace_rays_async(rt_ctx*, const float* dev_rays, int64_t n, const rt_aov* dev_out, void* hip_stream);
int rt_cpu_trace_rays(rt_ctx*, const float* rays, int64_t n, const rt_aov* out);        /* CPU backend */

/* Shadow-filter (occlusion) queries of arbitrary segments — an addition
 * within ABI 8 (rt_abi_version() stays 8; test for RT_HAS_FILTER_RAYS): "how
 * much light gets from A to B", the any-hit half of the ray queries, as
 * CScene::ObtenirFiltreDeSurface (Scene.cpp:1842-1861) computes it for a
 * shadow ray: for area lights, ambient occlusion, visibility between agents.
 * Input.  segs: n records of 6 floats [Px Py Pz Lx Ly Lz] (a C-order (n, 6)
 * float32 array).  The segment runs from P to P + L; L is the UNNORMALISED
 * vector, exactly the LumiereRayon the reference hands to that function.
 * Output.  filter: n x 3 float32.
 * Definition, one float32 operation per step:
 *   dist = sqrtf((Lx*Lx + Ly*Ly) + Lz*Lz);  inv = 1.0f / dist;
 *   D = (Lx*inv, Ly*inv, Lz*inv);  F = (1, 1, 1)
 *   for every surface i in file order:  t_i = Intersection(P, D)
 *       if (t_i > EPSILON && t_i < dist)  F *= colour_i * Kt_i
 * (componentwise; colour * Kt first).  White when nothing is in the way,
 * exactly zero behind an opaque surface, a tint behind translucent ones.  No
 * special cases: a zero, tiny, huge or non-finite L gives whatever this
 * arithmetic gives (usually no comparison holds: white), a NaN stays a NaN.
 * Lights, camera, bounce depth and background play no part.
 * rt_filter_rays is synchronous; each of its two pointers is independently a
 * host or a device pointer.  rt_last_stats afterwards: kernel
 * ("rt_filter_kernel<0>": the file-order product, or any-hit tests of every
 * opaque surface; "rt_filter_kernel<1>": the triangles through a segment
 * any-hit walk of the exact BVH, csrc/rt_filter.h), kernel_ms, shadow_rays =
 * n, everything else 0.  <1> runs when the scene has the BVH (as for
 * rt_trace_rays), RT_OPT_BVH is 1 and every factor colour * Kt is finite and
 * >= +0; the same bits either way.
 * rt_filter_rays_async takes device pointers only and enqueues one kernel on
 * `hip_stream`: it allocates nothing, builds nothing and reads or writes no
 * device state of the context besides the uploaded scene, so it can be
 * recorded into a hipGraph capture on a context that never rendered; the
 * stream rules are rt_trace_rays_async's.  Device pointers must be 8-byte
 * aligned.
 * RT_OK and nothing written: n == 0.  RT_E_ARG: n < 0 or n > INT32_MAX, a NULL
 * segs / filter, a misaligned device pointer, a host pointer given to
 * rt_filter_rays_async.  RT_E_STATE: before rt_upload_scene, or on the other
 * backend's context (rt_cpu_filter_rays is the CPU backend's: host pointers,
 * the same bits). */
#define RT_HAS_FILTER_RAYS 1
int rt_filter_rays(rt_ctx*, const float* segs, int64_t n, float* filter);                       /* sync; host or device ptrs */
int rt_filter_rays_async(rt_ctx*, const float* dev_segs, int64_t n, float* dev_filter, void* hip_stream);
int rt_cpu_filter_rays(rt_ctx*, const float* segs, int64_t n, float* filter);                   /* CPU backend */

/* Radiance queries of arbitrary rays — an addition within ABI 8
 * (rt_abi_version() stays 8; test for RT_HAS_SHADE_RAYS): "what colour comes
 * along this ray", the third piece beside the closest-hit and the filter
 * queries, for cameras the pinhole frame cannot express (fisheye, panorama,
 * orthographic, depth of field), reflection and light probes, foveated or
 * re-projected sample patterns, sensors.
 * Input.  rays: n records of 6 floats [Ox Oy Oz Dx Dy Dz] (a C-order (n, 6)
 * float32 array).  D is used AS GIVEN, not normalised, as in rt_trace_rays.
 * params: an rt_frame of which max_bounces, min_energy, scene_ior and
 * background are read; its camera, resolution, slab and band fields are
 * ignored, and so is RT_FLAG_STATS in its flags.
 * Output.  rgb: n x 3 float32.
 * Definition: CScene::ObtenirCouleur (Scene.cpp:1705-1826, with the commented
 * reflect / refract recursion re-enabled below max_bounces, as for a render)
 * of a CRayon with origin O, direction D, energy 1, 0 bounces and IOR 1 — the
 * state the pixel loop gives a camera ray: the background on a miss, else
 * ambient + shadow-filtered Lambert and Phong of every light, + Kr x the
 * reflected ray's colour + Kt x the refracted ray's.  The float image of a
 * frame therefore equals this query of the frame's camera rays (bit for bit
 * on the CPU backend; on the GPU within the renders' own allowance for powf
 * on materials with a shininess).  No special cases: a zero or non-finite O
 * or D gives whatever this arithmetic gives, usually the background.
 * rt_shade_rays is synchronous; each of its two array pointers is
 * independently a host or a device pointer.  rt_last_stats afterwards: kernel
 * ("rt_shade_rays_kernel<MAXD,1,flags>", csrc/rt_shaderays.h: MAXD the
 * smallest compiled bounce stack of 0 1 2 3 5 8 16 32 that covers the
 * reachable depth; flags 16 every surface per ray, 21 / 22 depth 0 with the
 * light buffer, 277 / 278 the exact BVH for every ray of the tree and the
 * light buffer — when the scene has the BVH as for rt_trace_rays,
 * RT_OPT_RAY_BVH included; the same bits whichever runs), kernel_ms,
 * primary_rays = n, stack_depth, everything else 0.
 * rt_shade_rays_async takes device pointers only and enqueues one kernel on
 * `hip_stream`: it allocates nothing, builds nothing and reads or writes no
 * device state of the context besides the uploaded scene (its light buffer
 * and BVH included), so it can be recorded into a hipGraph capture on a
 * context that never rendered; the stream rules are rt_trace_rays_async's.
 * Device pointers must be 8-byte aligned.  `params` is read during the call.
 * RT_OK and nothing written: n == 0.  RT_E_ARG: a NULL params, n < 0 or n >
 * INT32_MAX, a NULL rays / rgb, a misaligned device pointer, a host pointer
 * given to rt_shade_rays_async.  RT_E_STATE: before rt_upload_scene, or on the
 * other backend's context (rt_cpu_shade_rays is the CPU backend's: host
 * pointers, the same bits).  RT_E_UNSUPPORTED: the reachable bounce depth
 * exceeds the deepest compiled stack (32), as for a render. */
#define RT_HAS_SHADE_RAYS 1
int rt_shade_rays(rt_ctx*, const rt_frame* params, const float* rays, int64_t n, float* rgb);      /* sync; host or device ptrs */
int rt_shade_rays_async(rt_ctx*, const rt_frame* params, const float* dev_rays, int64_t n, float* dev_rgb, void* hip_stream);
int rt_cpu_shade_rays(rt_ctx*, const rt_frame* params, const float* rays, int64_t n, float* rgb);  /* CPU backend */

/* Adaptive supersampling — an addition within ABI 8 (rt_abi_version() stays 8;
 * test for RT_HAS_ADAPTIVE_SS): s x s samples where neighbouring pixels
 * disagree and one sample everywhere else, the anti-aliasing of Whitted's own
 * paper, joined from rt_render_ss, rt_render_aov and rt_shade_rays.
 * `samples` is the SAMPLE frame exactly as for rt_render_ss (s W x s H, slab
 * fields in sample rows); the output is W x rt_ss_rows(samples, s), row 0 =
 * bottom, packed like rt_render_ss's.  Every step is one float32 operation.
 * Base frame.  B is `samples` with width / s, height / s, inv_w s, inv_h s,
 * row_begin / s, row_end / s, everything else equal.  For s = 2, 4, 8 the
 * products are exact, so B's pixels are the sample lattice S[s y][s x] bit for
 * bit (not so for s = 3, 5, 6, 7: fl(1 / (3 W)) 3 != fl(1 / W); they are
 * refused).  C(p) is B's float colour of pixel p as rt_render_float(B) gives
 * it, I(p) and N(p) its rt_render_aov(B) id and normal.
 * Mask.  mask(p) is the OR, over the 4-neighbours q of p inside the WHOLE
 * frame [0, W) x [0, H) (a slab changes nothing: its edge rows look at the
 * rows beyond) and over the requested criteria, of
 *   RT_EDGE_ID      I(p) != I(q)
 *   RT_EDGE_NORMAL  exactly one of I(p), I(q) is -1; or both are >= 0 and
 *                   ((Np.x*Nq.x + Np.y*Nq.y) + Np.z*Nq.z) < normal_cos
 *   RT_EDGE_COLOUR  fabsf(C(p).c - C(q).c) > colour_delta in some channel
 *                   (unclamped floats; a NaN compares false: no special case)
 * Output.  mask(p) == 0: C(p).  Else the box filter of rt_render_ss over the
 * pixel's s x s samples in its order, sample (i, j) being rt_shade_rays of the
 * camera ray of sample-frame pixel (s x + i, s y + j) with the frame's
 * max_bounces, min_energy, scene_ior and background.  RGBA8 is rt_render's
 * unorm8 of the float; the mask plane holds mask(p) as RT_EDGE_* bits, one
 * byte per pixel.  So an all-zero mask gives rt_render_float(B) and an
 * all-set one rt_render_ss_float(samples, s): exactly on the CPU backend, on
 * the GPU but for the renders' allowance for powf on materials with a
 * shininess.
 * rt_render_adaptive is synchronous; each output is independently a host or a
 * device pointer, or NULL (not all three).  rt_render_adaptive_async takes
 * device pointers and enqueues on `hip_stream` with rt_render_async's ordering
 * rules; the base planes and the list of flagged pixels live in buffers of
 * the context that its streams share, ordered by events and allocated only
 * when they grow, and no count is read back: the refine kernel
 * (rt_refine_kernel, csrc/rt_adaptive.h) runs a fixed grid bounded by the
 * device-resident count.
 * RT_E_ARG, nothing enqueued and nothing written: s not 2, 4 or 8; s not
 * dividing width, height, row_begin or row_end; band_rows != 0; criteria zero
 * or with unknown bits; all three outputs NULL; RT_FLAG_STATS set; a host
 * pointer given to the async call.  RT_E_STATE: before rt_upload_scene; on
 * the other backend's context (rt_cpu_render_adaptive is the CPU backend's:
 * host pointers, the same arithmetic); the async call on a capturing stream
 * (hipGraph capture is not supported).  RT_E_UNSUPPORTED: as for a render
 * beyond the deepest compiled stack.
 * rt_last_stats after the synchronous call: kernel the refine kernel's name
 * and variant ("rt_refine_kernel<MAXD,1,flags>", rt_shade_rays's variants;
 * the CPU backend: "cpu_render_adaptive"), kernel_ms base, classify and refine
 * together, primary_rays = output pixels + s s x flagged output pixels,
 * stack_depth, everything else 0.  A call that asks for the mask alone (rgba8
 * and rgb NULL) traces no sample — the refine pass is skipped on both
 * backends — and reports primary_rays = output pixels. */
#define RT_HAS_ADAPTIVE_SS 1
enum { RT_EDGE_ID = 1, RT_EDGE_NORMAL = 2, RT_EDGE_COLOUR = 4 };
typedef struct rt_adaptive {
    int32_t s;           /* 2, 4 or 8 */
    int32_t criteria;    /* RT_EDGE_* bits, at least one */
    float normal_cos;    /* RT_EDGE_NORMAL */
    float colour_delta;  /* RT_EDGE_COLOUR */
} rt_adaptive;
typedef struct rt_adaptive_out {
    uint8_t* rgba8;
    float* rgb;
    uint8_t* mask;
} rt_adaptive_out; /* each may be NULL, not all */
int rt_render_adaptive(rt_ctx*, const rt_frame* samples, const rt_adaptive*, const rt_adaptive_out* out);     /* sync; host or device ptr each */
int rt_render_adaptive_async(rt_ctx*, const rt_frame* samples, const rt_adaptive*, const rt_adaptive_out* dev, void* hip_stream);
int rt_cpu_render_adaptive(rt_ctx*, const rt_frame* samples, const rt_adaptive*, const rt_adaptive_out* out); /* CPU backend */

/* ABI 4: context options.  A/B and test switches and tuning knobs; no option
 * changes a single bit of any image.  Upload options take effect at the next
 * rt_upload_scene, launch options at the next render.                      */
enum {
    RT_OPT_LIGHT_BUFFER = 1,    /* upload+launch: shadow rays through the light buffer:
                                   1 every depth-0 scene with opaque triangles (default),
                                   2 only above 1,024 triangles, 0 never (wave culling) */
    RT_OPT_CAMERA_BUFFER = 2,   /* launch: per-camera tile lists: 1 (default) built by
                                   synchronous renders, by an async frame repeating the
                                   previous async frame's camera, and by async / sequence
                                   frames of a new camera where the build pays (more than
                                   1,024 triangles and at least 4 Mpx of output rows);
                                   2 by every frame; 0 never */
    RT_OPT_UNION_PRETEST = 3,   /* launch: small lists' union cone pre-test, 1 (default) / 0 */
    RT_OPT_LB_SCALE = 4,        /* upload: light-buffer cells per cone radius; 0 = auto (4,
                                   at least 128 cells per face edge; 6 above 1,024
                                   triangles); > 0 sets R alone */
    RT_OPT_DCOV_NEAR = 5,       /* upload: big lists' near light-buffer distance, x the
                                   light's farthest triangle; 0 = default (1.25) */
    RT_OPT_CB_INLINE_MAX_MB = 6,/* launch: camera-buffer entries carry inline camera
                                   records while they fit this many MiB (default 0 =
                                   never: the index walk, whose records are staged in
                                   LDS per window; 128 was the round-1 default) */
    RT_OPT_HOST_CHUNK_MB = 7,   /* launch: synchronous renders into host memory render
                                   and copy in row chunks of this many MiB of output,
                                   each copy overlapping the next chunk (default 8;
                                   0 = one kernel, then one copy) */
    RT_OPT_CB_CAPACITY = 8,     /* launch (ABI 5): camera-buffer entries allocated;
                                   0 (default) = sized from earlier builds' totals.  A
                                   tile whose list does not fit renders by the per-wave
                                   path (tests: a small value exercises that path) */
    RT_OPT_BVH = 13,            /* launch (ABI 7): bounce rays of scenes with at least
                                   64 triangles and a reflective or refractive surface
                                   walk the exact BVH built at upload (rt_bvh.h), with
                                   the depth-0 kernels' camera buffer and light-buffer
                                   shadows: 1 (default) / 0 (every triangle per bounce ray) */
    RT_OPT_WAVEFRONT = 14,      /* launch (ABI 7): such frames (RT_OPT_BVH) render their
                                   bounce levels as compacted queues in HBM, one launch
                                   per level then a fold per level (up to 8 levels,
                                   not inside a hipGraph capture or a sequence): 1
                                   (default) / 0 (one kernel, a per-lane DFS stack) */
    RT_OPT_WF_SORT = 15,        /* launch (ABI 8): such wavefront frames order each level's
                                   live rays by counting sorts on the device: bit 0 by
                                   their parent surface's bin (BVH leaf order) and branch
                                   before the BVH walk, bit 1 by their hit surface's bin
                                   before the shading (with bit 2: by the hit point's
                                   light-buffer cell seen from light 0 instead); 0 queue
                                   order; default 1; never changes an image */
    RT_OPT_XCD_DEAL = 16,       /* launch (ABI 8): how the big-list kernels (more than
                                   1,024 triangles) deal 8 x 8 tiles to the 8 XCDs: 1
                                   (default) runs of 8 along a tile row, 2 column stripes
                                   (each XCD walks its own 1/8 of the columns row by row),
                                   3 4 x 2 super-tiles round-robin, 0 hardware order;
                                   never changes an image */
    RT_OPT_XCD_STRIPE = 17,     /* launch (ABI 8): RT_OPT_XCD_DEAL 2's stripe width in tiles,
                                   stripe s on XCD s % 8; 0 (default) one stripe per XCD */
    RT_OPT_LB_UNROLL = 18,      /* launch (ABI 8): depth-0 frames of more than 1,024 triangles
                                   under 4 Mpx of output rows walk the light buffer's
                                   per-lane lists two entries per round: 1 (default) / 0;
                                   never changes an image */
    RT_OPT_WF_OVERLAP = 19,     /* launch (ABI 8): wavefront frames finish each level's
                                   straggling BVH walks and shade their rays on a second
                                   stream while the level's other rays are shaded (one
                                   event fork and join per level): 1 (default) / 0;
                                   never changes an image */
    RT_OPT_LAUNCH_CAMERA = 12   /* launch (ABI 6): depth-0 frames of scenes of 1-20
                                   triangles with light-buffer shadows take their camera
                                   records with the kernel launch — per-triangle camera
                                   values, nearest-hit bounds and tile-mask planes
                                   computed on the host per camera; the trace kernel
                                   computes its tile masks (stored per stream from a
                                   camera's second frame) — so no camera prepass or
                                   camera buffer exists and a moving camera renders
                                   like a static one: 1 (default) / 0 (the device
                                   camera buffer) */
    /* 9-11 (ABI 5: the async camera-state ring, the bounce lane-refill kernel,
       compact light-buffer entries) were measured slower or no faster and are
       removed in ABI 6: rt_set_option returns RT_E_ARG for them.  Their code
       and measurements: profiles/r04/set_aside/. */
};
/* Added within ABI 8 with the supersampled renders (a macro, not an
 * enumerator: the enum above is ABI 8's option list as released).  Launch:
 * output rows per chunk of rt_render_ss* on slab frames that do not render
 * as a wavefront, rounded up to a multiple of 16 (a chunk is then a multiple
 * of 16 s sample rows); 0 (default) = auto: the fewest equal chunks whose
 * float samples stay within 224 MiB each (one chunk up to 3840 x 2160
 * samples and beyond; two at 7680 x 4320).  Never changes an image. */
#define RT_OPT_SS_CHUNK_ROWS 20
/* Added within ABI 8 (a macro like the one above).  Launch: the launch-camera
 * kernels (RT_OPT_LAUNCH_CAMERA) skip a shadow ray's light-buffer cell lookup
 * where its direction from the light lies outside the cone — found at upload,
 * carried in the light's record — that contains every cell of that light's
 * buffer holding an entry: 1 (default) / 0 (every ray looks its cell up).
 * A skipped lookup would have read an empty list: never changes an image or
 * a tally. */
#define RT_OPT_LB_REGION 21
/* Added within ABI 8 with the ray queries (a macro like the ones above).
 * Upload: 1 builds the bounce-ray BVH also for a scene with no reflective or
 * refractive surface (still at least 64 triangles, and a tree that fits the
 * walk's stack), for rt_trace_rays* alone: such a scene has no bounce rays,
 * and no colour frame, AOV frame or wavefront decision reads that tree.
 * Default 0: the build costs upload time and memory on big meshes. */
#define RT_OPT_RAY_BVH 22
int rt_set_option(rt_ctx*, int32_t option, double value);
int rt_get_option(rt_ctx*, int32_t option, double* value);
/* ABI 4, upload: the far light-buffer ladder of big lists — rising distance
 * factors (x the light's farthest triangle), n <= 8; n = 0: none; factors =
 * NULL and n < 0: the default 2.5, 6, 16, 64. */
int rt_set_far_ladder(rt_ctx*, const double* factors, int32_t n);
int rt_last_stats(rt_ctx*, rt_stats* out);
const char* rt_last_error(rt_ctx*);
void rt_destroy(rt_ctx*);

int rt_abi_version(void);
/* Output rows of one rank's band set (see rt_frame.band_rows); -1 if invalid. */
int32_t rt_band_rows(int32_t height, int32_t band_rows, int32_t band_count, int32_t band_index);

#ifdef __cplusplus
}
#endif
#endif /* RT_AMD_RT_H */
