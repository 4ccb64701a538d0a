// rt_main.cpp — headless counterpart of the reference's Main.cpp entry point.
//
//   rt_render <scene.dat> [-x W] [-y H] [-d depth] [-o out.ppm] [-g gpus]
//             [--device first] [--bands] [-n frames] [-s]
//             [--gather rccl|host] [--backend hip|cpu] [--threads N]
//             [--ssaa N] [--aov PREFIX] [--rays IN.npy --hits PREFIX [--ray-bvh]]
//             [--segments IN.npy --filters OUT.npy [--ray-bvh]]
//             [--rays IN.npy --colours OUT.npy [-d N] [--ray-bvh]]
//             [--adaptive N [--edge id,normal,colour] [--edge-cos X] [--edge-delta X] [--mask OUT.npy]]
//
// Kept from Main.cpp:51-199: argv[1] is the scene file, -x / -y set the
// resolution (default 512x256, Var.cpp:4-5), the same [ETAT]/[ERREUR] log
// lines, and one wall-clock timer around the render (Main.cpp:168-198) — here
// with microsecond resolution (the Linux branch divides tv_usec by 10^6 in
// integer arithmetic, Main.cpp:192-193) and excluding GL set-up.
// Changed: the power-of-two check (Main.cpp:79-84) is advisory only, because
// the render core has no such restriction; there is no GLUT window — the
// frame is written as a binary PPM (top row first) instead; -d sets
// m_NbRebondsMax (default 0 = the shipped executable, whose recursion is
// commented out); -n renders N frames (the scene is prepared once, unlike
// LancerRayons which re-runs Pretraitement); -s prints ray counters.
// Multi-GPU from the command line: -g N renders the frame
// with N contexts, one per GPU from --device on, every context rendering its
// row slab (or, with --bands, its cyclic 16-row bands) into device memory on
// its own GPU, enqueued on its rank's stream; then ONE RCCL gather
// (librt_gather.so, include/rt_gather.h: ncclCommInitAll over the N GPUs, one
// ncclGroupStart / ncclSend / ncclRecv group) brings every part into the root
// GPU's frame over xGMI — the north star's "single RCCL gather" — and the
// frame crosses PCIe once, from the root.  --gather rccl uses it for -g 1 too
// (a send of the root's slab to itself).  With more contexts than GPUs
// (contexts wrapping round onto shared GPUs: RCCL needs one rank per GPU) or
// --gather host, each context renders straight into its part of the host
// frame on a host thread of its own and the parts are assembled in host
// memory — the same partition, without a collective.  --backend cpu renders
// on host threads instead (rt_create_cpu,
// the reference's CPU branch, chosen there by CVar::g_ComputerShadersON):
// the same image, the GPU never touched.  --ssaa N (1..8) writes the W x H
// image resolved from N x N samples per pixel (rt_render_ss / rt_cpu_render_ss:
// the scene is prepared at N W x N H), on either backend, one GPU.
// --aov PREFIX also writes the frame's primary-hit buffers (rt_render_aov /
// rt_cpu_render_aov) as PREFIX_t.npy (float32, H x W), PREFIX_id.npy (int32,
// H x W) and PREFIX_n.npy (float32, H x W x 3): NumPy format 1.0,
// little-endian, row 0 = the bottom scanline like the library (with --ssaa:
// of the N W x N H sample grid); on either backend, one GPU.
// --rays IN.npy --hits PREFIX traces the caller's own rays (rt_trace_rays /
// rt_cpu_trace_rays): IN.npy is a little-endian float32 (N, 6) C-order array
// [Ox Oy Oz Dx Dy Dz] in NumPy format 1.0 or 2.0, and PREFIX_t.npy (float32,
// N), PREFIX_id.npy (int32, N) and PREFIX_n.npy (float32, N x 3) are written
// by --aov's writer; on either backend, one GPU; --ray-bvh sets
// RT_OPT_RAY_BVH for the upload.  The frame itself is then rendered only when
// -o names a file.
// --segments IN.npy --filters OUT.npy asks for the shadow filter of the
// caller's own segments (rt_filter_rays / rt_cpu_filter_rays): IN.npy is read
// by --rays' reader as (N, 6) [Px Py Pz Lx Ly Lz] (from P to P + L), OUT.npy
// is float32 (N, 3); the same rules as --rays, with which it can be combined.
// --rays IN.npy --colours OUT.npy asks for the colour along the caller's own
// rays (rt_shade_rays / rt_cpu_shade_rays) with the scene's parameters and
// -d's bounce depth: OUT.npy is float32 (N, 3).  Alone or beside --hits; the
// same rules as --hits.
// --adaptive N (2, 4 or 8) writes the W x H image with adaptive supersampling
// (rt_render_adaptive / rt_cpu_render_adaptive: the scene is prepared at
// N W x N H as for --ssaa): N x N samples only where a pixel differs from a
// 4-neighbour by one of --edge's criteria (default id,normal,colour; --edge-cos
// the normals' cosine, default 0.9; --edge-delta the colour step, default
// 0.1), one sample elsewhere.  --mask OUT.npy also writes the criteria that
// flagged each pixel (uint8, H x W, RT_EDGE_* bits, row 0 = the bottom
// scanline).  On either backend, one GPU; not with --ssaa, --aov or the queries.
#include <hip/hip_runtime_api.h>

#include <dlfcn.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rt.h"
#include "../../include/rt_gather.h"

static int fail(const char* what, int rc, const char* msg)
{
    std::fprintf(stderr, "[ERREUR]: %s (code %d): %s\n", what, rc, msg ? msg : "");
    return 1;
}

// The frame (memory row 0 = bottom scanline) as a binary PPM, top row first.
static int write_ppm(const char* path, int W, int H, const std::vector<uint8_t>& img)
{
    FILE* f = std::fopen(path, "wb");
    if (!f) return 1;
    std::fprintf(f, "P6\n%d %d\n255\n", W, H);
    for (int y = H - 1; y >= 0; --y)
        for (int x = 0; x < W; ++x) std::fwrite(&img[((size_t)y * W + x) * 4], 1, 3, f);
    std::fclose(f);
    std::printf("[ETAT]: Image ecrite dans %s\n", path);
    return 0;
}

// One array as a NumPy format 1.0 file: magic, version, the header's length
// (little-endian u16) and the header dict padded with spaces to a multiple of
// 64 bytes, newline last; then the C-order data as they lie in memory.
static int write_npy(const std::string& path, const char* descr, int rows, int width, int comps, const void* data,
                     size_t bytes)
{
    char shape[64];
    if (width <= 0)  // one-dimensional (--hits: a value per ray)
        std::snprintf(shape, sizeof shape, "(%d,)", rows);
    else if (comps > 1)
        std::snprintf(shape, sizeof shape, "(%d, %d, %d)", rows, width, comps);
    else
        std::snprintf(shape, sizeof shape, "(%d, %d)", rows, width);
    std::string h = std::string("{'descr': '") + descr + "', 'fortran_order': False, 'shape': " + shape + ", }";
    while ((10 + h.size() + 1) % 64 != 0) h += ' ';
    h += '\n';
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return 1;
    const unsigned char head[10] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0, (unsigned char)(h.size() & 0xFF),
                                    (unsigned char)(h.size() >> 8)};
    bool ok = std::fwrite(head, 1, sizeof head, f) == sizeof head && std::fwrite(h.data(), 1, h.size(), f) == h.size();
    ok = ok && (bytes == 0 || std::fwrite(data, 1, bytes, f) == bytes);
    ok = (std::fclose(f) == 0) && ok;
    if (ok) std::printf("[ETAT]: AOV ecrit dans %s\n", path.c_str());
    return ok ? 0 : 1;
}

// --aov: the frame's primary-hit buffers from context c (either backend).
static int write_aov(rt_ctx* c, bool cpu, rt_frame frame, const char* prefix)
{
    frame.flags &= ~RT_FLAG_STATS;  // (not accepted by the AOV pass)
    const int W = frame.width, H = frame.height;
    const size_t px = (size_t)W * H;
    std::vector<float> t(px), n(px * 3);
    std::vector<int32_t> id(px);
    const rt_aov out{t.data(), id.data(), n.data()};
    const int rc = cpu ? rt_cpu_render_aov(c, &frame, &out) : rt_render_aov(c, &frame, &out);
    if (rc) return fail("rt_render_aov", rc, rt_last_error(c));
    const std::string p(prefix);
    static_assert(sizeof(float) == 4, "float32 planes");
    const uint16_t probe = 1;
    if (*(const unsigned char*)&probe != 1) return fail("--aov", RT_E_UNSUPPORTED, "little-endian hosts only");
    if (write_npy(p + "_t.npy", "<f4", H, W, 1, t.data(), px * 4)) return fail("fopen", -1, (p + "_t.npy").c_str());
    if (write_npy(p + "_id.npy", "<i4", H, W, 1, id.data(), px * 4)) return fail("fopen", -1, (p + "_id.npy").c_str());
    if (write_npy(p + "_n.npy", "<f4", H, W, 3, n.data(), px * 12)) return fail("fopen", -1, (p + "_n.npy").c_str());
    return 0;
}

// --rays: a NumPy format 1.0 / 2.0 file holding a little-endian float32
// (N, 6) C-order array.  false with `why` set for anything else.
static bool read_rays_npy(const char* path, std::vector<float>& rays, std::string& why)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) {
        why = "cannot open the file";
        return false;
    }
    std::vector<unsigned char> raw;
    unsigned char buf[65536];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) raw.insert(raw.end(), buf, buf + got);
    std::fclose(f);
    static const unsigned char magic[6] = {0x93, 'N', 'U', 'M', 'P', 'Y'};
    if (raw.size() < 10 || std::memcmp(raw.data(), magic, 6) != 0) {
        why = "not a .npy file";
        return false;
    }
    size_t hlen, hoff;
    if (raw[6] == 1 && raw[7] == 0) {
        hlen = (size_t)raw[8] | ((size_t)raw[9] << 8);
        hoff = 10;
    } else if (raw[6] == 2 && raw[7] == 0 && raw.size() >= 12) {
        hlen = (size_t)raw[8] | ((size_t)raw[9] << 8) | ((size_t)raw[10] << 16) | ((size_t)raw[11] << 24);
        hoff = 12;
    } else {
        why = ".npy format version 1.0 or 2.0 only";
        return false;
    }
    if (hlen > raw.size() - hoff) {
        why = "truncated header";
        return false;
    }
    const std::string h((const char*)raw.data() + hoff, hlen);
    // the value that follows 'key': up to the next top-level comma
    auto value = [&](const char* key, std::string& v) {
        const size_t k = h.find(std::string("'") + key + "'");
        if (k == std::string::npos) return false;
        size_t a = h.find(':', k);
        if (a == std::string::npos) return false;
        ++a;
        while (a < h.size() && h[a] == ' ') ++a;
        size_t b = a;
        int par = 0;
        while (b < h.size() && !((h[b] == ',' || h[b] == '}') && par == 0)) {
            par += h[b] == '(' ? 1 : h[b] == ')' ? -1 : 0;
            ++b;
        }
        while (b > a && h[b - 1] == ' ') --b;
        v = h.substr(a, b - a);
        return true;
    };
    std::string descr, order, shape;
    if (!value("descr", descr) || !value("fortran_order", order) || !value("shape", shape)) {
        why = "header without descr / fortran_order / shape";
        return false;
    }
    if (descr != "'<f4'" && descr != "\"<f4\"") {
        why = "dtype " + descr + ": little-endian float32 ('<f4') only";
        return false;
    }
    if (order != "False") {
        why = "Fortran order: C order only";
        return false;
    }
    long long n = -1;
    int cols = -1, used = 0;
    if (std::sscanf(shape.c_str(), "(%lld , %d )%n", &n, &cols, &used) != 2 || used != (int)shape.size() || cols != 6 ||
        n < 0 || n > INT32_MAX) {
        why = "shape " + shape + ": (N, 6) only";
        return false;
    }
    const size_t bytes = (size_t)n * 6 * sizeof(float);
    if (raw.size() - hoff - hlen != bytes) {
        why = "the data are not N x 6 x 4 bytes";
        return false;
    }
    rays.resize((size_t)n * 6);
    if (bytes) std::memcpy(rays.data(), raw.data() + hoff + hlen, bytes);
    return true;
}

// The head of every query verb: refuses a big-endian host (the .npy are written little-endian).
static int little_endian(const char* verb)
{
    const uint16_t probe = 1;
    return *(const unsigned char*)&probe == 1 ? 0 : fail(verb, RT_E_UNSUPPORTED, "little-endian hosts only");
}

// After the query `call` returned rc for n items: the error, or the [ETAT] line.
static int query_done(rt_ctx* c, const char* call, int rc, size_t n, const char* noun)
{
    if (rc) return fail(call, rc, rt_last_error(c));
    rt_stats st;
    rt_last_stats(c, &st);
    if (n) std::printf("[ETAT]: %zu %s, %s, %.3f ms\n", n, noun, st.kernel, st.kernel_ms);
    return 0;
}

// --rays / --hits: the closest hits of the file's rays from context c (either backend).
static int write_hits(rt_ctx* c, bool cpu, const std::vector<float>& rays, const char* prefix)
{
    if (little_endian("--hits")) return 1;
    const size_t n = rays.size() / 6;
    std::vector<float> t(n), nrm(n * 3);
    std::vector<int32_t> id(n);
    const rt_aov out{t.data(), id.data(), nrm.data()};
    const int rc = n == 0 ? 0
                   : cpu  ? rt_cpu_trace_rays(c, rays.data(), (int64_t)n, &out)
                          : rt_trace_rays(c, rays.data(), (int64_t)n, &out);
    if (query_done(c, "rt_trace_rays", rc, n, "rayons")) return 1;
    const std::string p(prefix);
    if (write_npy(p + "_t.npy", "<f4", (int)n, 0, 1, t.data(), n * 4)) return fail("fopen", -1, (p + "_t.npy").c_str());
    if (write_npy(p + "_id.npy", "<i4", (int)n, 0, 1, id.data(), n * 4)) return fail("fopen", -1, (p + "_id.npy").c_str());
    if (write_npy(p + "_n.npy", "<f4", (int)n, 3, 1, nrm.data(), n * 12)) return fail("fopen", -1, (p + "_n.npy").c_str());
    return 0;
}

// --segments / --filters (frame null): the shadow filters of the file's segments; --rays / --colours:
// the colours along the file's rays with frame's parameters.  From context c (either backend), one
// (N, 3) float32 .npy.
static int write_n3(rt_ctx* c, bool cpu, const rt_frame* frame, const std::vector<float>& in, const char* path)
{
    if (little_endian(frame ? "--colours" : "--filters")) return 1;
    const size_t n = in.size() / 6;
    std::vector<float> out(n * 3);
    int rc = 0;
    if (n && frame)
        rc = cpu ? rt_cpu_shade_rays(c, frame, in.data(), (int64_t)n, out.data())
                 : rt_shade_rays(c, frame, in.data(), (int64_t)n, out.data());
    else if (n)
        rc = cpu ? rt_cpu_filter_rays(c, in.data(), (int64_t)n, out.data())
                 : rt_filter_rays(c, in.data(), (int64_t)n, out.data());
    if (query_done(c, frame ? "rt_shade_rays" : "rt_filter_rays", rc, n, frame ? "rayons" : "segments")) return 1;
    if (write_npy(path, "<f4", (int)n, 3, 1, out.data(), n * 12)) return fail("fopen", -1, path);
    return 0;
}

static void print_done(rt_ctx* c0, double total, int frames, int gpus, int band, bool stats)
{
    rt_stats st;
    rt_last_stats(c0, &st);
    std::printf("[ETAT]: Termine! --> Temps total de rendu : %.6f secondes (%d frame(s), %d GPU(s)%s, kernel %.3f ms)\n",
                total, frames, gpus, band ? " bands" : "", st.kernel_ms);
    if (stats)
        std::printf("[STATS]: primary=%llu bounce=%llu shadow=%llu shadow_tests_skipped=%llu stack=%d "
                    "tests: triangle=%llu plane=%llu quadric=%llu (context 0)\n",
                    (unsigned long long)st.primary_rays, (unsigned long long)st.bounce_rays,
                    (unsigned long long)st.shadow_rays, (unsigned long long)st.shadow_tests_skipped,
                    st.stack_depth, (unsigned long long)st.triangle_tests, (unsigned long long)st.plane_tests,
                    (unsigned long long)st.quadric_tests);
}

// librt_gather.so, loaded only by the RCCL path (dlopen next to this
// binary): every other mode — --backend cpu, one GPU, --gather host — runs
// without RCCL present.
struct GatherLib {
    void* h = nullptr;
    int (*create)(int32_t, const int32_t*, rt_gather**) = nullptr;
    void* (*stream)(rt_gather*, int32_t) = nullptr;
    int (*chunks)(rt_gather*, int32_t, const rt_gather_chunk*, void*) = nullptr;
    int (*sync)(rt_gather*) = nullptr;
    int (*version)(void) = nullptr;
    const char* (*error)(rt_gather*) = nullptr;
    void (*destroy)(rt_gather*) = nullptr;
};

static bool load_gather(GatherLib& L, std::string& why)
{
    char exe[4096];
    const ssize_t n = readlink("/proc/self/exe", exe, sizeof exe - 1);
    std::string dir = ".";
    if (n > 0) {
        exe[n] = '\0';
        dir = exe;
        dir = dir.substr(0, dir.find_last_of('/'));
    }
    const std::string path = dir + "/librt_gather.so";
    L.h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!L.h) {
        const char* e = dlerror();
        why = path + ": " + (e ? e : "dlopen failed");
        return false;
    }
    auto sym = [&](const char* name) { return dlsym(L.h, name); };
    L.create = (decltype(L.create))sym("rt_gather_create");
    L.stream = (decltype(L.stream))sym("rt_gather_stream");
    L.chunks = (decltype(L.chunks))sym("rt_gather_chunks");
    L.sync = (decltype(L.sync))sym("rt_gather_sync");
    L.version = (decltype(L.version))sym("rt_gather_rccl_version");
    L.error = (decltype(L.error))sym("rt_gather_error");
    L.destroy = (decltype(L.destroy))sym("rt_gather_destroy");
    if (!L.create || !L.stream || !L.chunks || !L.sync || !L.version || !L.error || !L.destroy) {
        why = path + ": missing rt_gather_* symbols";
        return false;
    }
    return true;
}

// The RCCL path of -g N (N distinct GPUs), pipelined: every rank renders
// frame k into one of two slabs in device memory on its own GPU (on a render
// stream of its own), and frame k's RCCL group — a slab is one chunk, a band
// set one chunk per 16-row band, each landing at its rows of the root GPU's
// frame — runs on the ranks' gather streams while frame k + 1 renders into
// the other slabs; ordering by events only (render k -> gather k on each
// rank; gather k -> render k + 2 into the same slab), one host sync at the
// end.  Reported per frame: the renders (slowest rank, events) and the
// gather (root's gather stream, events), and the wall time of all frames.
static int render_rccl(std::vector<rt_ctx*>& ctx, std::vector<rt_frame>& part,
                       const std::vector<std::vector<uint8_t>>& img, int W, int H, int band, int dev0, int ndev,
                       int frames, bool stats, const char* out, rt_scene* scene)
{
    GatherLib G;
    std::string why;
    if (!load_gather(G, why)) return fail("librt_gather.so", RT_E_UNSUPPORTED, why.c_str());
    const int n = (int)ctx.size();
    std::vector<int32_t> devs((size_t)n);
    for (int r = 0; r < n; ++r) devs[r] = (dev0 + r) % ndev;
    rt_gather* g = nullptr;
    int rc = G.create(n, devs.data(), &g);
    if (rc) return fail("rt_gather_create", rc, G.error(g));
    const size_t rowb = (size_t)W * 4;
    // per rank: two slabs, a render stream, events (render done / gather
    // done per slab, timing pairs per frame)
    std::vector<void*> slab((size_t)2 * n, nullptr);
    std::vector<hipStream_t> rs((size_t)n, nullptr);
    std::vector<hipEvent_t> ev_r((size_t)2 * n, nullptr), ev_g((size_t)2 * n, nullptr);
    std::vector<hipEvent_t> t_r0((size_t)n * frames, nullptr), t_r1((size_t)n * frames, nullptr);
    std::vector<hipEvent_t> t_g0((size_t)frames, nullptr), t_g1((size_t)frames, nullptr);
    void* full = nullptr;
    for (int r = 0; r < n; ++r) {
        (void)hipSetDevice(devs[r]);
        for (int b = 0; b < 2; ++b)
            if (!img[r].empty() && hipMalloc(&slab[2 * r + b], img[r].size()) != hipSuccess)
                return fail("hipMalloc", RT_E_HIP, "slab");
        if (r == 0 && hipMalloc(&full, rowb * H) != hipSuccess) return fail("hipMalloc", RT_E_HIP, "frame");
        if (hipStreamCreateWithFlags(&rs[r], hipStreamNonBlocking) != hipSuccess) return fail("hipStreamCreate", RT_E_HIP, "");
        for (int b = 0; b < 2; ++b) {
            if (hipEventCreateWithFlags(&ev_r[2 * r + b], hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&ev_g[2 * r + b], hipEventDisableTiming) != hipSuccess)
                return fail("hipEventCreate", RT_E_HIP, "");
        }
        for (int k = 0; k < frames; ++k)
            if (hipEventCreate(&t_r0[(size_t)r * frames + k]) != hipSuccess ||
                hipEventCreate(&t_r1[(size_t)r * frames + k]) != hipSuccess)
                return fail("hipEventCreate", RT_E_HIP, "");
        if (r == 0)
            for (int k = 0; k < frames; ++k)
                if (hipEventCreate(&t_g0[k]) != hipSuccess || hipEventCreate(&t_g1[k]) != hipSuccess)
                    return fail("hipEventCreate", RT_E_HIP, "");
    }
    auto chunks_of = [&](int b) {
        std::vector<rt_gather_chunk> ch;
        for (int r = 0; r < n; ++r) {
            if (img[r].empty()) continue;
            const char* src = (const char*)slab[2 * r + b];
            if (band) {  // packed band j of rank r -> frame rows (j n + r) band ...
                const int q = (int)(img[r].size() / rowb) / band;
                for (int j = 0; j < q; ++j) {
                    const int y0 = (j * n + r) * band, rows = std::min(band, H - y0);
                    if (rows > 0) ch.push_back({r, src + (size_t)j * band * rowb, (size_t)rows * rowb, (size_t)y0 * rowb});
                }
            } else {
                ch.push_back({r, src, img[r].size(), (size_t)part[r].row_begin * rowb});
            }
        }
        return ch;
    };
    const std::vector<rt_gather_chunk> ch[2] = {chunks_of(0), chunks_of(1)};
    size_t gbytes = 0;
    for (const auto& c : ch[0]) gbytes += c.bytes;
    const int ver = G.version();
    std::printf("[ETAT]: gather: RCCL %d.%d.%d, %d rank(s), %zu chunk(s), %.1f MB into GPU %d, pipelined (2 slabs)\n",
                ver / 10000, (ver / 100) % 100, ver % 100, n, ch[0].size(), gbytes / 1e6, devs[0]);
    std::printf("[ETAT]: Lancer de rayons...\n");
    const auto t0 = std::chrono::steady_clock::now();
    for (int k = 0; k < frames; ++k) {
        const int b = k & 1;
        for (int r = 0; r < n; ++r) {
            if (img[r].empty()) continue;
            (void)hipSetDevice(devs[r]);
            if (k >= 2 && hipStreamWaitEvent(rs[r], ev_g[2 * r + b], 0) != hipSuccess)  // gather k-2 read this slab
                return fail("hipStreamWaitEvent", RT_E_HIP, "");
            (void)hipEventRecord(t_r0[(size_t)r * frames + k], rs[r]);
            if ((rc = rt_render_async(ctx[r], &part[r], (uint8_t*)slab[2 * r + b], nullptr, rs[r])))
                return fail("LancerRayons", rc, rt_last_error(ctx[r]));
            (void)hipEventRecord(t_r1[(size_t)r * frames + k], rs[r]);
            (void)hipEventRecord(ev_r[2 * r + b], rs[r]);
            if (hipStreamWaitEvent((hipStream_t)G.stream(g, r), ev_r[2 * r + b], 0) != hipSuccess)
                return fail("hipStreamWaitEvent", RT_E_HIP, "");
        }
        (void)hipSetDevice(devs[0]);
        // the root's gather stream starts timing once EVERY rank's slab is
        // rendered (its receives wait for them anyway), so the reported
        // gather time is the exchange, not the slowest rank's render
        for (int r = 1; r < n; ++r)
            if (!img[r].empty() && hipStreamWaitEvent((hipStream_t)G.stream(g, 0), ev_r[2 * r + b], 0) != hipSuccess)
                return fail("hipStreamWaitEvent", RT_E_HIP, "");
        (void)hipEventRecord(t_g0[k], (hipStream_t)G.stream(g, 0));
        if ((rc = G.chunks(g, (int32_t)ch[b].size(), ch[b].data(), full)))
            return fail("rt_gather_chunks", rc, G.error(g));
        (void)hipEventRecord(t_g1[k], (hipStream_t)G.stream(g, 0));
        for (int r = 0; r < n; ++r) {
            if (img[r].empty()) continue;
            (void)hipSetDevice(devs[r]);
            (void)hipEventRecord(ev_g[2 * r + b], (hipStream_t)G.stream(g, r));
        }
    }
    if ((rc = G.sync(g))) return fail("rt_gather_sync", rc, G.error(g));
    for (int r = 0; r < n; ++r) {
        (void)hipSetDevice(devs[r]);
        (void)hipStreamSynchronize(rs[r]);
    }
    const double total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    double rsum = 0.0, gsum = 0.0;
    for (int k = 0; k < frames; ++k) {
        float worst = 0.f, gm = 0.f;
        for (int r = 0; r < n; ++r) {
            if (img[r].empty()) continue;
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, t_r0[(size_t)r * frames + k], t_r1[(size_t)r * frames + k]) == hipSuccess)
                worst = std::max(worst, ms);
        }
        (void)hipEventElapsedTime(&gm, t_g0[k], t_g1[k]);
        rsum += worst;
        gsum += gm;
    }
    std::vector<uint8_t> host(rowb * H);
    (void)hipSetDevice(devs[0]);
    if (hipMemcpy(host.data(), full, host.size(), hipMemcpyDeviceToHost) != hipSuccess)
        return fail("hipMemcpy", RT_E_HIP, "frame to host");
    std::printf("[ETAT]: per frame: render %.3f ms (slowest rank), gather %.3f ms (RCCL group of %zu send/recv "
                "pair(s)), wall %.3f ms\n",
                rsum / frames, gsum / frames, ch[0].size(), total * 1e3 / frames);
    print_done(ctx[0], total, frames, n, band, stats);
    if (out && write_ppm(out, W, H, host)) return fail("fopen", -1, out);
    for (int r = 0; r < n; ++r) {
        (void)hipSetDevice(devs[r]);
        for (int b = 0; b < 2; ++b) {
            (void)hipFree(slab[2 * r + b]);
            (void)hipEventDestroy(ev_r[2 * r + b]);
            (void)hipEventDestroy(ev_g[2 * r + b]);
        }
        for (int k = 0; k < frames; ++k) {
            (void)hipEventDestroy(t_r0[(size_t)r * frames + k]);
            (void)hipEventDestroy(t_r1[(size_t)r * frames + k]);
        }
        (void)hipStreamDestroy(rs[r]);
    }
    (void)hipSetDevice(devs[0]);
    for (int k = 0; k < frames; ++k) {
        (void)hipEventDestroy(t_g0[k]);
        (void)hipEventDestroy(t_g1[k]);
    }
    (void)hipFree(full);
    G.destroy(g);
    for (rt_ctx* c : ctx) rt_destroy(c);
    rt_scene_destroy(scene);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) {
        std::fprintf(stderr, "[ERREUR]: Aucune fichier de scene ne fut passe en argument !\n");
        return 1;
    }
    int W = 512, H = 256, depth = 0, dev0 = 0, frames = 1, gpus = 1, threads = 0, ssaa = 1;
    bool stats = false, bands = false, cpu = false, dev_given = false, g_given = false;
    int gather = -1;  // -1 auto (RCCL for -g > 1 on distinct GPUs), 0 host, 1 RCCL
    const char* out = nullptr;
    const char* aov = nullptr;
    const char* rays_in = nullptr;
    const char* hits = nullptr;
    bool ray_bvh = false;
    const char* colours = nullptr;
    const char* segs_in = nullptr;
    const char* filters = nullptr;
    int adaptive = 0, edge = RT_EDGE_ID | RT_EDGE_NORMAL | RT_EDGE_COLOUR;
    bool adaptive_given = false;
    float edge_cos = 0.9f, edge_delta = 0.1f;
    const char* mask_out = nullptr;
    for (int i = 2; i < argc; ++i) {
        if (argv[i][0] != '-') continue;
        auto next = [&](int& v) {
            if (i + 1 < argc) v = std::atoi(argv[++i]);
        };
        if (std::strcmp(argv[i], "--device") == 0) {
            next(dev0);
            dev_given = true;
            continue;
        }
        if (std::strcmp(argv[i], "--bands") == 0) {
            bands = true;
            continue;
        }
        if (std::strcmp(argv[i], "--ssaa") == 0) {
            ssaa = 0;
            next(ssaa);
            continue;
        }
        if (std::strcmp(argv[i], "--adaptive") == 0) {
            adaptive_given = true;
            next(adaptive);
            continue;
        }
        if (std::strcmp(argv[i], "--edge") == 0) {
            std::string list = i + 1 < argc ? argv[++i] : "";
            edge = 0;
            for (size_t a = 0; a <= list.size();) {
                const size_t b = std::min(list.find(',', a), list.size());
                const std::string w = list.substr(a, b - a);
                if (w == "id")
                    edge |= RT_EDGE_ID;
                else if (w == "normal")
                    edge |= RT_EDGE_NORMAL;
                else if (w == "colour")
                    edge |= RT_EDGE_COLOUR;
                else
                    return fail("arguments", RT_E_ARG, "--edge is a comma-separated list of id, normal, colour");
                a = b + 1;
            }
            continue;
        }
        if (std::strcmp(argv[i], "--edge-cos") == 0 || std::strcmp(argv[i], "--edge-delta") == 0) {
            if (i + 1 >= argc) return fail("arguments", RT_E_ARG, "--edge-cos / --edge-delta need a number");
            (argv[i][7] == 'c' ? edge_cos : edge_delta) = (float)std::atof(argv[i + 1]);
            ++i;
            continue;
        }
        if (std::strcmp(argv[i], "--mask") == 0) {
            if (i + 1 >= argc) return fail("arguments", RT_E_ARG, "--mask needs a .npy file to write");
            mask_out = argv[++i];
            continue;
        }
        if (std::strcmp(argv[i], "--aov") == 0) {
            if (i + 1 >= argc) return fail("arguments", RT_E_ARG, "--aov needs a file prefix");
            aov = argv[++i];
            continue;
        }
        if (std::strcmp(argv[i], "--rays") == 0) {
            if (i + 1 >= argc) return fail("arguments", RT_E_ARG, "--rays needs a .npy file");
            rays_in = argv[++i];
            continue;
        }
        if (std::strcmp(argv[i], "--hits") == 0) {
            if (i + 1 >= argc) return fail("arguments", RT_E_ARG, "--hits needs a file prefix");
            hits = argv[++i];
            continue;
        }
        if (std::strcmp(argv[i], "--colours") == 0) {
            if (i + 1 >= argc) return fail("arguments", RT_E_ARG, "--colours needs a .npy file to write");
            colours = argv[++i];
            continue;
        }
        if (std::strcmp(argv[i], "--segments") == 0) {
            if (i + 1 >= argc) return fail("arguments", RT_E_ARG, "--segments needs a .npy file");
            segs_in = argv[++i];
            continue;
        }
        if (std::strcmp(argv[i], "--filters") == 0) {
            if (i + 1 >= argc) return fail("arguments", RT_E_ARG, "--filters needs a .npy file to write");
            filters = argv[++i];
            continue;
        }
        if (std::strcmp(argv[i], "--ray-bvh") == 0) {
            ray_bvh = true;
            continue;
        }
        if (std::strcmp(argv[i], "--threads") == 0) {
            next(threads);
            continue;
        }
        if (std::strcmp(argv[i], "--gather") == 0) {
            const char* b = i + 1 < argc ? argv[++i] : "";
            if (std::strcmp(b, "rccl") == 0)
                gather = 1;
            else if (std::strcmp(b, "host") == 0)
                gather = 0;
            else
                return fail("arguments", RT_E_ARG, "--gather is rccl or host");
            continue;
        }
        if (std::strcmp(argv[i], "--backend") == 0) {
            const char* b = i + 1 < argc ? argv[++i] : "";
            if (std::strcmp(b, "cpu") == 0)
                cpu = true;
            else if (std::strcmp(b, "hip") != 0)
                return fail("arguments", RT_E_ARG, "--backend is hip or cpu");
            continue;
        }
        switch (argv[i][1]) {
        case 'x': next(W); break;
        case 'y': next(H); break;
        case 'd': next(depth); break;
        case 'g':
            next(gpus);
            g_given = true;
            break;
        case 'n': next(frames); break;
        case 's': stats = true; break;
        case 'o':
            if (i + 1 < argc) out = argv[++i];
            break;
        }
    }
    if (W <= 0 || H <= 0 || gpus <= 0 || frames <= 0) return fail("arguments", RT_E_ARG, "-x/-y/-g/-n must be > 0");
    // -g was the HIP device index before ABI 3; it is now the GPU count
    if (g_given && !dev_given)
        std::fprintf(stderr, "[NOTE]: -g %d = number of GPUs (from device 0); the device index is --device\n", gpus);
    if (ssaa < 1 || ssaa > 8) return fail("arguments", RT_E_ARG, "--ssaa is 1..8");
    if (ssaa > 1 && (gpus != 1 || bands || gather == 1))
        return fail("arguments", RT_E_ARG,
                    "--ssaa renders on one GPU: it cannot be combined with -g above 1, --bands or --gather rccl");
    if (adaptive_given && adaptive != 2 && adaptive != 4 && adaptive != 8)
        return fail("arguments", RT_E_ARG, "--adaptive is 2, 4 or 8");
    if (adaptive_given && (ssaa > 1 || aov || rays_in || segs_in || gpus != 1 || bands || gather == 1))
        return fail("arguments", RT_E_ARG,
                    "--adaptive renders on one GPU: it cannot be combined with --ssaa, --aov, --rays, --segments, -g "
                    "above 1, --bands or --gather rccl");
    if (mask_out && !adaptive_given) return fail("arguments", RT_E_ARG, "--mask goes with --adaptive");
    if (aov && (gpus != 1 || bands || gather == 1))
        return fail("arguments", RT_E_ARG,
                    "--aov renders on one GPU: it cannot be combined with -g above 1, --bands or --gather rccl");
    if ((rays_in != nullptr) != (hits != nullptr || colours != nullptr))
        return fail("arguments", RT_E_ARG, "--rays IN.npy goes with --hits PREFIX, --colours OUT.npy or both");
    if (rays_in && (gpus != 1 || bands || gather == 1))
        return fail("arguments", RT_E_ARG,
                    "--rays traces on one GPU: it cannot be combined with -g above 1, --bands or --gather rccl");
    if ((segs_in != nullptr) != (filters != nullptr))
        return fail("arguments", RT_E_ARG, "--segments IN.npy and --filters OUT.npy go together");
    if (segs_in && (gpus != 1 || bands || gather == 1))
        return fail("arguments", RT_E_ARG,
                    "--segments filters on one GPU: it cannot be combined with -g above 1, --bands or --gather rccl");
    if (ray_bvh && !rays_in && !segs_in) return fail("arguments", RT_E_ARG, "--ray-bvh goes with --rays or --segments");
    std::vector<float> rays;
    if (rays_in) {
        std::string why;
        if (!read_rays_npy(rays_in, rays, why)) return fail("--rays", RT_E_ARG, (std::string(rays_in) + ": " + why).c_str());
    }
    std::vector<float> segs;
    if (segs_in) {
        std::string why;
        if (!read_rays_npy(segs_in, segs, why))
            return fail("--segments", RT_E_ARG, (std::string(segs_in) + ": " + why).c_str());
    }
    if (((W - 1) & W) || ((H - 1) & H))
        std::fprintf(stderr, "[ATTENTION]: Resolution %dx%d n'est pas une puissance de deux "
                             "(accepted: the render core has no such restriction)\n", W, H);

    rt_scene* scene = nullptr;
    int rc = rt_scene_create(&scene);
    if (rc) return fail("rt_scene_create", rc, "");
    const int grid = adaptive_given ? adaptive : ssaa;
    rt_scene_set_resolution(scene, W * grid, H * grid);  // (--ssaa, --adaptive: the sample grid)
    rt_scene_set_max_bounces(scene, depth);
    std::printf("[ETAT]: Traitement du fichier de donnees de la scene...\n");
    if ((rc = rt_scene_load_file(scene, argv[1]))) return fail("TraiterFichierDeScene", rc, rt_scene_error(scene));
    if ((rc = rt_scene_prepare(scene))) return fail("Initialiser", rc, rt_scene_error(scene));
    rt_scene_flat flat;
    rt_scene_get_flat(scene, &flat);
    rt_frame frame;
    rt_scene_get_frame(scene, &frame);
    if (stats) frame.flags |= RT_FLAG_STATS;

    if (adaptive_given) {  // one context of either backend, the sample frame refined where its pixels disagree
        if (little_endian("--adaptive")) return 1;
        rt_ctx* c = nullptr;
        if (cpu) {
            if ((rc = rt_create_cpu(threads, &c))) return fail("rt_create_cpu", rc, "");
        } else {
            int nd = 0;
            if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) return fail("rt_create", RT_E_HIP, "no HIP device");
            if ((rc = rt_create(dev0 % nd, &c))) return fail("rt_create", rc, c ? rt_last_error(c) : "");
        }
        if ((rc = rt_upload_scene(c, &flat))) return fail("rt_upload_scene", rc, rt_last_error(c));
        frame.flags &= ~RT_FLAG_STATS;  // (not accepted by the adaptive render: its rt_stats carry the ray count)
        std::vector<uint8_t> img((size_t)W * H * 4), mask((size_t)W * H);
        const rt_adaptive how{adaptive, edge, edge_cos, edge_delta};
        const rt_adaptive_out to{img.data(), nullptr, mask.data()};
        std::printf("[ETAT]: Lancer de rayons (adaptatif, %d x %d echantillons par pixel de contour)...\n", adaptive,
                    adaptive);
        double total = 0.0;
        for (int k = 0; k < frames; ++k) {
            const auto t0 = std::chrono::steady_clock::now();
            if ((rc = cpu ? rt_cpu_render_adaptive(c, &frame, &how, &to) : rt_render_adaptive(c, &frame, &how, &to)))
                return fail("LancerRayons", rc, rt_last_error(c));
            total += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }
        size_t flagged = 0;
        for (uint8_t m : mask) flagged += m != 0;
        std::printf("[ETAT]: %zu pixels de contour sur %zu (%.1f %%)\n", flagged, mask.size(),
                    100.0 * (double)flagged / (double)mask.size());
        print_done(c, total, frames, 1, 0, stats);
        if (out && write_ppm(out, W, H, img)) return fail("fopen", -1, out);
        if (mask_out && write_npy(mask_out, "|u1", H, W, 1, mask.data(), mask.size())) return fail("fopen", -1, mask_out);
        rt_destroy(c);
        rt_scene_destroy(scene);
        return 0;
    }
    if (rays_in || segs_in) {  // ray / filter queries: one context of either backend; the frame only for -o
        rt_ctx* c = nullptr;
        if (cpu) {
            if ((rc = rt_create_cpu(threads, &c))) return fail("rt_create_cpu", rc, "");
        } else {
            int nd = 0;
            if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) return fail("rt_create", RT_E_HIP, "no HIP device");
            if ((rc = rt_create(dev0 % nd, &c))) return fail("rt_create", rc, c ? rt_last_error(c) : "");
        }
        if (ray_bvh && (rc = rt_set_option(c, RT_OPT_RAY_BVH, 1.0))) return fail("rt_set_option", rc, rt_last_error(c));
        if ((rc = rt_upload_scene(c, &flat))) return fail("rt_upload_scene", rc, rt_last_error(c));
        if (rays_in) {
            std::printf("[ETAT]: Lancer de rayons (%zu rayons de %s)...\n", rays.size() / 6, rays_in);
            if (hits && write_hits(c, cpu, rays, hits)) return 1;
            if (colours && write_n3(c, cpu, &frame, rays, colours)) return 1;
        }
        if (segs_in) {
            std::printf("[ETAT]: Filtres d'ombre (%zu segments de %s)...\n", segs.size() / 6, segs_in);
            if (write_n3(c, cpu, nullptr, segs, filters)) return 1;
        }
        if (out) {
            std::vector<uint8_t> img((size_t)W * H * 4);
            rc = cpu ? (ssaa > 1 ? rt_cpu_render_ss(c, &frame, ssaa, img.data()) : rt_cpu_render(c, &frame, img.data()))
                     : (ssaa > 1 ? rt_render_ss(c, &frame, ssaa, img.data()) : rt_render(c, &frame, img.data()));
            if (rc) return fail("LancerRayons", rc, rt_last_error(c));
            if (write_ppm(out, W, H, img)) return fail("fopen", -1, out);
        }
        if (aov && write_aov(c, cpu, frame, aov)) return 1;
        rt_destroy(c);
        rt_scene_destroy(scene);
        return 0;
    }
    if (cpu) {  // the CPU backend: one context, host threads
        if (gpus != 1 || bands) return fail("arguments", RT_E_ARG, "-g / --bands are for the hip backend");
        rt_ctx* c = nullptr;
        if ((rc = rt_create_cpu(threads, &c))) return fail("rt_create_cpu", rc, "");
        if ((rc = rt_upload_scene(c, &flat))) return fail("rt_upload_scene", rc, rt_last_error(c));
        std::vector<uint8_t> img((size_t)W * H * 4);
        std::printf("[ETAT]: Lancer de rayons (CPU)...\n");
        double total = 0.0;
        for (int k = 0; k < frames; ++k) {
            const auto t0 = std::chrono::steady_clock::now();
            if ((rc = ssaa > 1 ? rt_cpu_render_ss(c, &frame, ssaa, img.data()) : rt_cpu_render(c, &frame, img.data())))
                return fail("LancerRayons", rc, rt_last_error(c));
            total += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }
        std::printf("[ETAT]: Termine! --> Temps total de rendu : %.6f secondes (%d frame(s), CPU)\n", total, frames);
        if (out && write_ppm(out, W, H, img)) return fail("fopen", -1, out);
        if (aov && write_aov(c, true, frame, aov)) return 1;
        rt_destroy(c);
        rt_scene_destroy(scene);
        return 0;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail("rt_create", RT_E_HIP, "no HIP device");
    // one context per GPU share; part r = rows of slab r, or band set r
    const int band = bands ? 16 : 0;
    if (ssaa > 1) {  // one context, the sample frame resolved on the device
        rt_ctx* c = nullptr;
        if ((rc = rt_create(dev0 % ndev, &c))) return fail("rt_create", rc, c ? rt_last_error(c) : "");
        if ((rc = rt_upload_scene(c, &flat))) return fail("rt_upload_scene", rc, rt_last_error(c));
        std::vector<uint8_t> img((size_t)W * H * 4);
        std::printf("[ETAT]: Lancer de rayons (%d x %d echantillons par pixel)...\n", ssaa, ssaa);
        double total = 0.0;
        for (int k = 0; k < frames; ++k) {
            const auto t0 = std::chrono::steady_clock::now();
            if ((rc = rt_render_ss(c, &frame, ssaa, img.data()))) return fail("LancerRayons", rc, rt_last_error(c));
            total += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }
        print_done(c, total, frames, 1, 0, stats);
        if (out && write_ppm(out, W, H, img)) return fail("fopen", -1, out);
        if (aov && write_aov(c, false, frame, aov)) return 1;
        rt_destroy(c);
        rt_scene_destroy(scene);
        return 0;
    }
    std::vector<rt_ctx*> ctx((size_t)gpus, nullptr);
    std::vector<rt_frame> part((size_t)gpus, frame);
    std::vector<std::vector<uint8_t>> img((size_t)gpus);
    const int slab = (H + gpus - 1) / gpus;
    for (int r = 0; r < gpus; ++r) {
        if ((rc = rt_create((dev0 + r) % ndev, &ctx[r]))) return fail("rt_create", rc, ctx[r] ? rt_last_error(ctx[r]) : "");
        if ((rc = rt_upload_scene(ctx[r], &flat))) return fail("rt_upload_scene", rc, rt_last_error(ctx[r]));
        rt_frame& f = part[r];
        int rows;
        if (band) {
            f.band_rows = band;
            f.band_count = gpus;
            f.band_index = r;
            rows = rt_band_rows(H, band, gpus, r);
        } else {
            f.row_begin = std::min(H, r * slab);
            f.row_end = std::min(H, (r + 1) * slab);
            rows = f.row_end - f.row_begin;
        }
        img[r].resize((size_t)std::max(rows, 0) * W * 4);
    }
    const bool distinct = gpus <= ndev;
    if (gather == 1 && !distinct)
        return fail("arguments", RT_E_ARG, "--gather rccl needs one GPU per context (-g <= the GPU count)");
    if (gather == 1 || (gather == -1 && gpus > 1 && distinct))
        return render_rccl(ctx, part, img, W, H, band, dev0, ndev, frames, stats, out, scene);
    if (gpus > 1)
        std::printf("[ETAT]: gather: host (%d contexts on %d GPU(s)%s)\n", gpus, ndev,
                    distinct ? ", --gather host" : "; RCCL needs one rank per GPU");
    std::printf("[ETAT]: Lancer de rayons...\n");
    double total = 0.0;
    std::vector<int> rcs((size_t)gpus, 0);
    for (int k = 0; k < frames; ++k) {
        const auto t0 = std::chrono::steady_clock::now();
        if (gpus == 1) {
            rcs[0] = rt_render(ctx[0], &part[0], img[0].data());
        } else {
            std::vector<std::thread> th;
            for (int r = 0; r < gpus; ++r)
                th.emplace_back([&, r] { rcs[r] = img[r].empty() ? 0 : rt_render(ctx[r], &part[r], img[r].data()); });
            for (auto& t : th) t.join();
        }
        const auto t1 = std::chrono::steady_clock::now();
        for (int r = 0; r < gpus; ++r)
            if (rcs[r]) return fail("LancerRayons", rcs[r], rt_last_error(ctx[r]));
        total += std::chrono::duration<double>(t1 - t0).count();
    }
    // the frame, bottom row first (memory row 0 = bottom scanline)
    std::vector<uint8_t> full((size_t)W * H * 4);
    for (int r = 0; r < gpus; ++r) {
        const size_t rowb = (size_t)W * 4;
        if (band) {
            const int q = (int)(img[r].size() / rowb) / band;
            for (int j = 0; j < q; ++j) {
                const int y0 = (j * gpus + r) * band;
                const int n = std::min(band, H - y0);
                if (n > 0) std::memcpy(&full[(size_t)y0 * rowb], &img[r][(size_t)j * band * rowb], (size_t)n * rowb);
            }
        } else if (!img[r].empty()) {
            std::memcpy(&full[(size_t)part[r].row_begin * rowb], img[r].data(), img[r].size());
        }
    }
    print_done(ctx[0], total, frames, gpus, band, stats);
    if (out && write_ppm(out, W, H, full)) return fail("fopen", -1, out);
    if (aov && write_aov(ctx[0], false, frame, aov)) return 1;
    for (rt_ctx* c : ctx) rt_destroy(c);
    rt_scene_destroy(scene);
    return 0;
}
