// Scalar-load round trip on gfx950 (diagnostic): one wave chases a chain of
// dependent wave-uniform loads (idx = p[idx], an s_load_dword behind an
// s_waitcnt each) through a ring of `n` words, and times the chain with the
// shader clock and with HIP events.
//   ring  1 KiB — resident in the CU group's 16 KiB scalar data cache
//   ring 16 MiB, 64-B stride — every load misses the scalar cache (L2 hits)
//   kernarg     — the same chain through a by-value kernel argument (the
//                 kernel-argument segment, as the launch's camera records)
// The clock of s_memtime is calibrated against the event time of the same
// launch, so the figures come out in ns and, at the measured rate, in
// shader cycles.  A second launch runs the chain in every wave of a full
// grid (8 waves per SIMD), the loaded round trip of a busy CU.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

constexpr int kSteps = 4096;

__global__ __launch_bounds__(64) void chase(const unsigned* __restrict__ p, unsigned start, int steps,
                                            unsigned long long* __restrict__ out)
{
    unsigned idx = start;  // kernel argument: wave-uniform
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < steps; ++i) idx = p[idx];
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        out[0] = t1 - t0;
        out[1] = idx;
    }
}

struct Ring {
    unsigned next[256];
};
__global__ __launch_bounds__(64) void chase_kernarg(const Ring r, unsigned start, int steps,
                                                    unsigned long long* __restrict__ out)
{
    unsigned idx = start;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < steps; ++i) idx = r.next[idx & 255u];
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        out[0] = t1 - t0;
        out[1] = idx;
    }
}

// the clock's own cost: the same loop with no load (an s_add per step)
__global__ __launch_bounds__(64) void clock_rate(int spin, unsigned long long* __restrict__ out)
{
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    unsigned long long t1 = t0;
    for (int i = 0; i < spin; ++i) t1 = __builtin_amdgcn_s_memtime();
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        out[0] = t1 - t0;
        out[1] = (unsigned long long)spin;
    }
}

#define CK(x)                                                          \
    do {                                                               \
        const hipError_t e_ = (x);                                     \
        if (e_ != hipSuccess) {                                        \
            std::printf("%s: %s\n", #x, hipGetErrorString(e_));        \
            return 1;                                                  \
        }                                                              \
    } while (0)

template <class F>
static int timed(const char* name, F launch, unsigned long long* dout, double ticks_per_ns)
{
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    launch();  // warm: code object, caches
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(e0, 0));
    launch();
    CK(hipEventRecord(e1, 0));
    CK(hipDeviceSynchronize());
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, e0, e1));
    unsigned long long h[2];
    CK(hipMemcpy(h, dout, sizeof h, hipMemcpyDeviceToHost));
    const double ticks = (double)h[0] / kSteps;
    std::printf("%-28s %8.2f clock ticks/load", name, ticks);
    if (ticks_per_ns > 0) std::printf("  %7.1f ns  %6.0f cycles at 2.4 GHz", ticks / ticks_per_ns, ticks / ticks_per_ns * 2.4);
    std::printf("  (launch %.1f us)\n", ms * 1e3);
    return 0;
}

int main()
{
    unsigned long long* dout = nullptr;
    CK(hipMalloc(&dout, 16));
    // the clock's rate: a long spin against its event time
    double ticks_per_ns = 0;
    {
        hipEvent_t e0, e1;
        CK(hipEventCreate(&e0));
        CK(hipEventCreate(&e1));
        hipLaunchKernelGGL(clock_rate, dim3(1), dim3(64), 0, 0, 1000, dout);
        CK(hipDeviceSynchronize());
        CK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(clock_rate, dim3(1), dim3(64), 0, 0, 2000000, dout);
        CK(hipEventRecord(e1, 0));
        CK(hipDeviceSynchronize());
        float ms = 0.f;
        CK(hipEventElapsedTime(&ms, e0, e1));
        unsigned long long h[2];
        CK(hipMemcpy(h, dout, sizeof h, hipMemcpyDeviceToHost));
        ticks_per_ns = (double)h[0] / (ms * 1e6);
        std::printf("s_memtime: %.4f ticks/ns (%.0f MHz) over %.2f ms\n", ticks_per_ns, ticks_per_ns * 1e3, ms);
    }
    // small ring: 256 words, odd stride (a full cycle)
    std::vector<unsigned> small(256);
    for (unsigned i = 0; i < 256; ++i) small[i] = (i + 37u) & 255u;
    // large ring: 16 MiB, one word per 64-B line, odd line stride
    const unsigned lines = (16u << 20) / 64u;
    std::vector<unsigned> large((size_t)lines * 16, 0u);
    for (unsigned i = 0; i < lines; ++i) large[(size_t)i * 16] = ((i + 4099u) % lines) * 16u;
    unsigned *ds = nullptr, *dl = nullptr;
    CK(hipMalloc(&ds, small.size() * 4));
    CK(hipMalloc(&dl, large.size() * 4));
    CK(hipMemcpy(ds, small.data(), small.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dl, large.data(), large.size() * 4, hipMemcpyHostToDevice));
    Ring r;
    for (unsigned i = 0; i < 256; ++i) r.next[i] = small[i];

    int rc = 0;
    rc |= timed("1 wave, 1 KiB ring (hit)", [&] { hipLaunchKernelGGL(chase, dim3(1), dim3(64), 0, 0, ds, 0u, kSteps, dout); },
                dout, ticks_per_ns);
    rc |= timed("1 wave, 16 MiB ring (miss)", [&] { hipLaunchKernelGGL(chase, dim3(1), dim3(64), 0, 0, dl, 0u, kSteps, dout); },
                dout, ticks_per_ns);
    rc |= timed("1 wave, kernarg ring", [&] { hipLaunchKernelGGL(chase_kernarg, dim3(1), dim3(64), 0, 0, r, 0u, kSteps, dout); },
                dout, ticks_per_ns);
    // a busy chip: 256 CUs x 4 SIMDs x 8 waves, every wave chasing
    rc |= timed("8192 waves, 1 KiB ring", [&] { hipLaunchKernelGGL(chase, dim3(8192), dim3(64), 0, 0, ds, 0u, kSteps, dout); },
                dout, ticks_per_ns);
    rc |= timed("8192 waves, kernarg ring",
                [&] { hipLaunchKernelGGL(chase_kernarg, dim3(8192), dim3(64), 0, 0, r, 0u, kSteps, dout); }, dout,
                ticks_per_ns);
    hipFree(ds);
    hipFree(dl);
    hipFree(dout);
    return rc;
}
