// Scalar-ALU issue rate of a CU on gfx950 (diagnostic): how many cycles a
// compute unit needs per scalar ALU instruction when 1, 2, 4 or 8 waves per
// SIMD run chains of independent s_add_u32 / s_and_b32, with one SIMD or all
// four SIMDs of the CU occupied, with not-taken and taken s_cbranch mixed in,
// and with waves of independent VALU work beside them (do the two pipes
// issue in the same cycles?).
//
// Layout: workgroups of 256 threads (four waves; the dispatcher spreads them
// over the CU's four SIMDs, which every wave checks by reading its SIMD id),
// and a dynamic LDS size that lets exactly w workgroups share a CU, so a
// SIMD holds w waves.  A wave's role comes from its SIMD id and the parity
// of its wave slot in that SIMD (HW_ID's wave id: at 8 waves per SIMD every
// SIMD holds four of each): idle (waits at the block's barrier, issues
// nothing), scalar loop, or vector loop.  The grid is one round (256 CUs x w
// blocks), so all waves run side by side; a wave times its loop with
// s_memtime and lane 0 stores the figure with a vector store.
//
// Scalar ALU and vector stores only.  The scalar loops' asm declares SCC
// clobbered: the compiler's own loop compare must stand behind the body.
//
//   hipcc -O3 --offload-arch=gfx950 -o tools/calib/salu_issue tools/calib/salu_issue.hip
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

constexpr int kBody = 256;  // instructions of the measured kind per loop pass
constexpr int kCUs = 256;  // MI355X; main() checks the device's count

#define S8(op0, op1)                \
    op0 " %0, %0, 1\n" op1 " %1, %1, -1\n" op0 " %2, %2, 1\n" op1 " %3, %3, -1\n" \
    op0 " %4, %4, 1\n" op1 " %5, %5, -1\n" op0 " %6, %6, 1\n" op0 " %7, %7, 1\n"
// eight scalar ALU instructions on eight registers; the last one is an
// s_add_u32 without carry, so SCC = 0 behind it
#define SALU8 S8("s_add_u32", "s_and_b32")
// ... then a branch on SCC that is not taken / taken (to the next instruction)
#define SALU8_NT SALU8 "s_cbranch_scc1 1f\n1:\n"
#define SALU8_T SALU8 "s_cbranch_scc0 1f\n1:\n"
#define R4(x) x x x x
#define R32(x) R4(x) R4(x) R4(x) R4(x) R4(x) R4(x) R4(x) R4(x)
#define SREGS "+s"(a[0]), "+s"(a[1]), "+s"(a[2]), "+s"(a[3]), "+s"(a[4]), "+s"(a[5]), "+s"(a[6]), "+s"(a[7])
#define VALU8                                                                                              \
    "v_add_f32 %0, 1.0, %0\nv_mul_f32 %1, 1.0, %1\nv_add_f32 %2, 1.0, %2\nv_mul_f32 %3, 1.0, %3\n"         \
    "v_add_f32 %4, 1.0, %4\nv_mul_f32 %5, 1.0, %5\nv_add_f32 %6, 1.0, %6\nv_mul_f32 %7, 1.0, %7\n"
#define VREGS "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7])

enum Role { kIdle = 0, kSalu = 1, kSaluNT = 2, kSaluT = 3, kValu = 4 };

struct WaveOut {
    unsigned long long ticks;
    unsigned role, where;  // where: xcc << 16 | the HW_ID bits of SE, SH, CU, SIMD
};

// roles: one nibble per SIMD id, low 16 bits for even wave slots, high for odd
__global__ __launch_bounds__(256) void issue(unsigned roles, int iters, unsigned seed, WaveOut* __restrict__ out)
{
    extern __shared__ unsigned lds[];
    const unsigned hw = __builtin_amdgcn_s_getreg((15 << 11) | (0 << 6) | 4);   // HW_REG_HW_ID[15:0]
    const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20);  // HW_REG_XCC_ID[3:0]
    const unsigned simd = (hw >> 4) & 3u;
    const unsigned role = (roles >> (16 * (hw & 1u) + 4 * simd)) & 15u;
    unsigned a[8];
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        a[k] = __builtin_amdgcn_readfirstlane(seed + k);
        v[k] = (float)(threadIdx.x + k);
    }
    unsigned long long t0 = 0, t1 = 0;
    if (role == kSalu) {
        t0 = __builtin_amdgcn_s_memtime();
        for (int i = 0; i < iters; ++i) asm volatile(R32(SALU8) : SREGS : : "scc");
        t1 = __builtin_amdgcn_s_memtime();
    } else if (role == kSaluNT) {
        t0 = __builtin_amdgcn_s_memtime();
        for (int i = 0; i < iters; ++i) asm volatile(R32(SALU8_NT) : SREGS : : "scc");
        t1 = __builtin_amdgcn_s_memtime();
    } else if (role == kSaluT) {
        t0 = __builtin_amdgcn_s_memtime();
        for (int i = 0; i < iters; ++i) asm volatile(R32(SALU8_T) : SREGS : : "scc");
        t1 = __builtin_amdgcn_s_memtime();
    } else if (role == kValu) {
        t0 = __builtin_amdgcn_s_memtime();
        for (int i = 0; i < iters; ++i) asm volatile(R32(VALU8) : VREGS);
        t1 = __builtin_amdgcn_s_memtime();
    }
    __syncthreads();  // idle waves wait here for the block's working waves
    if ((threadIdx.x & 63u) == 0) {
        unsigned keep = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) keep ^= a[k] ^ __float_as_uint(v[k]);
        if (keep == 0x12345u) lds[0] = keep;  // (keeps the chains' results alive)
        WaveOut o;
        o.ticks = t1 - t0;
        o.role = role;
        o.where = (xcc << 16) | (hw & 0xFFF0u);
        out[blockIdx.x * 4 + (threadIdx.x >> 6)] = o;
    }
}

// the clock of s_memtime against the event time of the same launch
__global__ __launch_bounds__(64) void clock_rate(int spin, unsigned long long* __restrict__ out)
{
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    unsigned long long t1 = t0;
    for (int i = 0; i < spin; ++i) t1 = __builtin_amdgcn_s_memtime();
    if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = t1 - t0;
}

#define CK(x)                                                   \
    do {                                                        \
        const hipError_t e_ = (x);                              \
        if (e_ != hipSuccess) {                                 \
            std::printf("%s: %s\n", #x, hipGetErrorString(e_)); \
            return 1;                                           \
        }                                                       \
    } while (0)

static unsigned roles_of(const int even[4], const int odd[4])
{
    unsigned r = 0;
    for (int s = 0; s < 4; ++s) r |= (unsigned)even[s] << (4 * s) | (unsigned)odd[s] << (16 + 4 * s);
    return r;
}

// One experiment: w workgroups per CU, the role table, `iters` loop passes.
static int run(const char* name, int w, unsigned roles, int iters, WaveOut* dout)
{
    // LDS per block so that w blocks fit a CU's 160 KiB and w + 1 do not
    static const int lds_kib[9] = {0, 96, 64, 0, 36, 0, 0, 0, 18};
    const size_t lds = (size_t)lds_kib[w] * 1024;
    CK(hipFuncSetAttribute((const void*)issue, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int blocks = kCUs * w;
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    hipLaunchKernelGGL(issue, dim3(blocks), dim3(256), lds, 0, roles, 64, 1u, dout);  // warm
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(issue, dim3(blocks), dim3(256), lds, 0, roles, iters, 1u, dout);
    CK(hipEventRecord(e1, 0));
    CK(hipDeviceSynchronize());
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, e0, e1));
    CK(hipEventDestroy(e0));
    CK(hipEventDestroy(e1));
    std::vector<WaveOut> h((size_t)blocks * 4);
    CK(hipMemcpy(h.data(), dout, h.size() * sizeof(WaveOut), hipMemcpyDeviceToHost));
    std::set<unsigned> cus;
    double sum[2] = {0, 0}, mx[2] = {0, 0};
    long n[2] = {0, 0}, simd_n[4] = {0, 0, 0, 0};
    for (const WaveOut& o : h) {
        if (o.role == kIdle) continue;
        const int c = o.role == kValu;
        sum[c] += (double)o.ticks;
        mx[c] = std::max(mx[c], (double)o.ticks);
        ++n[c];
        ++simd_n[(o.where >> 4) & 3u];
        cus.insert(o.where & ~0xFFu);  // XCC, SE, SH, CU
    }
    const double per_wave = (double)kBody * iters;
    std::printf("%-34s w=%d  CUs %3zu  SIMD waves %ld/%ld/%ld/%ld  launch %7.1f us", name, w, cus.size(), simd_n[0],
                simd_n[1], simd_n[2], simd_n[3], ms * 1e3);
    for (int c = 0; c < 2; ++c) {
        if (!n[c]) continue;
        const double mean = sum[c] / n[c];
        const double per_cu = per_wave * n[c] / (double)cus.size();  // instructions of this kind per CU
        std::printf("  | %s: %ld waves, %.3f ticks/inst/wave (max %.3f), %.4f ticks/inst/CU = %.3f inst/tick/CU",
                    c ? "VALU" : "SALU", n[c], mean / per_wave, mx[c] / per_wave, mean / per_cu, per_cu / mean);
    }
    std::printf("\n");
    return 0;
}

int main()
{
    std::setvbuf(stdout, nullptr, _IOLBF, 0);  // a line at a time, also into a pipe
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    if (prop.multiProcessorCount != kCUs) {
        std::printf("this device has %d CUs, the grids are sized for %d\n", prop.multiProcessorCount, kCUs);
        return 1;
    }
    unsigned long long* dclk = nullptr;
    CK(hipMalloc(&dclk, 16));
    {
        hipEvent_t e0, e1;
        CK(hipEventCreate(&e0));
        CK(hipEventCreate(&e1));
        hipLaunchKernelGGL(clock_rate, dim3(1), dim3(64), 0, 0, 1000, dclk);
        CK(hipDeviceSynchronize());
        CK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(clock_rate, dim3(1), dim3(64), 0, 0, 2000000, dclk);
        CK(hipEventRecord(e1, 0));
        CK(hipDeviceSynchronize());
        float ms = 0.f;
        CK(hipEventElapsedTime(&ms, e0, e1));
        CK(hipEventDestroy(e0));
        CK(hipEventDestroy(e1));
        unsigned long long t = 0;
        CK(hipMemcpy(&t, dclk, sizeof t, hipMemcpyDeviceToHost));
        const double ticks_per_ns = (double)t / (ms * 1e6);
        std::printf("s_memtime: %.4f ticks/ns (%.0f MHz) over %.2f ms\n", ticks_per_ns, ticks_per_ns * 1e3, ms);
    }
    WaveOut* dout = nullptr;
    CK(hipMalloc(&dout, sizeof(WaveOut) * kCUs * 8 * 4));
    CK(hipMemset(dout, 0, sizeof(WaveOut) * kCUs * 8 * 4));
    const int all_s[4] = {kSalu, kSalu, kSalu, kSalu}, one_s[4] = {kSalu, kIdle, kIdle, kIdle};
    const int all_nt[4] = {kSaluNT, kSaluNT, kSaluNT, kSaluNT}, all_t[4] = {kSaluT, kSaluT, kSaluT, kSaluT};
    const int all_v[4] = {kValu, kValu, kValu, kValu}, idle[4] = {kIdle, kIdle, kIdle, kIdle};
    const int s0_v123[4] = {kSalu, kValu, kValu, kValu};
    const int iters = 2000;  // 512 k instructions per wave
    int rc = 0;
    for (int w : {1, 2, 4, 8}) rc |= run("SALU, four SIMDs", w, roles_of(all_s, all_s), iters, dout);
    for (int w : {1, 2, 4, 8}) rc |= run("SALU, one SIMD", w, roles_of(one_s, one_s), iters, dout);
    for (int w : {1, 8}) rc |= run("SALU + 1/8 branch not taken", w, roles_of(all_nt, all_nt), iters, dout);
    for (int w : {1, 8}) rc |= run("SALU + 1/8 branch taken", w, roles_of(all_t, all_t), iters, dout);
    // the two pipes: each alone in every other wave slot of every SIMD (the
    // other slots idle), then both together, 4 + 4 waves on every SIMD; then
    // scalar waves on SIMD 0 and vector waves on SIMDs 1..3
    rc |= run("VALU alone, four SIMDs", 4, roles_of(all_v, all_v), iters, dout);
    rc |= run("SALU alone (even slots of w=8)", 8, roles_of(all_s, idle), iters, dout);
    rc |= run("VALU alone (odd slots of w=8)", 8, roles_of(idle, all_v), iters, dout);
    rc |= run("SALU even + VALU odd slots", 8, roles_of(all_s, all_v), iters, dout);
    rc |= run("SALU SIMD 0 + VALU SIMDs 1-3", 8, roles_of(s0_v123, s0_v123), iters, dout);
    rc |= run("SALU SIMD 0 + VALU SIMDs 1-3", 2, roles_of(s0_v123, s0_v123), iters, dout);
    (void)hipFree(dout);
    (void)hipFree(dclk);
    return rc;
}
