// Micro-benchmark: what a wave-uniform scalar branch costs on gfx950, taken and not taken.
// The loop body is 16 short blocks of four independent v_add_f32; the first K of them (K = 0, 4, 8, 16) end in
// s_cmp + s_cbranch_scc1, which either never leaves the block (falls through into the next one) or always does: forward,
// over PAD bytes of instructions that never run, to the next block -- the shape of the trace kernel's step loop when the
// common side of a branch is the jump.  The vector work is the same in every variant, so
//   (clocks per iteration at K) - (clocks at K = 0), divided by K = the cost of one compare-and-branch,
// and taken minus not taken = the cost of the redirect.  Stamped with s_memtime around the loop (tick = shader clock),
// once with ONE wave on the device and once with 4 waves per SIMD on every CU (HIP events beside the stamps: the
// throughput the CU loses when sixteen waves share its fetch path).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(call) do { if ((call) != hipSuccess) { printf("%s failed\n", #call); exit(1); } } while (0)
#define FILL "v_add_f32 %0, %0, %4\n\tv_add_f32 %1, %1, %4\n\tv_add_f32 %2, %2, %4\n\tv_add_f32 %3, %3, %4\n\t"
// `zero` is a kernel argument that is 0: s_cmp_lg leaves scc = 0 (never taken), s_cmp_eq scc = 1 (always taken)
#define OPERANDS : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "v"(inc), "s"(zero) : "scc"

// MODE 0: no branch; 1: never taken; 2 .. 5: always taken over 1, 2, 4, 8 KB (at 8 KB the sixteen blocks span 128 KB, more than
// the 64 KB instruction cache and than the loop's 16-bit back edge reaches: that row stops at K = 8, a 64 KB body)
template <int MODE>
__device__ __forceinline__ void block(float &a, float &b, float &c, float &d, float inc, int zero)
{
    if constexpr (MODE == 0) asm volatile(FILL "; %5" OPERANDS);
    if constexpr (MODE == 1) asm volatile(FILL "s_cmp_lg_u32 %5, 0\n\ts_cbranch_scc1 .Lbc_%=\n.Lbc_%=:" OPERANDS);
    if constexpr (MODE == 2)
        asm volatile(FILL "s_cmp_eq_u32 %5, 0\n\ts_cbranch_scc1 .Lbc_%=\n\t.rept 256\n\ts_nop 0\n\t.endr\n.Lbc_%=:" OPERANDS);
    if constexpr (MODE == 3)
        asm volatile(FILL "s_cmp_eq_u32 %5, 0\n\ts_cbranch_scc1 .Lbc_%=\n\t.rept 512\n\ts_nop 0\n\t.endr\n.Lbc_%=:" OPERANDS);
    if constexpr (MODE == 4)
        asm volatile(FILL "s_cmp_eq_u32 %5, 0\n\ts_cbranch_scc1 .Lbc_%=\n\t.rept 1024\n\ts_nop 0\n\t.endr\n.Lbc_%=:" OPERANDS);
    if constexpr (MODE == 5)
        asm volatile(FILL "s_cmp_eq_u32 %5, 0\n\ts_cbranch_scc1 .Lbc_%=\n\t.rept 2048\n\ts_nop 0\n\t.endr\n.Lbc_%=:" OPERANDS);
}

constexpr int kBlocks = 16;

template <int K, int MODE>
__global__ void __launch_bounds__(256) k(int iters, int zero, unsigned long long *clocks, float *sink)
{
    float a = threadIdx.x, b = a + 1, c = a + 2, d = a + 3;
    const float inc = 1.0f + zero;
    unsigned long long t0, t1;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(t0) : : "memory");
#pragma nounroll
    for (int it = 0; it < iters; ++it) {
        // the first K blocks branch, the others do not (u < K is resolved at compile time)
#define B(u) if constexpr (u < K) block<MODE>(a, b, c, d, inc, zero); else block<0>(a, b, c, d, inc, zero);
        B(0) B(1) B(2) B(3) B(4) B(5) B(6) B(7) B(8) B(9) B(10) B(11) B(12) B(13) B(14) B(15)
#undef B
    }
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(t1) : "v"(a), "v"(b), "v"(c), "v"(d) : "memory");
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) / 64;
    if ((threadIdx.x & 63) == 0) clocks[wave] = t1 - t0;
    sink[blockIdx.x * blockDim.x + threadIdx.x] = a + b + c + d;
}

struct Result {
    double clocks;   // median over waves, per iteration
    double ms;       // HIP events
};

template <int K, int MODE>
Result run(int blocks, int threads, unsigned long long *clocks, float *sink)
{
    const int iters = 4000, waves = blocks * threads / 64;
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    hipLaunchKernelGGL((k<K, MODE>), dim3(blocks), dim3(threads), 0, 0, 100, 0, clocks, sink);
    CHECK(hipEventRecord(e0));
    hipLaunchKernelGGL((k<K, MODE>), dim3(blocks), dim3(threads), 0, 0, iters, 0, clocks, sink);
    CHECK(hipGetLastError());
    CHECK(hipEventRecord(e1));
    CHECK(hipEventSynchronize(e1));
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    std::vector<unsigned long long> h(waves);
    CHECK(hipMemcpy(h.data(), clocks, sizeof(unsigned long long) * waves, hipMemcpyDeviceToHost));
    std::sort(h.begin(), h.end());
    CHECK(hipEventDestroy(e0));
    CHECK(hipEventDestroy(e1));
    return {(double)h[waves / 2] / iters, ms};
}

template <int MODE>
void table(const char *name, int blocks, int threads, unsigned long long *clocks, float *sink, const Result &base)
{
    const Result r4 = run<4, MODE>(blocks, threads, clocks, sink), r8 = run<8, MODE>(blocks, threads, clocks, sink);
    if constexpr (MODE == 5) {
        printf("  %-22s K=4 %8.1f  K=8 %8.1f clocks/iteration | per branch %6.2f %6.2f clocks | K=8 %.3f ms (%+.1f %%)\n", name, r4.clocks,
               r8.clocks, (r4.clocks - base.clocks) / 4, (r8.clocks - base.clocks) / 8, r8.ms, 100.0 * (r8.ms - base.ms) / base.ms);
    } else {
        const Result r16 = run<16, MODE>(blocks, threads, clocks, sink);
        printf("  %-22s K=4 %8.1f  K=8 %8.1f  K=16 %8.1f clocks/iteration | per branch %6.2f %6.2f %6.2f clocks | K=16 %.3f ms (%+.1f %%)\n",
               name, r4.clocks, r8.clocks, r16.clocks, (r4.clocks - base.clocks) / 4, (r8.clocks - base.clocks) / 8,
               (r16.clocks - base.clocks) / 16, r16.ms, 100.0 * (r16.ms - base.ms) / base.ms);
    }
}

void sweep(const char *what, int blocks, int threads, unsigned long long *clocks, float *sink)
{
    const Result base = run<0, 0>(blocks, threads, clocks, sink);
    printf("%s: %d blocks of vector work, no branch: %.1f clocks/iteration, %.3f ms\n", what, kBlocks, base.clocks, base.ms);
    table<1>("never taken", blocks, threads, clocks, sink, base);
    table<2>("taken, 1 KB forward", blocks, threads, clocks, sink, base);
    table<3>("taken, 2 KB forward", blocks, threads, clocks, sink, base);
    table<4>("taken, 4 KB forward", blocks, threads, clocks, sink, base);
    table<5>("taken, 8 KB forward", blocks, threads, clocks, sink, base);
}

int main()
{
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) { printf("no device\n"); return 1; }
    const int cus = prop.multiProcessorCount, blocks = cus * 4, threads = 256;   // 4 workgroups of 4 waves per CU = 4 waves per SIMD
    unsigned long long *clocks;
    float *sink;
    CHECK(hipMalloc(&clocks, sizeof(unsigned long long) * blocks * threads / 64));
    CHECK(hipMalloc(&sink, sizeof(float) * blocks * threads));
    printf("%s, %d CUs, clock %d MHz; the loop's own latch (s_add, s_cmp, one taken s_cbranch) is in every figure, the base included\n",
           prop.gcnArchName, cus, prop.clockRate / 1000);
    sweep("one wave", 1, 64, clocks, sink);
    sweep("4 waves per SIMD on every CU", blocks, threads, clocks, sink);
    CHECK(hipFree(clocks));
    CHECK(hipFree(sink));
    return 0;
}
