// cbet_trace_diag.h -- the diagnostic builds of cbet_trace_window.hip (never shipped) behind ONE hook: the kernel calls
// WaveDiag's methods at fixed places, and every method is empty unless the file is compiled with one of
//   -DCBET_DIAG_CLOCKS  shader-clock cycles a wave spends in the record wait, in the window arm, in the write-backs of
//                       follow_box and in all of its life (scripts/diag_clocks.py)
//   -DCBET_DIAG_FACES   wave-steps that start near a face, the near axes summed over them, wave-steps that enter the window
//                       arm (scripts/face_share.py)
//   -DCBET_DIAG_CHAIN   shader-clock cycles of the dependent chain, from right behind the record wait to right behind the
//                       issue of the next gather, so that whatever the compiler puts in front of the gather is inside
//                       (scripts/diag_chain.py)
// A diagnostic build reports through the kernel's counter slots in place of what they usually hold (report).  The stamps
// and their waits cost time themselves: compare builds that carry the same stamps with each other only.
#ifndef CBET_TRACE_DIAG_H_
#define CBET_TRACE_DIAG_H_

#include "cbet_trace_common.h"

namespace cbet {

#ifdef CBET_DIAG_CLOCKS
#define CBET_IF_CLOCKS(...) __VA_ARGS__
#else
#define CBET_IF_CLOCKS(...)
#endif
#ifdef CBET_DIAG_FACES
#define CBET_IF_FACES(...) __VA_ARGS__
#else
#define CBET_IF_FACES(...)
#endif
#ifdef CBET_DIAG_CHAIN
#define CBET_IF_CHAIN(...) __VA_ARGS__
#else
#define CBET_IF_CHAIN(...)
#endif

struct WaveDiag {   // (an empty struct unless a flag is set; its state is wave-uniform)
    typedef unsigned long long u64;
    // a diagnostic build counts wave-steps as the kernel's STATS instantiations do
    static constexpr bool kCountsWaveSteps = (0 CBET_IF_CLOCKS(+1) CBET_IF_FACES(+1) CBET_IF_CHAIN(+1)) != 0;
    CBET_IF_CLOCKS(u64 wait = 0, arm = 0, n_arm = 0, ret = 0, n_ret = 0, t_start, t_wait, t_arm, t_ret;)
    CBET_IF_FACES(unsigned near_steps = 0, near_axes = 0, arm_steps = 0;)
    CBET_IF_CHAIN(u64 chain = 0, t_chain = 0;)

    static __device__ __forceinline__ void stamp(u64 &t) { asm volatile("s_memtime %0" : "=&s"(t) : : "memory"); }
    // ... and waited for
    static __device__ __forceinline__ void stamp_wait(u64 &t) { asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(t) : : "memory"); }
    // cycles since the stamp t0 (which the new stamp is ordered behind)
    static __device__ __forceinline__ u64 since(u64 t0)
    {
        u64 t1;
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(t1) : "s"(t0) : "memory");
        return t1 - t0;
    }

    // the wave starts (its LDS tiles are zero)
    __device__ __forceinline__ void begin() { CBET_IF_CLOCKS(stamp_wait(t_start);) }
    // top of a step; near = the kernel's near-face bits
    __device__ __forceinline__ void step_begin(int near)
    {
        (void)near;
        CBET_IF_FACES(near_steps += near != 0 ? 1 : 0; near_axes += __builtin_popcount((unsigned)near);)
    }
    // around the record wait; the chain starts right behind it ...
    __device__ __forceinline__ void wait_begin() { CBET_IF_CLOCKS(stamp(t_wait);) }
    __device__ __forceinline__ void wait_end()
    {
        CBET_IF_CLOCKS(wait += since(t_wait);)
        CBET_IF_CHAIN(stamp_wait(t_chain);)
    }
    // ... and ends right behind the issue of the step's gather
    __device__ __forceinline__ void chain_end() { CBET_IF_CHAIN(chain += since(t_chain);) }
    // around the window arm of a step
    __device__ __forceinline__ void arm_begin()
    {
        CBET_IF_FACES(arm_steps += 1;)
        CBET_IF_CLOCKS(stamp(t_arm);)
    }
    __device__ __forceinline__ void arm_end() { CBET_IF_CLOCKS(arm += since(t_arm); n_arm += 1;) }
    // around the write-backs of one axis in follow_box
    __device__ __forceinline__ void retire_begin() { CBET_IF_CLOCKS(stamp(t_ret);) }
    __device__ __forceinline__ void retire_end() { CBET_IF_CLOCKS(ret += since(t_ret); n_ret += 1;) }
    // The end of the wave: true when a diagnostic build has written the counter slots (the kernel then writes none).  Every
    // build keeps ray-steps and wave-steps in their slots; of the others
    //   clocks: global atomics = record-wait cycles, evictions = window-arm cycles, wave-steps wide = window-arm entries, slabs
    //           retired = the wave's cycles, rays = the write-backs' cycles, wave-steps miss = their number
    //   chain:  global atomics = the chain's cycles
    //   faces:  wave-steps wide = near steps, wave-steps miss = near axes, slabs retired = window-arm entries
    __device__ __forceinline__ bool report(const TraceArgs &a, int lane, int tot_steps, int tot_rays, unsigned wave_steps)
    {
        auto put = [&](int slot, u64 v) { atomicAdd(&a.counters[slot], v); };
        if (kCountsWaveSteps && lane == 0) {
            CBET_IF_CLOCKS(u64 t_end; stamp_wait(t_end);)
            put(kCntSteps, (u64)tot_steps);
            put(kCntWaveSteps, (u64)wave_steps);
#if defined(CBET_DIAG_CLOCKS)
            put(kCntGlobalAtomics, wait);
            put(kCntEvictions, arm);
            put(kCntWaveStepsWide, n_arm);
            put(kCntSlabsRetired, t_end - t_start);
            put(kCntRays, ret);
            put(kCntWaveStepsMiss, n_ret);
#elif defined(CBET_DIAG_CHAIN)
            put(kCntRays, (u64)tot_rays);
            put(kCntGlobalAtomics, chain);
#elif defined(CBET_DIAG_FACES)
            put(kCntRays, (u64)tot_rays);
            put(kCntWaveStepsWide, (u64)near_steps);
            put(kCntWaveStepsMiss, (u64)near_axes);
            put(kCntSlabsRetired, (u64)arm_steps);
#endif
        }
        (void)tot_rays;
        return kCountsWaveSteps;
    }
};
#undef CBET_IF_CLOCKS
#undef CBET_IF_FACES
#undef CBET_IF_CHAIN

}  // namespace cbet

#endif  // CBET_TRACE_DIAG_H_
