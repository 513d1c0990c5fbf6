// cbet_target.hip -- node tables of a perturbed target (include/cbet_mi355x.h "perturbed targets").
//
// k_tabulate_target<L>: k_tabulate's layout -- one thread per node, z fastest, grid-stride, the 3 x nprofile profile staged
// in LDS -- with the node's radius taken about the target's centre and divided by 1 + delta, delta the target's
// spherical-harmonic distortion in the node's direction (cbet_target_model.h: the statements, shared with the host twin).
//   * the coefficients travel in the kernel argument and the recurrence factors lie in constant memory; every index into
//     them is a compile-time constant of the unrolled (m, l) loops, so they are read by scalar loads into SGPRs, one m's
//     entries at a time (TablePin);
//   * the recurrence runs in registers, m outermost: a thread holds the direction (ct, st, c1, s1), the m-chain (pmm, cr,
//     si), the l-chain (p1, p2), the two sums of the current m and delta -- no per-thread array;
//   * L = 0 is the pure offset (and the monopole): delta is one scalar for the launch and no harmonic is evaluated.
// Built with -ffp-contract=off like the rest of the library: the tables equal the host twin's bit for bit.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "cbet_target_model.h"

namespace cbet {
namespace {

__constant__ double g_target_factors[kTargetFactors];

typedef const __attribute__((address_space(4))) double *ConstDoubles;   // constant address space: read by scalar loads
typedef const __attribute__((address_space(4))) char *ConstBytes;

// From L = 8 on the two tables outgrow the 102 SGPRs.  Left alone, the compiler loads all of them ahead of the node loop
// and parks the values in VGPR lanes (L = 16: 6,400 v_readlane per node against 1,950 fp64 operations).  So the tables'
// addresses pass through an empty asm statement once per m, which also names a value of the m before: the loads of one m
// cannot move ahead of the arithmetic of the last, and no more than one m's entries are live.  The addresses stay in SGPRs.
template <bool PIN>
struct TablePin {
    __device__ __forceinline__ void operator()(ConstDoubles &F, ConstDoubles &c, double after) const
    {
        if (PIN) {
            unsigned long long f = (unsigned long long)F, v = (unsigned long long)c;
            asm volatile("" : "+s"(f), "+s"(v) : "v"(after));
            F = (ConstDoubles)f;
            c = (ConstDoubles)v;
        }
    }
};

template <int L>
__global__ void __launch_bounds__(256) k_tabulate_target(const TargetArgs a)
{
    extern __shared__ double s_prof[];
    const TabulateArgs &t = a.t;
    double *s_r = s_prof, *s_ne = s_prof + t.nprofile, *s_te = s_prof + 2 * t.nprofile;
    for (int i = threadIdx.x; i < t.nprofile; i += blockDim.x) {
        s_r[i] = t.r[i];
        s_ne[i] = t.ne[i];
        s_te[i] = t.te[i];
    }
    __syncthreads();
    const long total = (long)t.nx * t.ny * t.nz;
    const long stride = (long)gridDim.x * blockDim.x;
    // the coefficients where they arrive: `a` is the kernel's only argument, at the start of the kernel-argument segment
    const ConstDoubles coeffs = (ConstDoubles)((ConstBytes)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(TargetArgs, c));
    const ConstDoubles factors = (ConstDoubles)(unsigned long long)g_target_factors;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const int k = (int)(idx % t.nz);
        const long ij = idx / t.nz;
        const int j = (int)(ij % t.ny);
        const int i = (int)(ij / t.ny);
        double ed, kap;
        target_node<L>(a, factors, coeffs, s_r, s_ne, s_te, i, j, k, ed, kap, TablePin<(L > 2)>());
        t.ne3d[idx] = ed;
        t.kap3d[idx] = kap;
    }
}

template <int L>
hipError_t launch(const TargetArgs &a, hipStream_t stream)
{
    const long total = (long)a.t.nx * a.t.ny * a.t.nz;
    long blocks = (total + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;  // k_tabulate's shape: 256 CUs x 16 blocks, grid-stride the rest
    const size_t lds = sizeof(double) * 3 * (size_t)a.t.nprofile;
    hipLaunchKernelGGL(k_tabulate_target<L>, dim3((unsigned)blocks), dim3(256), lds, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t target_upload_factors()
{
    return hipMemcpyToSymbol(HIP_SYMBOL(g_target_factors), target_factors(), sizeof(double) * kTargetFactors);
}

hipError_t launch_tabulate_target(const TargetArgs &a, int inst, hipStream_t stream)
{
    switch (inst) {
    case 0: return launch<0>(a, stream);
    case 2: return launch<2>(a, stream);
    case 8: return launch<8>(a, stream);
    case 16: return launch<16>(a, stream);
    }
    return hipErrorInvalidValue;
}

}  // namespace cbet
