// cbet_target.hip -- the two node kernels of a perturbed target: its plasma tables (include/cbet_mi355x.h "perturbed
// targets") and the flow table of the CBET gain kernels (include/cbet_mi355x.h "flow table", DESIGN.md
// section 13).
//
// k_tabulate_target<L>: k_tabulate's layout -- one thread per node, z fastest, grid-stride, the 3 x nprofile profile staged
// in LDS -- with the node's radius taken about the target's centre and divided by 1 + delta, delta the target's
// spherical-harmonic distortion in the node's direction (cbet_target_model.h: the statements, shared with the host twin).
//   * the coefficients travel in the kernel argument and the recurrence factors lie in constant memory; every index into
//     them is a compile-time constant of the unrolled (m, l) loops, so they are read by scalar loads into SGPRs, one m's
//     entries at a time (TablePin, cbet_node_kernel.h);
//   * the recurrence runs in registers, m outermost: a thread holds the direction (ct, st, c1, s1), the m-chain (pmm, cr,
//     si), the l-chain (p1, p2), the two sums of the current m and delta -- no per-thread array;
//   * L = 0 is the pure offset (and the monopole): delta is one scalar for the launch and no harmonic is evaluated.
// k_tabulate_flow<L>: the same layout without the profile (no LDS): the node's radius on the target goes through the Mach
// ramp of the gain kernels' cell_state, and the velocity points along s / rho (target_flow).  The table is component-major,
// [3][nx][ny][nz]: each component is written -- and read by the gain kernels -- along z like ne3d.
// Built with -ffp-contract=off like the rest of the library: the tables equal the host twins' bit for bit.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "cbet_node_kernel.h"
#include "cbet_target_model.h"

namespace cbet {
namespace {

__constant__ double g_target_factors[kTargetFactors];

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
__global__ void __launch_bounds__(256) k_tabulate_flow(const FlowArgs a)
{
    const long total = (long)a.nx * a.ny * a.nz;
    const long stride = (long)gridDim.x * blockDim.x;
    // the coefficients where they arrive: `a` is the kernel's only argument, at the start of the kernel-argument segment
    const ConstDoubles coeffs = (ConstDoubles)((ConstBytes)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(FlowArgs, c));
    const ConstDoubles factors = (ConstDoubles)(unsigned long long)g_target_factors;
    double *const fx = a.flow, *const fy = fx + total, *const fz = fy + total;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const int k = (int)(idx % a.nz);
        const long ij = idx / a.nz;
        const int j = (int)(ij % a.ny);
        const int i = (int)(ij / a.ny);
        double ux, uy, uz;
        target_flow<L>(a, factors, coeffs, i, j, k, ux, uy, uz, TablePin<(L > 2)>());
        fx[idx] = ux;
        fy[idx] = uy;
        fz[idx] = uz;
    }
}

}  // namespace

hipError_t target_upload_factors()
{
    return hipMemcpyToSymbol(HIP_SYMBOL(g_target_factors), target_factors(), sizeof(double) * kTargetFactors);
}

hipError_t launch_tabulate_target(const TargetArgs &a, int inst, hipStream_t stream)
{
    const size_t lds = sizeof(double) * 3 * (size_t)a.t.nprofile;
    const bool known = dispatch_lmax(inst, [&](auto l) {
        hipLaunchKernelGGL(k_tabulate_target<decltype(l)::value>, dim3(node_blocks((long)a.t.nx * a.t.ny * a.t.nz)), dim3(256),
                           lds, stream, a);
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_tabulate_flow(const FlowArgs &a, int inst, hipStream_t stream)
{
    const bool known = dispatch_lmax(inst, [&](auto l) {
        hipLaunchKernelGGL(k_tabulate_flow<decltype(l)::value>, dim3(node_blocks((long)a.nx * a.ny * a.nz)), dim3(256), 0,
                           stream, a);
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace cbet
