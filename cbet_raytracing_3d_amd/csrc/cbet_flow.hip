// cbet_flow.hip -- the node flow table of the CBET gain kernels on a perturbed target (include/cbet_mi355x.h "flow table",
// DESIGN.md section 13).
//
// k_tabulate_flow<L>: k_tabulate_target's layout -- one thread per node, z fastest, grid-stride -- without the profile (no
// LDS): the node's radius about the target's centre, divided by 1 + delta, goes through the Mach ramp of the gain kernels'
// cell_state, and the velocity points along s / rho (cbet_target_model.h target_flow: the statements, shared with the
// host twin).  Coefficients in the kernel argument, recurrence factors in constant memory, one m's entries live at a time
// (TablePin), as in cbet_target.hip.  The table is component-major, [3][nx][ny][nz]: each component is written -- and read
// by the gain kernels -- along z like ne3d.
// Built with -ffp-contract=off like the rest of the library: the table equals the host twin's bit for bit.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "cbet_target_model.h"

namespace cbet {
namespace {

__constant__ double g_flow_factors[kTargetFactors];

typedef const __attribute__((address_space(4))) double *ConstDoubles;   // constant address space: read by scalar loads
typedef const __attribute__((address_space(4))) char *ConstBytes;

// cbet_target.hip's TablePin: the tables' addresses pass through an empty asm statement once per m, together with a value
// of the m before, so that no more than one m's factors and coefficients are loaded ahead of their use.
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
__global__ void __launch_bounds__(256) k_tabulate_flow(const FlowArgs a)
{
    const long total = (long)a.nx * a.ny * a.nz;
    const long stride = (long)gridDim.x * blockDim.x;
    // the coefficients where they arrive: `a` is the kernel's only argument, at the start of the kernel-argument segment
    const ConstDoubles coeffs = (ConstDoubles)((ConstBytes)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(FlowArgs, c));
    const ConstDoubles factors = (ConstDoubles)(unsigned long long)g_flow_factors;
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

template <int L>
hipError_t launch(const FlowArgs &a, hipStream_t stream)
{
    const long total = (long)a.nx * a.ny * a.nz;
    long blocks = (total + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;  // k_tabulate_target's shape: 256 CUs x 16 blocks, grid-stride the rest
    hipLaunchKernelGGL(k_tabulate_flow<L>, dim3((unsigned)blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t flow_upload_factors()
{
    return hipMemcpyToSymbol(HIP_SYMBOL(g_flow_factors), target_factors(), sizeof(double) * kTargetFactors);
}

hipError_t launch_tabulate_flow(const FlowArgs &a, int inst, hipStream_t stream)
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
