// cbet_node_kernel.h -- what the per-node table kernels share on the device (cbet_kernels.hip, cbet_target.hip,
// cbet_mesh.hip): the launch shape of their grid-stride walk over the nodes, and the scalar-load plumbing of the perturbed
// target's two constant tables.
// The walk itself (idx -> (i, j, k), z fastest) and the staging of the profile in LDS are written out in each kernel:
// the compiler folds blockDim.x to the workgroup size of the launch only where the kernel's own body reads it, and a
// kernel that takes either loop from a function inlined here comes out with other instructions than the one that spells
// it.
#ifndef CBET_NODE_KERNEL_H_
#define CBET_NODE_KERNEL_H_

#include <hip/hip_runtime.h>

#include "cbet_device.h"

namespace cbet {

// Workgroups of 256 threads for the walk: one thread per node up to 256 CUs x 16 blocks, grid-stride the rest.
inline unsigned node_blocks(long total)
{
    const long blocks = (total + 255) / 256;
    return (unsigned)(blocks > 256 * 16 ? 256 * 16 : blocks);
}

typedef const __attribute__((address_space(4))) double *ConstDoubles;   // constant address space: read by scalar loads
typedef const __attribute__((address_space(4))) char *ConstBytes;

// A perturbed target's factor and coefficient tables (cbet_target_model.h target_delta).  From L = 8 on the two outgrow
// the 102 SGPRs.  Left alone, the compiler loads all of them ahead of the node loop and parks the values in VGPR lanes
// (L = 16: 6,400 v_readlane per node against 1,950 fp64 operations).  So the tables' addresses pass through an empty asm
// statement once per m, which also names a value of the m before: the loads of one m cannot move ahead of the arithmetic
// of the last, and no more than one m's entries are live.  The addresses stay in SGPRs.
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

}  // namespace cbet
#endif
