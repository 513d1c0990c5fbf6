// cbet_mesh_deposit.hip -- the energy of deposit grids binned into the cells of a spherical-polar mesh
// (include/cbet_mi355x.h "deposit on the hydro mesh").
//
// k_mesh_deposit<LDS_ARM>: k_mesh's layout -- one thread per node of the haloed grid, z fastest, grid-stride over at most
// 4096 workgroups of 256 -- with the cells' four lookup tables staged in LDS (r edges, cosines of the interior theta edges,
// diamond angles of the phi edges, sub-sample offsets), where the three bisections of a sample run.  A thread walks its
// node's S^3 samples in order (cbet_mesh_deposit_model.h: the statements, shared with the host twin) and books a run of
// consecutive samples that share a cell as ONE contribution of n samples: a mesh coarser than the sub-sample spacing costs
// a node one or two contributions, not S^3.  The cells of a node are found once and serve every grid of the workgroup's
// part of the stack (blockIdx.y; a.chunk grids): a node whose grids all hold zero costs a workgroup with blockIdx.y > 0
// nothing but the loads, and the counts are blockIdx.y == 0's alone.
//   * LDS_ARM false: every contribution is a global atomic -- native global_atomic_add_f64 for the energies, a 64-bit
//     integer atomic for the counts.  For meshes with many cells, where few contributions meet at one address.
//   * LDS_ARM true: the workgroup keeps a.chunk x cells fp64 accumulators and one 32-bit count per cell in LDS
//     (workgroup-scope atomics) and issues one global atomic per non-zero accumulator at its end.  For the 1-D and coarse
//     2-D meshes, where millions of nodes would otherwise meet at a few hundred addresses.  A workgroup sees at most
//     ceil(nodes / (4096 * 256)) * 256 * 64 samples, far below 2^32 for any grid that fits a device.
// k_mesh_deposit_zero clears the outputs first: the call overwrites them.
// In both arms the energy outside every shell is summed per workgroup in LDS first (one address per grid).
// Built with -ffp-contract=off like the rest of the library.  No inline assembly.
#include <hip/hip_runtime.h>

#include "cbet_mesh_deposit_model.h"
#include "cbet_node_kernel.h"

namespace cbet {
namespace {

__device__ __forceinline__ void lds_add(double *p, double v)
{
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The outputs start from zero: a kernel of the library's own ahead of the deposit, so that a captured call is two kernel
// nodes and nothing else.  energy / outside are NULL in a counts-only call.
__global__ void __launch_bounds__(256) k_mesh_deposit_zero(double *energy, long nenergy, double *outside, int noutside,
                                                           long long *samples, long nsamples)
{
    const long stride = (long)gridDim.x * blockDim.x, first = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (energy) {
        for (long i = first; i < nenergy; i += stride) energy[i] = 0.0;
        for (long i = first; i < noutside; i += stride) outside[i] = 0.0;
    }
    for (long i = first; i < nsamples; i += stride) samples[i] = 0;
}

template <bool LDS_ARM>
__global__ void __launch_bounds__(256) k_mesh_deposit(const MeshDepositArgs a)
{
    extern __shared__ double s_tab[];
    // tables first (doubles), then the per-grid outside sums, the accumulators and the counts of the LDS arm
    double *s_re = s_tab, *s_ct = s_re + (a.nr + 1), *s_pe = s_ct + (a.nth - 1), *s_off = s_pe + a.nph;
    double *s_out = s_off + a.S;
    const int ncell = a.nr * a.nth * a.nph;
    const int g0 = (int)blockIdx.y * a.chunk;
    const int G = min(a.chunk, a.ngrids - g0);                 // >= 1: the launch has ceil(ngrids / chunk) parts
    double *s_acc = s_out + a.chunk;
    unsigned *s_cnt = (unsigned *)(s_acc + (LDS_ARM ? (long)a.chunk * ncell : 0));
    for (int i = threadIdx.x; i <= a.nr; i += blockDim.x) s_re[i] = a.re[i];
    for (int i = threadIdx.x; i < a.nth - 1; i += blockDim.x) s_ct[i] = a.ct[i];
    for (int i = threadIdx.x; i < a.nph; i += blockDim.x) s_pe[i] = a.pe[i];
    for (int i = threadIdx.x; i < a.S; i += blockDim.x) s_off[i] = a.off[i];
    for (int i = threadIdx.x; i < a.chunk; i += blockDim.x) s_out[i] = 0.0;
    if (LDS_ARM) {
        for (int i = threadIdx.x; i < a.chunk * ncell; i += blockDim.x) s_acc[i] = 0.0;
        for (int i = threadIdx.x; i < ncell; i += blockDim.x) s_cnt[i] = 0u;
    }
    __syncthreads();

    const bool counting = blockIdx.y == 0;
    const int hz = a.nz + 2, hy = a.ny + 2;
    const long plane = (long)hy * a.row_pitch;
    const long total = (long)(a.nx + 2) * hy * hz;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const int K = (int)(idx % hz);
        const long ij = idx / hz;
        const int J = (int)(ij % hy);
        const int I = (int)(ij / hy);
        const double *node = a.edep ? a.edep + ((long)g0 * a.grid_stride + (long)I * plane + (long)J * a.row_pitch + K) : nullptr;
        if (!counting) {                                        // a node that holds no energy in this part of the stack
            bool any = false;
            if (node)
                for (int g = 0; g < G; ++g) any = any || node[(long)g * a.grid_stride] != 0.0;
            if (!any) continue;
        }
        // n samples of this node in `cell` (-1: outside every shell)
        auto book = [&](int cell, int n) {
            if (counting && cell >= 0) {
                if (LDS_ARM) atomicAdd(&s_cnt[cell], (unsigned)n);
                else atomicAdd((unsigned long long *)&a.cell_samples[cell], (unsigned long long)n);
            }
            if (!node) return;
            for (int g = 0; g < G; ++g) {
                const double e = node[(long)g * a.grid_stride];
                if (e == 0.0) continue;
                const double v = (e * a.inv) * n;
                if (cell < 0) lds_add(&s_out[g], v);
                else if (LDS_ARM) lds_add(&s_acc[(long)g * ncell + cell], v);
                else unsafeAtomicAdd(&a.cell_energy[(long)(g0 + g) * ncell + cell], v);   // native global_atomic_add_f64
            }
        };
        int run_cell = 0, run_n = 0;
        deposit_samples(a, s_re, s_ct, s_pe, s_off, I, J, K, [&](int cell) {
            if (run_n > 0 && cell != run_cell) {
                book(run_cell, run_n);
                run_n = 0;
            }
            run_cell = cell;
            ++run_n;
        });
        book(run_cell, run_n);                                  // S >= 1: the last run holds a sample
    }
    __syncthreads();

    if (a.edep)
        for (int g = threadIdx.x; g < G; g += blockDim.x)
            if (s_out[g] != 0.0) unsafeAtomicAdd(&a.outside[g0 + g], s_out[g]);
    if (LDS_ARM) {
        if (a.edep)
            for (int i = threadIdx.x; i < G * ncell; i += blockDim.x)
                if (s_acc[i] != 0.0) unsafeAtomicAdd(&a.cell_energy[(long)g0 * ncell + i], s_acc[i]);
        if (counting)
            for (int i = threadIdx.x; i < ncell; i += blockDim.x)
                if (s_cnt[i] != 0u) atomicAdd((unsigned long long *)&a.cell_samples[i], (unsigned long long)s_cnt[i]);
    }
}

}  // namespace

size_t mesh_deposit_lds(const MeshDepositArgs &a, bool lds_arm)
{
    const size_t ncell = (size_t)a.nr * a.nth * a.nph;
    size_t bytes = sizeof(double) * ((size_t)a.nr + a.nth + a.nph + a.S + a.chunk);
    if (lds_arm) bytes += ncell * (sizeof(double) * a.chunk + sizeof(unsigned));
    return bytes;
}

hipError_t launch_mesh_deposit(const MeshDepositArgs &a, bool lds_arm, hipStream_t stream)
{
    const long ncell = (long)a.nr * a.nth * a.nph;
    hipLaunchKernelGGL(k_mesh_deposit_zero, dim3(node_blocks(ncell * (a.edep ? a.ngrids : 1))), dim3(256), 0, stream,
                       a.edep ? a.cell_energy : nullptr, ncell * a.ngrids, a.outside, a.ngrids, a.cell_samples, ncell);
    if (hipError_t e = hipGetLastError()) return e;
    const long total = (long)(a.nx + 2) * (a.ny + 2) * (a.nz + 2);
    const dim3 grid(node_blocks(total), (unsigned)((a.ngrids + a.chunk - 1) / a.chunk));
    const size_t lds = mesh_deposit_lds(a, lds_arm);
    if (lds_arm) hipLaunchKernelGGL(k_mesh_deposit<true>, grid, dim3(256), lds, stream, a);
    else hipLaunchKernelGGL(k_mesh_deposit<false>, grid, dim3(256), lds, stream, a);
    return hipGetLastError();
}

}  // namespace cbet
