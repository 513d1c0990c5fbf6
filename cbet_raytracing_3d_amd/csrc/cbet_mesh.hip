// cbet_mesh.hip -- node tables and node flow from a plasma given on a spherical-polar mesh (include/cbet_mi355x.h
// "hydro-mesh plasma").
//
// k_mesh<OUT>: k_tabulate_target's layout -- one thread per node, z fastest, grid-stride -- with the mesh's three coordinate
// arrays staged in LDS (at most CBET_MESH_MAX_COORDS doubles, 20 KiB: eight workgroups per CU, full occupancy).  A thread
// finds its node's direction from the mesh's centre and its r, theta and phi brackets (cbet_mesh_model.h: the statements,
// shared with the host twins), then
//   * k_tabulate_mesh = k_mesh<kMeshTables>: interpolates ne and Te and writes the context's ne3d / kap3d;
//   * k_mesh_flow     = k_mesh<kMeshFlow>:   interpolates (ur, utheta, uphi), turns them into (ux, uy, uz) and writes the
//     component-major flow table the gain kernels read (k_tabulate_flow's layout);
//   * k_mesh_state    = k_mesh<kMeshState>:  interpolates Te and, where the caller has them, Ti and Z, applies the state
//     model (cbet_state_model.h) and writes the component-major state table (cs, gain_const) the gain kernels read.
// One walk serves all three, so they are one template.  The mesh's fields are read by plain vector gathers, up to eight per
// field and node (two shells x two rows x two columns; fewer where a bracket clamps).  phi does not depend on z, so the
// nodes of one z-row -- a wave's lanes -- share their phi bracket and walk through the (r, theta) cells: the two columns
// of a row are neighbours in memory (one 16-byte piece, except across the period's seam), and a gather instruction
// touches one such piece per distinct (shell, row) pair among its lanes -- a handful for a mesh coarser than the grid, one
// per lane for a mesh whose shells are closer than dz (DESIGN.md section 14 has the measured traffic).
// Built with -ffp-contract=off like the rest of the library.  No inline assembly.
#include <hip/hip_runtime.h>

#include "cbet_mesh_model.h"
#include "cbet_node_kernel.h"

namespace cbet {
namespace {

enum MeshOut { kMeshTables = 0, kMeshFlow = 1, kMeshState = 2 };

template <MeshOut OUT>
__global__ void __launch_bounds__(256) k_mesh(const MeshArgs a)
{
    extern __shared__ double s_coord[];
    double *s_r = s_coord, *s_th = s_coord + a.nr, *s_ph = s_coord + a.nr + a.nth;
    for (int i = threadIdx.x; i < a.nr; i += blockDim.x) s_r[i] = a.r[i];
    for (int i = threadIdx.x; i < a.nth; i += blockDim.x) s_th[i] = a.theta[i];
    for (int i = threadIdx.x; i < a.nph; i += blockDim.x) s_ph[i] = a.phi[i];
    __syncthreads();
    const long total = (long)a.nx * a.ny * a.nz;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const int k = (int)(idx % a.nz);
        const long ij = idx / a.nz;
        const int j = (int)(ij % a.ny);
        const int i = (int)(ij / a.ny);
        MeshNode n;
        mesh_locate(a, s_r, s_th, s_ph, i, j, k, n);
        if (OUT == kMeshFlow) {
            double ux, uy, uz;
            mesh_velocity(a, n, ux, uy, uz);
            a.flow[idx] = ux;
            a.flow[idx + total] = uy;
            a.flow[idx + 2 * total] = uz;
        } else if (OUT == kMeshState) {
            double cs, gc;
            mesh_state(a, n, cs, gc);
            a.state[idx] = cs;
            a.state[idx + total] = gc;
        } else {
            double ed, kap;
            mesh_tables(a, n, ed, kap);
            a.ne3d[idx] = ed;
            a.kap3d[idx] = kap;
        }
    }
}

template <MeshOut OUT>
hipError_t launch(const MeshArgs &a, hipStream_t stream)
{
    const size_t lds = sizeof(double) * ((size_t)a.nr + a.nth + a.nph);
    hipLaunchKernelGGL(k_mesh<OUT>, dim3(node_blocks((long)a.nx * a.ny * a.nz)), dim3(256), lds, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_tabulate_mesh(const MeshArgs &a, hipStream_t stream) { return launch<kMeshTables>(a, stream); }
hipError_t launch_mesh_flow(const MeshArgs &a, hipStream_t stream) { return launch<kMeshFlow>(a, stream); }
hipError_t launch_mesh_state(const MeshArgs &a, hipStream_t stream) { return launch<kMeshState>(a, stream); }

}  // namespace cbet
