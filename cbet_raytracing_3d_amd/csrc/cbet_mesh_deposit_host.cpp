// cbet_mesh_deposit_host.cpp -- deposit on the hydro mesh (include/cbet_mi355x.h "deposit on the hydro mesh", DESIGN.md
// section 15): the cells' handle with its checks and lookup tables, the argument block, the device entry of
// k_mesh_deposit (cbet_mesh_deposit.hip) and its host twin, plain loops over the nodes running the kernel's own statements
// (cbet_mesh_deposit_model.h).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "cbet_host_internal.h"
#include "cbet_mesh_deposit_model.h"

// The cells as the kernel and the twin read them: one table, r_edges [nr+1] | ct [nth-1] | pe [nph] | off of S = 1 | off of
// S = 2 | ... | off of S = smax (off of S starts S (S-1) / 2 doubles into that part).
struct cbet_mesh_cells_handle {
    int gpu = -1;
    double center[3] = {0, 0, 0};
    int nr = 0, nth = 0, nph = 0, smax = 0;
    std::vector<double> tab;
    double *d_tab = nullptr;
};

namespace {

using cbet::fail;

constexpr double kTwoPi = 6.283185307179586;
constexpr double kEdgeTol = 1e-12;

int check_edges(const char *name, const double *x, int n)
{
    for (int i = 0; i <= n; ++i)
        if (!std::isfinite(x[i])) return fail(CBET_EINVAL, "mesh_cells: %s[%d] is not finite", name, i);
    for (int i = 1; i <= n; ++i)
        if (!(x[i] > x[i - 1]))
            return fail(CBET_EINVAL, "mesh_cells: %s must be strictly ascending (%s[%d] = %g after %g)", name, name, i, x[i], x[i - 1]);
    return CBET_OK;
}

// Everything a deposit call checks beside the handle; fills the argument block up to the outputs.
int deposit_args(const cbet_mesh_cells_handle *h, const double *edep, int ngrids, long grid_stride, const cbet_params *p,
                 int subsamples, double *cell_energy, double *outside, long long *cell_samples, bool device,
                 cbet::MeshDepositArgs *out)
{
    if (!h) return fail(CBET_EINVAL, "mesh_deposit: NULL cells handle");
    if (ngrids < 1 || ngrids > CBET_SPH_MAX_GRIDS)
        return fail(CBET_EINVAL, "mesh_deposit: ngrids = %d outside [1, %d]", ngrids, CBET_SPH_MAX_GRIDS);
    if (subsamples < 1 || subsamples > h->smax)
        return fail(CBET_EINVAL, "mesh_deposit: subsamples = %d outside [1, %d] (the handle's subsamples_max)", subsamples, h->smax);
    if (!edep && ngrids != 1) return fail(CBET_EINVAL, "mesh_deposit: counts alone (edep NULL) take one grid, not %d", ngrids);
    if (!cell_samples || (edep && (!cell_energy || !outside))) return fail(CBET_EINVAL, "mesh_deposit: NULL output");
    cbet_derived d;
    if (int rc = cbet::derive_grid(p, &d)) return rc;
    const long pitch = p->edep_zpitch ? p->edep_zpitch : p->nz + 2;
    const long gsize = (long)(p->nx + 2) * (p->ny + 2) * pitch;
    if (ngrids > 1 && grid_stride < gsize)
        return fail(CBET_EINVAL, "mesh_deposit: grid_stride %ld is shorter than one grid (%ld doubles)", grid_stride, gsize);
    if (device && !h->d_tab) return fail(CBET_EINVAL, "mesh_deposit_device: the cells handle is host-only (created with gpu = -1)");
    cbet::MeshDepositArgs a{};
    a.edep = edep;
    a.grid_stride = ngrids > 1 ? grid_stride : 0;
    a.row_pitch = pitch;
    a.ngrids = ngrids;
    cbet::grid_args(a, p, d);
    a.ox = h->center[0]; a.oy = h->center[1]; a.oz = h->center[2];
    a.nr = h->nr; a.nth = h->nth; a.nph = h->nph;
    a.S = subsamples;
    a.inv = 1.0 / (double)(subsamples * subsamples * subsamples);
    const double *tab = device ? h->d_tab : h->tab.data();
    a.re = tab;
    a.ct = a.re + (h->nr + 1);
    a.pe = a.ct + (h->nth - 1);
    a.off = a.pe + h->nph + subsamples * (subsamples - 1) / 2;
    a.cell_energy = cell_energy;
    a.outside = outside;
    a.cell_samples = cell_samples;
    a.chunk = ngrids;
    *out = a;
    return CBET_OK;
}

}  // namespace

extern "C" {

int cbet_mesh_cells_create(cbet_mesh_cells_handle **out, const cbet_mesh_cells *c, int subsamples_max, int gpu)
{
    if (!out) return fail(CBET_EINVAL, "mesh_cells_create: NULL out");
    *out = nullptr;
    if (!c) return fail(CBET_EINVAL, "mesh_cells: cells is NULL");
    if (subsamples_max < 1 || subsamples_max > CBET_MESH_MAX_SUBSAMPLES)
        return fail(CBET_EINVAL, "mesh_cells: subsamples_max = %d outside [1, %d]", subsamples_max, CBET_MESH_MAX_SUBSAMPLES);
    if (gpu < -1) return fail(CBET_EINVAL, "mesh_cells: gpu = %d (a device, or -1 for a host-only handle)", gpu);
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(c->center[i])) return fail(CBET_EINVAL, "mesh_cells: center is not finite");
    if (c->nr < 1 || c->ntheta < 1 || c->nphi < 1)
        return fail(CBET_EINVAL, "mesh_cells: nr = %d, ntheta = %d, nphi = %d (each >= 1)", c->nr, c->ntheta, c->nphi);
    if ((long)c->nr + c->ntheta + c->nphi + 3 > CBET_MESH_MAX_COORDS)
        return fail(CBET_EINVAL, "mesh_cells: nr + ntheta + nphi + 3 = %ld edges exceed CBET_MESH_MAX_COORDS = %d",
                    (long)c->nr + c->ntheta + c->nphi + 3, CBET_MESH_MAX_COORDS);
    if ((long)c->nr * c->ntheta * c->nphi >= (1L << 31))
        return fail(CBET_EINVAL, "mesh_cells: nr * ntheta * nphi = %ld cells (fewer than 2^31)", (long)c->nr * c->ntheta * c->nphi);
    if (!c->r_edges) return fail(CBET_EINVAL, "mesh_cells: NULL r_edges");
    if (!c->theta_edges && c->ntheta != 1) return fail(CBET_EINVAL, "mesh_cells: NULL theta_edges with ntheta = %d", c->ntheta);
    if (!c->phi_edges && c->nphi != 1) return fail(CBET_EINVAL, "mesh_cells: NULL phi_edges with nphi = %d", c->nphi);
    if (int rc = check_edges("r_edges", c->r_edges, c->nr)) return rc;
    if (!(c->r_edges[0] >= 0.0)) return fail(CBET_EINVAL, "mesh_cells: r_edges[0] = %g must be >= 0", c->r_edges[0]);
    if (c->theta_edges) {
        const double *t = c->theta_edges;
        if (int rc = check_edges("theta_edges", t, c->ntheta)) return rc;
        if (!(std::fabs(t[0]) <= kEdgeTol)) return fail(CBET_EINVAL, "mesh_cells: theta_edges[0] = %g must be 0", t[0]);
        if (!(std::fabs(t[c->ntheta] - M_PI) <= kEdgeTol))
            return fail(CBET_EINVAL, "mesh_cells: theta_edges[%d] = %.17g must be pi", c->ntheta, t[c->ntheta]);
    }
    if (c->phi_edges) {
        const double *f = c->phi_edges;
        if (int rc = check_edges("phi_edges", f, c->nphi)) return rc;
        if (f[0] < -M_PI || !(f[0] < M_PI)) return fail(CBET_EINVAL, "mesh_cells: phi_edges[0] = %g outside [-pi, pi)", f[0]);
        if (!(std::fabs(f[c->nphi] - f[0] - kTwoPi) <= kEdgeTol))
            return fail(CBET_EINVAL, "mesh_cells: phi_edges must span one period (phi_edges[%d] - phi_edges[0] = %.17g, not 2 pi)",
                        c->nphi, f[c->nphi] - f[0]);
    }
    cbet_mesh_cells_handle *h = new (std::nothrow) cbet_mesh_cells_handle;
    if (!h) return fail(CBET_ENOMEM, "mesh_cells: out of host memory");
    h->gpu = gpu;
    for (int i = 0; i < 3; ++i) h->center[i] = c->center[i];
    h->nr = c->nr; h->nth = c->ntheta; h->nph = c->nphi; h->smax = subsamples_max;
    std::vector<double> &tab = h->tab;
    tab.assign(c->r_edges, c->r_edges + c->nr + 1);
    for (int e = 1; e < c->ntheta; ++e) tab.push_back(std::cos(c->theta_edges[e]));
    const size_t pe0 = tab.size();
    for (int k = 0; k < c->nphi; ++k) {
        double d = c->phi_edges ? cbet::deposit_diamond(std::cos(c->phi_edges[k]), std::sin(c->phi_edges[k])) : 0.0;
        if (k > 0 && d < tab[pe0]) d = d + 4.0;
        tab.push_back(d);
    }
    for (int k = 1; k < c->nphi; ++k)
        if (!(tab[pe0 + k] > tab[pe0 + k - 1]) || !(tab[pe0 + k] < tab[pe0] + 4.0)) {
            delete h;
            return fail(CBET_EINVAL, "mesh_cells: column %d is too thin: the diamond angles of its phi edges do not ascend (%.17g after %.17g)",
                        k - 1, tab[pe0 + k], tab[pe0 + k - 1]);
        }
    for (int S = 1; S <= subsamples_max; ++S)
        for (int s = 0; s < S; ++s) tab.push_back((double)(2 * s + 1 - S) / (2.0 * S));
    if (gpu >= 0) {
        cbet::DeviceGuard guard;
        hipError_t e = hipSetDevice(gpu);
        if (e == hipSuccess) e = hipMalloc((void **)&h->d_tab, sizeof(double) * tab.size());
        if (e == hipSuccess) e = hipMemcpy(h->d_tab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (h->d_tab) (void)hipFree(h->d_tab);
            delete h;
            return cbet::fail_hip(CBET_EHIP, "mesh_cells_create: upload to device %d failed: %s", gpu, hipGetErrorString(e));
        }
    }
    *out = h;
    return CBET_OK;
}

void cbet_mesh_cells_destroy(cbet_mesh_cells_handle *h)
{
    if (!h) return;
    if (h->d_tab) {
        cbet::DeviceGuard guard;
        if (hipSetDevice(h->gpu) == hipSuccess) (void)hipFree(h->d_tab);
        (void)hipGetLastError();
    }
    delete h;
}

int cbet_mesh_deposit_device(const cbet_mesh_cells_handle *h, const double *edep, int ngrids, long grid_stride,
                             const cbet_params *p, int subsamples, int method, double *cell_energy, double *outside,
                             long long *cell_samples, void *stream)
{
    cbet::MeshDepositArgs a;
    if (int rc = deposit_args(h, edep, ngrids, grid_stride, p, subsamples, cell_energy, outside, cell_samples, true, &a)) return rc;
    if (method < CBET_MESH_DEPOSIT_AUTO || method > CBET_MESH_DEPOSIT_LDS)
        return fail(CBET_EINVAL, "mesh_deposit_device: method = %d (0 auto, 1 global atomics, 2 LDS accumulators)", method);
    // the LDS arm: ceil(ngrids / 8) grids per workgroup, if their accumulators fit beside the tables
    cbet::MeshDepositArgs l = a;
    l.chunk = (ngrids + cbet::kMeshDepositChunks - 1) / cbet::kMeshDepositChunks;
    const bool fits = cbet::mesh_deposit_lds(l, true) <= cbet::kMeshDepositLds;
    if (method == CBET_MESH_DEPOSIT_LDS && !fits)
        return fail(CBET_EINVAL, "mesh_deposit_device: the LDS arm needs %zu bytes for %d x %d x %d cells and %d grids per workgroup (at most %zu)",
                    cbet::mesh_deposit_lds(l, true), a.nr, a.nth, a.nph, l.chunk, cbet::kMeshDepositLds);
    const bool lds_arm = method == CBET_MESH_DEPOSIT_LDS || (method == CBET_MESH_DEPOSIT_AUTO && fits);
    hipStream_t s = (hipStream_t)stream;
    cbet::DeviceGuard guard;
    CBET_HIP(hipSetDevice(h->gpu));
    CBET_HIP(cbet::launch_mesh_deposit(lds_arm ? l : a, lds_arm, s));   // the zero-fill of the outputs, then the deposit
    return CBET_OK;
}

int cbet_mesh_deposit(const cbet_mesh_cells_handle *h, const double *edep, int ngrids, long grid_stride, const cbet_params *p,
                      int subsamples, int method, double *cell_energy, double *outside, long long *cell_samples, void *stream)
{
    (void)method;
    (void)stream;
    cbet::MeshDepositArgs a;
    if (int rc = deposit_args(h, edep, ngrids, grid_stride, p, subsamples, cell_energy, outside, cell_samples, false, &a)) return rc;
    const long ncell = (long)a.nr * a.nth * a.nph;
    std::fill(cell_samples, cell_samples + ncell, 0LL);
    if (edep) {
        std::fill(cell_energy, cell_energy + ncell * ngrids, 0.0);
        std::fill(outside, outside + ngrids, 0.0);
    }
    const long plane = (long)(a.ny + 2) * a.row_pitch;
    for (int I = 0; I <= a.nx + 1; ++I)
        for (int J = 0; J <= a.ny + 1; ++J)
            for (int K = 0; K <= a.nz + 1; ++K) {
                const double *node = edep ? edep + (I * plane + J * a.row_pitch + K) : nullptr;
                cbet::deposit_samples(a, a.re, a.ct, a.pe, a.off, I, J, K, [&](int cell) {
                    if (cell >= 0) ++cell_samples[cell];
                    if (!node) return;
                    for (int g = 0; g < ngrids; ++g) {
                        const double v = node[g * a.grid_stride] * a.inv;
                        if (cell >= 0) cell_energy[g * ncell + cell] += v; else outside[g] += v;
                    }
                });
            }
    return CBET_OK;
}

}  // extern "C"
