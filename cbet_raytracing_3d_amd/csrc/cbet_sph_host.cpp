// cbet_sph_host.cpp -- C ABI of the mode spectra (include/cbet_mi355x.h): the argument checks,
// the device entry (cbet_sph_modes.hip) and its host twin, plain loops over the nodes in logical order.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "cbet_host_internal.h"

namespace {

using cbet::fail;

int sph_check(const double *edep, int ngrids, long grid_stride, const cbet_params *p, const double *center,
              const double *r_edges, int nshell, int lmax, const void *coeffs, const void *shell_energy,
              const void *shell_nodes, cbet_derived *d, long *pitch)
{
    if (lmax < 0 || lmax > CBET_SPH_LMAX) return fail(CBET_EINVAL, "sph_modes: lmax = %d outside [0, %d]", lmax, CBET_SPH_LMAX);
    if (nshell < 1 || nshell > CBET_SPH_MAX_SHELLS)
        return fail(CBET_EINVAL, "sph_modes: nshell = %d outside [1, %d]", nshell, CBET_SPH_MAX_SHELLS);
    if (ngrids < 1 || ngrids > CBET_SPH_MAX_GRIDS)
        return fail(CBET_EINVAL, "sph_modes: ngrids = %d outside [1, %d]", ngrids, CBET_SPH_MAX_GRIDS);
    if (!edep && ngrids != 1) return fail(CBET_EINVAL, "sph_modes: geometry mode (edep NULL) projects one grid, not %d", ngrids);
    if (!center || !r_edges) return fail(CBET_EINVAL, "sph_modes: NULL centre / shell edges");
    if (!coeffs || !shell_energy || !shell_nodes) return fail(CBET_EINVAL, "sph_modes: NULL output");
    if (int rc = cbet::derive_grid(p, d)) return rc;
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(center[i])) return fail(CBET_EINVAL, "sph_modes: centre is not finite");
    if (!(r_edges[0] >= 0.0)) return fail(CBET_EINVAL, "sph_modes: r_edges[0] = %g must be >= 0", r_edges[0]);
    for (int s = 0; s < nshell; ++s)
        if (!(r_edges[s + 1] > r_edges[s])) return fail(CBET_EINVAL, "sph_modes: r_edges not strictly increasing at %d", s + 1);
    if (!std::isfinite(r_edges[nshell])) return fail(CBET_EINVAL, "sph_modes: r_edges[%d] is not finite", nshell);
    *pitch = p->edep_zpitch ? p->edep_zpitch : p->nz + 2;
    const long gsize = (long)(p->nx + 2) * (p->ny + 2) * *pitch;
    if (ngrids > 1 && grid_stride < gsize)
        return fail(CBET_EINVAL, "sph_modes: grid_stride %ld is shorter than one grid (%ld doubles)", grid_stride, gsize);
    return CBET_OK;
}

}  // namespace

extern "C" int cbet_sph_modes_device(const double *edep, int ngrids, long grid_stride, const cbet_params *p,
                                     const double center[3], const double *r_edges, int nshell, int lmax, double *coeffs,
                                     double *shell_energy, long long *shell_nodes, void *stream)
{
    cbet_derived d;
    long pitch;
    if (int rc = sph_check(edep, ngrids, grid_stride, p, center, r_edges, nshell, lmax, coeffs, shell_energy, shell_nodes,
                           &d, &pitch))
        return rc;
    cbet::SphArgs a;
    std::memset(&a, 0, sizeof a);
    a.edep = edep;
    a.grid_stride = ngrids > 1 ? grid_stride : 0;
    a.row_pitch = pitch;
    a.ngrids = ngrids;
    cbet::grid_args(a, p, d);
    a.nshell = nshell;
    a.lmax = lmax;
    a.cx = center[0]; a.cy = center[1]; a.cz = center[2];
    a.coeffs = coeffs;
    a.shell_energy = shell_energy;
    a.shell_nodes = shell_nodes;
    std::memcpy(a.r_edges, r_edges, sizeof(double) * (nshell + 1));
    const hipError_t e = cbet::launch_sph_modes(a, (hipStream_t)stream);
    if (e != hipSuccess) return cbet::fail_hip(CBET_EHIP, "cbet_sph_modes_device: launch failed: %s", hipGetErrorString(e));
    return CBET_OK;
}

// The same sums node by node in logical order.  Y of a node is the device's recurrence, operation for operation;
// only the order of the sums over nodes differs.
extern "C" int cbet_sph_modes(const double *edep, int ngrids, long grid_stride, const cbet_params *p, const double center[3],
                              const double *r_edges, int nshell, int lmax, double *coeffs, double *shell_energy,
                              long long *shell_nodes, void *stream)
{
    (void)stream;
    cbet_derived d;
    long pitch;
    if (int rc = sph_check(edep, ngrids, grid_stride, p, center, r_edges, nshell, lmax, coeffs, shell_energy, shell_nodes,
                           &d, &pitch))
        return rc;
    const int L = lmax, C = (L + 1) * (L + 1);
    std::fill(coeffs, coeffs + (long)ngrids * nshell * C, 0.0);
    std::fill(shell_energy, shell_energy + (long)ngrids * nshell, 0.0);
    std::fill(shell_nodes, shell_nodes + nshell, 0LL);
    std::vector<double> ca((L + 1) * (L + 1), 0.0), cb((L + 1) * (L + 1), 0.0), dd(L + 1, 0.0), Y(C);
    for (int l = 0; l <= L; ++l)
        for (int m = 0; m < l; ++m) {
            ca[l * (L + 1) + m] = std::sqrt((double)(4 * l * l - 1) / (double)(l * l - m * m));
            cb[l * (L + 1) + m] = std::sqrt((double)((l - 1) * (l - 1) - m * m) / (double)(4 * (l - 1) * (l - 1) - 1));
        }
    for (int k = 1; k <= L; ++k) dd[k] = std::sqrt((double)(2 * k + 1) / (double)(2 * k));
    const double y00 = 1.0 / std::sqrt(4.0 * M_PI), sqrt2 = std::sqrt(2.0);
    const long plane = (long)(p->ny + 2) * pitch;
    for (int I = 0; I <= p->nx + 1; ++I)
        for (int J = 0; J <= p->ny + 1; ++J)
            for (int K = 0; K <= p->nz + 1; ++K) {
                const double x = ((I - 1) * d.dx + p->xmin) - center[0];
                const double y = ((J - 1) * d.dy + p->ymin) - center[1];
                const double z = ((K - 1) * d.dz + p->zmin) - center[2];
                const double r = std::sqrt(x * x + y * y + z * z);
                const int s = (int)(std::upper_bound(r_edges, r_edges + nshell + 1, r) - r_edges) - 1;
                if (s < 0 || s >= nshell) continue;
                double ct = 0.0, st = 0.0, c1 = 1.0, s1 = 0.0, hi = 0.0;
                if (r > 0.0) {
                    const double rho = std::sqrt(x * x + y * y);
                    ct = z / r;
                    st = rho / r;
                    if (rho > 0.0) { c1 = x / rho; s1 = y / rho; }
                    hi = 1.0;
                }
                double pmm = y00, cr = 1.0, si = 0.0;
                for (int m = 0; m <= L; ++m) {
                    if (m > 0) {
                        pmm = (pmm * dd[m]) * st;
                        const double cn = cr * c1 - si * s1;
                        si = cr * s1 + si * c1;
                        cr = cn;
                    }
                    const double cm = m ? sqrt2 * cr : 1.0, sm = m ? sqrt2 * si : 0.0;
                    double p1 = pmm, p2 = 0.0;
                    for (int l = m; l <= L; ++l) {
                        double yv = pmm;
                        if (l > m) {
                            yv = ca[l * (L + 1) + m] * std::fma(ct, p1, -(cb[l * (L + 1) + m] * p2));
                            p2 = p1;
                            p1 = yv;
                        }
                        Y[l * l + l + m] = yv * cm;
                        if (m) Y[l * l + l - m] = yv * sm;
                    }
                }
                for (int g = 0; g < ngrids; ++g) {
                    const double E = edep ? edep[(long)g * grid_stride + I * plane + J * pitch + K] : 1.0;
                    const double Eh = E * hi;
                    double *acc = coeffs + ((long)g * nshell + s) * C;
                    acc[0] = std::fma(E, Y[0], acc[0]);
                    for (int c = 1; c < C; ++c) acc[c] = std::fma(Eh, Y[c], acc[c]);
                    shell_energy[(long)g * nshell + s] += E;
                }
                ++shell_nodes[s];
            }
    return CBET_OK;
}
