// cbet_exchange_host.cpp -- the host twin of the pairwise exchange matrix (include/cbet_mi355x.h cbet_exchange_matrix_host;
// DESIGN.md section 18): plain loops over the haloed cells in index order running the ORDERED gain kernel's statements
// (cbet_grid_kernels.hip k_gain_field: cell_state, cell_pref, cell_sat_limit and the pair body), one IEEE operation per
// written operator -- the library is built with -ffp-contract=off -- with every pair's two sums compensated (Neumaier).
// No HIP call: it is the reference of the device path at any size.
#include <cmath>
#include <vector>

#include "cbet_host_internal.h"
#include "cbet_node_model.h"

namespace cbet {
namespace {

// sum += x, the rounding error of the add collected in comp (Neumaier's variant of Kahan's sum)
inline void add_compensated(double &sum, double &comp, double x)
{
    const double t = sum + x;
    if (std::fabs(sum) >= std::fabs(x)) comp += (sum - t) + x;
    else comp += (x - t) + sum;
    sum = t;
}

// The cell's plasma state as cell_state<FLOW, STATE> forms it (cbet_grid_kernels.hip): node (i, j, k) is the cell's, clamped.
struct HostCell {
    double frac, eps, rt, ux, uy, uz, cs, gc;
};

HostCell host_cell(const GainArgs &a, int i, int j, int k)
{
    const long nodes = (long)a.nx * a.ny * a.nz, node = ((long)i * a.ny + j) * a.nz + k;
    HostCell c;
    c.frac = a.ne3d[node] / a.ncrit;
    c.eps = 1.0 - c.frac;
    c.rt = c.eps > 0.0 ? sqrt(c.eps) : 0.0;
    if (a.state) {
        c.cs = a.state[node];
        c.gc = a.state[node + nodes];
    } else {
        c.cs = a.cs;
        c.gc = a.gain_const;
    }
    if (a.flow) {
        c.ux = a.flow[node];
        c.uy = a.flow[node + nodes];
        c.uz = a.flow[node + 2 * nodes];
        return c;
    }
    double xc, yc, zc, rr;
    node_centre(a, i, j, k, 0.0, 0.0, 0.0, xc, yc, zc, rr);
    radial_flow(a, rr, rr, xc, yc, zc, c.ux, c.uy, c.uz);
    return c;
}

}  // namespace
}  // namespace cbet

extern "C" int cbet_exchange_matrix_host(const double *fields, const double *ne3d, double *out, double *gross, int hx_lo,
                                         int hx_hi, const cbet_params *p, const cbet_gain_params *g, const double *flow,
                                         const double *state, double dn_max)
{
    using namespace cbet;
    cbet_derived d;
    if (int rc = derive_grid(p, &d)) return rc;
    if (p->nbeams > CBET_MAX_CBET_BEAMS)
        return fail(CBET_EINVAL, "cbet_exchange_matrix_host: nbeams = %d exceeds CBET_MAX_CBET_BEAMS = %d", p->nbeams, CBET_MAX_CBET_BEAMS);
    double cs = 0, gc = 0;
    if (int rc = cbet_gain_constants(p, g, nullptr, &cs, &gc)) return rc;   // (validates the gain parameters)
    if (!fields) return fail(CBET_EINVAL, "cbet_exchange_matrix_host: fields is NULL");
    if (!ne3d) return fail(CBET_EINVAL, "cbet_exchange_matrix_host: ne3d is NULL (there is no context to take a table from)");
    if (!out) return fail(CBET_EINVAL, "cbet_exchange_matrix_host: out is NULL");
    if (hx_lo < 0 || hx_hi > p->nx + 2 || hx_hi < hx_lo)
        return fail(CBET_EINVAL, "cbet_exchange_matrix_host: slab [%d,%d) outside the haloed grid [0,%d)", hx_lo, hx_hi, p->nx + 2);
    if (!(dn_max >= 0.0) || std::isinf(dn_max))
        return fail(CBET_EINVAL, "cbet_exchange_matrix_host: dn_max must be finite and >= 0 (0 = no limit)");
    const int nb = p->nbeams;
    if (nb < 2 || hx_hi == hx_lo) return CBET_OK;
    GainArgs a{};
    grid_args(a, p, d);
    a.nbeams = nb; a.dt = d.dt;
    a.ncrit = d.ncrit; a.k0 = d.omega / kC;
    a.cs = cs; a.gain_const = gc; a.iaw = g->iaw;
    a.mach_r0 = g->mach_r0; a.mach_0 = g->mach_0; a.mach_r1 = g->mach_r1; a.mach_1 = g->mach_1;
    a.ne3d = ne3d; a.flow = flow; a.state = state; a.sat = dn_max;
    const int HY = a.ny + 2, HZ = a.nz + 2;
    const long hsize = (long)(a.nx + 2) * HY * HZ, total = hsize * nb;
    const double iaw2 = a.iaw * a.iaw;
    const bool sat = dn_max > 0.0;
    // per ordered pair index i * nb + j, i < j: the sums of x and |x| with their compensations
    std::vector<double> st((size_t)nb * nb, 0.0), ct((size_t)nb * nb, 0.0), sg((size_t)nb * nb, 0.0), cg((size_t)nb * nb, 0.0);
    int present[CBET_MAX_CBET_BEAMS];
    for (int hi = hx_lo; hi < hx_hi; ++hi)
        for (int hj = 0; hj < HY; ++hj)
            for (int hk = 0; hk < HZ; ++hk) {
                const long h = ((long)hi * HY + hj) * HZ + hk;
                const double *fI = fields + h, *fx = fI + total, *fy = fx + total, *fz = fy + total;
                int n = 0;
                for (int b = 0; b < nb; ++b)
                    if (fI[(long)b * hsize] > 0.0) present[n++] = b;
                if (n < 2) continue;
                const int i = hi < 1 ? 0 : (hi > a.nx ? a.nx - 1 : hi - 1);
                const int j = hj < 1 ? 0 : (hj > a.ny ? a.ny - 1 : hj - 1);
                const int k = hk < 1 ? 0 : (hk > a.nz ? a.nz - 1 : hk - 1);
                const HostCell c = host_cell(a, i, j, k);
                if (!(c.eps > 0.0)) continue;
                const double ds_node = (kC * c.rt) * a.dt;
                const double pref = c.gc * c.frac * (1.0 / a.iaw) / c.rt;
                const double kap = ((0.5 * a.k0) * c.frac) / c.rt;
                const double lim = a.sat * kap;
                for (int ia = 0; ia < n; ++ia) {
                    const int bi = present[ia];
                    const long oi = (long)bi * hsize;
                    const double Ii = fI[oi], kxi = fx[oi], kyi = fy[oi], kzi = fz[oi];
                    for (int ib = ia + 1; ib < n; ++ib) {
                        const int bj = present[ib];
                        const long oj = (long)bj * hsize;
                        const double Ij = fI[oj];
                        const double qx = fx[oj] - kxi, qy = fy[oj] - kyi, qz = fz[oj] - kzi;
                        const double kiaw = sqrt(qx * qx + qy * qy + qz * qz);
                        if (!(kiaw > 0.0)) continue;
                        const double eta = (0.0 - (qx * c.ux + qy * c.uy + qz * c.uz)) / (kiaw * c.cs + 1e-10);
                        const double e2 = eta * eta;
                        const double P = iaw2 * eta / ((e2 - 1.0) * (e2 - 1.0) + iaw2 * e2);
                        double gn = pref * P;
                        if (sat) {
                            const double w = fabs(gn) * sqrt(Ii * Ij);
                            if (w > lim) gn = gn * (lim / w);
                        }
                        const double x = ((ds_node * gn) * Ii) * Ij;
                        const size_t at = (size_t)bi * nb + bj;
                        add_compensated(st[at], ct[at], x);
                        add_compensated(sg[at], cg[at], fabs(x));
                    }
                }
            }
    for (int i = 0; i < nb; ++i) {
        out[(size_t)i * nb + i] = 0.0;
        if (gross) gross[(size_t)i * nb + i] = 0.0;
        for (int j = i + 1; j < nb; ++j) {
            const size_t up = (size_t)i * nb + j, low = (size_t)j * nb + i;
            const double t = out[up] + (st[up] + ct[up]);
            out[up] = t;
            out[low] = -t;
            if (gross) {
                const double s = gross[up] + (sg[up] + cg[up]);
                gross[up] = s;
                gross[low] = s;
            }
        }
    }
    return CBET_OK;
}
