// cbet_node_model.h -- the statements every per-node table shares, each written once for the gfx950 kernels and their host
// twins: the clamped bisection bracket and the two-table interpolation of launch_ray_XZ.cu:16-63, the node's centre and
// radius (:296), the absorbed fraction (:299-305) and the Mach ramp with its radial flow.  The plain
// tabulation (cbet_kernels.hip), perturbed targets (cbet_target_model.h), the hydro mesh (cbet_mesh_model.h) and the gain
// stage's cell state (cbet_gain_model.h, for the gain kernels and the exchange matrix's host twin) are written over them.
// Built with -ffp-contract=off on both sides: every operator below is one IEEE fp64 operation, in the order written, so a
// kernel and its twin agree bit for bit.  The includer provides sqrt(double): <hip/hip_runtime.h> in device code, <cmath>
// on the host.
#ifndef CBET_NODE_MODEL_H_
#define CBET_NODE_MODEL_H_

#include "cbet_device.h"
#include "cbet_hd.h"

namespace cbet {

// launch_ray_XZ.cu:16-63, the search: where xp lies in x[0 .. n-1], either abscissa order, n >= 2.  Calls at_end(e) when xp
// is at or beyond an end of x (e = 0 or n - 1: the lookup is that node's value), else inside(mid) with xp between x[mid]
// and x[mid + 1], mid <= n - 2.  No index leaves the array whatever x and xp hold, NaN included.
template <class AtEnd, class Inside>
CBET_HD void bracket(const double *x, int n, const double xp, AtEnd at_end, Inside inside)
{
    const bool ascending = x[0] <= x[n - 1];
    if (ascending ? (xp <= x[0]) : (xp >= x[0])) { at_end(0); return; }
    if (ascending ? (xp >= x[n - 1]) : (xp <= x[n - 1])) { at_end(n - 1); return; }
    unsigned lo = 0, hi = n - 1, mid = (lo + hi) >> 1;
    while (lo < hi - 1) {
        const bool go_low = ascending ? (x[mid] >= xp) : !(x[mid] <= xp);  // :31 / :52 (as written there)
        if (go_low) hi = mid; else lo = mid;
        mid = (lo + hi) >> 1;
    }
    inside(mid);            // lo < hi throughout and hi == lo + 1 here: mid == lo <= n - 2
}

// ... as two indices: i1 == i0 at or beyond an end (that node alone), else i1 == i0 + 1.
CBET_HD void bracket(const double *x, int n, const double xp, int &i0, int &i1)
{
    bracket(x, n, xp, [&](int e) { i0 = i1 = e; }, [&](unsigned mid) { i0 = (int)mid; i1 = (int)mid + 1; });
}

// Two tables over ONE abscissa (ne and Te share r_data, :297-298): the bracket depends only on (x, xp), so it is found
// once and both values are interpolated from the same segment -- bit for bit what two single-table lookups return.
CBET_HD void interp2(const double *y1, const double *y2, const double *x, const double xp, int n, double &o1, double &o2)
{
    bracket(x, n, xp, [&](int e) { o1 = y1[e]; o2 = y2[e]; }, [&](unsigned mid) {
        const double dx = x[mid + 1] - x[mid], t = xp - x[mid];
        o1 = y1[mid] + (y1[mid + 1] - y1[mid]) / dx * t;
        o2 = y2[mid] + (y2[mid + 1] - y2[mid]) / dx * t;
    });
}

// :296 -- node (i, j, k)'s centre taken from (ox, oy, oz), and its radius, squares summed x, y, z.  G: an argument block
// with the grid's xmin .. dz.
template <class G>
CBET_HD void node_centre(const G &g, int i, int j, int k, double ox, double oy, double oz, double &sx, double &sy,
                         double &sz, double &rho)
{
    const double xc = i * g.dx + g.xmin, yc = j * g.dy + g.ymin, zc = k * g.dz + g.zmin;
    sx = xc - ox; sy = yc - oy; sz = zc - oz;
    rho = sqrt(sx * sx + sy * sy + sz * sz);
}

// :299-305 -- the absorbed fraction of a step at density ed and temperature etemp, up to the trailing "* uray".
CBET_HD double kappa(double ed, double etemp, double ncrit, double dt)
{
    const double eta = 5.2e-5 * 10.0 / (etemp * sqrt(etemp));       // :299
    const double nuei = (1e6 * ed * (kEc * kEc) / kMe) * eta;       // :300
    return ed / ncrit * nuei * dt;                                  // :305
}

// The Mach ramp at radius rhop, then the flow along s / rho; zero at the centre.  M: an argument block with mach_r0,
// mach_0, mach_r1, mach_1 and cs.
template <class M>
CBET_HD void radial_flow(const M &m, double rhop, double rho, double sx, double sy, double sz, double &ux, double &uy,
                         double &uz)
{
    double t = (rhop - m.mach_r0) / (m.mach_r1 - m.mach_r0);
    if (t < 0.0) t = 0.0;
    if (t > 1.0) t = 1.0;
    const double um = (m.mach_0 + (m.mach_1 - m.mach_0) * t) * m.cs;
    ux = uy = uz = 0.0;
    if (rho > 0.0) { ux = um * (sx / rho); uy = um * (sy / rho); uz = um * (sz / rho); }
}

}  // namespace cbet
#endif
