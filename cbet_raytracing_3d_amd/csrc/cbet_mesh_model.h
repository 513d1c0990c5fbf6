// cbet_mesh_model.h -- one node of a plasma given on a spherical-polar mesh (include/cbet_mi355x.h, "hydro-mesh plasma";
// DESIGN.md section 14), written once for the gfx950 kernels (cbet_mesh.hip) and their host twins (cbet_mesh_host.cpp).
// Built with -ffp-contract=off on both sides: every operator below is one IEEE fp64 operation, in the order the header
// fixes.  The includer provides sqrt(double) and atan2(double, double): <hip/hip_runtime.h> in device code, <cmath> on the
// host -- two different atan2, so the two sides may put a node that lies on a bracket's edge into neighbouring brackets;
// the interpolant is continuous there, and a field that does not depend on the angles comes out bit for bit the same.
//
// Degenerate nodes.  atan2(0, 0) is 0 on both sides.  A node at the mesh's centre (rho == 0) therefore reads theta = 0 and
// phi = 0: the brackets that hold theta = 0 and phi = 0 (phi + 2 pi where phi[0] > 0), on the innermost shell alone.  A
// node on the polar axis (rxy == 0) reads phi = 0 in the same way, with theta = 0 above the centre and theta = pi below.
//
// Bounds.  Every index the three searches produce lies inside its array whatever the coordinates and the node hold, NaN
// included (nr >= 2, ntheta >= 1, nphi >= 1 are the entry points' checks): a bad mesh gives wrong numbers, never a read
// out of range.
#ifndef CBET_MESH_MODEL_H_
#define CBET_MESH_MODEL_H_

#include "cbet_device.h"
#include "cbet_node_model.h"
#include "cbet_state_model.h"

namespace cbet {

// Where a node lies in the mesh: its direction from the centre and its three brackets.  A bracket whose two indices are
// equal is a clamped one (that node alone).
struct MeshNode {
    double sx, sy, sz, rho, rxy;
    int m0, m1;             // shells; m1 == m0: rho at or beyond an end of r
    double dr, tr;          // r[m1] - r[m0], rho - r[m0]
    int j0, j1;             // theta rows; j1 == j0: theta at or beyond an end, or ntheta == 1
    double wt;
    int k0, k1;             // phi columns, periodic (k1 == 0 after the last); k1 == k0: nphi == 1
    double wp;
};

// The node's centre and radius about the mesh's centre, then the angles and the three brackets.
// r / th / ph: the mesh's coordinate arrays (LDS in the kernel).
CBET_HD void mesh_locate(const MeshArgs &a, const double *r, const double *th, const double *ph, int i, int j, int k,
                         MeshNode &n)
{
    node_centre(a, i, j, k, a.ox, a.oy, a.oz, n.sx, n.sy, n.sz, n.rho);
    n.rxy = sqrt(n.sx * n.sx + n.sy * n.sy);
    n.j0 = n.j1 = 0; n.wt = 0.0;
    if (a.nth > 1) {
        const double theta = atan2(n.rxy, n.sz);
        bracket(th, a.nth, theta, n.j0, n.j1);
        if (n.j1 != n.j0) n.wt = (theta - th[n.j0]) / (th[n.j1] - th[n.j0]);
    }
    n.k0 = n.k1 = 0; n.wp = 0.0;
    if (a.nph > 1) {
        double phi = atan2(n.sy, n.sx);
        if (phi < ph[0]) phi = phi + 6.283185307179586;
        int lo = 0, hi = a.nph;                 // the last index with ph[k] <= phi, 0 if there is none: lo < nph always
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (ph[mid] <= phi) lo = mid; else hi = mid;
        }
        double upper;
        if (lo < a.nph - 1) { n.k1 = lo + 1; upper = ph[lo + 1]; }
        else { n.k1 = 0; upper = ph[0] + 6.283185307179586; }
        n.k0 = lo;
        double wp = (phi - ph[lo]) / (upper - ph[lo]);
        if (wp < 0.0) wp = 0.0;
        if (wp > 1.0) wp = 1.0;
        n.wp = wp;
    }
    bracket(r, a.nr, n.rho, n.m0, n.m1);
    n.dr = r[n.m1] - r[n.m0];
    n.tr = n.rho - r[n.m0];
}

// Field f ([nr][ntheta][nphi], phi fastest) on shell s: along phi first, then along theta.
CBET_HD double mesh_shell(const MeshArgs &a, const double *f, const MeshNode &n, int s)
{
    const double *row0 = f + ((long)s * a.nth + n.j0) * a.nph;
    double a0 = row0[n.k0];
    if (n.k1 != n.k0) a0 = a0 + (row0[n.k1] - a0) * n.wp;
    if (n.j1 == n.j0) return a0;
    const double *row1 = f + ((long)s * a.nth + n.j1) * a.nph;
    double a1 = row1[n.k0];
    if (n.k1 != n.k0) a1 = a1 + (row1[n.k1] - a1) * n.wp;
    return a0 + (a1 - a0) * n.wt;
}

// ... and along r last, with interp2's own statement (cbet_node_model.h): for a field that does not depend on the angles
// mesh_shell returns f[s] exactly ((b - a) is 0), and the value is, bit for bit, interp2's.
CBET_HD double mesh_value(const MeshArgs &a, const double *f, const MeshNode &n)
{
    const double v0 = mesh_shell(a, f, n, n.m0);
    if (n.m1 == n.m0) return v0;
    const double v1 = mesh_shell(a, f, n, n.m1);
    return v0 + (v1 - v0) / n.dr * n.tr;
}

// The node's table entries: ne and Te of the mesh, then the absorbed fraction.
CBET_HD void mesh_tables(const MeshArgs &a, const MeshNode &n, double &ed, double &kap)
{
    ed = mesh_value(a, a.ne, n);
    kap = kappa(ed, mesh_value(a, a.te, n), a.ncrit, a.dt);
}

// The node's flow velocity: the mesh's (ur, utheta, uphi), a NULL component zero, turned into Cartesian components with
// the node's own direction (target_delta's ct, st, c1, s1: (c1, s1) = (1, 0) on the polar axis); zero at the centre.
CBET_HD void mesh_velocity(const MeshArgs &a, const MeshNode &n, double &ux, double &uy, double &uz)
{
    ux = uy = uz = 0.0;
    if (!(n.rho > 0.0)) return;
    const double ur = a.ur ? mesh_value(a, a.ur, n) : 0.0;
    const double uth = a.uth ? mesh_value(a, a.uth, n) : 0.0;
    const double uph = a.uph ? mesh_value(a, a.uph, n) : 0.0;
    const double ct = n.sz / n.rho, st = n.rxy / n.rho;
    double c1 = 1.0, s1 = 0.0;
    if (n.rxy > 0.0) { c1 = n.sx / n.rxy; s1 = n.sy / n.rxy; }
    const double h = ur * st + uth * ct;
    ux = h * c1 - uph * s1;
    uy = h * s1 + uph * c1;
    uz = ur * ct - uth * st;
}

// The node's local plasma state for the gain kernels: Te of the mesh, Ti and Z of the mesh or (NULL arrays) of the gain
// parameters, then the state model (cbet_state_model.h).
CBET_HD void mesh_state(const MeshArgs &a, const MeshNode &n, double &cs, double &gc)
{
    const double te = mesh_value(a, a.te, n);
    const double ti = a.ti ? mesh_value(a, a.ti, n) : a.ti0;
    const double z = a.zbar ? mesh_value(a, a.zbar, n) : a.z0;
    state_model(a.sc, te, ti, z, cs, gc);
}

}  // namespace cbet
#endif
