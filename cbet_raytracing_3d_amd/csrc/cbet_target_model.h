// cbet_target_model.h -- one node of a perturbed target (include/cbet_mi355x.h, "perturbed targets"), written once for
// the gfx950 kernel (cbet_target.hip) and its host twin (cbet_target_host.cpp).  Built with -ffp-contract=off on both
// sides: every operator below is one IEEE fp64 operation, in the order the header fixes, so the two agree bit for bit.
// The includer provides sqrt(double): <hip/hip_runtime.h> in device code, <cmath> on the host.
#ifndef CBET_TARGET_MODEL_H_
#define CBET_TARGET_MODEL_H_

#include "cbet_device.h"

#if defined(__HIP__)
#define CBET_HD __attribute__((host)) __attribute__((device)) __attribute__((always_inline)) inline
#else
#define CBET_HD inline
#endif

namespace cbet {

// interp_table2 of cbet_kernels.hip restated (launch_ray_XZ.cu:16-63: clamped piecewise-linear lookup by bisection, the
// two tables sharing one abscissa).  Restated rather than shared so that k_tabulate's and k_plasma_records' code stays as
// it is.
CBET_HD void target_interp2(const double *y1, const double *y2, const double *x, const double xp, int n, double &o1,
                            double &o2)
{
    const bool ascending = x[0] <= x[n - 1];
    if (ascending ? (xp <= x[0]) : (xp >= x[0])) { o1 = y1[0]; o2 = y2[0]; return; }
    if (ascending ? (xp >= x[n - 1]) : (xp <= x[n - 1])) { o1 = y1[n - 1]; o2 = y2[n - 1]; return; }
    unsigned lo = 0, hi = n - 1, mid = (lo + hi) >> 1;
    while (lo < hi - 1) {
        const bool go_low = ascending ? (x[mid] >= xp) : !(x[mid] <= xp);
        if (go_low) hi = mid; else lo = mid;
        mid = (lo + hi) >> 1;
    }
    const double dx = x[mid + 1] - x[mid], t = xp - x[mid];
    o1 = y1[mid] + (y1[mid + 1] - y1[mid]) / dx * t;
    o2 = y2[mid] + (y2[mid + 1] - y2[mid]) / dx * t;
}

// delta = sum_c c[c] Y_c(s / rho) with the header's recurrence and summation order; L is the instantiation, c holds
// (L + 1)^2 coefficients at least.  F: the factor table (cbet_device.h).  m outermost; per m the Legendre chain runs in
// p1 / p2 and the cos and sin members' sums in A / B: no array indexed by a run-time value, so nothing lands in scratch.
// FP / CP: pointers to double -- plain on the host, constant-address-space ones in the kernel (scalar loads).  pin(F, c, v)
// is called once per m with a value of the m before: arithmetic-free, it is where the kernel keeps the compiler from
// loading every m's factors and coefficients ahead of their use (cbet_target.hip); the host passes TargetNoPin.
struct TargetNoPin {
    template <class FP, class CP>
    CBET_HD void operator()(FP &, CP &, double) const {}
};

template <int L, class FP, class CP, class Pin>
CBET_HD double target_delta(FP F, CP c, double sx, double sy, double sz, double rho, Pin pin)
{
    const double y00 = F[kTfY00];
    if (L == 0 || !(rho > 0.0)) return c[0] * y00;
    const double q2 = F[kTfSqrt2];
    const double rxy = sqrt(sx * sx + sy * sy);
    const double ct = sz / rho, st = rxy / rho;
    double c1 = 1.0, s1 = 0.0;
    if (rxy > 0.0) { c1 = sx / rxy; s1 = sy / rxy; }
    double delta = 0.0, pmm = y00, cr = 1.0, si = 0.0;
#pragma unroll
    for (int m = 0; m <= L; ++m) {
        pin(F, c, delta);
        if (m > 0) {
            pmm = (pmm * F[kTfD + m]) * st;
            const double cn = cr * c1 - si * s1;
            si = cr * s1 + si * c1;
            cr = cn;
        }
        double p1 = pmm, p2 = 0.0;
        double A = c[m * m + m + m] * pmm, B = 0.0;
        if (m > 0) B = c[m * m + m - m] * pmm;
#pragma unroll
        for (int l = m + 1; l <= L; ++l) {
            const double y = F[kTfA + l * kTargetS + m] * (ct * p1 - F[kTfB + l * kTargetS + m] * p2);
            p2 = p1;
            p1 = y;
            A = A + c[l * l + l + m] * y;
            if (m > 0) B = B + c[l * l + l - m] * y;
        }
        if (m == 0) delta = A;
        else delta = delta + ((q2 * cr) * A + (q2 * si) * B);
    }
    return delta;
}

// One node's table entries: node_plasma of cbet_kernels.hip (launch_ray_XZ.cu:296-305) with the radius taken on the
// perturbed target.  F: the factor table, c: the coefficients (a.c), r / ne / te: the profile (LDS in the kernel).
template <int L, class FP, class CP, class Pin>
CBET_HD void target_node(const TargetArgs &a, FP F, CP c, const double *r, const double *ne, const double *te, int i, int j,
                         int k, double &ed, double &kap, Pin pin)
{
    const TabulateArgs &t = a.t;
    const double xc = i * t.dx + t.xmin, yc = j * t.dy + t.ymin, zc = k * t.dz + t.zmin;
    const double sx = xc - a.ox, sy = yc - a.oy, sz = zc - a.oz;
    const double rho = sqrt(sx * sx + sy * sy + sz * sz);
    const double q = 1.0 + target_delta<L>(F, c, sx, sy, sz, rho, pin);
    double rhop = rho;
    if (q != 1.0) rhop = rho / q;                                   // (rho / 1.0 is rho: the division is skipped, not changed)
    double etemp;
    target_interp2(ne, te, r, rhop, t.nprofile, ed, etemp);
    const double eta = 5.2e-5 * 10.0 / (etemp * sqrt(etemp));       // :299
    const double nuei = (1e6 * ed * (kEc * kEc) / kMe) * eta;       // :300
    kap = ed / t.ncrit * nuei * t.dt;                               // :305 up to "* uray"
}

// One node's flow velocity on the target (include/cbet_mi355x.h, "flow table"): target_node's radius statements, then
// cell_state's ramp (cbet_grid_kernels.hip) with rho' in the ramp and s / rho as the direction.  With a zero offset and
// zero coefficients every statement is cell_state's own, in its order.
template <int L, class FP, class CP, class Pin>
CBET_HD void target_flow(const FlowArgs &a, FP F, CP c, int i, int j, int k, double &ux, double &uy, double &uz, Pin pin)
{
    const double xc = i * a.dx + a.xmin, yc = j * a.dy + a.ymin, zc = k * a.dz + a.zmin;
    const double sx = xc - a.ox, sy = yc - a.oy, sz = zc - a.oz;
    const double rho = sqrt(sx * sx + sy * sy + sz * sz);
    const double q = 1.0 + target_delta<L>(F, c, sx, sy, sz, rho, pin);
    double rhop = rho;
    if (q != 1.0) rhop = rho / q;
    double t = (rhop - a.mach_r0) / (a.mach_r1 - a.mach_r0);
    if (t < 0.0) t = 0.0;
    if (t > 1.0) t = 1.0;
    const double um = (a.mach_0 + (a.mach_1 - a.mach_0) * t) * a.cs;
    ux = uy = uz = 0.0;
    if (rho > 0.0) { ux = um * (sx / rho); uy = um * (sy / rho); uz = um * (sz / rho); }
}

}  // namespace cbet
#endif
