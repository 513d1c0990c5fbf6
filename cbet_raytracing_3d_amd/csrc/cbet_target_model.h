// cbet_target_model.h -- one node of a perturbed target (include/cbet_mi355x.h, "perturbed targets"), written once for
// the gfx950 kernels (cbet_target.hip) and their host twins (cbet_target_host.cpp) over the shared node statements
// (cbet_node_model.h).  Built with -ffp-contract=off on both sides: every operator below is one IEEE fp64 operation, in the
// order the header fixes, so the two agree bit for bit.  The includer provides sqrt(double): <hip/hip_runtime.h> in device
// code, <cmath> on the host.
#ifndef CBET_TARGET_MODEL_H_
#define CBET_TARGET_MODEL_H_

#include "cbet_device.h"
#include "cbet_node_model.h"

namespace cbet {

// The instantiations of target_delta: f(LmaxTag<L>()) for the one target_check chose, false if inst is none of them.
template <int L>
struct LmaxTag {
    static constexpr int value = L;
};
template <class F>
bool dispatch_lmax(int inst, F f)
{
    switch (inst) {
    case 0: f(LmaxTag<0>()); return true;
    case 2: f(LmaxTag<2>()); return true;
    case 8: f(LmaxTag<8>()); return true;
    case 16: f(LmaxTag<16>()); return true;
    }
    return false;
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

// The node's radius on the perturbed target: rho / (1 + delta).
template <int L, class FP, class CP, class Pin>
CBET_HD double target_radius(FP F, CP c, double sx, double sy, double sz, double rho, Pin pin)
{
    const double q = 1.0 + target_delta<L>(F, c, sx, sy, sz, rho, pin);
    double rhop = rho;
    if (q != 1.0) rhop = rho / q;                                   // (rho / 1.0 is rho: the division is skipped, not changed)
    return rhop;
}

// One node's table entries: the plain tabulation's statements (launch_ray_XZ.cu:296-305) with the radius taken about the
// target's centre, on the perturbed target.  F: the factor table, c: the coefficients (a.c), r / ne / te: the profile (LDS
// in the kernel).
template <int L, class FP, class CP, class Pin>
CBET_HD void target_node(const TargetArgs &a, FP F, CP c, const double *r, const double *ne, const double *te, int i, int j,
                         int k, double &ed, double &kap, Pin pin)
{
    double sx, sy, sz, rho, etemp;
    node_centre(a.t, i, j, k, a.ox, a.oy, a.oz, sx, sy, sz, rho);
    const double rhop = target_radius<L>(F, c, sx, sy, sz, rho, pin);
    interp2(ne, te, r, rhop, a.t.nprofile, ed, etemp);
    kap = kappa(ed, etemp, a.t.ncrit, a.t.dt);
}

// One node's flow velocity on the target (include/cbet_mi355x.h, "flow table"): target_node's radius, then the Mach ramp
// of the gain kernels' cell state with rho' in the ramp and s / rho as the direction.  With a zero offset and zero
// coefficients every statement is cell_state's own (cbet_grid_kernels.hip), in its order.
template <int L, class FP, class CP, class Pin>
CBET_HD void target_flow(const FlowArgs &a, FP F, CP c, int i, int j, int k, double &ux, double &uy, double &uz, Pin pin)
{
    double sx, sy, sz, rho;
    node_centre(a, i, j, k, a.ox, a.oy, a.oz, sx, sy, sz, rho);
    radial_flow(a, target_radius<L>(F, c, sx, sy, sz, rho, pin), rho, sx, sy, sz, ux, uy, uz);
}

}  // namespace cbet
#endif
