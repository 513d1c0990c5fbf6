// cbet_mesh_deposit_model.h -- the samples of one node of a deposit grid and the spherical-polar cell each of them lies in
// (include/cbet_mi355x.h, "deposit on the hydro mesh"), written once for the gfx950 kernel
// (cbet_mesh_deposit.hip) and its host twin (cbet_mesh_deposit_host.cpp).
// Built with -ffp-contract=off on both sides: every operator below is one IEEE fp64 operation, in the order the header
// fixes.  The includer provides sqrt(double) and fabs(double): <hip/hip_runtime.h> in device code, <cmath> on the host.
// Both are correctly rounded / exact on either side and nothing else is called, so the two sides find the same cell for
// every sample, bit for bit.
//
// Degenerate samples.  rho == 0: row 0, column 0.  On the polar axis (|sx| + |sy| == 0, rho > 0): d = 0, the column that
// holds phi = 0, and row 0 above the centre, the last row below.  sy == -0.0 counts as sy >= 0.
//
// Bounds.  The three searches return indices inside [0, nr), [0, nth) and [0, nph) whatever the tables and the sample hold,
// NaN included: every comparison with a NaN is false, and a false comparison only moves a search's upper end down.  A
// NaN or infinite rho fails the shell test and the sample is outside (-1).
#ifndef CBET_MESH_DEPOSIT_MODEL_H_
#define CBET_MESH_DEPOSIT_MODEL_H_

#include "cbet_device.h"
#include "cbet_hd.h"

namespace cbet {

// One coordinate of a sample relative to the centre: node N of the haloed axis, offset `off` (in cells), centre o.
CBET_HD double deposit_coord(int N, double d, double mn, double off, double o)
{
    const double xs = ((N - 1) * d + mn) + off * d;
    return xs - o;
}

// The last k in [0, n) with x[k] <= v, 0 if there is none.  n >= 1.
CBET_HD int deposit_last_le(const double *x, int n, double v)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (x[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// The "diamond angle" of (sx, sy): in [0, 4), ascending with atan2(sy, sx) taken from 0 round to 2 pi; 0 for (0, 0).
CBET_HD double deposit_diamond(double sx, double sy)
{
    const double a = fabs(sx) + fabs(sy);
    if (a == 0.0) return 0.0;
    const double t = sx / a;
    return (sy >= 0.0) ? 1.0 - t : 3.0 + t;
}

// The column of the direction (sx, sy): it does not depend on sz, so the samples of one (a, b) pair share it.
CBET_HD int deposit_column(const double *pe, int nph, double sx, double sy)
{
    if (nph == 1) return 0;
    double d = deposit_diamond(sx, sy);
    if (d < pe[0]) d = d + 4.0;
    return deposit_last_le(pe, nph, d);
}

// The row of a sample with rho > 0: the number of interior theta edges e (nth - 1 of them, ct descending) with c <= ct[e].
CBET_HD int deposit_row(const double *ct, int nth, double sz, double rho)
{
    const double c = sz / rho;
    int lo = 0, hi = nth - 1;                // the count lies in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (c <= ct[mid]) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The cell (m * nth + row) * nph + column of the sample (sx, sy, sz), q = sx*sx + sy*sy, whose direction has column `col`;
// -1: in no shell.
CBET_HD int deposit_cell(const MeshDepositArgs &a, const double *re, const double *ct, double q, double sz, int col)
{
    const double rho = sqrt(q + sz * sz);
    if (!(re[0] <= rho && rho < re[a.nr])) return -1;
    const int m = deposit_last_le(re, a.nr, rho);
    if (rho == 0.0) return m * a.nth * a.nph;
    return (m * a.nth + deposit_row(ct, a.nth, sz, rho)) * a.nph + col;
}

// The S^3 samples of node (I, J, K) of the haloed grid in (a, b, c) order, c fastest: each(cell) once per sample.
// re / ct / pe / off: the handle's tables (LDS in the kernel).
template <class Each>
CBET_HD void deposit_samples(const MeshDepositArgs &a, const double *re, const double *ct, const double *pe,
                             const double *off, int I, int J, int K, Each each)
{
    for (int sa = 0; sa < a.S; ++sa) {
        const double sx = deposit_coord(I, a.dx, a.xmin, off[sa], a.ox);
        for (int sb = 0; sb < a.S; ++sb) {
            const double sy = deposit_coord(J, a.dy, a.ymin, off[sb], a.oy);
            const double q = sx * sx + sy * sy;
            const int col = deposit_column(pe, a.nph, sx, sy);
            for (int sc = 0; sc < a.S; ++sc) {
                const double sz = deposit_coord(K, a.dz, a.zmin, off[sc], a.oz);
                each(deposit_cell(a, re, ct, q, sz, col));
            }
        }
    }
}

}  // namespace cbet
#endif
