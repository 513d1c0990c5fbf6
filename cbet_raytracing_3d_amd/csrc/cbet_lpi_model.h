// cbet_lpi_model.h -- the statements of the quarter-critical LPI maps, each written once for the gfx950
// kernel (cbet_lpi.hip k_lpi_map) and its host twin (cbet_lpi_host.cpp cbet_lpi_map_host): for a cell of the haloed deposit grid
// inside a density band around n_c / 4, the overlapped intensity of the beams present there (their sum, their maximum, and
// the largest sum over beams that share a cone about the density gradient -- the beams that can drive a common
// electron-plasma wave), the density scale length L_n, and the two-plasmon-decay threshold parameter of Simon et al., Phys.
// Fluids 26, 3107 (1983), eta = I_14 L_um lambda_um / (81.86 T_keV).  No reference counterpart: parity UNPINNED, like the
// whole CBET stage.  Built with -ffp-contract=off on both sides: every operator below is one IEEE fp64 operation, in the order
// written, and there is no trigonometry, no pow and no cbrt, so the kernel and the twin agree bit for bit.  The includer
// provides sqrt of a double: <hip/hip_runtime.h> or <cmath>.
#ifndef CBET_LPI_MODEL_H_
#define CBET_LPI_MODEL_H_

#include "cbet_hd.h"
#include "cbet_mi355x.h"

namespace cbet {

// The argument block of k_lpi_map and of the twin: its own, GainArgs keeps its members and their offsets.
struct LpiArgs {
    int nx, ny, nz, nbeams;
    double dx, dy, dz;
    double ncrit, lambda_um;                // lambda_um: the vacuum wavelength in micrometres (lpi_lambda_um)
    double frac_lo, frac_hi;                // the band of ne / ncrit, both ends included
    double te_ev;                           // the uniform electron temperature in eV, read where te3d is NULL
    int cone_bins;                          // NB, 1 .. CBET_LPI_MAX_BINS
    int hx_lo, hx_hi;                       // planes [hx_lo, hx_hi) of the haloed grid
    long hsize;                             // (nx+2)(ny+2)(nz+2): entries per beam of `fields`, per quantity of `lpi`
    const double *fields;                   // [4][nbeams][hsize] NORMALISED (I, kx, ky, kz), read only
    const double *ne3d, *te3d;              // [nx][ny][nz] node tables; te3d may be NULL
    double *lpi;                            // [CBET_LPI_NQ][hsize]
};

// Deposit-grid cell h = ((hi * (ny+2)) + hj) * (nz+2) + hk takes its plasma from node (hi-1, hj-1, hk-1), clamped: the
// statements of cbet_gain_model.h's cell_node on this block.
CBET_HD void lpi_cell_node(const LpiArgs &a, long h, int &i, int &j, int &k)
{
    const int sYh = a.nz + 2;
    const long sXh = (long)(a.ny + 2) * sYh;
    const int hi = (int)(h / sXh);
    const int rem = (int)(h - hi * sXh);
    const int hj = rem / sYh, hk = rem - hj * sYh;
    i = hi < 1 ? 0 : (hi > a.nx ? a.nx - 1 : hi - 1);
    j = hj < 1 ? 0 : (hj > a.ny ? a.ny - 1 : hj - 1);
    k = hk < 1 ? 0 : (hk > a.nz ? a.nz - 1 : hk - 1);
}

// The band: frac_lo <= ne / ncrit <= frac_hi.
CBET_HD bool lpi_in_band(const LpiArgs &a, double frac) { return a.frac_lo <= frac && frac <= a.frac_hi; }

// The density gradient along one axis at node c of n, `at` the node's index into ne and `stride` the axis' stride in doubles:
// (ne[c + p] - ne[c + m]) / (2.0 d) with (m, p) the project's face rule (cbet_trace_common.h face_pair: this -+ 1, one-sided
// on the faces, 0 -> (0, 2) and n-1 -> (n-3, n-1), also two spacings apart).  An axis of fewer than 3 nodes has no gradient.
CBET_HD double lpi_axis_gradient(const double *ne, long at, int c, int n, long stride, double d)
{
    if (n < 3) return 0.0;
    const long m = (c == 0) ? 0 : ((c == n - 1) ? -2 * stride : -stride);
    const long p = (c == 0) ? 2 * stride : ((c == n - 1) ? 0 : stride);
    return (ne[at + p] - ne[at + m]) / (2.0 * d);
}

// A band cell's plasma: the gradient at its node, its norm (squares summed x, y, z), the scale length ne / |grad ne| in cm (0
// where the gradient vanishes) and the threshold factor T with eta_x = (I_x * 1e-14) * T.
struct LpiPlasma { double gx, gy, gz, gn, Ln, T; };
CBET_HD double lpi_threshold(const LpiArgs &a, double Ln, double te)
{
    if (!(te > 0.0) || Ln == 0.0) return 0.0;
    return ((Ln * 1e4) * a.lambda_um) / (81.86 * (te * 1e-3));
}
CBET_HD LpiPlasma lpi_plasma(const LpiArgs &a, int i, int j, int k, double ne)
{
    const long node = ((long)i * a.ny + j) * a.nz + k;
    LpiPlasma q;
    q.gx = lpi_axis_gradient(a.ne3d, node, i, a.nx, (long)a.ny * a.nz, a.dx);
    q.gy = lpi_axis_gradient(a.ne3d, node, j, a.ny, (long)a.nz, a.dy);
    q.gz = lpi_axis_gradient(a.ne3d, node, k, a.nz, 1L, a.dz);
    q.gn = sqrt(q.gx * q.gx + q.gy * q.gy + q.gz * q.gz);
    q.Ln = q.gn == 0.0 ? 0.0 : ne / q.gn;
    q.T = lpi_threshold(a, q.Ln, a.te3d ? a.te3d[node] : a.te_ev);
    return q;
}

// One beam in a band cell.  Present: I > 0 and |k| > 0 (squares summed x, y, z).  The cone bin of a present beam: the cosine of
// its angle with the density gradient, mu = ((kx gx + ky gy) + kz gz) / (kn gn) clamped to [-1, 1] (1 where the gradient
// vanishes), cut into NB equal steps of mu from 1 down: bin = min(NB - 1, (int)((1.0 - mu) * (0.5 * NB))).
CBET_HD double lpi_knorm(double kx, double ky, double kz) { return sqrt(kx * kx + ky * ky + kz * kz); }
CBET_HD bool lpi_present(double I, double kn) { return I > 0.0 && kn > 0.0; }
CBET_HD int lpi_bin(const LpiPlasma &q, double kx, double ky, double kz, double kn, int nbins)
{
    double mu = 1.0;
    if (q.gn != 0.0) {
        mu = ((kx * q.gx + ky * q.gy) + kz * q.gz) / (kn * q.gn);
        if (!(mu <= 1.0)) mu = 1.0;
        if (mu < -1.0) mu = -1.0;
    }
    const int bin = (int)((1.0 - mu) * (0.5 * nbins));
    return bin < nbins - 1 ? bin : nbins - 1;
}

// What a cell's beam loop leaves (beams in increasing order, every sum in that order) and the cell's seven quantities from
// it: out-of-band cells hold 0.0 everywhere.  Icw: the largest bin sum.  eta_max is the summary's only, not a map quantity.
struct LpiCell { double Isum, Icw, Imax; int npresent; };
CBET_HD double lpi_eta(double I, double T) { return (I * 1e-14) * T; }
CBET_HD void lpi_store(const LpiArgs &a, long h, bool band, const LpiCell &c, const LpiPlasma &q)
{
    double *o = a.lpi + h;
    o[CBET_LPI_BAND * a.hsize] = band ? 1.0 : 0.0;
    o[CBET_LPI_I_SUM * a.hsize] = band ? c.Isum : 0.0;
    o[CBET_LPI_I_CW * a.hsize] = band ? c.Icw : 0.0;
    o[CBET_LPI_I_MAX * a.hsize] = band ? c.Imax : 0.0;
    o[CBET_LPI_LN * a.hsize] = band ? q.Ln : 0.0;
    o[CBET_LPI_ETA_SUM * a.hsize] = band ? lpi_eta(c.Isum, q.T) : 0.0;
    o[CBET_LPI_ETA_CW * a.hsize] = band ? lpi_eta(c.Icw, q.T) : 0.0;
}

// The summary (cbet_lpi_summary): one band cell merged in, and one summary merged into another -- counts and sums add, maxima
// take the maximum, argmax_cw follows max_eta_cw (the lowest cell index among ties; -1 = no band cell yet).  The kernel's
// lanes, wavefronts and workgroups and the twin's cells merge through the same two functions.
CBET_HD void lpi_summary_clear(cbet_lpi_summary &s)
{
    s.band_cells = s.lit_cells = s.above_max = s.above_cw = s.above_sum = 0;
    s.argmax_cw = -1;
    s.max_eta_max = s.max_eta_cw = s.max_eta_sum = 0.0;
    s.sum_I_sum = s.sum_I_cw = 0.0;
    s.max_present = 0;
    s.reserved = 0;
}
CBET_HD void lpi_summary_argmax(cbet_lpi_summary &s, double eta, long long h)
{
    if (h < 0) return;
    if (s.argmax_cw < 0 || eta > s.max_eta_cw || (eta == s.max_eta_cw && h < s.argmax_cw)) s.argmax_cw = h;
}
CBET_HD void lpi_summary_cell(cbet_lpi_summary &s, long h, const LpiCell &c, const LpiPlasma &q)
{
    const double es = lpi_eta(c.Isum, q.T), ec = lpi_eta(c.Icw, q.T), em = lpi_eta(c.Imax, q.T);
    s.band_cells += 1;
    s.lit_cells += c.npresent >= 1 ? 1 : 0;
    s.above_max += em >= 1.0 ? 1 : 0;
    s.above_cw += ec >= 1.0 ? 1 : 0;
    s.above_sum += es >= 1.0 ? 1 : 0;
    lpi_summary_argmax(s, ec, h);            // before max_eta_cw moves
    if (em > s.max_eta_max) s.max_eta_max = em;
    if (ec > s.max_eta_cw) s.max_eta_cw = ec;
    if (es > s.max_eta_sum) s.max_eta_sum = es;
    s.sum_I_sum = s.sum_I_sum + c.Isum;
    s.sum_I_cw = s.sum_I_cw + c.Icw;
    if (c.npresent > s.max_present) s.max_present = c.npresent;
}
CBET_HD void lpi_summary_merge(cbet_lpi_summary &s, const cbet_lpi_summary &t)
{
    s.band_cells += t.band_cells;
    s.lit_cells += t.lit_cells;
    s.above_max += t.above_max;
    s.above_cw += t.above_cw;
    s.above_sum += t.above_sum;
    lpi_summary_argmax(s, t.max_eta_cw, t.argmax_cw);
    if (t.max_eta_max > s.max_eta_max) s.max_eta_max = t.max_eta_max;
    if (t.max_eta_cw > s.max_eta_cw) s.max_eta_cw = t.max_eta_cw;
    if (t.max_eta_sum > s.max_eta_sum) s.max_eta_sum = t.max_eta_sum;
    s.sum_I_sum = s.sum_I_sum + t.sum_I_sum;
    s.sum_I_cw = s.sum_I_cw + t.sum_I_cw;
    if (t.max_present > s.max_present) s.max_present = t.max_present;
}

}  // namespace cbet
#endif
