// cbet_gain_model.h -- the statements of the CBET gain stage (DESIGN.md sections 9, 16, 17), each written once for the gfx950
// kernels (cbet_grid_kernels.hip) and the host twin of the exchange matrix (cbet_exchange_host.cpp): a deposit-grid cell's
// plasma state, the prefactor and the saturation limit that follow from it, and the gain of an ORDERED beam pair with its
// clamp.  The pair-once kernels' fast pair function (pair_gain_fast, saturate_fast) is device-only and stays with them.
// Built with -ffp-contract=off on both sides: every operator below is one IEEE fp64 operation, in the order written, so a
// kernel and the twin agree bit for bit.  The includer provides sqrt and fabs of a double: <hip/hip_runtime.h> or <cmath>.
#ifndef CBET_GAIN_MODEL_H_
#define CBET_GAIN_MODEL_H_

#include "cbet_device.h"
#include "cbet_hd.h"
#include "cbet_node_model.h"

namespace cbet {

struct CellState {
    double frac, eps, rt, ux, uy, uz;   // ne/ncrit, 1 - ne/ncrit, sqrt(eps), flow velocity
    double cs, gc;                      // sound speed and gain_const: the node's (state table) or the uniform ones
};

// Deposit-grid cell h = ((hi * (ny+2)) + hj) * (nz+2) + hk takes its plasma state from node (hi-1, hj-1, hk-1), clamped.
CBET_HD void cell_node(const GainArgs &a, long h, int &i, int &j, int &k)
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

// FLOW: the flow velocity is read from GainArgs.flow (a node table, cbet_target.hip k_tabulate_flow) instead of the closed-form
// radial ramp about the origin.  STATE: the sound speed and gain_const are read from GainArgs.state (a node table,
// cbet_mesh.hip k_mesh_state) instead of the uniform GainArgs.cs / gain_const.  Template arguments, the kernels' own: as plain
// bool parameters the same statements compile to other code in the pair-once kernels, whose register budget is spent.
template <bool FLOW, bool STATE>
CBET_HD CellState cell_state(const GainArgs &a, long h)
{
    int i, j, k;
    cell_node(a, h, i, j, k);
    CellState c;
    c.frac = a.ne3d[((long)i * a.ny + j) * a.nz + k] / a.ncrit;
    c.eps = 1.0 - c.frac;
    c.rt = c.eps > 0.0 ? sqrt(c.eps) : 0.0;
    if (STATE) {
        const long nodes = (long)a.nx * a.ny * a.nz, node = ((long)i * a.ny + j) * a.nz + k;
        c.cs = a.state[node];
        c.gc = a.state[node + nodes];
    } else {
        c.cs = a.cs;
        c.gc = a.gain_const;
    }
    if (FLOW) {
        const long nodes = (long)a.nx * a.ny * a.nz, node = ((long)i * a.ny + j) * a.nz + k;
        c.ux = a.flow[node];
        c.uy = a.flow[node + nodes];
        c.uz = a.flow[node + 2 * nodes];
        return c;
    }
    double xc, yc, zc, rr;                                            // the sphere about the origin: no offset, rho' == rho
    node_centre(a, i, j, k, 0.0, 0.0, 0.0, xc, yc, zc, rr);
    radial_flow(a, rr, rr, xc, yc, zc, c.ux, c.uy, c.uz);
    return c;
}
// ... chosen at run time by the tables the block carries (the host twin).
CBET_HD CellState cell_state(const GainArgs &a, long h)
{
    if (a.flow) return a.state ? cell_state<true, true>(a, h) : cell_state<true, false>(a, h);
    return a.state ? cell_state<false, true>(a, h) : cell_state<false, false>(a, h);
}

// The prefactor of a cell's pair gains, gain_const (ne / ncrit) / (iaw sqrt(eps)); zero at and above critical density.
CBET_HD double cell_pref(const GainArgs &a, const CellState &c) { return c.eps > 0.0 ? c.gc * c.frac * (1.0 / a.iaw) / c.rt : 0.0; }

// Saturation of the ion-acoustic wave.  Scattering off a grating of relative amplitude dn/n exchanges
// intensity at the rate kap (dn/n) sqrt(Ii Ij), kap = (k0 / 2) (ne / ncrit) / sqrt(eps); the amplitude this model's pair gain
// corresponds to is therefore |G_ij| sqrt(Ii Ij) / kap.  cell_sat_limit: the value w = |G_ij| sqrt(Ii Ij) may reach under
// the limit dn_max; zero at and above critical density, where the gain is zero too.
CBET_HD double cell_kap(const GainArgs &a, const CellState &c) { return c.eps > 0.0 ? ((0.5 * a.k0) * c.frac) / c.rt : 0.0; }
CBET_HD double cell_sat_limit(const GainArgs &a, const CellState &c) { return a.sat * cell_kap(a, c); }

// One beam's normalised entry of a cell, and the ion-acoustic wave of the ordered pair (i, j): q = k_j - k_i and |q|.
struct BeamAtCell { double I, kx, ky, kz; };
struct PairWave { double qx, qy, qz, kiaw; };
CBET_HD BeamAtCell beam_at(const double *fI, const double *fx, const double *fy, const double *fz, long o) { return {fI[o], fx[o], fy[o], fz[o]}; }
CBET_HD PairWave pair_wave(const BeamAtCell &bi, const BeamAtCell &bj)
{
    PairWave w;
    w.qx = bj.kx - bi.kx; w.qy = bj.ky - bi.ky; w.qz = bj.kz - bi.kz;
    w.kiaw = sqrt(w.qx * w.qx + w.qy * w.qy + w.qz * w.qz);
    return w;
}
// Both beams are present in the cell and not parallel: the pair exchanges something.
CBET_HD bool pair_present(const BeamAtCell &bi, const BeamAtCell &bj, const PairWave &w) { return bi.I > 0.0 && bj.I > 0.0 && w.kiaw > 0.0; }
// G_ij = pref P(eta_ij) of a present pair, iaw2 = iaw^2; G_ji = -G_ij exactly (q and with it eta change sign, P is odd).
CBET_HD double pair_gain(const CellState &c, double pref, double iaw2, const PairWave &w)
{
    const double eta = (0.0 - (w.qx * c.ux + w.qy * c.uy + w.qz * c.uz)) / (w.kiaw * c.cs + 1e-10);
    const double e2 = eta * eta;
    const double P = iaw2 * eta / ((e2 - 1.0) * (e2 - 1.0) + iaw2 * e2);
    return pref * P;
}
// Wavelength detuning.  Beam b's angular frequency is omega + w_b (rad/s), omega the nominal one of
// cbet_derive; the ion-acoustic wave of the ordered pair (i, j) is driven at the beat frequency, so the Doppler term of the
// resonance gains dw = w_j - w_i:  eta_ij = ((0.0 - q . u) + (w_j - w_i)) / (|q| cs + 1e-10).  Beam i gains where its
// frequency in the plasma frame is the lower one: in still plasma the red-shifted beam gains.  (w_i - w_j) = -(w_j - w_i)
// exactly, so G_ji = -G_ij stays exact and a cell's exchange sum_i I_i K_i still cancels; dw = 0 adds an exact zero.  Only
// the beat frequency enters: each beam's own k0, ncrit and refraction keep the nominal wavelength (relative change ~1e-3),
// and the Manley-Rowe photon-number correction of the same order is left out.  pair_present is unchanged: two exactly
// parallel beams exchange nothing, detuned or not.
// pair_resonance: P(eta), the statements pair_gain above runs after its eta, for the detuned form.
CBET_HD double pair_resonance(double eta, double iaw2)
{
    const double e2 = eta * eta;
    return iaw2 * eta / ((e2 - 1.0) * (e2 - 1.0) + iaw2 * e2);
}
CBET_HD double pair_gain(const CellState &c, double pref, double iaw2, const PairWave &w, double dw)
{
    const double eta = ((0.0 - (w.qx * c.ux + w.qy * c.uy + w.qz * c.uz)) + dw) / (w.kiaw * c.cs + 1e-10);
    return pref * pair_resonance(eta, iaw2);
}
// Polarization smoothing.  Every beam is an equal, incoherent mix of two orthogonal polarizations (a
// distributed polarization rotator on every beam); two such beams crossing at the angle theta exchange (1 + cos^2 theta) / 4
// of what two beams polarized alike do.  In a cell a present pair has |k_i| = |k_j| = kmag = k0 sqrt(eps), the value the
// normalisation wrote (a.k0 * c.rt), so
//     cth = ((k_i.x k_j.x + k_i.y k_j.y) + k_i.z k_j.z) / (kmag kmag),    f = 0.25 (1.0 + cth cth),    g = (pref P(eta)) f
// with f between 1/4 (beams at right angles) and 1/2 (parallel or opposed).  The products commute and the sum keeps its order,
// so f is the same bits for (i, j) and (j, i): G_ji = -G_ij stays exact and a cell's exchange still cancels.  The factor
// multiplies the gain BEFORE the clamp -- this model's choice: the clamp, pair_swing, the amplitude map and the exchange matrix
// see f G_ij, and the ion-acoustic amplitude reported is that of the pair's total exchange, not of the s-s and p-p gratings
// separately.  eta is untouched, so detuning composes unchanged; pair_present is unchanged (such a pair has eps > 0, so
// kmag kmag > 0).  Left out: linearly polarized beams with per-beam polarization vectors ((e_i . e_j)^2) and the spatial offset
// between a rotator's two sub-beams.
CBET_HD double pair_smoothing(const BeamAtCell &bi, const BeamAtCell &bj, double kmag)
{
    const double cth = ((bi.kx * bj.kx + bi.ky * bj.ky) + bi.kz * bj.kz) / (kmag * kmag);
    return 0.25 * (1.0 + cth * cth);
}
// Laser bandwidth.  Every beam carries the SAME spectrum about its own centre frequency omega + w_b: L
// lines with offsets o_a (rad/s) and weights p_a > 0, sum p_a = 1.  The lines are mutually incoherent (line spacing >> the
// ion-acoustic damping rate): line a of beam i and line b of beam j drive their own grating at the beat
// (w_j - w_i) + (o_b - o_a), and the pair gain is the weighted sum of their resonances,
//     G_ij = pref sum_a sum_b p_a p_b P((N + (o_b - o_a)) / D),    N = (0.0 - q . u) + (w_j - w_i),    D = |q| cs + 1e-10.
// The spectrum is shared, so the double sum collapses onto its autocorrelation, the difference table `band` of M entries
// (GainArgs.band, built by band_table): c_0 = sum p_a^2, and per entry d_m > 0 with c_m = sum_{a < b, |o_b - o_a| = d_m} p_a p_b:
//     S = c_0 P(N / D)
//     for m = 0 .. M-1:   S = S + c_m (P((N + d_m) / D) + P((N - d_m) / D))
//     g = pref S          then the factor f (section 20), then the clamp (section 17), as without a spectrum.
// N -> -N exactly for (j, i), (-N + d) = -(N - d) exactly, P is odd and the bracket is one commutative add: G_ji = -G_ij stays
// exact and a cell's exchange still cancels.  Still plasma without shifts has N = 0, every bracket is P(d / D) + P(-(d / D)) = 0
// and S = 0 exactly: bandwidth alone transfers nothing, it only smears a resonance that flow or detuning creates.  Far off
// resonance (d_m >> |q| cs) only the centre term survives: G -> c_0 G_mono, 1/L for L equal lines.  M = 0 is no table at all
// (one line, or equal offsets): the forms above run.  The field model keeps ONE intensity per beam: the spectral shape is not
// changed by the exchange (no per-line depletion).  The clamp sees the SUMMED pair gain, and the amplitude map reports the
// amplitude of the pair's total exchange, not of one line pair's grating -- section 20's choice.  Left out: per-beam spectra,
// per-line fields or depletion, coherent or FM (SSD phase-modulated) spectra, any effect on refraction, ncrit or k0.
CBET_HD double pair_gain_band(const CellState &c, double pref, double iaw2, const PairWave &w, double dw, const double *band, int nband)
{
    const double N = (0.0 - (w.qx * c.ux + w.qy * c.uy + w.qz * c.uz)) + dw;
    const double D = w.kiaw * c.cs + 1e-10;
    double S = band[0] * pair_resonance(N / D, iaw2);
    for (int m = 0; m < nband; ++m) {
        const double d = band[1 + 2 * m];
        S = S + band[2 + 2 * m] * (pair_resonance((N + d) / D, iaw2) + pair_resonance((N - d) / D, iaw2));
    }
    return pref * S;
}
// The clamp: g scaled by min(1, lim / w), w = |g| sqrt(Ii Ij) (pair_swing) -- one factor for (i, j) and (j, i); a
// pair below the limit keeps its bits.
CBET_HD double pair_swing(double g, double Ii, double Ij) { return fabs(g) * sqrt(Ii * Ij); }
CBET_HD double pair_clamp(double g, double Ii, double Ij, double lim)
{
    const double w = pair_swing(g, Ii, Ij);
    if (w > lim) g = g * (lim / w);
    return g;
}

}  // namespace cbet
#endif
