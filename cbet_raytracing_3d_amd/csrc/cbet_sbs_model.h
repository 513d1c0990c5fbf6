// cbet_sbs_model.h -- the statements of the backscatter SBS gain spectra along rays (include/cbet_mi355x.h
// cbet_trace_backscatter), each written once for the gfx950 kernel (cbet_backscatter.hip k_trace_backscatter) and the host twin
// (cbet_backscatter_host.cpp).  PARITY UNPINNED, as sections 9 and 23 are: the reference has no such code.
// Built with -ffp-contract=off on both sides: every operator below is one IEEE fp64 operation, in the order written, so the
// kernel and the twin agree bit for bit.  The includer provides sqrt of a double: <hip/hip_runtime.h> or <cmath>.
//
// The model.  Stimulated Brillouin backscatter is the ion-acoustic coupling of the gain stage (cbet_gain_model.h) with the
// ray's own reversed light as the second beam: the ordered pair is (i = the backscattered seed, j = the ray's light as pump),
// its ion-acoustic wave q = k_j - k_i = 2 k_ray, and the seed's frequency shift delta relative to its beam detunes the
// resonance exactly as a beam's colour does (section 19) with dw = w_j - w_i = 0.0 - delta.  Along a ray the convective gain
// exponent of shift m is
//     Gamma_m = sum over the steps, in step order from +0.0, of (g_m * I) * ds
// with the step's displacement d = p_t - p_(t-1) (sbs_step), the deposit-grid cell h of the ray's node after the step
// (sbs_cell), that cell's plasma state and prefactor (cell_state, cell_pref of cbet_gain_model.h, unchanged: the flow table of
// sections 13 / 14 and the state table of section 16 are honoured), g_m the gain stage's own detuned pair gain (sbs_gain) and
// I the beam's own normalised intensity in the cell.
//
// OUT OF SCOPE.  The context's saturation limit, per-beam detuning and line spectrum are NOT applied: the seed's shift is the
// scan variable and the gain is linear.  Left out as well: pump depletion, shared-wave (multi-beam) SBS, sidescatter,
// absorption of the scattered light, and where along the ray the gain accrues -- for that, re-trace chosen rays with the path
// recorder (section 22).  The record carries uray0 and uray_end, so a caller can net the pump's absorption themselves.
#ifndef CBET_SBS_MODEL_H_
#define CBET_SBS_MODEL_H_

#include "cbet_device.h"
#include "cbet_gain_model.h"
#include "cbet_hd.h"

namespace cbet {

// A step's path length and the ion-acoustic wave it drives: with k_ray = (omega / c^2) v and v = d / dt, q = 2 k_ray = qs d,
// qs = ((2.0 * k0) / kC) / dt computed ONCE on the host (sbs_qs) and carried in SbsArgs -- both sides read the same double.
struct SbsStep { double ds; PairWave w; };
inline double sbs_qs(double k0, double dt) { return ((2.0 * k0) / kC) / dt; }
CBET_HD SbsStep sbs_step(double qs, double dx, double dy, double dz)
{
    SbsStep t;
    t.ds = sqrt((dx * dx + dy * dy) + dz * dz);
    t.w.qx = qs * dx; t.w.qy = qs * dy; t.w.qz = qs * dz;
    t.w.kiaw = sqrt((t.w.qx * t.w.qx + t.w.qy * t.w.qy) + t.w.qz * t.w.qz);
    return t;
}

// The deposit-grid cell whose cell_node is exactly node (ci, cj, ck).
CBET_HD long sbs_cell(const GainArgs &a, int ci, int cj, int ck) { return ((long)(ci + 1) * (a.ny + 2) + (cj + 1)) * (a.nz + 2) + (ck + 1); }

// g of one shift: delta is the scattered light's angular-frequency shift relative to its own beam (rad/s, negative = red).
// smoothed: the context's polarization mode; pair_smoothing at cos theta = -1 is 0.25 * (1.0 + 1.0) = 0.5 exactly.
CBET_HD double sbs_gain(const CellState &c, double pref, double iaw2, const PairWave &w, double delta, bool smoothed)
{
    const double dw = 0.0 - delta;
    double g = pair_gain(c, pref, iaw2, w, dw);
    if (smoothed) g = g * 0.5;
    return g;
}

// One step's term of one shift, added in step order.
CBET_HD double sbs_add(double gamma, double g, double I, double ds) { return gamma + (g * I) * ds; }

// The ray's record from its spectrum: the first maximum wins.
CBET_HD void sbs_max(double gamma, int m, double &gmax, int &imax)
{
    if (m == 0 || gamma > gmax) { gmax = gamma; imax = m; }
}

}  // namespace cbet
#endif
