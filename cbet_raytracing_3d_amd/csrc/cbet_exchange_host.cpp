// cbet_exchange_host.cpp -- the host twin of the pairwise exchange matrix (include/cbet_mi355x.h cbet_exchange_matrix_host;
// DESIGN.md section 18): one loop over the haloed cells in index order running the ORDERED gain kernel's statements, which
// are cbet_gain_model.h's for k_gain_field and for this file alike (cell_state, cell_pref, cell_sat_limit, pair_gain,
// pair_clamp), on an argument block filled by the kernels' own builder (gain_args) -- one IEEE operation per written
// operator, the library is built with -ffp-contract=off -- with every pair's two sums compensated (Neumaier).
// No HIP call: it is the reference of the device path at any size.  cbet_exchange_matrix_host_shifted is the twin with per-beam
// frequency shifts, cbet_exchange_matrix_host_polarized the one with a polarization mode on top (section
// 20), cbet_exchange_matrix_host_banded the one with a line spectrum on top of that (section 21): the loop itself, its options
// in the kernels' GainOptions record (cbet_host_internal.h).  The argument builder the kernels and the twin share (gain_args) and
// the builder of the spectrum's difference table (band_table), which the twin and the context share, live here too.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "cbet_gain_model.h"
#include "cbet_host_internal.h"

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

}  // namespace
}  // namespace cbet

// The argument block of the gain kernels, of k_pair_amplitude, of k_exchange_matrix and of the twin below (cbet_host_internal.h):
// here, beside the twin, so that the twin links without the HIP runtime.
cbet::GainArgs cbet::gain_args(const cbet_params *p, const cbet_derived &d, const cbet_gain_params *g, double cs, double gc,
                               const double *fields, const double *ne3d, const GainOptions &o, int hx_lo, int hx_hi, bool packed)
{
    GainArgs a{};
    grid_args(a, p, d);
    a.nbeams = p->nbeams; a.dt = d.dt;
    a.ncrit = d.ncrit; a.k0 = d.omega / kC;
    ramp_args(a, g, cs);
    a.gain_const = gc; a.iaw = g->iaw; a.relax = g->relax;
    a.fields = const_cast<double *>(fields); a.ne3d = ne3d; a.flow = o.flow; a.state = o.state; a.sat = o.sat; a.shift = o.shift;
    a.pol = o.pol; a.band = o.band; a.nband = o.band ? o.nband : 0;
    a.hx_lo = hx_lo; a.hx_hi = hx_hi;
    const long plane = (long)(p->ny + 2) * (p->nz + 2);
    a.store0 = packed ? (long)hx_lo * plane : 0;
    a.bstride = packed ? (long)(hx_hi - hx_lo) * plane : d.edep_size;
    return a;
}

// The lines of a spectrum as the caller gives them: what cbet_context_set_bandwidth and the banded twin refuse, by one text.
int cbet::band_check(const char *who, const double *line_domega, const double *line_weight, int nlines)
{
    if (nlines < 0) return fail(CBET_EINVAL, "%s: nlines = %d is negative (0 = no spectrum)", who, nlines);
    if (nlines > CBET_MAX_BAND_LINES) return fail(CBET_EINVAL, "%s: nlines = %d exceeds CBET_MAX_BAND_LINES = %d", who, nlines, CBET_MAX_BAND_LINES);
    if (nlines == 0 || (!line_domega && !line_weight)) return CBET_OK;
    if (!line_domega) return fail(CBET_EINVAL, "%s: line_domega is NULL but line_weight is not (both, or neither = no spectrum)", who);
    if (!line_weight) return fail(CBET_EINVAL, "%s: line_weight is NULL but line_domega is not (both, or neither = no spectrum)", who);
    for (int a = 0; a < nlines; ++a) {
        if (std::isnan(line_domega[a])) return fail(CBET_EINVAL, "%s: line_domega[%d] is NaN (finite offsets in rad/s)", who, a);
        if (std::isinf(line_domega[a])) return fail(CBET_EINVAL, "%s: line_domega[%d] is infinite (finite offsets in rad/s)", who, a);
        if (!std::isfinite(line_weight[a]) || !(line_weight[a] > 0.0))
            return fail(CBET_EINVAL, "%s: line_weight[%d] = %g is not finite and > 0", who, a, line_weight[a]);
    }
    return CBET_OK;
}

// The difference table of a line spectrum (GainArgs.band; cbet_gain_model.h pair_gain_band), deterministic:
//   * the weights are normalised, p_a = w_a / (w_0 + w_1 + ...), the sum taken in line order (norm[] receives them);
//   * c_0 = p_0 p_0 + p_1 p_1 + ..., in line order;
//   * the differences |o_b - o_a| in fp64 for a < b, a ascending and b ascending inside a, each with p_a p_b; a difference of
//     exactly zero (two lines at one offset) adds 2 p_a p_b to c_0; bitwise-equal differences are merged, their weights added
//     in the order met;
//   * the entries are sorted by d, ascending.
// table holds 1 + 2 M doubles {c_0, d_0, c_0', d_1, c_1', ...}; returns M (0: one line, or all offsets equal -- no spectrum).
int cbet::band_table(const double *line_domega, const double *line_weight, int nlines, double *table, double *norm)
{
    double p[CBET_MAX_BAND_LINES], sum = 0.0;
    for (int a = 0; a < nlines; ++a) sum = sum + line_weight[a];
    for (int a = 0; a < nlines; ++a) p[a] = line_weight[a] / sum;
    if (norm) std::memcpy(norm, p, (size_t)nlines * sizeof(double));
    double c0 = 0.0, d[kBandMax], c[kBandMax];
    int M = 0;
    for (int a = 0; a < nlines; ++a) c0 = c0 + p[a] * p[a];
    for (int a = 0; a < nlines; ++a)
        for (int b = a + 1; b < nlines; ++b) {
            const double diff = std::fabs(line_domega[b] - line_domega[a]), w = p[a] * p[b];
            if (diff == 0.0) { c0 = c0 + (w + w); continue; }
            int m = 0;
            while (m < M && d[m] != diff) ++m;
            if (m == M) { d[M] = diff; c[M] = w; ++M; }
            else c[m] = c[m] + w;
        }
    int order[kBandMax];
    for (int m = 0; m < M; ++m) order[m] = m;
    std::sort(order, order + M, [&](int x, int y) { return d[x] < d[y]; });   // the differences are distinct
    table[0] = c0;
    for (int m = 0; m < M; ++m) { table[1 + 2 * m] = d[order[m]]; table[2 + 2 * m] = c[order[m]]; }
    return M;
}

int cbet::slab_check(const char *who, int hx_lo, int hx_hi, const cbet_params *p)
{
    if (hx_lo < 0 || hx_hi > p->nx + 2 || hx_hi < hx_lo)
        return fail(CBET_EINVAL, "%sslab [%d,%d) outside the haloed grid [0,%d)", who, hx_lo, hx_hi, p->nx + 2);
    return CBET_OK;
}

extern "C" int cbet_exchange_matrix_host(const double *fields, const double *ne3d, double *out, double *gross, int hx_lo,
                                         int hx_hi, const cbet_params *p, const cbet_gain_params *g, const double *flow,
                                         const double *state, double dn_max)
{
    return cbet_exchange_matrix_host_shifted(fields, ne3d, out, gross, hx_lo, hx_hi, p, g, flow, state, dn_max, nullptr);
}

// ... with per-beam frequency shifts: shift[nbeams] rad/s, or NULL.
extern "C" int cbet_exchange_matrix_host_shifted(const double *fields, const double *ne3d, double *out, double *gross, int hx_lo,
                                                 int hx_hi, const cbet_params *p, const cbet_gain_params *g, const double *flow,
                                                 const double *state, double dn_max, const double *shift)
{
    return cbet_exchange_matrix_host_polarized(fields, ne3d, out, gross, hx_lo, hx_hi, p, g, flow, state, dn_max, shift, CBET_POL_ALIGNED);
}

// ... and a polarization mode.
extern "C" int cbet_exchange_matrix_host_polarized(const double *fields, const double *ne3d, double *out, double *gross, int hx_lo,
                                                   int hx_hi, const cbet_params *p, const cbet_gain_params *g, const double *flow,
                                                   const double *state, double dn_max, const double *shift, int pol)
{
    return cbet_exchange_matrix_host_banded(fields, ne3d, out, gross, hx_lo, hx_hi, p, g, flow, state, dn_max, shift, pol, nullptr, nullptr, 0);
}

// ... and a line spectrum: the loop.  The ordered statement with the beat frequency (pair_gain's
// second form) wherever shift is given -- equal shifts add an exact zero to every pair --, pair_gain_band's sum over the
// spectrum's difference table where the lines make one (no lines, one line or equal offsets: the statements above, bit for
// bit), times pair_smoothing's factor where pol is CBET_POL_SMOOTHED, before the clamp.
extern "C" int cbet_exchange_matrix_host_banded(const double *fields, const double *ne3d, double *out, double *gross, int hx_lo,
                                                int hx_hi, const cbet_params *p, const cbet_gain_params *g, const double *flow,
                                                const double *state, double dn_max, const double *shift, int pol,
                                                const double *line_domega, const double *line_weight, int nlines)
{
    using namespace cbet;
    if (int rc = band_check("cbet_exchange_matrix_host_banded", line_domega, line_weight, nlines)) return rc;
    if (pol != CBET_POL_ALIGNED && pol != CBET_POL_SMOOTHED)
        return fail(CBET_EINVAL, "cbet_exchange_matrix_host_polarized: pol = %d is unknown (CBET_POL_ALIGNED = %d or CBET_POL_SMOOTHED = %d)",
                    pol, CBET_POL_ALIGNED, CBET_POL_SMOOTHED);
    cbet_derived d;
    if (int rc = derive_grid(p, &d)) return rc;
    if (p->nbeams > CBET_MAX_CBET_BEAMS)
        return fail(CBET_EINVAL, "cbet_exchange_matrix_host: nbeams = %d exceeds CBET_MAX_CBET_BEAMS = %d", p->nbeams, CBET_MAX_CBET_BEAMS);
    double cs = 0, gc = 0;
    if (int rc = cbet_gain_constants(p, g, nullptr, &cs, &gc)) return rc;   // (validates the gain parameters)
    if (!fields) return fail(CBET_EINVAL, "cbet_exchange_matrix_host: fields is NULL");
    if (!ne3d) return fail(CBET_EINVAL, "cbet_exchange_matrix_host: ne3d is NULL (there is no context to take a table from)");
    if (!out) return fail(CBET_EINVAL, "cbet_exchange_matrix_host: out is NULL");
    if (int rc = slab_check("cbet_exchange_matrix_host: ", hx_lo, hx_hi, p)) return rc;
    if (!(dn_max >= 0.0) || std::isinf(dn_max))
        return fail(CBET_EINVAL, "cbet_exchange_matrix_host: dn_max must be finite and >= 0 (0 = no limit)");
    const int nb = p->nbeams;
    double table[CBET_MAX_CBET_BEAMS] = {};   // the kernels' table: an entry per possible beam, zero past nbeams
    for (int b = 0; shift && b < nb; ++b) {
        if (!std::isfinite(shift[b])) return fail(CBET_EINVAL, "cbet_exchange_matrix_host_shifted: shift[%d] is not finite", b);
        table[b] = shift[b];
    }
    if (nb < 2 || hx_hi == hx_lo) return CBET_OK;
    double band[1 + 2 * kBandMax];
    GainOptions o;
    o.flow = flow; o.state = state; o.sat = dn_max; o.shift = shift ? table : nullptr; o.pol = pol;
    o.nband = (line_domega && line_weight && nlines > 1) ? band_table(line_domega, line_weight, nlines, band, nullptr) : 0;
    o.band = o.nband ? band : nullptr;
    carry_shifts(o, table);   // as the kernels' block (without shifts the table holds zeros)
    const GainArgs a = gain_args(p, d, g, cs, gc, fields, ne3d, o, hx_lo, hx_hi, false);
    const int HY = a.ny + 2, HZ = a.nz + 2;
    const long hsize = a.bstride, total = hsize * nb;
    const double iaw2 = a.iaw * a.iaw;
    const bool sat = dn_max > 0.0;
    // per ordered pair index i * nb + j, i < j: the sums of x and |x| with their compensations
    std::vector<double> st((size_t)nb * nb, 0.0), ct((size_t)nb * nb, 0.0), sg((size_t)nb * nb, 0.0), cg((size_t)nb * nb, 0.0);
    int present[CBET_MAX_CBET_BEAMS];
    for (long h = (long)hx_lo * HY * HZ; h < (long)hx_hi * HY * HZ; ++h) {
        const double *fI = fields + h, *fx = fI + total, *fy = fx + total, *fz = fy + total;
        int n = 0;
        for (int b = 0; b < nb; ++b)
            if (fI[(long)b * hsize] > 0.0) present[n++] = b;
        if (n < 2) continue;
        const CellState c = cell_state(a, h);
        if (!(c.eps > 0.0)) continue;
        const double ds_node = (kC * c.rt) * a.dt;
        const double pref = cell_pref(a, c);
        const double lim = cell_sat_limit(a, c);
        const double kmag = a.k0 * c.rt;
        for (int ia = 0; ia < n; ++ia) {
            const int bi = present[ia];
            const BeamAtCell Bi = beam_at(fI, fx, fy, fz, (long)bi * hsize);
            for (int ib = ia + 1; ib < n; ++ib) {
                const int bj = present[ib];
                const BeamAtCell Bj = beam_at(fI, fx, fy, fz, (long)bj * hsize);
                const PairWave w = pair_wave(Bi, Bj);
                if (!pair_present(Bi, Bj, w)) continue;
                double gn;
                if (a.band) gn = pair_gain_band(c, pref, iaw2, w, a.shift[bj] - a.shift[bi], a.band, a.nband);
                else gn = a.shift ? pair_gain(c, pref, iaw2, w, a.shift[bj] - a.shift[bi]) : pair_gain(c, pref, iaw2, w);
                if (a.pol) gn = gn * pair_smoothing(Bi, Bj, kmag);
                if (sat) gn = pair_clamp(gn, Bi.I, Bj.I, lim);
                const double x = ((ds_node * gn) * Bi.I) * Bj.I;
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
