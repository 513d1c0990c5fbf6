// cbet_lpi_host.cpp -- the host twin of the quarter-critical LPI maps (include/cbet_mi355x.h cbet_lpi_map_host; DESIGN.md
// section 23): one loop over the haloed cells in index order running cbet_lpi_model.h's statements, which are k_lpi_map's
// too, on an argument block filled by the kernel's own builder (lpi_args) -- one IEEE operation per written operator, the
// library is built with -ffp-contract=off.  No HIP call: it is the reference of the device path at any size.  The checks and
// the builder the device entry (cbet_gain_abi.cpp cbet_lpi_map) shares live here, so that the twin links without the HIP runtime.
#include <cmath>
#include <cstdio>

#include "cbet_host_internal.h"
#include "cbet_lpi_model.h"

static_assert(sizeof(cbet_lpi_summary) == 96, "work holds one cbet_lpi_summary per workgroup; api.py mirrors the layout");

int cbet::lpi_check(const char *who, const double *fields, const double *te3d, double te_ev, double frac_lo, double frac_hi,
                    int cone_bins, const double *lpi, int hx_lo, int hx_hi, const cbet_params *p, cbet_derived *d)
{
    if (int rc = derive_grid(p, d)) return rc;
    if (p->nbeams > CBET_MAX_CBET_BEAMS)
        return fail(CBET_EINVAL, "%s: nbeams = %d exceeds CBET_MAX_CBET_BEAMS = %d", who, p->nbeams, CBET_MAX_CBET_BEAMS);
    if (!fields) return fail(CBET_EINVAL, "%s: fields is NULL", who);
    if (!lpi) return fail(CBET_EINVAL, "%s: lpi is NULL", who);
    if (!(0.0 <= frac_lo && frac_lo <= frac_hi && frac_hi < 1.0))
        return fail(CBET_EINVAL, "%s: band [frac_lo, frac_hi] = [%g, %g] is not 0 <= frac_lo <= frac_hi < 1", who, frac_lo, frac_hi);
    if (cone_bins < 1 || cone_bins > CBET_LPI_MAX_BINS)
        return fail(CBET_EINVAL, "%s: cone_bins = %d outside 1 .. %d", who, cone_bins, CBET_LPI_MAX_BINS);
    if (!te3d && !(te_ev > 0.0)) return fail(CBET_EINVAL, "%s: te_ev = %g is not > 0 and te3d is NULL", who, te_ev);
    char prefix[64];
    std::snprintf(prefix, sizeof prefix, "%s: ", who);
    return slab_check(prefix, hx_lo, hx_hi, p);
}

cbet::LpiArgs cbet::lpi_args(const cbet_params *p, const cbet_derived &d, const double *fields, const double *ne3d,
                             const double *te3d, double te_ev, double frac_lo, double frac_hi, int cone_bins, double *lpi,
                             int hx_lo, int hx_hi)
{
    LpiArgs a{};
    grid_dims(a, p);
    a.nbeams = p->nbeams;
    a.dx = d.dx; a.dy = d.dy; a.dz = d.dz;
    a.ncrit = d.ncrit;
    a.lambda_um = (((2.0 * M_PI) * kC) / d.omega) * 1e4;      // the vacuum wavelength 2 pi c / omega, cm -> micrometres
    a.frac_lo = frac_lo; a.frac_hi = frac_hi; a.te_ev = te_ev;
    a.cone_bins = cone_bins;
    a.hx_lo = hx_lo; a.hx_hi = hx_hi;
    a.hsize = d.edep_size;
    a.fields = fields; a.ne3d = ne3d; a.te3d = te3d; a.lpi = lpi;
    return a;
}

// The bricks of the slab (2 x 4 x 8 cells, the gain stage's walk), four to a workgroup, capped: the slab's alone.
long cbet::lpi_groups(const cbet_params *p, int hx_lo, int hx_hi)
{
    const long bricks = (long)(((hx_hi + 1) >> 1) - (hx_lo >> 1)) * ((p->ny + 5) / 4) * ((p->nz + 9) / 8);
    const long groups = (bricks + 3) / 4;
    return groups < CBET_LPI_MAX_GROUPS ? groups : CBET_LPI_MAX_GROUPS;
}

extern "C" size_t cbet_lpi_work_bytes(const cbet_params *p)
{
    if (!p || cbet::validate(p) != CBET_OK || p->nbeams > CBET_MAX_CBET_BEAMS) return 0;
    return (size_t)cbet::lpi_groups(p, 0, p->nx + 2) * sizeof(cbet_lpi_summary);
}

extern "C" int cbet_lpi_summary_init(cbet_lpi_summary *s)
{
    if (!s) return cbet::fail(CBET_EINVAL, "cbet_lpi_summary_init: summary is NULL");
    cbet::lpi_summary_clear(*s);
    return CBET_OK;
}

extern "C" int cbet_lpi_map_host(const double *fields, const double *ne3d, const double *te3d, double te_ev, double frac_lo,
                                 double frac_hi, int cone_bins, double *lpi, cbet_lpi_summary *summary, int hx_lo, int hx_hi,
                                 const cbet_params *p)
{
    using namespace cbet;
    cbet_derived d;
    if (int rc = lpi_check("cbet_lpi_map_host", fields, te3d, te_ev, frac_lo, frac_hi, cone_bins, lpi, hx_lo, hx_hi, p, &d)) return rc;
    if (!ne3d) return fail(CBET_EINVAL, "cbet_lpi_map_host: ne3d is NULL (there is no context to take a table from)");
    const LpiArgs a = lpi_args(p, d, fields, ne3d, te3d, te_ev, frac_lo, frac_hi, cone_bins, lpi, hx_lo, hx_hi);
    const long plane = (long)(a.ny + 2) * (a.nz + 2), total = a.hsize * a.nbeams;
    cbet_lpi_summary s;
    lpi_summary_clear(s);
    for (long h = hx_lo * plane; h < hx_hi * plane; ++h) {
        int i, j, k;
        lpi_cell_node(a, h, i, j, k);
        const double ne = a.ne3d[((long)i * a.ny + j) * a.nz + k];
        LpiCell c = {0.0, 0.0, 0.0, 0};
        LpiPlasma q = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const bool band = lpi_in_band(a, ne / a.ncrit);
        if (band) {
            q = lpi_plasma(a, i, j, k, ne);
            double bins[CBET_LPI_MAX_BINS] = {};
            const double *fI = a.fields + h, *fx = fI + total, *fy = fx + total, *fz = fy + total;
            for (int b = 0; b < a.nbeams; ++b) {
                const long o = (long)b * a.hsize;
                const double I = fI[o];
                if (!(I > 0.0)) continue;
                const double kx = fx[o], ky = fy[o], kz = fz[o], kn = lpi_knorm(kx, ky, kz);
                if (!lpi_present(I, kn)) continue;
                const int bin = lpi_bin(q, kx, ky, kz, kn, a.cone_bins);
                c.Isum = c.Isum + I;
                if (I > c.Imax) c.Imax = I;
                c.npresent += 1;
                bins[bin] = bins[bin] + I;
            }
            for (int n = 0; n < a.cone_bins; ++n)
                if (bins[n] > c.Icw) c.Icw = bins[n];
            lpi_summary_cell(s, h, c, q);
        }
        lpi_store(a, h, band, c, q);
    }
    if (summary) lpi_summary_merge(*summary, s);
    return CBET_OK;
}
