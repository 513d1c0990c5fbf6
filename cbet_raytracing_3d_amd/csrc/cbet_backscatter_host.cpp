// cbet_backscatter_host.cpp -- the host twin of the backscatter SBS gain spectra (include/cbet_mi355x.h cbet_backscatter_host;
// DESIGN.md section 24): one loop over the items and over each item's stride-1 path samples running cbet_sbs_model.h's
// statements, which are k_trace_backscatter's too, on a GainArgs filled by the gain stage's own builder (gain_args) and an
// SbsArgs filled by the kernel's (sbs_args) -- one IEEE operation per written operator, the library is built with
// -ffp-contract=off.  The positions and nodes come from the path recorder, which publishes them bit for bit equal to the
// pinned oracle, so the twin is exact by construction.  No HIP call.  The checks and the builder the device entry
// (cbet_trace_abi.cpp cbet_trace_backscatter) shares live here, so that the twin links without the HIP runtime.
#include <climits>
#include <cmath>

#include "cbet_host_internal.h"
#include "cbet_sbs_model.h"

int cbet::sbs_check(const char *who, long nitems, const int *beams, const double *fields, const double *shifts, int nshift,
                    const double *gamma, const cbet_ray_sbs *rays, const cbet_params *p, const cbet_gain_params *g)
{
    if (int rc = validate(p)) return rc;
    if (nshift < 1 || nshift > CBET_SBS_MAX_SHIFTS)
        return fail(CBET_EINVAL, "%s: nshift = %d outside 1 .. %d", who, nshift, CBET_SBS_MAX_SHIFTS);
    if (!shifts) return fail(CBET_EINVAL, "%s: NULL shifts", who);
    for (int m = 0; m < nshift; ++m)
        if (!std::isfinite(shifts[m])) return fail(CBET_EINVAL, "%s: shift %d is not finite", who, m);
    if (!fields) return fail(CBET_EINVAL, "%s: fields is NULL", who);
    if (!g) return fail(CBET_EINVAL, "%s: NULL gain params (the model's damping, Mach ramp and plasma state)", who);
    if (int rc = validate_gain(p, g)) return rc;
    if (p->nbeams > CBET_MAX_CBET_BEAMS)
        return fail(CBET_EINVAL, "%s: nbeams = %d exceeds CBET_MAX_CBET_BEAMS = %d", who, p->nbeams, CBET_MAX_CBET_BEAMS);
    if (nitems < 0) return fail(CBET_EINVAL, "%s: nitems = %ld, must be >= 0", who, nitems);
    if (nitems > LONG_MAX / (long)sizeof(cbet_ray_sbs) / nshift)
        return fail(CBET_EINVAL, "%s: nitems = %ld times nshift = %d entries overflow a 64-bit byte count", who, nitems, nshift);
    if ((nitems + kWave - 1) / kWave > (long)INT_MAX)
        return fail(CBET_EINVAL, "%s: nitems = %ld is more than one launch takes (2^31 - 1 wavefronts of 64)", who, nitems);
    if (!rays) return fail(CBET_EINVAL, "%s: NULL ray-record array", who);
    if (!gamma) return fail(CBET_EINVAL, "%s: NULL gamma array", who);
    if (nitems > 0 && !beams) return fail(CBET_EINVAL, "%s: NULL beams with nitems = %ld", who, nitems);
    return CBET_OK;
}

cbet::SbsArgs cbet::sbs_args(const GainArgs &g, const int *beams, const int *raynums, long nitems, int nrays, const double *shifts,
                             int nshift, double *gamma, cbet_ray_sbs *rays)
{
    SbsArgs q{};
    q.beams = beams; q.raynums = raynums; q.nitems = nitems;
    q.nbeams = g.nbeams; q.nrays = nrays;
    q.nshift = nshift;
    q.qs = sbs_qs(g.k0, g.dt);
    q.iaw2 = g.iaw * g.iaw;
    for (int m = 0; m < nshift; ++m) q.shifts[m] = shifts[m];
    q.gamma = gamma; q.rays = rays;
    return q;
}

extern "C" size_t cbet_backscatter_work_bytes(long nitems, int nshift, int nbeams)
{
    if (nitems < 0 || nshift < 1 || nshift > CBET_SBS_MAX_SHIFTS || nbeams < 1 || nbeams > CBET_MAX_CBET_BEAMS) return 0;
    return (size_t)cbet::sbs_chunks(nitems) * nshift * nbeams * CBET_SBS_TALLY_COLUMNS * sizeof(double);
}

extern "C" int cbet_backscatter_host(const cbet_path_sample *samples, const cbet_ray_turn *turns, const int *beams, long nitems,
                                     int capacity, const double *fields, const double *ne3d, const double *flow,
                                     const double *state, int pol, const double *shifts, int nshift, double *gamma,
                                     cbet_ray_sbs *rays, const cbet_params *p, const cbet_gain_params *g)
{
    using namespace cbet;
    const char *const who = "cbet_backscatter_host";
    if (int rc = sbs_check(who, nitems, beams, fields, shifts, nshift, gamma, rays, p, g)) return rc;
    if (!ne3d) return fail(CBET_EINVAL, "%s: ne3d is NULL (there is no context to take a table from)", who);
    if (pol != CBET_POL_ALIGNED && pol != CBET_POL_SMOOTHED) return fail(CBET_EINVAL, "%s: unknown polarization mode %d", who, pol);
    if (capacity < 0) return fail(CBET_EINVAL, "%s: capacity = %d, must be >= 0", who, capacity);
    if (!turns) return fail(CBET_EINVAL, "%s: NULL turn-record array", who);
    if (capacity > 0 && !samples) return fail(CBET_EINVAL, "%s: NULL sample array with capacity = %d", who, capacity);
    cbet_derived d;
    if (int rc = derive_grid(p, &d)) return rc;
    double cs = 0, gc = 0;
    if (int rc = cbet_gain_constants(p, g, nullptr, &cs, &gc)) return rc;
    GainOptions o;
    o.flow = flow; o.state = state; o.pol = pol;
    const GainArgs a = gain_args(p, d, g, cs, gc, fields, ne3d, o, 0, p->nx + 2, false);
    const SbsArgs q = sbs_args(a, beams, nullptr, nitems, 0, shifts, nshift, gamma, rays);
    const bool smoothed = a.pol != 0;
    // the records first: an item the twin refuses leaves no half-written spectrum behind a success code
    for (long k = 0; k < nitems; ++k) {
        const cbet_ray_turn &t = turns[k];
        if (t.status == 0) continue;
        if (t.nsamples < 1 || t.nsamples > capacity)
            return fail(CBET_EINVAL, "%s: item %ld has nsamples = %d, capacity = %d (stride-1 samples, none truncated)", who, k, t.nsamples, capacity);
        if (beams[k] < 0 || beams[k] >= a.nbeams) return fail(CBET_EINVAL, "%s: item %ld is launched but its beam %d is outside [0, %d)", who, k, beams[k], a.nbeams);
        for (int n = 1; n < t.nsamples; ++n) {
            const cbet_path_sample &s = samples[(long)n * nitems + k];
            if (s.ci < 0 || s.ci >= a.nx || s.cj < 0 || s.cj >= a.ny || s.ck < 0 || s.ck >= a.nz)
                return fail(CBET_EINVAL, "%s: item %ld, sample %d: node (%d, %d, %d) outside the grid", who, k, n, s.ci, s.cj, s.ck);
        }
    }
    for (long k = 0; k < nitems; ++k) {
        const cbet_ray_turn &t = turns[k];
        cbet_ray_sbs r = {};
        double gam[CBET_SBS_MAX_SHIFTS] = {};
        if (t.status != 0) {
            const double *const fI = a.fields + (long)beams[k] * a.bstride;
            const int steps = t.nsamples - 1;
            for (int n = 1; n <= steps; ++n) {
                const cbet_path_sample &s0 = samples[(long)(n - 1) * nitems + k], &s1 = samples[(long)n * nitems + k];
                const double dx = s1.x - s0.x, dy = s1.y - s0.y, dz = s1.z - s0.z;
                const SbsStep st = sbs_step(q.qs, dx, dy, dz);
                if (st.ds != 0.0) {
                    const long h = sbs_cell(a, s1.ci, s1.cj, s1.ck);
                    const CellState c = cell_state(a, h);
                    const double pref = cell_pref(a, c);
                    const double I = fI[h];
                    for (int m = 0; m < q.nshift; ++m)
                        gam[m] = sbs_add(gam[m], sbs_gain(c, pref, q.iaw2, st.w, q.shifts[m], smoothed), I, st.ds);
                }
            }
            double gmax = 0.0;
            int imax = 0;
            for (int m = 0; m < q.nshift; ++m) sbs_max(gam[m], m, gmax, imax);
            r.gmax = gmax; r.uray0 = samples[k].uray;
            r.uray_end = samples[(long)steps * nitems + k].uray;
            r.steps = t.steps; r.imax = (short)imax; r.status = (short)t.status;
        }
        rays[k] = r;
        for (int m = 0; m < q.nshift; ++m) gamma[(long)m * nitems + k] = gam[m];
    }
    return CBET_OK;
}
