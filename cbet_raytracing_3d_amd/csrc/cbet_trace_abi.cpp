// cbet_trace_abi.cpp -- the trace launch of the C ABI (include/cbet_mi355x.h): trace_impl, which every ray-tracing entry
// goes through, its wrappers (plain, reference-shaped, exit pass, path recorder, backscatter spectra) and the small kernels that consume a trace's output.
// Citations are into /root/reference/.
#include <climits>
#include <cmath>

#include "cbet_host_internal.h"

using namespace cbet;

int cbet::trace_impl(int b, unsigned nindices, const double *ne3d, const double *kappa3d, double *edep,
                     const double *bbeam_norm, const double *beam_norm, const double *pow_r, const double *phase_r,
                     double xconst, double yconst, double zconst, const cbet_params *p, cbet_context *ctx, void *stream,
                     const CbetHooks &hooks)
{
    if (int rc = entry_checks(ctx, p)) return rc;
    if (!edep || !beam_norm || !pow_r || !phase_r) return fail(CBET_EINVAL, "NULL device pointer");
    if (nindices == 0) return CBET_OK;  // launch_ray_XZ.cu:155: the ray loop does not run
    if ((int)nindices != ctx->d.nindices)
        return fail(CBET_EINVAL, "nindices=%u but def.cuh:129 gives %d for these parameters", nindices, ctx->d.nindices);

    int beam_lo = p->beam_lo, beam_hi = p->beam_hi;
    // "unset" is beam_hi < 0 (CBET_BEAMS_BY_GPU, the default); every empty range [k,k), [0,0) included, is an
    // explicit no-op (a rank that owns no beam), handled below
    if (beam_hi >= 0 && beam_hi < beam_lo) return fail(CBET_EINVAL, "beam range [%d,%d) is reversed", beam_lo, beam_hi);
    if (beam_hi < 0) {  // launch_ray_XZ.cu:123 with grid.x = nbeams/nGPUs (main.cu:161)
        const int ng = p->ngpus > 0 ? p->ngpus : 1;
        const int per = p->nbeams / ng;
        beam_lo = b * per;
        beam_hi = beam_lo + per;
    }
    if (beam_lo < 0 || beam_hi > p->nbeams || beam_hi < beam_lo)
        return fail(CBET_EINVAL, "beam range [%d,%d) outside [0,%d)", beam_lo, beam_hi, p->nbeams);
    // (the recorder's rays are its caller's list, not the context's)
    if (beam_hi == beam_lo || (ctx->nlive == 0 && !hooks.paths && !hooks.sbs)) return CBET_OK;

    int variant = p->kernel_variant;
    if (variant == CBET_KERNEL_DEFAULT) variant = CBET_KERNEL_LDS_WINDOW;
    if (variant != CBET_KERNEL_GLOBAL_ATOMICS && variant != CBET_KERNEL_LDS_COMBINE &&
        variant != CBET_KERNEL_LDS_WINDOW)
        return fail(CBET_EINVAL, "unknown kernel_variant %d", p->kernel_variant);
    const bool cbet_hooks = hooks.gain || hooks.quantity != 0 || hooks.beam_gain;
    if (cbet_hooks && variant != CBET_KERNEL_LDS_WINDOW)
        return fail(CBET_EINVAL, "the CBET hooks exist for the default kernel (CBET_KERNEL_LDS_WINDOW) only");

    const cbet_derived &d = ctx->d;
    // the shipped kernel keeps two per-wave step counters in 16-bit halves of a register (WaveCounters)
    if (variant == CBET_KERNEL_LDS_WINDOW && d.nt >= 65536)
        return fail(CBET_EINVAL, "nt = %d steps per ray: the default kernel counts a bundle's steps in 16 bits (courant_mult too small)", d.nt);
    TraceArgs a{};
    grid_args(a, p, d);
    a.dt = d.dt;
    a.inv_dx = 1 / d.dx; a.inv_dy = 1 / d.dy; a.inv_dz = 1 / d.dz;      // launch_ray_XZ.cu:276-278
    a.fx_hi = p->nx - 3.0; a.fy_hi = p->ny - 3.0; a.fz_hi = p->nz - 3.0;
    a.bounds = ctx->bounds;                                              // :352-354, see context_create
    host_exit_planes(&ctx->p, ctx->d, a.exit_planes);                    // ... and by value, from the values context_create uploaded
    a.tol_x = 0.5001 * d.dx; a.tol_y = 0.5001 * d.dy; a.tol_z = 0.5001 * d.dz;  // :164-176
    a.xconst = xconst; a.yconst = yconst; a.zconst = zconst;
    a.nt = d.nt; a.absorption = p->absorption;
    a.rpz = p->rays_per_zone; a.zones = d.zones_spanned; a.nrays_x = d.nrays_x;
    a.z_launch = kFocal - d.dz / 2;                                       // :97
    a.uray_mult = d.uray_mult; a.omega = d.omega; a.ncrit = d.ncrit;
    a.xlaunch = ctx->xlaunch; a.ylaunch = ctx->ylaunch;
    a.live = ctx->live; a.nlive = ctx->nlive;
    a.beam_lo = beam_lo; a.nbeams_local = beam_hi - beam_lo;
    a.bundles_per_beam = (ctx->nlive + kWave - 1) / kWave;
    a.total_bundles = (long)a.nbeams_local * a.bundles_per_beam;
    {   // this launch's share: a contiguous, near-equal part of the list (cbet_params.shard_index / shard_count)
        const long K = p->shard_count > 1 ? p->shard_count : 1, r = p->shard_count > 1 ? p->shard_index : 0;
        a.first_item = (r * a.total_bundles) / K;
        a.item_count = ((r + 1) * a.total_bundles) / K - a.first_item;
    }
    a.ne3d = ne3d ? ne3d : ctx->ne3d;
    a.kap3d = kappa3d ? kappa3d : ctx->kap3d;
    a.beam_norm = beam_norm; a.bbeam_norm = bbeam_norm; a.pow_r = pow_r; a.phase_r = phase_r;
    a.edep = edep;
    a.sYh = p->edep_zpitch > 0 ? p->edep_zpitch : p->nz + 2;
    a.sXh = (p->ny + 2) * a.sYh;
    if (p->edep_zpitch > 0 && (p->per_beam_grids || cbet_hooks))
        return fail(CBET_EINVAL, "edep_zpitch applies to the plain path's single deposit grid (no per-beam grids, no CBET hooks)");
    a.grid_stride = (p->per_beam_grids || hooks.quantity != 0) ? d.edep_size : 0;  // field passes are always beam-resolved
    if (hooks.exits) a.grid_stride = (long)kExitDoubles * ctx->nlive;            // exit records: L per beam (launch_trace_exit)
    // beam-resolved arrays may hold only the grids of beams [grid_beam0, grid_beam0 + grid_beams)
    const int gb_n = p->grid_beams > 0 ? p->grid_beams : p->nbeams, gb_0 = p->grid_beams > 0 ? p->grid_beam0 : 0;
    if ((a.grid_stride != 0 || hooks.gain) && (beam_lo < gb_0 || beam_hi > gb_0 + gb_n))
        return fail(CBET_EINVAL, "beams [%d,%d) are not all inside the beam-resolved arrays' range [%d,%d)", beam_lo, beam_hi,
                    gb_0, gb_0 + gb_n);
    a.grid_beam0 = gb_0;
    a.comp_stride = (long)gb_n * d.edep_size;
    a.counters = ctx->counters;
    a.stats = p->window_stats != 0;
    a.gain = hooks.gain; a.hsize = d.edep_size; a.quantity = hooks.quantity;
    a.max_exponent = hooks.max_exponent; a.beam_gain = hooks.beam_gain;
    CBET_ENTER_DEVICE(ctx);
    if (variant == CBET_KERNEL_LDS_WINDOW) {
        // the shipped kernel gathers one 32-byte record per node; built here (unless still valid) because only
        // the launch knows both the tables -- possibly the caller's -- and the gradient constants
        if (int rc = step_records(ctx, p, ne3d, kappa3d, xconst, yconst, zconst, stream, false)) return rc;
        a.steprec = ctx->steprec;
    }
    CBET_HIP(launch_trace(a, hooks.sbs ? kTraceBackscatter : hooks.paths ? kTracePaths : hooks.exits ? kTraceExits : variant,
                          p->force_wide_index != 0, (hipStream_t)stream, hooks.paths, hooks.sbs, hooks.sbs_gain));
    return CBET_OK;
}

extern "C" {

int cbet_trace_nodes(int b, unsigned nindices, const double *ne3d, const double *kappa3d,
                     double *edep, const double *bbeam_norm, const double *beam_norm,
                     const double *pow_r, const double *phase_r, double xconst, double yconst,
                     double zconst, const cbet_params *p, cbet_context *ctx, void *stream)
{
    return trace_impl(b, nindices, ne3d, kappa3d, edep, bbeam_norm, beam_norm, pow_r, phase_r, xconst, yconst,
                      zconst, p, ctx, stream, CbetHooks{});
}

int cbet_launch_ray_XYZ(int b, unsigned nindices, double *te_data_g, double *r_data_g,
                        double *ne_data_g, double *edep, double *bbeam_norm, double *beam_norm,
                        double *pow_r, double *phase_r, double xconst, double yconst,
                        double zconst, const cbet_params *p, cbet_context *ctx, void *stream)
{
    if (int rc = validate(p)) return rc;
    if (!ctx) {
        if (int rc = default_context(p, &ctx)) return rc;
    }
    // the default kernel gathers step records: tables and records in one kernel; the cross-check kernels read the tables
    const bool records = p->kernel_variant == CBET_KERNEL_DEFAULT || p->kernel_variant == CBET_KERNEL_LDS_WINDOW;
    if (int rc = records ? cbet_prepare_plasma(ctx, p, te_data_g, r_data_g, ne_data_g, xconst, yconst, zconst, stream)
                         : cbet_tabulate_plasma(ctx, p, te_data_g, r_data_g, ne_data_g, stream)) return rc;
    return cbet_trace_nodes(b, nindices, nullptr, nullptr, edep, bbeam_norm, beam_norm, pow_r, phase_r,
                            xconst, yconst, zconst, p, ctx, stream);
}

int cbet_edep_average_device(const double *edep, double *edepavg, int nx, int ny, int nz, void *stream)
{
    if (!edep || !edepavg || nx < 1 || ny < 1 || nz < 1) return fail(CBET_EINVAL, "cbet_edep_average_device: bad array");
    if ((long)(nx + 2) * (ny + 2) * (nz + 2) >= (1L << 31)) return fail(CBET_EINVAL, "cbet_edep_average_device: grid too large");
    CBET_HIP(launch_edep_average(edep, edepavg, nx, ny, nz, (hipStream_t)stream));
    return CBET_OK;
}

// ---- the no-deposit passes: exit pass and path recorder ------------------------------------------------
// Absorbing mode and the gain arguments.  `prefix` and `pass` are the entry's own words in the messages.
static int no_deposit_checks(const char *prefix, const char *pass, const double *gain, const cbet_params *p, const cbet_gain_params *g)
{
    if (p->absorption != 1)
        return fail(CBET_EINVAL, "%sthe %s needs absorbing mode (absorption = 1): in bookkeeping mode the increment is no energy loss", prefix, pass);
    if (gain && !g) return fail(CBET_EINVAL, "%sa gain grid needs gain params (max_exponent)", prefix);
    return g ? validate_gain(p, g) : CBET_OK;
}

// The parameters such a pass hands to trace_impl for the trace's own checks and set-up (geometry, beam range against
// grid_beam0 / grid_beams, shards, step records): the deposit-grid options do not apply.
static cbet_params no_deposit_params(const cbet_params *p)
{
    cbet_params q = *p;
    q.kernel_variant = CBET_KERNEL_LDS_WINDOW;
    q.per_beam_grids = 0;
    q.edep_zpitch = 0;
    q.window_stats = 0;
    return q;
}

// ---- exit pass ---------------------------------------------------------------
int cbet_trace_exits(const double *ne3d, const double *kappa3d, const double *gain, cbet_ray_exit *exits,
                     const double *bbeam_norm, const double *beam_norm, const double *pow_r, const double *phase_r,
                     double xconst, double yconst, double zconst, const cbet_params *p, const cbet_gain_params *g,
                     cbet_context *ctx, void *stream)
{
    if (int rc = validate(p)) return rc;
    if (!ctx) return fail(CBET_EINVAL, "NULL context");
    if (!exits) return fail(CBET_EINVAL, "NULL exit-record array");
    if (int rc = no_deposit_checks("", "exit pass", gain, p, g)) return rc;
    cbet_params q = no_deposit_params(p);
    if (q.beam_hi < 0) { q.beam_lo = 0; q.beam_hi = q.nbeams; }
    CbetHooks h;
    h.gain = gain; h.max_exponent = g ? g->max_exponent : 0.0; h.exits = true;
    return trace_impl(0, (unsigned)ctx->d.nindices, ne3d, kappa3d, reinterpret_cast<double *>(exits), bbeam_norm,
                      beam_norm, pow_r, phase_r, xconst, yconst, zconst, &q, ctx, stream, h);
}

// ---- path recorder --------------------------------------------------------------
int cbet_trace_paths(const double *ne3d, const double *kappa3d, const double *gain, const int *beams, const int *raynums,
                     long nitems, int stride, int capacity, const double *center, cbet_path_sample *samples,
                     cbet_ray_turn *turns, const double *bbeam_norm, const double *beam_norm, const double *pow_r,
                     const double *phase_r, double xconst, double yconst, double zconst, const cbet_params *p,
                     const cbet_gain_params *g, cbet_context *ctx, void *stream)
{
    if (int rc = validate(p)) return rc;
    // the argument checks: before the context and before any HIP call
    if (stride < 1) return fail(CBET_EINVAL, "cbet_trace_paths: stride = %d, must be >= 1", stride);
    if (capacity < 0) return fail(CBET_EINVAL, "cbet_trace_paths: capacity = %d, must be >= 0", capacity);
    if (nitems < 0) return fail(CBET_EINVAL, "cbet_trace_paths: nitems = %ld, must be >= 0", nitems);
    {
        const long per_item = capacity > 1 ? capacity : 1, max_records = LONG_MAX / (long)sizeof(cbet_path_sample);
        if (nitems > max_records / per_item)
            return fail(CBET_EINVAL, "cbet_trace_paths: nitems = %ld times capacity = %d records overflow a 64-bit byte count", nitems,
                        capacity);
        if ((nitems + kWave - 1) / kWave > (long)INT_MAX)
            return fail(CBET_EINVAL, "cbet_trace_paths: nitems = %ld is more than one launch takes (2^31 - 1 wavefronts of 64)", nitems);
    }
    if (!turns) return fail(CBET_EINVAL, "cbet_trace_paths: NULL turn-record array");
    if (nitems > 0 && (!beams || !raynums)) return fail(CBET_EINVAL, "cbet_trace_paths: NULL beams / raynums with nitems = %ld", nitems);
    if (capacity > 0 && !samples) return fail(CBET_EINVAL, "cbet_trace_paths: NULL sample array with capacity = %d", capacity);
    if (!center) return fail(CBET_EINVAL, "cbet_trace_paths: NULL center");
    if (!std::isfinite(center[0]) || !std::isfinite(center[1]) || !std::isfinite(center[2]))
        return fail(CBET_EINVAL, "cbet_trace_paths: center is not finite");
    if (int rc = no_deposit_checks("cbet_trace_paths: ", "recorder", gain, p, g)) return rc;
    if (!ctx) return fail(CBET_EINVAL, "NULL context");
    if (nitems == 0) return CBET_OK;
    // ... and here the beam range, the shard split and the beam-resolved arrays' range do not apply either
    cbet_params q = no_deposit_params(p);
    q.beam_lo = 0; q.beam_hi = q.nbeams;
    q.shard_index = 0; q.shard_count = 1;
    q.grid_beam0 = 0; q.grid_beams = 0;
    PathArgs path{};
    path.beams = beams; path.raynums = raynums; path.nitems = nitems;
    path.nbeams = p->nbeams; path.nrays = ctx->d.nrays;
    path.stride = stride; path.capacity = capacity;
    path.cx = center[0]; path.cy = center[1]; path.cz = center[2];
    path.samples = samples; path.turns = turns;
    CbetHooks h;
    h.gain = gain; h.max_exponent = g ? g->max_exponent : 0.0; h.paths = &path;
    return trace_impl(0, (unsigned)ctx->d.nindices, ne3d, kappa3d, reinterpret_cast<double *>(turns), bbeam_norm, beam_norm,
                      pow_r, phase_r, xconst, yconst, zconst, &q, ctx, stream, h);
}

// ---- backscatter SBS gain spectra ------------------------------------------------
int cbet_trace_backscatter(const double *ne3d, const double *kappa3d, const double *gain, const int *beams, const int *raynums,
                           long nitems, const double *fields, const double *shifts, int nshift, double *gamma,
                           cbet_ray_sbs *rays, const double *bbeam_norm, const double *beam_norm, const double *pow_r,
                           const double *phase_r, double xconst, double yconst, double zconst, const cbet_params *p,
                           const cbet_gain_params *g, cbet_context *ctx, void *stream)
{
    // the argument checks: before the context and before any HIP call; the twin's own (cbet_backscatter_host.cpp)
    if (int rc = sbs_check("cbet_trace_backscatter", nitems, beams, fields, shifts, nshift, gamma, rays, p, g)) return rc;
    if (nitems > 0 && !raynums) return fail(CBET_EINVAL, "cbet_trace_backscatter: NULL raynums with nitems = %ld", nitems);
    if (int rc = no_deposit_checks("cbet_trace_backscatter: ", "backscatter pass", gain, p, g)) return rc;
    if (int rc = entry_checks(ctx, p)) return rc;
    if (nitems == 0) return CBET_OK;
    double cs = 0, gc = 0;
    if (int rc = cbet_gain_constants(p, g, nullptr, &cs, &gc)) return rc;
    // as cbet_trace_paths: the beam range, the shard split and the beam-resolved arrays' range do not apply
    cbet_params q = no_deposit_params(p);
    q.beam_lo = 0; q.beam_hi = q.nbeams;
    q.shard_index = 0; q.shard_count = 1;
    q.grid_beam0 = 0; q.grid_beams = 0;
    // the context's flow table, state table and polarization mode; its limit, shifts and spectrum are not applied (linear gain,
    // the seed's shift is the scan variable)
    GainOptions o;
    o.flow = ctx->flow; o.state = ctx->state; o.pol = ctx->pol;
    const GainArgs ga = gain_args(p, ctx->d, g, cs, gc, fields, ne3d ? ne3d : ctx->ne3d, o, 0, p->nx + 2, false);
    const SbsArgs sbs = sbs_args(ga, beams, raynums, nitems, ctx->d.nrays, shifts, nshift, gamma, rays);
    CbetHooks h;
    h.gain = gain; h.max_exponent = g->max_exponent; h.sbs = &sbs; h.sbs_gain = &ga;
    return trace_impl(0, (unsigned)ctx->d.nindices, ne3d, kappa3d, reinterpret_cast<double *>(rays), bbeam_norm, beam_norm,
                      pow_r, phase_r, xconst, yconst, zconst, &q, ctx, stream, h);
}

int cbet_backscatter_tally(const double *gamma, const cbet_ray_sbs *rays, const int *beams, long nitems, int nshift, int nbeams,
                           double *tally, void *work, void *stream)
{
    if (nshift < 1 || nshift > CBET_SBS_MAX_SHIFTS)
        return fail(CBET_EINVAL, "cbet_backscatter_tally: nshift = %d outside 1 .. %d", nshift, CBET_SBS_MAX_SHIFTS);
    if (nbeams < 1 || nbeams > CBET_MAX_CBET_BEAMS)
        return fail(CBET_EINVAL, "cbet_backscatter_tally: nbeams = %d outside 1 .. %d", nbeams, CBET_MAX_CBET_BEAMS);
    if (nitems < 0) return fail(CBET_EINVAL, "cbet_backscatter_tally: nitems = %ld, must be >= 0", nitems);
    if (!tally) return fail(CBET_EINVAL, "cbet_backscatter_tally: NULL tally");
    if (nitems == 0) return CBET_OK;
    if (!gamma || !rays || !beams) return fail(CBET_EINVAL, "cbet_backscatter_tally: NULL gamma / rays / beams with nitems = %ld", nitems);
    if (!work) return fail(CBET_EINVAL, "cbet_backscatter_tally: work is NULL (cbet_backscatter_work_bytes)");
    CBET_HIP(launch_backscatter_tally(gamma, rays, beams, nitems, nshift, nbeams, tally, (double *)work, (hipStream_t)stream));
    return CBET_OK;
}

int cbet_exit_tally(const cbet_ray_exit *exits, long L, int nbeams, double *tally, void *stream)
{
    if (!exits || !tally) return fail(CBET_EINVAL, "NULL exit records / tally");
    if (L < 0 || nbeams < 0) return fail(CBET_EINVAL, "L = %ld, nbeams = %d", L, nbeams);
    CBET_HIP(launch_exit_tally(exits, L, nbeams, tally, (hipStream_t)stream));
    return CBET_OK;
}

int cbet_farfield(const cbet_ray_exit *exits, long n, int ntheta, int nphi, double *hist, void *stream)
{
    if (!exits || !hist) return fail(CBET_EINVAL, "NULL exit records / histogram");
    if (n < 0 || ntheta <= 0 || nphi <= 0) return fail(CBET_EINVAL, "n = %ld, ntheta = %d, nphi = %d", n, ntheta, nphi);
    CBET_HIP(launch_farfield(exits, n, ntheta, nphi, hist, (hipStream_t)stream));
    return CBET_OK;
}

}  // extern "C"
