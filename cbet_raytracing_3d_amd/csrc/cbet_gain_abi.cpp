// cbet_gain_abi.cpp -- the CBET stage of the C ABI (include/cbet_mi355x.h; SURVEY 8(f) f1, parity unpinned -- see the
// header): the gain update, the trace with the CBET hooks, the sparse exchange's pack / unpack and the native one-device
// fixed-point loop, the amplitude map of the saturation clamp, the pairwise exchange matrix, the quarter-critical LPI maps.
#include <cmath>

#include "cbet_host_internal.h"
#include "cbet_lpi_model.h"

using namespace cbet;

int cbet::gain_field_impl(double *fields, const double *ne3d, double *gain, double *scratch, double *change, int hx_lo,
                          int hx_hi, bool packed, const cbet_params *p, const cbet_gain_params *g, cbet_context *ctx,
                          void *stream, bool consume)
{
    if (int rc = entry_checks(ctx, p)) return rc;
    if (int rc = validate_gain(p, g)) return rc;
    if (!fields || !gain) return fail(CBET_EINVAL, "NULL device pointer");
    if (int rc = slab_check("", hx_lo, hx_hi, p)) return rc;
    double cs = 0, gc = 0;
    if (int rc = cbet_gain_constants(p, g, nullptr, &cs, &gc)) return rc;
    if (hx_hi == hx_lo) return CBET_OK;   // an empty slab (more ranks than planes)
    GainArgs a = gain_args(p, ctx->d, g, cs, gc, fields, ne3d ? ne3d : ctx->ne3d, context_gain_options(ctx), hx_lo, hx_hi, packed);
    a.gain = gain; a.scratch = scratch; a.change = change;
    a.consume = (consume && scratch) ? 1 : 0;
    a.frozen = g->directions_frozen ? 1 : 0;
    CBET_ENTER_DEVICE(ctx);
    CBET_HIP(launch_gain_field(a, (hipStream_t)stream));
    return CBET_OK;
}

extern "C" {

int cbet_trace_cbet(int b, unsigned nindices, const double *ne3d, const double *kappa3d,
                    const double *gain, int quantity, double *out, double *beam_gain,
                    const double *bbeam_norm, const double *beam_norm, const double *pow_r,
                    const double *phase_r, double xconst, double yconst, double zconst,
                    const cbet_params *p, const cbet_gain_params *g, cbet_context *ctx, void *stream)
{
    if (int rc = validate(p)) return rc;
    if (int rc = validate_gain(p, g)) return rc;
    if (quantity != CBET_DEPOSIT_ENERGY && quantity != CBET_DEPOSIT_FIELDS && quantity != CBET_DEPOSIT_FIELD_ENERGY)
        return fail(CBET_EINVAL, "quantity must be CBET_DEPOSIT_ENERGY (0), CBET_DEPOSIT_FIELDS (1) or CBET_DEPOSIT_FIELD_ENERGY (2)");
    CbetHooks h;
    h.gain = gain; h.quantity = quantity; h.beam_gain = beam_gain; h.max_exponent = g->max_exponent;
    return trace_impl(b, nindices, ne3d, kappa3d, out, bbeam_norm, beam_norm, pow_r, phase_r, xconst, yconst, zconst,
                      p, ctx, stream, h);
}

int cbet_gain_field(double *fields, const double *ne3d, double *gain, double *scratch, double *change,
                    const cbet_params *p, const cbet_gain_params *g, cbet_context *ctx, void *stream)
{
    return cbet_gain_field_slab(fields, ne3d, gain, scratch, change, 0, p ? p->nx + 2 : 0, p, g, ctx, stream);
}

int cbet_gain_field_slab(double *fields, const double *ne3d, double *gain, double *scratch, double *change,
                         int hx_lo, int hx_hi, const cbet_params *p, const cbet_gain_params *g,
                         cbet_context *ctx, void *stream)
{
    return gain_field_impl(fields, ne3d, gain, scratch, change, hx_lo, hx_hi, false, p, g, ctx, stream);
}

int cbet_gain_field_packed(double *fields, const double *ne3d, double *gain, double *scratch, double *change,
                           int hx_lo, int hx_hi, const cbet_params *p, const cbet_gain_params *g,
                           cbet_context *ctx, void *stream)
{
    return gain_field_impl(fields, ne3d, gain, scratch, change, hx_lo, hx_hi, true, p, g, ctx, stream);
}

int cbet_pair_amplitude(const double *fields, const double *ne3d, double *amp, int hx_lo, int hx_hi, const cbet_params *p,
                        const cbet_gain_params *g, cbet_context *ctx, void *stream)
{
    // the arguments first, the context last: what is wrong with a call does not depend on there being a device
    if (int rc = validate(p)) return rc;
    if (int rc = validate_gain(p, g)) return rc;
    if (!fields) return fail(CBET_EINVAL, "cbet_pair_amplitude: fields is NULL");
    if (!amp) return fail(CBET_EINVAL, "cbet_pair_amplitude: amp is NULL");
    if (int rc = slab_check("cbet_pair_amplitude: ", hx_lo, hx_hi, p)) return rc;
    if (int rc = entry_checks(ctx, p)) return rc;
    double cs = 0, gc = 0;
    if (int rc = cbet_gain_constants(p, g, nullptr, &cs, &gc)) return rc;
    if (hx_hi == hx_lo) return CBET_OK;
    // sat = 0: the map is the unclamped amplitude (of the detuned gain, if the context has shifts; of the smoothed one, if that is its mode; of the summed one, if it has a line spectrum)
    GainOptions o = context_gain_options(ctx); o.sat = 0.0;
    const GainArgs a = gain_args(p, ctx->d, g, cs, gc, fields, ne3d ? ne3d : ctx->ne3d, o, hx_lo, hx_hi, false);
    CBET_ENTER_DEVICE(ctx);
    CBET_HIP(launch_pair_amplitude(a, amp, (hipStream_t)stream));
    return CBET_OK;
}

// ---- pairwise exchange matrix (cbet_grid_kernels.hip k_exchange_matrix, k_exchange_reduce) --------
size_t cbet_exchange_matrix_work_bytes(const cbet_params *p)
{
    if (!p || validate(p) != CBET_OK || p->nbeams > CBET_MAX_CBET_BEAMS) return 0;
    const size_t npairs = (size_t)p->nbeams * (p->nbeams - 1) / 2;
    return (size_t)exchange_groups((long)(p->nx + 2) * (p->ny + 2)) * 2 * npairs * sizeof(double);
}

int cbet_exchange_matrix(const double *fields, const double *ne3d, double *out, double *gross, void *work, int hx_lo, int hx_hi,
                         const cbet_params *p, const cbet_gain_params *g, cbet_context *ctx, void *stream)
{
    // the arguments first, the context last, as cbet_pair_amplitude
    if (int rc = validate(p)) return rc;
    if (p->nbeams > CBET_MAX_CBET_BEAMS)
        return fail(CBET_EINVAL, "cbet_exchange_matrix: nbeams = %d exceeds CBET_MAX_CBET_BEAMS = %d", p->nbeams, CBET_MAX_CBET_BEAMS);
    if (int rc = validate_gain(p, g)) return rc;
    if (!fields) return fail(CBET_EINVAL, "cbet_exchange_matrix: fields is NULL");
    if (!out) return fail(CBET_EINVAL, "cbet_exchange_matrix: out is NULL");
    if (!work) return fail(CBET_EINVAL, "cbet_exchange_matrix: work is NULL");
    if (int rc = slab_check("cbet_exchange_matrix: ", hx_lo, hx_hi, p)) return rc;
    if (int rc = entry_checks(ctx, p)) return rc;
    double cs = 0, gc = 0;
    if (int rc = cbet_gain_constants(p, g, nullptr, &cs, &gc)) return rc;
    if (p->nbeams < 2 || hx_hi == hx_lo) return CBET_OK;   // one beam exchanges with nobody; an empty slab adds nothing
    // the context's options, all of them: the matrix decomposes the K the solve uses, the limit, the detuning, the polarization mode and the line spectrum are honoured
    const GainArgs a = gain_args(p, ctx->d, g, cs, gc, fields, ne3d ? ne3d : ctx->ne3d, context_gain_options(ctx), hx_lo, hx_hi, false);
    CBET_ENTER_DEVICE(ctx);
    CBET_HIP(launch_exchange_matrix(a, (double *)work, out, gross, (hipStream_t)stream));
    return CBET_OK;
}

// ---- quarter-critical LPI maps (cbet_lpi.hip k_lpi_map, k_lpi_reduce) ------------------------------
int cbet_lpi_map(const double *fields, const double *ne3d, const double *te3d, double te_ev, double frac_lo, double frac_hi,
                 int cone_bins, double *lpi, cbet_lpi_summary *summary, void *work, int hx_lo, int hx_hi, const cbet_params *p,
                 cbet_context *ctx, void *stream)
{
    // the arguments first, the context last, as cbet_pair_amplitude; the checks are the host twin's (cbet_lpi_host.cpp)
    cbet_derived d;
    if (int rc = lpi_check("cbet_lpi_map", fields, te3d, te_ev, frac_lo, frac_hi, cone_bins, lpi, hx_lo, hx_hi, p, &d)) return rc;
    if (summary && !work) return fail(CBET_EINVAL, "cbet_lpi_map: work is NULL but summary is not (cbet_lpi_work_bytes)");
    if (int rc = entry_checks(ctx, p)) return rc;
    if (hx_hi == hx_lo) return CBET_OK;
    const LpiArgs a = lpi_args(p, ctx->d, fields, ne3d ? ne3d : ctx->ne3d, te3d, te_ev, frac_lo, frac_hi, cone_bins, lpi, hx_lo, hx_hi);
    CBET_ENTER_DEVICE(ctx);
    CBET_HIP(launch_lpi_map(a, summary, (cbet_lpi_summary *)work, lpi_groups(p, hx_lo, hx_hi), (hipStream_t)stream));
    return CBET_OK;
}

// ---- sparse exchange of the slab-owned CBET loop (cbet_grid_kernels.hip) -----------------------------------------
int cbet_pack_segments(const double *src, long beam_stride, int hy, int hz, const int *segments, long nseg, double *out,
                       void *stream)
{
    if (nseg < 0 || hy < 1 || hz < 1 || beam_stride < 0) return fail(CBET_EINVAL, "cbet_pack_segments: bad shape");
    if (nseg > 0 && (!src || !segments || !out)) return fail(CBET_EINVAL, "cbet_pack_segments: NULL pointer");
    if (nseg * 8 >= (1L << 31) * 256L) return fail(CBET_EINVAL, "cbet_pack_segments: too many segments for one launch");
    CBET_HIP(launch_pack_segments(src, beam_stride, hy, hz, segments, nseg, out, (hipStream_t)stream));
    return CBET_OK;
}

int cbet_unpack_segments(double *dst, long beam_stride, int hy, int hz, const int *segments, long nseg, const double *in,
                         void *stream)
{
    if (nseg < 0 || hy < 1 || hz < 1 || beam_stride < 0) return fail(CBET_EINVAL, "cbet_unpack_segments: bad shape");
    if (nseg > 0 && (!dst || !segments || !in)) return fail(CBET_EINVAL, "cbet_unpack_segments: NULL pointer");
    if (nseg * 8 >= (1L << 31) * 256L) return fail(CBET_EINVAL, "cbet_unpack_segments: too many segments for one launch");
    CBET_HIP(launch_unpack_segments(dst, beam_stride, hy, hz, segments, nseg, in, (hipStream_t)stream));
    return CBET_OK;
}

int cbet_cbet_solve(double *te_data_g, double *r_data_g, double *ne_data_g, double *edep,
                    double *bbeam_norm, double *beam_norm, double *pow_r, double *phase_r,
                    const cbet_params *p, const cbet_gain_params *g, void *workspace,
                    cbet_context *ctx, void *stream, cbet_cbet_report *report)
{
    if (int rc = validate(p)) return rc;
    if (int rc = validate_gain(p, g)) return rc;
    if (p->shard_count > 1) return fail(CBET_EINVAL, "cbet_cbet_solve runs on one device; the sharded loop is tracer.cbet_solve");
    if (g->max_passes < 1) return fail(CBET_EINVAL, "max_passes must be >= 1");
    if (!edep || !beam_norm || !pow_r || !phase_r) return fail(CBET_EINVAL, "NULL device pointer");
    if (!ctx) {
        if (int rc = default_context(p, &ctx)) return rc;
    }
    if (int rc = check_geometry(ctx, p)) return rc;
    if (ctx->flow)   // this loop tabulates the radial plasma about the origin itself: it does not mix that with another flow
        return fail(CBET_EINVAL, "cbet_cbet_solve models a spherical target about the origin: the context has a flow table "
                                 "selected (cbet_context_set_flow(ctx, NULL), or the loop above the C ABI: tracer.cbet_solve)");
    if (ctx->state)   // ... and its gain constants are cbet_gain_params' own, everywhere
        return fail(CBET_EINVAL, "cbet_cbet_solve takes the sound speed and the gain constant from the gain parameters: the context "
                                 "has a state table selected (cbet_context_set_state(ctx, NULL), or the loop above the C ABI: tracer.cbet_solve)");
    const cbet_derived &d = ctx->d;
    hipStream_t s = (hipStream_t)stream;
    CBET_ENTER_DEVICE(ctx);

    const size_t hsize = (size_t)d.edep_size, nb = (size_t)p->nbeams;
    const size_t bytes = cbet_cbet_workspace_bytes(p);
    double *ws = (double *)workspace;
    bool own = false;
    if (!ws) {
        hipError_t e = hipMalloc((void **)&ws, bytes);
        if (e != hipSuccess) return fail_hip(e == hipErrorOutOfMemory ? CBET_ENOMEM : CBET_EHIP, "hipMalloc(cbet workspace, %zu bytes): %s", bytes, hipGetErrorString(e));
        own = true;
    }
    double *fields = ws, *gain = ws + 4 * nb * hsize, *change = gain + nb * hsize, *beam_gain = change + 2;
    double *const pair_once = gain;   // any non-NULL pointer selects the pair-once gain kernel; it is not dereferenced
    int rc = CBET_OK;
    cbet_counters c0{}, c1{};
    cbet_cbet_report rep{};
    auto body = [&]() -> int {
        if (int r = cbet_tabulate_plasma(ctx, p, te_data_g, r_data_g, ne_data_g, stream)) return r;
        if (int r = cbet_context_counters(ctx, stream, &c0, 0)) return r;
        CBET_HIP(hipMemsetAsync(gain, 0, nb * hsize * sizeof(double), s));
        cbet_params pf = *p;            // field passes: every beam (always beam-resolved)
        pf.beam_lo = 0; pf.beam_hi = p->nbeams;
        cbet_params pd = *p;            // deposition pass: the caller's grid layout, every beam
        pd.beam_lo = 0; pd.beam_hi = p->nbeams;
        // the fields are cleared once; every gain update hands them back zeroed (GainArgs.consume)
        CBET_HIP(hipMemsetAsync(fields, 0, 4 * nb * hsize * sizeof(double), s));
        cbet_gain_params gg = *g;
        for (int pass = 0; pass < g->max_passes; ++pass) {
            // the first direction_passes passes deposit all four fields and build k; later ones the energy field only
            const bool full = pass < g->direction_passes;
            if (full && pass > 0)   // a second direction-building pass accumulates into cleared direction entries
                CBET_HIP(hipMemsetAsync(fields + nb * hsize, 0, 3 * nb * hsize * sizeof(double), s));
            {
                CbetHooks h;
                h.gain = pass == 0 ? nullptr : gain; h.quantity = full ? CBET_DEPOSIT_FIELDS : CBET_DEPOSIT_FIELD_ENERGY;
                h.max_exponent = g->max_exponent;
                if (int r = trace_impl(0, (unsigned)d.nindices, nullptr, nullptr, fields, bbeam_norm, beam_norm, pow_r, phase_r,
                                       d.xconst, d.yconst, d.zconst, &pf, ctx, stream, h))
                    return r;
            }
            CBET_HIP(hipMemsetAsync(change, 0, 2 * sizeof(double), s));
            gg.directions_frozen = full ? 0 : 1;
            if (int r = gain_field_impl(fields, nullptr, gain, pair_once, change, 0, p->nx + 2, false, p, &gg, ctx, stream, true)) return r;
            double hc[2];
            CBET_HIP(hipMemcpyAsync(hc, change, sizeof hc, hipMemcpyDeviceToHost, s));
            CBET_HIP(hipStreamSynchronize(s));
            rep.passes = pass + 1;
            rep.change = hc[1] > 0.0 ? hc[0] / hc[1] : 0.0;
            if (rep.change < g->tolerance) { rep.converged = 1; break; }
        }
        CBET_HIP(hipMemsetAsync(beam_gain, 0, CBET_MAX_CBET_BEAMS * sizeof(double), s));
        if (int r = cbet_context_counters(ctx, stream, &c1, 0)) return r;
        rep.ray_steps = c1.ray_steps - c0.ray_steps;
        CbetHooks h;
        h.gain = gain; h.quantity = 0; h.beam_gain = beam_gain; h.max_exponent = g->max_exponent;
        if (int r = trace_impl(0, (unsigned)d.nindices, nullptr, nullptr, edep, bbeam_norm, beam_norm, pow_r, phase_r,
                               d.xconst, d.yconst, d.zconst, &pd, ctx, stream, h))
            return r;
        CBET_HIP(hipMemcpyAsync(rep.beam_gain, beam_gain, nb * sizeof(double), hipMemcpyDeviceToHost, s));
        cbet_counters c2{};
        if (int r = cbet_context_counters(ctx, stream, &c2, 0)) return r;   // synchronises
        rep.ray_steps_final = c2.ray_steps - c1.ray_steps;
        rep.ray_steps += rep.ray_steps_final;
        double net = 0.0, mag = 0.0;
        for (size_t bb = 0; bb < nb; ++bb) { net += rep.beam_gain[bb]; mag += std::fabs(rep.beam_gain[bb]); }
        rep.imbalance = mag > 0.0 ? std::fabs(net) / mag : 0.0;
        return CBET_OK;
    };
    rc = body();
    if (own) {
        (void)hipStreamSynchronize(s);
        (void)hipFree(ws);
    }
    if (rc == CBET_OK && report) *report = rep;
    return rc;
}

const double *cbet_cbet_workspace_gain(const cbet_params *p, const void *workspace)
{
    if (!p || !workspace || validate(p) != CBET_OK) return nullptr;
    const size_t hsize = (size_t)(p->nx + 2) * (p->ny + 2) * (p->nz + 2);
    return (const double *)workspace + 4 * (size_t)p->nbeams * hsize;   // the layout of cbet_cbet_solve's workspace
}

}  // extern "C"
