// cbet_context.cpp -- the multi_gpu.cuh helper counterparts, the per-device context with its accessors, the checks
// a launch makes against it and the default-context map.
// Citations are into /root/reference/.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "cbet_host_internal.h"

using namespace cbet;

// The launch must describe the grid / ray geometry the workspace was sized for.
int cbet::check_geometry(const cbet_context *ctx, const cbet_params *p)
{
    const cbet_params &q = ctx->p;
    if (p->nx != q.nx || p->ny != q.ny || p->nz != q.nz || p->xmin != q.xmin || p->xmax != q.xmax ||
        p->ymin != q.ymin || p->ymax != q.ymax || p->zmin != q.zmin || p->zmax != q.zmax ||
        p->rays_per_zone != q.rays_per_zone || p->nbeams != q.nbeams || p->nprofile != q.nprofile ||
        p->max_threads != q.max_threads || p->threads_per_block != q.threads_per_block ||
        p->courant_mult != q.courant_mult || p->patch_order != q.patch_order || p->rim_merge != q.rim_merge)
        return fail(CBET_EINVAL, "launch parameters do not match the geometry the context was created for");
    return CBET_OK;
}

int cbet::entry_checks(const cbet_context *ctx, const cbet_params *p)
{
    if (!ctx) return fail(CBET_EINVAL, "NULL context");
    if (int rc = validate(p)) return rc;
    return check_geometry(ctx, p);
}

// One lazily created workspace per device for callers that pass ctx == NULL (the reference's
// launch site has nothing to pass).  Recreated when the geometry changes.
static std::mutex g_ctx_mu;
static std::map<int, cbet_context *> g_default_ctx;

int cbet::default_context(const cbet_params *p, cbet_context **out)
{
    int dev = 0;
    CBET_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    auto it = g_default_ctx.find(dev);
    if (it != g_default_ctx.end()) {
        if (check_geometry(it->second, p) == CBET_OK) {
            *out = it->second;
            return CBET_OK;
        }
        cbet_context_destroy(it->second);
        g_default_ctx.erase(it);
    }
    cbet_context *ctx = nullptr;
    if (int rc = cbet_context_create(&ctx, p, dev)) return rc;
    g_default_ctx[dev] = ctx;
    *out = ctx;
    return CBET_OK;
}

extern "C" {

// ---- multi_gpu.cpp:3-28 ---------------------------------------------------------------------
int cbet_safeGPUAlloc(void **dst, size_t size, int gpu)
{
    if (!dst) return fail(CBET_EINVAL, "dst is NULL");
    hipError_t e = hipSetDevice(gpu);  // stays current, as in the reference (:7)
    if (e != hipSuccess) return fail_hip(CBET_ENODEVICE, "hipSetDevice(%d): %s", gpu, hipGetErrorString(e));
    size_t free_b = 0, total_b = 0;
    e = hipMemGetInfo(&free_b, &total_b);
    if (e != hipSuccess) return fail_hip(CBET_EHIP, "Error encountered during hipMemGetInfo: %s", hipGetErrorString(e));
    if (free_b < size) return fail_hip(CBET_ENOMEM, "GPU: %d is out of memory", gpu);
    e = hipMalloc(dst, size);
    if (e != hipSuccess) return fail_hip(CBET_EHIP, "Error encountered during hipMalloc: %s", hipGetErrorString(e));
    return CBET_OK;
}

// ---- multi_gpu.cpp:44-59 --------------------------------------------------------------------
int cbet_moveToAndFromGPU(void *dst, void *src, size_t size, int gpu)
{
    if (gpu == -1) return fail_hip(CBET_ENODEVICE, "Attempting to move data that has not been assigned a GPU");
    if (size && (!dst || !src)) return fail(CBET_EINVAL, "NULL pointer");
    DeviceGuard guard;
    hipError_t e = hipSetDevice(gpu);
    if (e != hipSuccess) return fail_hip(CBET_ENODEVICE, "hipSetDevice(%d): %s", gpu, hipGetErrorString(e));
    e = hipMemcpy(dst, src, size, hipMemcpyDefault);
    if (e != hipSuccess) return fail_hip(CBET_EHIP, "Error encountered during hipMemcpy: %s", hipGetErrorString(e));
    return CBET_OK;
}

int cbet_gpuFree(void *ptr, int gpu)
{
    DeviceGuard guard;
    hipError_t e = hipSetDevice(gpu);
    if (e != hipSuccess) return fail_hip(CBET_ENODEVICE, "hipSetDevice(%d): %s", gpu, hipGetErrorString(e));
    CBET_HIP(hipFree(ptr));
    return CBET_OK;
}

// ---- the per-device context --------------------------------------------------------------------------------
int cbet_context_destroy(cbet_context *ctx)
{
    if (!ctx) return CBET_OK;
    DeviceGuard guard;
    (void)hipSetDevice(ctx->gpu);
    (void)hipFree(ctx->ne3d);
    (void)hipFree(ctx->kap3d);
    (void)hipFree(ctx->steprec);
    (void)hipFree(ctx->xlaunch);
    (void)hipFree(ctx->ylaunch);
    (void)hipFree(ctx->bounds);
    (void)hipFree(ctx->live);
    (void)hipFree(ctx->counters);
    (void)hipFree(ctx->flow_own);
    (void)hipFree(ctx->state_own);
    (void)hipFree(ctx->shift_own);
    (void)hipFree(ctx->band_own);
    delete ctx;
    return CBET_OK;
}

// A caller that knows how long its rays live (a previous pass's per-ray step counts, a model) may regroup the bundles:
// the same rays, every one exactly once, in any grouping of 64 and any order.  Synchronises the device (a launch may
// still be reading the old list).
int cbet_context_set_launch_list(cbet_context *ctx, const int *list, long n)
{
    if (!ctx || !list) return fail(CBET_EINVAL, "NULL context or list");
    if (n <= 0 || n % kWave != 0) return fail(CBET_EINVAL, "a launch list is a whole number of 64-entry bundles (got %ld entries)", n);
    CBET_ENTER_DEVICE(ctx);
    CBET_HIP(hipDeviceSynchronize());
    std::vector<int> cur((size_t)ctx->nlive), want, got;
    if (ctx->nlive) CBET_HIP(hipMemcpy(cur.data(), ctx->live, cur.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int v : cur) if (v >= 0) want.push_back(v);
    for (long i = 0; i < n; ++i) {
        if (list[i] >= 0) got.push_back(list[i]);
        else if (list[i] != -1) return fail(CBET_EINVAL, "launch list entry %ld is %d (a ray id or -1)", i, list[i]);
    }
    for (long b = 0; b < n; b += kWave) {
        bool any = false;
        for (int l = 0; l < kWave; ++l) any = any || list[b + l] >= 0;
        if (!any) return fail(CBET_EINVAL, "bundle %ld of the launch list is empty", b / kWave);
    }
    std::sort(want.begin(), want.end());
    std::sort(got.begin(), got.end());
    if (want != got) return fail(CBET_EINVAL, "the launch list must hold exactly the context's live rays, each once (%zu given, %zu expected)", got.size(), want.size());
    int *fresh = nullptr;
    CBET_HIP(hipMalloc((void **)&fresh, (size_t)n * sizeof(int)));
    hipError_t e = hipMemcpy(fresh, list, (size_t)n * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(fresh); return fail_hip(CBET_EHIP, "hipMemcpy(launch list): %s", hipGetErrorString(e)); }
    (void)hipFree(ctx->live);
    ctx->live = fresh;
    ctx->nlive = (int)n;
    return CBET_OK;
}

int cbet_context_create(cbet_context **out, const cbet_params *p, int gpu)
{
    if (!out) return fail(CBET_EINVAL, "ctx out-pointer is NULL");
    *out = nullptr;
    cbet_derived d;
    std::vector<double> xl, yl;
    std::vector<int> live;
    if (int rc = derive_launch(p, &d, xl, yl, live)) return rc;   // (validates p)

    DeviceGuard guard;
    hipError_t e = hipSetDevice(gpu);
    if (e != hipSuccess) return fail_hip(CBET_ENODEVICE, "hipSetDevice(%d): %s", gpu, hipGetErrorString(e));
    cbet_context *ctx = new cbet_context;
    ctx->gpu = gpu;
    ctx->p = *p;
    ctx->d = d;
    ctx->nlive = (int)live.size();
    const size_t nodes = (size_t)p->nx * p->ny * p->nz;
    auto bail = [&](hipError_t err, const char *what) {
        cbet_context_destroy(ctx);
        return fail_hip(err == hipErrorOutOfMemory ? CBET_ENOMEM : CBET_EHIP, "%s: %s", what, hipGetErrorString(err));
    };
    if ((e = hipMalloc((void **)&ctx->ne3d, nodes * sizeof(double))) != hipSuccess) return bail(e, "hipMalloc(ne3d)");
    if ((e = hipMalloc((void **)&ctx->kap3d, nodes * sizeof(double))) != hipSuccess) return bail(e, "hipMalloc(kappa3d)");
    if ((e = hipMalloc((void **)&ctx->steprec, nodes * sizeof(StepRecord))) != hipSuccess) return bail(e, "hipMalloc(step records)");
    if ((e = hipMalloc((void **)&ctx->xlaunch, xl.size() * sizeof(double))) != hipSuccess) return bail(e, "hipMalloc(xlaunch)");
    if ((e = hipMalloc((void **)&ctx->ylaunch, yl.size() * sizeof(double))) != hipSuccess) return bail(e, "hipMalloc(ylaunch)");
    if ((e = hipMalloc((void **)&ctx->bounds, 6 * sizeof(double))) != hipSuccess) return bail(e, "hipMalloc(bounds)");
    {
        double hb[6];
        host_exit_planes(p, d, hb);
        if ((e = hipMemcpy(ctx->bounds, hb, sizeof hb, hipMemcpyHostToDevice)) != hipSuccess) return bail(e, "hipMemcpy(bounds)");
    }
    if ((e = hipMalloc((void **)&ctx->live, std::max<size_t>(1, live.size()) * sizeof(int))) != hipSuccess) return bail(e, "hipMalloc(live)");
    if ((e = hipMalloc((void **)&ctx->counters, kCntSlots * sizeof(unsigned long long))) != hipSuccess) return bail(e, "hipMalloc(counters)");
    if ((e = hipMemcpy(ctx->xlaunch, xl.data(), xl.size() * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess) return bail(e, "hipMemcpy(xlaunch)");
    if ((e = hipMemcpy(ctx->ylaunch, yl.data(), yl.size() * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess) return bail(e, "hipMemcpy(ylaunch)");
    if (!live.empty() &&
        (e = hipMemcpy(ctx->live, live.data(), live.size() * sizeof(int), hipMemcpyHostToDevice)) != hipSuccess)
        return bail(e, "hipMemcpy(live)");
    if ((e = hipMemset(ctx->counters, 0, kCntSlots * sizeof(unsigned long long))) != hipSuccess) return bail(e, "hipMemset(counters)");
    // the recurrence factors of cbet_tabulate_target and cbet_tabulate_flow into this device's constant memory (the same
    // bytes every time)
    if ((e = target_upload_factors()) != hipSuccess) return bail(e, "hipMemcpyToSymbol(target factors)");
    *out = ctx;
    return CBET_OK;
}

int cbet_context_counters(cbet_context *ctx, void *stream, cbet_counters *out, int reset)
{
    if (!ctx || !out) return fail(CBET_EINVAL, "NULL context/counters");
    CBET_ENTER_DEVICE(ctx);
    hipStream_t s = (hipStream_t)stream;
    unsigned long long h[kCntSlots];
    CBET_HIP(hipMemcpyAsync(h, ctx->counters, sizeof h, hipMemcpyDeviceToHost, s));
    if (reset) CBET_HIP(hipMemsetAsync(ctx->counters, 0, sizeof h, s));
    CBET_HIP(hipStreamSynchronize(s));
    std::memset(out, 0, sizeof *out);
    out->ray_steps = h[kCntSteps];
    out->rays_traced = h[kCntRays];
    out->global_atomics = h[kCntGlobalAtomics];
    out->lds_evictions = h[kCntEvictions];
    out->wave_steps = h[kCntWaveSteps];
    out->wave_steps_miss = h[kCntWaveStepsMiss];
    out->wave_steps_wide = h[kCntWaveStepsWide];
    out->slabs_retired = h[kCntSlabsRetired];
    return CBET_OK;
}

int cbet_debug_bounds_violations(unsigned long long *out, int reset, void *stream)
{
    if (!out) return fail(CBET_EINVAL, "out is NULL");
    hipError_t e = audit_violations(out, reset != 0, (hipStream_t)stream);
    if (e == hipErrorNotSupported) return fail(CBET_EINVAL, "not a bounds-audit build (compile with -DCBET_DEBUG_BOUNDS)");
    if (e != hipSuccess) return fail_hip(CBET_EHIP, "audit_violations: %s", hipGetErrorString(e));
    return CBET_OK;
}

int cbet_context_list_length(const cbet_context *ctx, long *length)
{
    if (!ctx || !length) return fail(CBET_EINVAL, "NULL context/length");
    *length = ctx->nlive;
    return CBET_OK;
}

int cbet_context_tables(cbet_context *ctx, double **ne3d, double **kappa3d)
{
    if (!ctx) return fail(CBET_EINVAL, "NULL context");
    if (ne3d) *ne3d = ctx->ne3d;
    if (kappa3d) *kappa3d = ctx->kap3d;
    ++ctx->tables_version;   // the pointers are writable: records built from the old contents are no longer trusted
    return CBET_OK;
}

int cbet_context_step_records(const cbet_context *ctx, const void **records, unsigned long long *builds)
{
    if (!ctx) return fail(CBET_EINVAL, "NULL context");
    if (records) *records = ctx->steprec;
    if (builds) *builds = ctx->rec_builds;
    return CBET_OK;
}

int cbet_context_set_flow(cbet_context *ctx, const double *flow)
{
    if (!ctx) return fail(CBET_EINVAL, "NULL context");
    ctx->flow = flow;
    return CBET_OK;
}

int cbet_context_flow(cbet_context *ctx, void **out)
{
    if (!ctx || !out) return fail(CBET_EINVAL, "NULL context/out");
    *out = const_cast<double *>(ctx->flow);
    return CBET_OK;
}

int cbet_context_set_state(cbet_context *ctx, const double *state)
{
    if (!ctx) return fail(CBET_EINVAL, "NULL context");
    ctx->state = state;
    return CBET_OK;
}

int cbet_context_state(cbet_context *ctx, void **out)
{
    if (!ctx || !out) return fail(CBET_EINVAL, "NULL context/out");
    *out = const_cast<double *>(ctx->state);
    return CBET_OK;
}

int cbet_context_set_saturation(cbet_context *ctx, double dn_max)
{
    if (std::isnan(dn_max)) return fail(CBET_EINVAL, "cbet_context_set_saturation: dn_max is NaN (a finite limit > 0, or 0 = none)");
    if (std::isinf(dn_max)) return fail(CBET_EINVAL, "cbet_context_set_saturation: dn_max is infinite (a finite limit > 0, or 0 = none)");
    if (dn_max < 0.0) return fail(CBET_EINVAL, "cbet_context_set_saturation: dn_max = %g is negative (a finite limit > 0, or 0 = none)", dn_max);
    if (!ctx) return fail(CBET_EINVAL, "NULL context");
    ctx->dn_max = dn_max;
    return CBET_OK;
}

int cbet_context_saturation(cbet_context *ctx, double *out)
{
    if (!ctx || !out) return fail(CBET_EINVAL, "NULL context/out");
    *out = ctx->dn_max;
    return CBET_OK;
}

// The values are judged before the context, as cbet_context_set_saturation judges its own: a refusal needs no device.
int cbet_context_set_detuning(cbet_context *ctx, const double *domega, int nbeams, void *stream)
{
    if (domega) {
        if (nbeams > CBET_MAX_CBET_BEAMS)
            return fail(CBET_EINVAL, "cbet_context_set_detuning: nbeams = %d exceeds CBET_MAX_CBET_BEAMS = %d", nbeams, CBET_MAX_CBET_BEAMS);
        if (nbeams < 1) return fail(CBET_EINVAL, "cbet_context_set_detuning: nbeams = %d (one shift per beam)", nbeams);
        for (int b = 0; b < nbeams; ++b) {
            if (std::isnan(domega[b])) return fail(CBET_EINVAL, "cbet_context_set_detuning: domega[%d] is NaN (finite shifts in rad/s, or NULL = none)", b);
            if (std::isinf(domega[b])) return fail(CBET_EINVAL, "cbet_context_set_detuning: domega[%d] is infinite (finite shifts in rad/s, or NULL = none)", b);
        }
    }
    if (!ctx) return fail(CBET_EINVAL, "NULL context");
    if (domega && nbeams != ctx->p.nbeams)
        return fail(CBET_EINVAL, "cbet_context_set_detuning: nbeams = %d, the context was created for %d beams", nbeams, ctx->p.nbeams);
    bool one_colour = true;
    for (int b = 1; domega && b < nbeams; ++b) one_colour = one_colour && domega[b] == domega[0];
    if (one_colour) {                       // only differences enter the model: nothing to carry
        ctx->shift = nullptr;
        return CBET_OK;
    }
    CBET_ENTER_DEVICE(ctx);
    if (int rc = own_table(&ctx->shift_own, CBET_MAX_CBET_BEAMS, "detuning table")) return rc;
    double fresh[CBET_MAX_CBET_BEAMS] = {};   // an entry per possible beam: zero past nbeams
    for (int b = 0; b < nbeams; ++b) fresh[b] = domega[b];
    CBET_HIP(hipStreamSynchronize((hipStream_t)stream));   // a launch in flight may still read the old values
    CBET_HIP(hipMemcpy(ctx->shift_own, fresh, sizeof fresh, hipMemcpyHostToDevice));
    std::memcpy(ctx->shift_host, fresh, sizeof fresh);
    ctx->shift = ctx->shift_own;
    return CBET_OK;
}

int cbet_context_detuning(cbet_context *ctx, double *out, int *nbeams)
{
    if (!ctx || !nbeams) return fail(CBET_EINVAL, "NULL context/nbeams");
    *nbeams = ctx->shift ? ctx->p.nbeams : 0;
    if (out)
        for (int b = 0; b < *nbeams; ++b) out[b] = ctx->shift_host[b];
    return CBET_OK;
}

int cbet_context_set_polarization(cbet_context *ctx, int mode)
{
    if (mode != CBET_POL_ALIGNED && mode != CBET_POL_SMOOTHED)
        return fail(CBET_EINVAL, "cbet_context_set_polarization: mode = %d is unknown (CBET_POL_ALIGNED = %d or CBET_POL_SMOOTHED = %d)",
                    mode, CBET_POL_ALIGNED, CBET_POL_SMOOTHED);
    if (!ctx) return fail(CBET_EINVAL, "cbet_context_set_polarization: NULL context");
    ctx->pol = mode;
    return CBET_OK;
}

int cbet_context_polarization(cbet_context *ctx, int *mode)
{
    if (!ctx || !mode) return fail(CBET_EINVAL, "NULL context/mode");
    *mode = ctx->pol;
    return CBET_OK;
}

// The lines are judged before the context, as cbet_context_set_detuning judges its shifts: a refusal needs no device.
int cbet_context_set_bandwidth(cbet_context *ctx, const double *line_domega, const double *line_weight, int nlines, void *stream)
{
    if (int rc = band_check("cbet_context_set_bandwidth", line_domega, line_weight, nlines)) return rc;
    if (!ctx) return fail(CBET_EINVAL, "cbet_context_set_bandwidth: NULL context");
    constexpr int kTable = 1 + 2 * kBandMax;
    double fresh[kTable + CBET_MAX_CBET_BEAMS] = {}, norm[CBET_MAX_BAND_LINES] = {};   // the table, then the zero shifts
    const int M = (line_domega && line_weight && nlines > 1) ? band_table(line_domega, line_weight, nlines, fresh, norm) : 0;
    if (M == 0) {                           // no lines, one line or equal offsets: only differences enter the model
        ctx->band = nullptr;
        ctx->nband = 0;
        ctx->nlines = 0;
        return CBET_OK;
    }
    CBET_ENTER_DEVICE(ctx);
    if (int rc = own_table(&ctx->band_own, sizeof fresh / sizeof(double), "bandwidth table")) return rc;
    CBET_HIP(hipStreamSynchronize((hipStream_t)stream));   // a launch in flight may still read the old values
    CBET_HIP(hipMemcpy(ctx->band_own, fresh, sizeof fresh, hipMemcpyHostToDevice));
    ctx->band = ctx->band_own;
    ctx->nband = M;
    ctx->nlines = nlines;
    for (int a = 0; a < nlines; ++a) { ctx->line_domega[a] = line_domega[a]; ctx->line_weight[a] = norm[a]; }
    return CBET_OK;
}

int cbet_context_bandwidth(cbet_context *ctx, double *line_domega, double *line_weight, int *nlines)
{
    if (!ctx || !nlines) return fail(CBET_EINVAL, "NULL context/nlines");
    *nlines = ctx->band ? ctx->nlines : 0;
    for (int a = 0; a < *nlines; ++a) {
        if (line_domega) line_domega[a] = ctx->line_domega[a];
        if (line_weight) line_weight[a] = ctx->line_weight[a];
    }
    return CBET_OK;
}

}  // extern "C"
