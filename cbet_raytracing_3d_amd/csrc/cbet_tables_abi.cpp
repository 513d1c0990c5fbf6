// cbet_tables_abi.cpp -- the table entry points of the C ABI (include/cbet_mi355x.h): node tables (plain, on a perturbed
// target), the gain kernels' flow table, the step records and the fused tables-and-records launch.
#include "cbet_host_internal.h"

using namespace cbet;

TabulateArgs cbet::tabulate_args(const cbet_params *p, const cbet_derived &d, double *ne3d, double *kap3d,
                                 const double *te, const double *r, const double *ne)
{
    TabulateArgs t{};
    grid_args(t, p, d);
    t.nprofile = p->nprofile;
    t.dt = d.dt;
    t.ncrit = d.ncrit;
    t.r = r; t.ne = ne; t.te = te;
    t.ne3d = ne3d; t.kap3d = kap3d;
    return t;
}

// The cache key of the context's step records: what they were built from (step_records compares against it).
static void key_records(cbet_context *ctx, unsigned long long version, const double *ne, const double *kap, double xconst,
                        double yconst, double zconst)
{
    ++ctx->rec_builds;
    ctx->rec_version = version;
    ctx->rec_ne3d = ne; ctx->rec_kap3d = kap;
    ctx->rec_const[0] = xconst; ctx->rec_const[1] = yconst; ctx->rec_const[2] = zconst;
}

// Build the per-node step records (cbet_device.h StepRecord) the LDS_WINDOW kernel gathers from: ne3d / kappa3d
// NULL = the context's own tables.  Records built from the context's tables stay valid until the next
// cbet_tabulate_plasma; records built from caller-owned tables are rebuilt by every launch (their contents may
// have changed).
int cbet::step_records(cbet_context *ctx, const cbet_params *p, const double *ne3d, const double *kappa3d,
                       double xconst, double yconst, double zconst, void *stream, bool force)
{
    const bool own = !ne3d && !kappa3d;
    const double *ne = ne3d ? ne3d : ctx->ne3d, *kap = kappa3d ? kappa3d : ctx->kap3d;
    if (!force && own && ctx->rec_version == ctx->tables_version && ctx->rec_ne3d == ne && ctx->rec_kap3d == kap &&
        ctx->rec_const[0] == xconst && ctx->rec_const[1] == yconst && ctx->rec_const[2] == zconst)
        return CBET_OK;
    StepTableArgs t{};
    grid_dims(t, p);
    t.xconst = xconst; t.yconst = yconst; t.zconst = zconst;
    t.ne3d = ne; t.kap3d = kap; t.rec = ctx->steprec;
    CBET_HIP(launch_step_table(t, (hipStream_t)stream));
    key_records(ctx, own ? ctx->tables_version : ~0ull, ne, kap, xconst, yconst, zconst);
    return CBET_OK;
}

// A context's own flow, state, detuning or bandwidth table, allocated by the first call on a context (not capturable).  The
// context's device is current.
int cbet::own_table(double **slot, size_t doubles, const char *what)
{
    if (*slot) return CBET_OK;
    hipError_t e = hipMalloc((void **)slot, doubles * sizeof(double));
    if (e != hipSuccess) {
        *slot = nullptr;
        return fail_hip(e == hipErrorOutOfMemory ? CBET_ENOMEM : CBET_EHIP, "hipMalloc(%s): %s", what, hipGetErrorString(e));
    }
    return CBET_OK;
}

extern "C" {

int cbet_tabulate_plasma(cbet_context *ctx, const cbet_params *p, const double *te_data_g,
                         const double *r_data_g, const double *ne_data_g, void *stream)
{
    if (int rc = entry_checks(ctx, p)) return rc;
    if (!te_data_g || !r_data_g || !ne_data_g) return fail(CBET_EINVAL, "NULL profile pointer");
    CBET_ENTER_DEVICE(ctx);
    const TabulateArgs a = tabulate_args(p, ctx->d, ctx->ne3d, ctx->kap3d, te_data_g, r_data_g, ne_data_g);
    CBET_HIP(launch_tabulate(a, (hipStream_t)stream));
    ++ctx->tables_version;   // step records built from the old tables are stale
    return CBET_OK;
}

// cbet_tabulate_plasma on a displaced, Y_lm-distorted target (k_tabulate_target): the same duties towards the context.
int cbet_tabulate_target(cbet_context *ctx, const cbet_params *p, const double *te_data_g, const double *r_data_g,
                         const double *ne_data_g, const cbet_target *target, void *stream)
{
    if (int rc = entry_checks(ctx, p)) return rc;
    if (!te_data_g || !r_data_g || !ne_data_g) return fail(CBET_EINVAL, "NULL profile pointer");
    int inst;
    if (int rc = target_check(target, &inst)) return rc;
    CBET_ENTER_DEVICE(ctx);
    TargetArgs a{};
    a.t = tabulate_args(p, ctx->d, ctx->ne3d, ctx->kap3d, te_data_g, r_data_g, ne_data_g);
    target_fill(target, &a);
    CBET_HIP(launch_tabulate_target(a, inst, (hipStream_t)stream));
    ++ctx->tables_version;   // step records built from the old tables are stale
    return CBET_OK;
}

int cbet_prepare_step_records(cbet_context *ctx, const cbet_params *p, const double *ne3d, const double *kappa3d,
                              double xconst, double yconst, double zconst, void *stream)
{
    if (int rc = entry_checks(ctx, p)) return rc;
    CBET_ENTER_DEVICE(ctx);
    return step_records(ctx, p, ne3d, kappa3d, xconst, yconst, zconst, stream, true);
}

// cbet_tabulate_plasma directly followed by cbet_prepare_step_records of the context's own tables, as ONE kernel
// (k_plasma_records): the same tables, the same records, the same cache key as the two calls leave behind.  A profile
// too long for the fused kernel's LDS budget (the ring beside the staged profile, 64 KB) takes the two kernels.
int cbet_prepare_plasma(cbet_context *ctx, const cbet_params *p, const double *te_data_g, const double *r_data_g,
                        const double *ne_data_g, double xconst, double yconst, double zconst, void *stream)
{
    if (int rc = entry_checks(ctx, p)) return rc;
    if (!te_data_g || !r_data_g || !ne_data_g) return fail(CBET_EINVAL, "NULL profile pointer");
    if (plasma_records_lds(p->nprofile) > 65536) {
        if (int rc = cbet_tabulate_plasma(ctx, p, te_data_g, r_data_g, ne_data_g, stream)) return rc;
        return cbet_prepare_step_records(ctx, p, nullptr, nullptr, xconst, yconst, zconst, stream);
    }
    CBET_ENTER_DEVICE(ctx);
    PlasmaRecordsArgs a{};
    a.t = tabulate_args(p, ctx->d, ctx->ne3d, ctx->kap3d, te_data_g, r_data_g, ne_data_g);
    a.xconst = xconst; a.yconst = yconst; a.zconst = zconst;
    a.rec = ctx->steprec;
    CBET_HIP(launch_plasma_records(a, (hipStream_t)stream));
    ++ctx->tables_version;
    key_records(ctx, ctx->tables_version, ctx->ne3d, ctx->kap3d, xconst, yconst, zconst);
    return CBET_OK;
}

// ---- flow table of the gain kernels --------------------------------------------
int cbet_tabulate_flow(cbet_context *ctx, const cbet_params *p, const cbet_gain_params *g, const cbet_target *target,
                       void *stream)
{
    if (int rc = entry_checks(ctx, p)) return rc;
    if (int rc = validate_gain(p, g)) return rc;
    int inst = 0;
    if (target)
        if (int rc = target_check(target, &inst)) return rc;
    double cs = 0;
    if (int rc = cbet_gain_constants(p, g, nullptr, &cs, nullptr)) return rc;
    CBET_ENTER_DEVICE(ctx);
    if (int rc = flow_own_table(ctx, p)) return rc;
    CBET_HIP(launch_tabulate_flow(flow_args(p, ctx->d, g, cs, target, ctx->flow_own), inst, (hipStream_t)stream));
    ctx->flow = ctx->flow_own;
    return CBET_OK;
}

}  // extern "C"
