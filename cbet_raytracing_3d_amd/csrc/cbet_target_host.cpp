// cbet_target_host.cpp -- perturbed targets (include/cbet_mi355x.h, DESIGN.md sections 12 and 13): the recurrence factors,
// the argument checks of the entry points and the host twins of k_tabulate_target and k_tabulate_flow, plain loops over the
// nodes running the kernels' own statements (cbet_target_model.h).
#include <hip/hip_runtime_api.h>

#include <array>
#include <cmath>
#include <cstring>

#include "cbet_host_internal.h"
#include "cbet_target_model.h"

namespace cbet {

const double *target_factors()
{
    static const std::array<double, kTargetFactors> table = [] {
        std::array<double, kTargetFactors> f{};
        f[kTfY00] = 1.0 / std::sqrt(4.0 * M_PI);
        f[kTfSqrt2] = std::sqrt(2.0);
        for (int k = 1; k <= CBET_TARGET_LMAX; ++k) f[kTfD + k] = std::sqrt((double)(2 * k + 1) / (double)(2 * k));
        for (int l = 1; l <= CBET_TARGET_LMAX; ++l)
            for (int m = 0; m < l; ++m) {
                f[kTfA + l * kTargetS + m] = std::sqrt((double)(4 * l * l - 1) / (double)(l * l - m * m));
                f[kTfB + l * kTargetS + m] = std::sqrt((double)((l - 1) * (l - 1) - m * m) / (double)(4 * (l - 1) * (l - 1) - 1));
            }
        return f;
    }();
    return table.data();
}

int target_check(const cbet_target *tg, int *inst)
{
    if (!tg) return fail(CBET_EINVAL, "target is NULL");
    if (tg->lmax < 0 || tg->lmax > CBET_TARGET_LMAX)
        return fail(CBET_EINVAL, "target: lmax = %d outside [0, %d]", tg->lmax, CBET_TARGET_LMAX);
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(tg->offset[i])) return fail(CBET_EINVAL, "target: offset is not finite");
    int top = 0;
    double bound = 0.0;                   // sum |c_lm| sqrt((2l+1) / (4 pi)) >= max |delta|
    if (tg->coeffs)
        for (int l = 0; l <= tg->lmax; ++l)
            for (int c = l * l; c < (l + 1) * (l + 1); ++c) {
                if (!std::isfinite(tg->coeffs[c])) return fail(CBET_EINVAL, "target: coefficient %d is not finite", c);
                if (tg->coeffs[c] != 0.0) top = l;
                bound += std::fabs(tg->coeffs[c]) * std::sqrt((2 * l + 1) / (4.0 * M_PI));
            }
    if (!(bound < 1.0))
        return fail(CBET_EINVAL, "target: sum |c_lm| sqrt((2l+1)/(4 pi)) = %g must stay below 1 (1 + delta > 0)", bound);
    *inst = top == 0 ? 0 : top <= 2 ? 2 : top <= 8 ? 8 : 16;
    return CBET_OK;
}

// Offset and coefficients (zero beyond the call's lmax) into an argument block that carries ox, oy, oz and c.
template <class Args>
static void fill_target(const cbet_target *tg, Args *a)
{
    a->ox = tg->offset[0]; a->oy = tg->offset[1]; a->oz = tg->offset[2];
    std::memset(a->c, 0, sizeof a->c);
    if (tg->coeffs) std::memcpy(a->c, tg->coeffs, sizeof(double) * (tg->lmax + 1) * (tg->lmax + 1));
}

void target_fill(const cbet_target *tg, TargetArgs *a) { fill_target(tg, a); }

FlowArgs flow_args(const cbet_params *p, const cbet_derived &d, const cbet_gain_params *g, double cs,
                   const cbet_target *target, double *out)
{
    FlowArgs a{};
    grid_args(a, p, d);
    ramp_args(a, g, cs);
    a.flow = out;
    if (target) fill_target(target, &a);
    return a;
}

namespace {

template <int L>
void host_tables(const TargetArgs &a, const double *r, const double *ne, const double *te)
{
    const TabulateArgs &t = a.t;
    const double *F = target_factors();
    for_each_node_host(t.nx, t.ny, t.nz, [&](int i, int j, int k, long idx) {
        target_node<L>(a, F, a.c, r, ne, te, i, j, k, t.ne3d[idx], t.kap3d[idx], TargetNoPin());
    });
}

template <int L>
void host_flow(const FlowArgs &a)
{
    const double *F = target_factors();
    const long nodes = (long)a.nx * a.ny * a.nz;
    for_each_node_host(a.nx, a.ny, a.nz, [&](int i, int j, int k, long idx) {
        target_flow<L>(a, F, a.c, i, j, k, a.flow[idx], a.flow[idx + nodes], a.flow[idx + 2 * nodes], TargetNoPin());
    });
}

}  // namespace
}  // namespace cbet

extern "C" int cbet_target_tables(const cbet_params *p, const double *te, const double *r, const double *ne,
                                  const cbet_target *target, double *ne3d, double *kappa3d)
{
    using namespace cbet;
    cbet_derived d;
    if (int rc = derive_grid(p, &d)) return rc;
    if (!te || !r || !ne) return fail(CBET_EINVAL, "NULL profile pointer");
    if (!ne3d || !kappa3d) return fail(CBET_EINVAL, "target_tables: NULL output");
    int inst;
    if (int rc = target_check(target, &inst)) return rc;
    TargetArgs a{};
    a.t = tabulate_args(p, d, ne3d, kappa3d, nullptr, nullptr, nullptr);   // the profiles go to host_tables beside the block
    target_fill(target, &a);
    dispatch_lmax(inst, [&](auto l) { host_tables<decltype(l)::value>(a, r, ne, te); });
    return CBET_OK;
}

// The host twin of k_tabulate_flow (cbet_target.hip).
extern "C" int cbet_flow_table(const cbet_params *p, const cbet_gain_params *g, const cbet_target *target, double *out)
{
    using namespace cbet;
    cbet_derived d;
    if (int rc = derive_grid(p, &d)) return rc;
    double cs = 0;
    if (int rc = cbet_gain_constants(p, g, nullptr, &cs, nullptr)) return rc;   // (validates the gain parameters)
    if (!out) return fail(CBET_EINVAL, "flow_table: NULL output");
    int inst = 0;
    if (target)
        if (int rc = target_check(target, &inst)) return rc;
    const FlowArgs a = flow_args(p, d, g, cs, target, out);
    dispatch_lmax(inst, [&](auto l) { host_flow<decltype(l)::value>(a); });
    return CBET_OK;
}
