// cbet_mesh_host.cpp -- plasma on a spherical-polar mesh (include/cbet_mi355x.h "hydro-mesh plasma", DESIGN.md section
// 14, the state table of section 16): the checks of a mesh, the argument block, the entry points of k_tabulate_mesh,
// k_mesh_flow and k_mesh_state (cbet_mesh.hip) and their host twins, plain loops over the nodes running the kernels' own
// statements (cbet_mesh_model.h).
#include <hip/hip_runtime_api.h>

#include <cmath>

#include "cbet_host_internal.h"
#include "cbet_mesh_model.h"

namespace cbet {

namespace {

// The first entry of f[n] that is not finite or lies below `least` (at it, if `strict`), -1 if none.
long first_bad(const double *f, long n, double least, bool strict)
{
    for (long i = 0; i < n; ++i)
        if (!std::isfinite(f[i]) || f[i] < least || (strict && f[i] == least)) return i;
    return -1;
}

int check_axis(const char *name, const double *x, int n)
{
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(x[i])) return fail(CBET_EINVAL, "mesh: %s[%d] is not finite", name, i);
    for (int i = 1; i < n; ++i)
        if (!(x[i] > x[i - 1]))
            return fail(CBET_EINVAL, "mesh: %s must be strictly ascending (%s[%d] = %g after %g)", name, name, i, x[i], x[i - 1]);
    return CBET_OK;
}

}  // namespace

int mesh_check(const cbet_mesh *m, bool whole)
{
    if (!m) return fail(CBET_EINVAL, "mesh is NULL");
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(m->center[i])) return fail(CBET_EINVAL, "mesh: center is not finite");
    if (m->nr < 2 || m->ntheta < 1 || m->nphi < 1)
        return fail(CBET_EINVAL, "mesh: nr = %d, ntheta = %d, nphi = %d (nr >= 2, ntheta >= 1, nphi >= 1)", m->nr, m->ntheta, m->nphi);
    if ((long)m->nr + m->ntheta + m->nphi > CBET_MESH_MAX_COORDS)
        return fail(CBET_EINVAL, "mesh: nr + ntheta + nphi = %ld exceeds CBET_MESH_MAX_COORDS = %d", (long)m->nr + m->ntheta + m->nphi,
                    CBET_MESH_MAX_COORDS);
    if (!m->r || !m->theta || !m->phi) return fail(CBET_EINVAL, "mesh: NULL coordinate pointer");
    if (!m->ne || !m->te) return fail(CBET_EINVAL, "mesh: NULL ne or te pointer");
    if (!whole) return CBET_OK;
    if (int rc = check_axis("r", m->r, m->nr)) return rc;
    if (m->r[0] < 0.0) return fail(CBET_EINVAL, "mesh: r[0] = %g is negative", m->r[0]);
    if (int rc = check_axis("theta", m->theta, m->ntheta)) return rc;
    if (m->theta[0] < 0.0 || m->theta[m->ntheta - 1] > M_PI) return fail(CBET_EINVAL, "mesh: theta outside [0, pi]");
    if (int rc = check_axis("phi", m->phi, m->nphi)) return rc;
    if (m->phi[0] < -M_PI || !(m->phi[0] < M_PI)) return fail(CBET_EINVAL, "mesh: phi[0] = %g outside [-pi, pi)", m->phi[0]);
    if (!(m->phi[m->nphi - 1] < m->phi[0] + 6.283185307179586))
        return fail(CBET_EINVAL, "mesh: phi spans a whole period or more (phi[nphi-1] = %g, phi[0] = %g)", m->phi[m->nphi - 1], m->phi[0]);
    const long n = (long)m->nr * m->ntheta * m->nphi;
    long bad;
    if ((bad = first_bad(m->ne, n, 0.0, false)) >= 0) return fail(CBET_EINVAL, "mesh: ne[%ld] = %g (finite and >= 0)", bad, m->ne[bad]);
    if ((bad = first_bad(m->te, n, 0.0, true)) >= 0) return fail(CBET_EINVAL, "mesh: te[%ld] = %g (finite and > 0)", bad, m->te[bad]);
    const double *u[3] = {m->ur, m->uth, m->uph};
    const char *names[3] = {"ur", "uth", "uph"};
    for (int c = 0; c < 3; ++c)
        if (u[c] && (bad = first_bad(u[c], n, -HUGE_VAL, false)) >= 0)
            return fail(CBET_EINVAL, "mesh: %s[%ld] is not finite", names[c], bad);
    return CBET_OK;
}

MeshArgs mesh_args(const cbet_params *p, const cbet_derived &d, const cbet_mesh *m, double *ne3d, double *kap3d, double *flow)
{
    MeshArgs a{};
    grid_args(a, p, d);
    a.dt = d.dt;
    a.ncrit = d.ncrit;
    a.ox = m->center[0]; a.oy = m->center[1]; a.oz = m->center[2];
    a.nr = m->nr; a.nth = m->ntheta; a.nph = m->nphi;
    a.r = m->r; a.theta = m->theta; a.phi = m->phi;
    a.ne = m->ne; a.te = m->te;
    a.ur = m->ur; a.uth = m->uth; a.uph = m->uph;
    a.ne3d = ne3d; a.kap3d = kap3d; a.flow = flow;
    return a;
}

MeshArgs mesh_state_args(const cbet_params *p, const cbet_derived &d, const cbet_gain_params *g, const StateConsts &sc,
                         const cbet_mesh *m, const cbet_mesh_ions *ions, double *state)
{
    MeshArgs a = mesh_args(p, d, m, nullptr, nullptr, nullptr);
    a.ti = ions ? ions->ti : nullptr;
    a.zbar = ions ? ions->zbar : nullptr;
    a.ti0 = g->ti_ev; a.z0 = g->z_ion;
    a.sc = sc;
    a.state = state;
    return a;
}

namespace {

enum HostOut { kHostTables, kHostFlow, kHostState };

template <HostOut OUT>
void host_mesh(const MeshArgs &a)
{
    const long nodes = (long)a.nx * a.ny * a.nz;
    for_each_node_host(a.nx, a.ny, a.nz, [&](int i, int j, int k, long idx) {
        MeshNode n;
        mesh_locate(a, a.r, a.theta, a.phi, i, j, k, n);
        if (OUT == kHostFlow) mesh_velocity(a, n, a.flow[idx], a.flow[idx + nodes], a.flow[idx + 2 * nodes]);
        else if (OUT == kHostState) mesh_state(a, n, a.state[idx], a.state[idx + nodes]);
        else mesh_tables(a, n, a.ne3d[idx], a.kap3d[idx]);
    });
}

}  // namespace
}  // namespace cbet

using namespace cbet;

extern "C" {

int cbet_tabulate_mesh(cbet_context *ctx, const cbet_params *p, const cbet_mesh *mesh, void *stream)
{
    if (int rc = entry_checks(ctx, p)) return rc;
    if (int rc = mesh_check(mesh, false)) return rc;
    CBET_ENTER_DEVICE(ctx);
    CBET_HIP(launch_tabulate_mesh(mesh_args(p, ctx->d, mesh, ctx->ne3d, ctx->kap3d, nullptr), (hipStream_t)stream));
    ++ctx->tables_version;   // step records built from the old tables are stale
    return CBET_OK;
}

int cbet_tabulate_mesh_flow(cbet_context *ctx, const cbet_params *p, const cbet_mesh *mesh, void *stream)
{
    if (int rc = entry_checks(ctx, p)) return rc;
    if (int rc = mesh_check(mesh, false)) return rc;
    CBET_ENTER_DEVICE(ctx);
    if (int rc = flow_own_table(ctx, p)) return rc;
    CBET_HIP(launch_mesh_flow(mesh_args(p, ctx->d, mesh, nullptr, nullptr, ctx->flow_own), (hipStream_t)stream));
    ctx->flow = ctx->flow_own;
    return CBET_OK;
}

int cbet_tabulate_mesh_state(cbet_context *ctx, const cbet_params *p, const cbet_gain_params *g, const cbet_mesh *mesh,
                             const cbet_mesh_ions *ions, void *stream)
{
    if (int rc = entry_checks(ctx, p)) return rc;
    StateConsts sc;
    if (int rc = state_consts(p, g, &sc)) return rc;   // (validates the gain parameters)
    if (int rc = mesh_check(mesh, false)) return rc;
    CBET_ENTER_DEVICE(ctx);
    if (int rc = state_own_table(ctx, p)) return rc;
    CBET_HIP(launch_mesh_state(mesh_state_args(p, ctx->d, g, sc, mesh, ions, ctx->state_own), (hipStream_t)stream));
    ctx->state = ctx->state_own;
    return CBET_OK;
}

int cbet_mesh_check(const cbet_mesh *mesh) { return mesh_check(mesh, true); }

int cbet_mesh_tables(const cbet_params *p, const cbet_mesh *mesh, double *ne3d, double *kappa3d)
{
    cbet_derived d;
    if (int rc = derive_grid(p, &d)) return rc;
    if (!ne3d || !kappa3d) return fail(CBET_EINVAL, "mesh_tables: NULL output");
    if (int rc = mesh_check(mesh, true)) return rc;
    host_mesh<kHostTables>(mesh_args(p, d, mesh, ne3d, kappa3d, nullptr));
    return CBET_OK;
}

int cbet_mesh_flow_table(const cbet_params *p, const cbet_mesh *mesh, double *flow)
{
    cbet_derived d;
    if (int rc = derive_grid(p, &d)) return rc;
    if (!flow) return fail(CBET_EINVAL, "mesh_flow_table: NULL output");
    if (int rc = mesh_check(mesh, true)) return rc;
    host_mesh<kHostFlow>(mesh_args(p, d, mesh, nullptr, nullptr, flow));
    return CBET_OK;
}

int cbet_mesh_state_table(const cbet_params *p, const cbet_gain_params *g, const cbet_mesh *mesh, const cbet_mesh_ions *ions,
                          double *out)
{
    cbet_derived d;
    if (int rc = derive_grid(p, &d)) return rc;
    StateConsts sc;
    if (int rc = state_consts(p, g, &sc)) return rc;   // (validates the gain parameters)
    if (!out) return fail(CBET_EINVAL, "mesh_state_table: NULL output");
    if (int rc = mesh_check(mesh, true)) return rc;
    const long n = (long)mesh->nr * mesh->ntheta * mesh->nphi;
    long bad;
    if (ions && ions->ti && (bad = first_bad(ions->ti, n, 0.0, false)) >= 0)
        return fail(CBET_EINVAL, "mesh ions: ti[%ld] = %g (finite and >= 0)", bad, ions->ti[bad]);
    if (ions && ions->zbar && (bad = first_bad(ions->zbar, n, 0.0, true)) >= 0)
        return fail(CBET_EINVAL, "mesh ions: zbar[%ld] = %g (finite and > 0)", bad, ions->zbar[bad]);
    host_mesh<kHostState>(mesh_state_args(p, d, g, sc, mesh, ions, out));
    return CBET_OK;
}

}  // extern "C"
