"""Hydro-mesh plasma on the host (include/cbet_mi355x.h cbet_mesh_tables / cbet_mesh_flow_table): the
host twins of k_tabulate_mesh and k_mesh_flow against the existing tabulation for angle-independent fields (bitwise),
against a numpy restatement for a genuinely 3-D mesh, at the degenerate nodes, for the flow, and their refusals.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

from helpers import mesh_cases as M


@pytest.fixture(scope="module")
def api():
    from cbet_raytracing_3d_amd import api as a
    a.lib()
    return a


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---- 1. angle-independent fields reproduce the existing tabulation ------------------------------------------------------
@pytest.mark.parametrize("shape", M.SHAPES, ids=M.SHAPE_IDS)
@pytest.mark.parametrize("angles", [(1, 1), (5, 7)], ids=["1d", "5x7"])
@pytest.mark.parametrize("center", [(0.0, 0.0, 0.0), M.OFFSET], ids=["centred", "offset"])
def test_angle_independent_mesh_is_the_target_tabulation_bitwise(api, inputs, shape, angles, center):
    _, r, ne, te = inputs
    p = M.params(api, shape)
    got = api.mesh_tables(p, M.profile_mesh(api, inputs, angles, center))
    want = api.target_tables(p, r, ne, te, api.Target(center))
    for g, w in zip(got, want):
        assert _same_bits(g, w)
    if center == M.OFFSET:                                                       # ... and the offset is not a no-op
        plain = api.target_tables(p, r, ne, te, api.Target())
        assert not np.array_equal(got[0], plain[0])


# ---- 2. a genuinely 3-D mesh against the numpy restatement --------------------------------------------------------------
@pytest.fixture(scope="module", params=M.SHAPES, ids=M.SHAPE_IDS)
def case3d(request, api):
    p = M.params(api, request.param)
    mesh, a = M.mesh3d(api)
    return p, mesh, a, M.Restatement(api, p, a["r"], a["theta"], a["phi"], a["center"])


def test_3d_mesh_matches_the_numpy_restatement(api, case3d):
    p, mesh, a, R = case3d
    ne3d, kap = api.mesh_tables(p, mesh)
    ed, kappa, ne_bound, kap_bound = R.tables(a["ne"], a["te"])
    for name, got, want, bound in (("ne3d", ne3d, ed, ne_bound), ("kappa3d", kap, kappa, kap_bound)):
        worst = float((np.abs(got - want) / bound).max()) * M.TOL
        print("%s: max |diff| = %.3e of the node's bound's base (bound %.0e)" % (name, worst, M.TOL))
        assert np.all(np.abs(got - want) <= bound), name
    # every branch is populated: the wrap bracket, each clamp, an interior node
    for name in ("wrap", "below", "above", "cap_lo", "cap_hi", "interior"):
        count = int(getattr(R, name).sum())
        print("%s: %d nodes" % (name, count))
        assert count > 0, name
    # and the mesh is genuinely 3-D: its tables are not those of its angle average
    flat = api.Mesh(a["r"], None, None, a["ne"].mean(axis=(1, 2)), a["te"].mean(axis=(1, 2)), None, a["center"])
    assert np.abs(api.mesh_tables(p, flat)[0] - ne3d).max() > 1e-2 * np.abs(ne3d).max()


# ---- 3. degenerate nodes --------------------------------------------------------------------------------------------------
def test_centre_node_and_polar_axis(api):
    shape, (i0, j0, k0) = (20, 17, 25), (7, 11, 12)
    p = M.params(api, shape)
    d = api.derive(p)
    centre = (i0 * d.dx + p.xmin, j0 * d.dy + p.ymin, k0 * d.dz + p.zmin)        # the node's own expression: s == 0 exactly
    mesh, a = M.mesh3d(api, center=centre)
    ne3d, kap = api.mesh_tables(p, mesh)
    flow = api.mesh_flow_table(p, mesh)
    phi, ne = a["phi"], a["ne"]
    # the centre: rho == 0 clamps to shell 0, theta = atan2(0, 0) = 0 to row 0, phi = 0 lies in the bracket k, k + 1
    k = int(np.searchsorted(phi, 0.0, side="right")) - 1
    wp = (0.0 - phi[k]) / (phi[k + 1] - phi[k])
    assert ne3d[i0, j0, k0] == ne[0, 0, k] + (ne[0, 0, k + 1] - ne[0, 0, k]) * wp
    assert not flow[:, i0, j0, k0].any()
    # the axis through the centre: rxy == 0, theta = 0 above (row 0) and pi below (the last row), phi = 0 as at the centre
    R = M.Restatement(api, p, a["r"], a["theta"], a["phi"], centre)
    assert not R.rxy[i0, j0].any() and R.rho[i0, j0, k0] == 0.0
    assert R.cap_lo[i0, j0, k0:].all() and R.cap_hi[i0, j0, :k0].all() and (R.k[i0, j0] == k).all()
    ed, kappa, ne_bound, kap_bound = R.tables(a["ne"], a["te"])
    axis = (i0, j0, slice(None))
    assert np.isfinite(ne3d[axis]).all() and np.isfinite(kap[axis]).all() and np.isfinite(flow[(slice(None),) + axis]).all()
    assert np.all(np.abs(ne3d - ed) <= ne_bound) and np.all(np.abs(kap - kappa) <= kap_bound)
    # on the axis (c1, s1) = (1, 0), st = 0, ct = +-1: ux = uth ct, uy = uph, uz = ur ct
    ur, uth, uph = (R.value(f)[0][axis] for f in a["u"])
    ct = np.sign(R.Z[axis])
    scale = np.abs(flow).max()
    for got, want in zip(flow[(slice(None),) + axis], (uth * ct, uph * np.abs(ct), ur * ct)):
        assert np.all(np.abs(got - want) <= M.TOL * scale)


# ---- 4. flow ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", M.SHAPES, ids=M.SHAPE_IDS)
def test_sampled_ramp_is_the_targets_flow_table(api, shape):
    p, gp = M.params(api, shape), api.default_gain_params()
    r = np.array([0.0, 0.01, gp.mach_r0, 0.07, 0.1, gp.mach_r1, 0.2])           # the ramp is linear between its two radii
    ur = M.ramp(api, p, gp, r)
    got = api.mesh_flow_table(p, api.Mesh(r, None, None, np.ones(r.size), np.ones(r.size), (ur, None, None), M.OFFSET))
    want = api.flow_table(p, gp, api.Target(M.OFFSET))
    err = np.abs(got - want).max() / np.abs(want).max()
    print("ramp: max |diff| / max |u| = %.3e" % err)
    assert err <= M.TOL
    assert np.abs(want - api.flow_table(p, gp)).max() > 1e-3 * np.abs(want).max()     # the offset is not lost in the bound
    zeros = np.zeros(r.size)
    same = api.mesh_flow_table(p, api.Mesh(r, None, None, np.ones(r.size), np.ones(r.size), (ur, zeros, zeros), M.OFFSET))
    assert _same_bits(same, got)                                                # a NULL component is a zero one


def test_full_velocity_field_matches_the_numpy_restatement(api, case3d):
    p, mesh, a, R = case3d
    got = api.mesh_flow_table(p, mesh)
    want = R.flow(*a["u"])
    scale = np.abs(want).max()
    err = np.abs(got - want).max() / scale
    print("flow: max |diff| / max |u| = %.3e" % err)
    assert err <= M.TOL
    radial = R.flow(a["u"][0], None, None)
    assert np.abs(want - radial).max() > 1e-2 * scale                           # utheta and uphi are not lost in the bound


# ---- 5. validation --------------------------------------------------------------------------------------------------------
def _good():
    r, theta, phi = np.array([0.0, 0.1, 0.2]), np.array([0.5, 1.5, 2.5]), np.array([-3.0, -1.0, 1.0, 3.0])
    f = np.ones((3, 3, 4))
    return dict(r=r, theta=theta, phi=phi, ne=f.copy(), te=f.copy(), velocity=[f.copy(), f.copy(), f.copy()],
                center=[0.0, 0.0, 0.0])


def _changed(**changes):
    kw = _good()
    for name, (index, value) in changes.items():
        target = kw["velocity"][0] if name == "ur" else kw[name]
        target[index] = value
    return kw


BAD = {
    "r not ascending": (_changed(r=(1, 0.2)), "ascending"),
    "r descending": (_changed(r=(2, 0.05)), "ascending"),
    "r negative": (_changed(r=(0, -0.01)), "negative"),
    "r nan": (_changed(r=(1, float("nan"))), "finite"),
    "theta below 0": (_changed(theta=(0, -0.1)), "theta"),
    "theta above pi": (_changed(theta=(2, 3.2)), "theta"),
    "theta not ascending": (_changed(theta=(1, 0.5)), "ascending"),
    "phi[0] below -pi": (_changed(phi=(0, -3.2)), "phi[0]"),
    "phi not ascending": (_changed(phi=(2, -1.0)), "ascending"),
    "phi a whole period": (_changed(phi=(3, -3.0 + 2 * math.pi)), "period"),
    "phi inf": (_changed(phi=(3, float("inf"))), "finite"),
    "ne negative": (_changed(ne=((1, 2, 3), -1.0)), "ne[23]"),
    "ne nan": (_changed(ne=((0, 0, 1), float("nan"))), "ne[1]"),
    "te zero": (_changed(te=((2, 2, 3), 0.0)), "te[35]"),
    "te inf": (_changed(te=((0, 0, 0), float("inf"))), "te[0]"),
    "ur nan": (_changed(ur=((0, 1, 0), float("nan"))), "ur[4]"),
    "center nan": (_changed(center=(1, float("nan"))), "center"),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_bad_meshes_are_refused(api, name):
    kw, word = BAD[name]
    p = M.params(api, (9, 9, 9))
    api.mesh_tables(p, api.Mesh(**_good()))                                     # the unchanged mesh is accepted
    for call in (lambda m: api.mesh_tables(p, m), lambda m: api.mesh_flow_table(p, m), api.mesh_check):
        with pytest.raises(api.CbetError) as ei:
            call(api.Mesh(**kw))
        assert ei.value.code == api.EINVAL and word in str(ei.value), str(ei.value)


def test_bad_sizes_and_pointers_are_refused(api):
    p = M.params(api, (9, 9, 9))

    def refused(mesh):
        with pytest.raises(api.CbetError) as ei:
            api.mesh_tables(p, mesh)
        assert ei.value.code == api.EINVAL
        return str(ei.value)

    one = np.ones(1)
    assert "nr" in refused(api.Mesh([0.1], None, None, one, one))               # nr >= 2
    far = np.array([3.0])                                                       # phi[0] < pi holds for one node too
    assert "phi[0]" in refused(api.Mesh([0.0, 0.1], None, np.array([3.2]), np.ones((2, 1, 1)), np.ones((2, 1, 1))))
    api.mesh_tables(p, api.Mesh([0.0, 0.1], None, far, np.ones((2, 1, 1)), np.ones((2, 1, 1))))
    n = api.MESH_MAX_COORDS
    long_r = np.linspace(0.0, 0.3, n - 1)
    assert "MAX_COORDS" in refused(api.Mesh(long_r, None, None, np.ones(n - 1), np.ones(n - 1)))      # n - 1 + 1 + 1 > n
    api.mesh_tables(p, api.Mesh(long_r[:-1], None, None, np.ones(n - 2), np.ones(n - 2)))             # ... and n fits
    for name in ("r", "theta", "phi", "ne", "te"):
        m = api.Mesh(**_good())
        setattr(m, name, None)
        assert "NULL" in refused(m)
    m = api.Mesh(**_good())
    m.ur = None                                                                 # a NULL velocity component is legal
    api.mesh_flow_table(p, m)
    out = np.zeros(3 * 9 ** 3)
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    good = api.Mesh(**_good())
    L = api.lib()
    assert L.cbet_mesh_tables(C.byref(p), C.byref(good), None, dp) == api.EINVAL
    assert L.cbet_mesh_tables(C.byref(p), C.byref(good), dp, None) == api.EINVAL
    assert L.cbet_mesh_tables(C.byref(p), None, dp, dp) == api.EINVAL
    assert L.cbet_mesh_flow_table(C.byref(p), C.byref(good), None) == api.EINVAL
    assert L.cbet_mesh_check(None) == api.EINVAL


def test_python_mesh_helper(api):
    kw = _good()
    m = api.Mesh(**kw)
    assert m.shape == (3, 3, 4) and m.has_velocity and list(m.center) == [0.0, 0.0, 0.0]
    kw["ne"][:] = -5.0                                                          # the mesh holds its own copies
    api.mesh_check(m)
    assert not api.Mesh(kw["r"], kw["theta"], kw["phi"], np.ones((3, 3, 4)), np.ones((3, 3, 4))).has_velocity
    with pytest.raises(ValueError):
        api.Mesh(kw["r"], kw["theta"], kw["phi"], np.ones((3, 3, 5)), np.ones((3, 3, 4)))
    with pytest.raises(ValueError):
        api.Mesh(kw["r"], None, None, np.ones(3), np.ones(3), velocity=[np.ones(3)])
