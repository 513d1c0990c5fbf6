"""The flow table of the CBET gain kernels on the host (include/cbet_mi355x.h cbet_flow_table): the
host twin of k_tabulate_flow against a numpy restatement of the gain kernels' closed-form ramp (zero target, bitwise),
against a numpy restatement with harmonics from closed forms and from scipy, its properties, a monopole, and its
refusals.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

from test_target_host import OFFSET, _nodes, _params, _random_coeffs, _ylm_closed, _ylm_scipy

TOL = 1e-12                     # of max |u|: a few hundred fp64 roundings of O(1) quantities stay below it


@pytest.fixture(scope="module")
def api():
    from cbet_raytracing_3d_amd import api as a
    a.lib()
    return a


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ---- numpy restatements ---------------------------------------------------------------------------------------------
def _ramp(api, p, gp, rad, X, Y, Z, rho):
    """The gain kernels' ramp at radius `rad`, direction (X, Y, Z) / rho: cell_state's statements, one numpy operation
    per IEEE operation, in its order."""
    cs = api.gain_constants(p, gp)[1]
    t = (rad - gp.mach_r0) / (gp.mach_r1 - gp.mach_r0)
    t = np.where(t < 0.0, 0.0, t)
    t = np.where(t > 1.0, 1.0, t)
    um = (gp.mach_0 + (gp.mach_1 - gp.mach_0) * t) * cs
    with np.errstate(divide="ignore", invalid="ignore"):
        u = [np.where(rho > 0.0, um * (S / rho), 0.0) for S in (X, Y, Z)]
    return np.stack(u)


def _cell_state_flow(api, p, gp):
    """cell_state of the gain kernels (and the oracle's gain_field) at every node, about the origin."""
    d = api.derive(p)
    xc, yc, zc = np.meshgrid(np.arange(p.nx) * d.dx + p.xmin, np.arange(p.ny) * d.dy + p.ymin,
                             np.arange(p.nz) * d.dz + p.zmin, indexing="ij")
    rr = np.sqrt(xc * xc + yc * yc + zc * zc)
    return _ramp(api, p, gp, rr, xc, yc, zc, rr)


def _numpy_flow(api, p, gp, offset, coeffs, ylm):
    X, Y, Z, rho = _nodes(api, p, offset)
    delta = np.tensordot(np.asarray(coeffs), ylm(X, Y, Z, rho), axes=1)
    return _ramp(api, p, gp, rho / (1.0 + delta), X, Y, Z, rho)


def _close(got, want, tol=TOL):
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print("flow: max |diff| / max |u| = %.3e" % err)
    assert err < tol, err


# ---- 1. zero target -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(24, 24, 24), (20, 17, 25)], ids=["24", "20x17x25"])
def test_zero_target_is_the_closed_form_ramp_bitwise(api, shape):
    p, gp = _params(api, shape), api.default_gain_params()
    want = _cell_state_flow(api, p, gp)
    assert np.abs(want).max() > 1e7                       # cm/s: a real flow
    for target in (None, api.Target(), api.Target((0.0, 0.0, 0.0), np.zeros(25), lmax=4)):
        got = api.flow_table(p, gp, target)
        assert got.shape == (3,) + shape and np.array_equal(_bits(got), _bits(want))
    # an odd grid has a node at the origin: no direction, no flow
    q = _params(api, (9, 9, 9))
    got = api.flow_table(q, gp)
    assert np.array_equal(_bits(got), _bits(_cell_state_flow(api, q, gp))) and not got[:, 4, 4, 4].any()


# ---- 2. offset and distortion against an independent restatement ----------------------------------------------------
@pytest.mark.parametrize("n", [9, 17])
@pytest.mark.parametrize("lmax", [0, 1, 2])
def test_host_matches_numpy_closed_forms(api, n, lmax):
    p, gp = _params(api, (n, n, n)), api.default_gain_params()
    c = _random_coeffs(lmax, 10 * n + lmax)
    got = api.flow_table(p, gp, api.Target(OFFSET, c))
    _close(got, _numpy_flow(api, p, gp, OFFSET, c, lambda X, Y, Z, rho: _ylm_closed(X, Y, Z, rho)[: c.size]))
    plain = api.flow_table(p, gp)
    assert np.abs(got - plain).max() > 1e-3 * np.abs(plain).max()          # and the perturbation is not lost in the bound


@pytest.mark.parametrize("n", [9, 17])
@pytest.mark.parametrize("lmax", [2, 5, 16])
def test_host_matches_numpy_scipy(api, n, lmax):
    p, gp = _params(api, (n, n, n)), api.default_gain_params()
    c = _random_coeffs(lmax, 100 * n + lmax)
    got = api.flow_table(p, gp, api.Target(OFFSET, c))
    _close(got, _numpy_flow(api, p, gp, OFFSET, c, lambda X, Y, Z, rho: _ylm_scipy(lmax, X, Y, Z, rho)))


# ---- 3. properties --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lmax", [0, 2, 5, 16])
def test_flow_is_radial_from_the_centre_bounded_and_zero_at_it(api, lmax):
    n, (i0, j0, k0) = 17, (5, 9, 3)
    p = _params(api, (n, n, n))
    gp = api.default_gain_params(mach_0=-0.7)                                 # an inflow inside: the bound takes |mach|
    d = api.derive(p)
    offset = (i0 * d.dx + p.xmin, j0 * d.dy + p.ymin, k0 * d.dz + p.zmin)     # the node's own expression: s == 0 exactly
    u = api.flow_table(p, gp, api.Target(offset, _random_coeffs(lmax, 7 + lmax)))
    assert np.isfinite(u).all()
    assert not u[:, i0, j0, k0].any()                                         # no direction at the centre: no flow
    X, Y, Z, rho = _nodes(api, p, offset)
    cs = api.gain_constants(p, gp)[1]
    top = max(abs(gp.mach_0), abs(gp.mach_1)) * cs
    speed = np.sqrt((u * u).sum(0))
    assert speed.max() <= top * (1.0 + 8 * np.finfo(float).eps) and speed.max() > 0.5 * top
    cross = np.stack([u[1] * Z - u[2] * Y, u[2] * X - u[0] * Z, u[0] * Y - u[1] * X])
    assert np.abs(cross).max() <= 8 * np.finfo(float).eps * top * rho.max()   # u x s = 0 to rounding
    outward = u[0] * X + u[1] * Y + u[2] * Z
    assert (outward < 0).any() and (outward > 0).any()                        # ... along -s inside, +s outside


# ---- 4. monopole ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lmax", [0, 3])
def test_monopole_scales_the_ramp_radii(api, lmax):
    p, a = _params(api, (17, 17, 17)), 0.03
    gp = api.default_gain_params()
    c = np.zeros((lmax + 1) ** 2)
    c[0] = a * math.sqrt(4.0 * math.pi)                                       # 1 + c00 Y00 = 1 + a
    got = api.flow_table(p, gp, api.Target(OFFSET, c))
    scaled = api.default_gain_params(mach_r0=gp.mach_r0 * (1.0 + a), mach_r1=gp.mach_r1 * (1.0 + a))
    want = api.flow_table(p, scaled, api.Target(OFFSET))
    _close(got, want)
    assert np.abs(got - api.flow_table(p, gp, api.Target(OFFSET))).max() > 1e-3 * np.abs(want).max()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused(api):
    p, gp = _params(api, (9, 9, 9)), api.default_gain_params()
    out = np.full(3 * 9 ** 3, -1.0)
    dp = out.ctypes.data_as(C.POINTER(C.c_double))

    def refused(target, gain=gp):
        with pytest.raises(api.CbetError) as ei:
            api.flow_table(p, gain, target)
        assert ei.value.code == api.EINVAL
        rc = api.lib().cbet_flow_table(C.byref(p), C.byref(gain), C.byref(target), dp)
        assert rc == api.EINVAL and np.all(out == -1.0)                       # ... before any work
        return str(ei.value)

    assert "lmax" in refused(api.Target(lmax=17))
    assert "lmax" in refused(api.Target(lmax=-1))
    assert "finite" in refused(api.Target((0.0, float("nan"), 0.0)))
    assert "finite" in refused(api.Target(coeffs=[0.0, float("inf"), 0.0, 0.0]))
    too_big = np.zeros(9)
    too_big[6] = 1.0 / math.sqrt(5.0 / (4.0 * math.pi)) * 1.0001              # |c_20| sqrt(5 / 4 pi) just above 1
    assert "below 1" in refused(api.Target(coeffs=too_big))
    too_big[6] *= 0.99                                                        # ... and just below: accepted
    api.flow_table(p, gp, api.Target(coeffs=too_big))
    assert "mach_r1" in refused(api.Target(), api.default_gain_params(mach_r1=0.01))
    assert "plasma constants" in refused(api.Target(), api.default_gain_params(te_ev=0.0))
    t = api.Target()
    assert api.lib().cbet_flow_table(C.byref(p), C.byref(gp), C.byref(t), None) == api.EINVAL
    assert api.lib().cbet_flow_table(C.byref(p), None, C.byref(t), dp) == api.EINVAL
    assert api.lib().cbet_flow_table(None, C.byref(gp), C.byref(t), dp) == api.EINVAL
    assert np.all(out == -1.0)


def test_exports(api):
    assert callable(api.tabulate_flow) and callable(api.flow_table)
    assert callable(api.Context.set_flow) and callable(api.Context.flow)
