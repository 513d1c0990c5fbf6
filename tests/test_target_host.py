"""Perturbed targets on the host (include/cbet_mi355x.h cbet_target_tables): the host twin of
k_tabulate_target against the oracle's node tables (zero perturbation, bitwise), against a numpy restatement with
harmonics from closed forms and from scipy, at the special nodes, for a monopole, and its refusals.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

UM = 1e-4                       # cm
OFFSET = (20 * UM, -35 * UM, 10 * UM)
K_EC, K_ME = 1.60217662e-19, 9.10938356e-31      # def.cuh:63-64, as the library has them


@pytest.fixture(scope="module")
def api():
    from cbet_raytracing_3d_amd import api as a
    a.lib()
    return a


def _params(api, shape):
    p = api.default_params(shape[0], nbeams=4)
    p.ny, p.nz = shape[1], shape[2]
    return p


# ---- numpy restatement ---------------------------------------------------------------------------------------------
def _nodes(api, p, offset):
    d = api.derive(p)
    ax = [(np.arange(n) * step + lo) - o
          for n, step, lo, o in ((p.nx, d.dx, p.xmin, offset[0]), (p.ny, d.dy, p.ymin, offset[1]), (p.nz, d.dz, p.zmin, offset[2]))]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    return X, Y, Z, np.sqrt(X * X + Y * Y + Z * Z)


def _ylm_closed(X, Y, Z, r):
    """Real harmonics without the Condon-Shortley phase for l <= 2, index l*l + l + m; Y_00 alone at r = 0."""
    pi = math.pi
    with np.errstate(divide="ignore", invalid="ignore"):
        x, y, z = (np.where(r > 0, v / r, 0.0) for v in (X, Y, Z))
    on = (r > 0) * 1.0
    k1, k2 = math.sqrt(3.0 / (4 * pi)), math.sqrt(15.0 / (4 * pi))
    return np.stack([np.full(r.shape, 0.5 / math.sqrt(pi)), k1 * y, k1 * z, k1 * x,
                     k2 * x * y, k2 * y * z, math.sqrt(5.0 / (16 * pi)) * (3 * z * z - 1.0) * on, k2 * x * z,
                     math.sqrt(15.0 / (16 * pi)) * (x * x - y * y)])


def _ylm_scipy(lmax, X, Y, Z, r):
    special = pytest.importorskip("scipy.special")
    with np.errstate(divide="ignore", invalid="ignore"):
        ct = np.where(r > 0, Z / r, 1.0)
    theta, phi = np.arccos(np.clip(ct, -1.0, 1.0)), np.arctan2(Y, X)      # on the z axis phi = atan2(0, 0) = 0: (1, 0)
    out = np.zeros(((lmax + 1) ** 2,) + r.shape)
    for l in range(lmax + 1):
        for m in range(l + 1):
            if hasattr(special, "sph_harm_y"):
                cy = special.sph_harm_y(l, m, theta, phi)
            else:                                              # older scipy: sph_harm(m, n, azimuth, polar)
                cy = special.sph_harm(m, l, phi, theta)
            cy = cy * (-1.0) ** m                              # remove the Condon-Shortley phase
            if m == 0:
                out[l * l + l] = cy.real
            else:
                out[l * l + l + m] = math.sqrt(2.0) * cy.real
                out[l * l + l - m] = math.sqrt(2.0) * cy.imag
    out[1:, r == 0] = 0.0                                      # a node at the centre: Y_00 only
    out[0, r == 0] = 0.5 / math.sqrt(math.pi)
    return out


def _tables_at(api, p, r, ne, te, rhop):
    """(ne3d, kappa3d) of the profile at radii rhop: launch_ray_XZ.cu:296-305 in numpy."""
    assert np.all(np.diff(r) > 0)                              # np.interp needs (and s83177 has) ascending radii
    d = api.derive(p)
    ed, etemp = np.interp(rhop, r, ne), np.interp(rhop, r, te)
    eta = 5.2e-5 * 10.0 / (etemp * np.sqrt(etemp))
    nuei = (1e6 * ed * (K_EC * K_EC) / K_ME) * eta
    return ed, ed / d.ncrit * nuei * d.dt


def _numpy_tables(api, p, r, ne, te, offset, coeffs, ylm):
    X, Y, Z, rho = _nodes(api, p, offset)
    delta = np.tensordot(np.asarray(coeffs), ylm(X, Y, Z, rho), axes=1)
    return _tables_at(api, p, r, ne, te, rho / (1.0 + delta))


def _random_coeffs(lmax, seed, total=0.05):
    c = np.random.default_rng(seed).standard_normal((lmax + 1) ** 2)
    return c * (total / np.abs(c).sum())


def _close(got, want, tol=1e-12):
    for g, w, name in zip(got, want, ("ne3d", "kappa3d")):
        err = float(np.abs(g - w).max() / np.abs(w).max())
        print("%s: max |diff| / max = %.3e" % (name, err))
        assert err < tol, (name, err)


# ---- 1. zero perturbation -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(24, 24, 24), (20, 17, 25)], ids=["24", "20x17x25"])
def test_zero_target_gives_the_oracle_tables_bitwise(api, oracle, inputs, shape):
    _, r, ne, te = inputs
    p = _params(api, shape)
    cfg = oracle.default_config(shape[0], ny=shape[1], nz=shape[2])
    want = oracle.node_tables(cfg, r, ne, te)
    for target in (api.Target(), api.Target((0.0, 0.0, 0.0), np.zeros(25), lmax=4)):
        got = api.target_tables(p, r, ne, te, target)
        for g, w in zip(got, want):
            assert g.shape == w.shape and np.array_equal(g.view(np.int64), w.view(np.int64))


# ---- 1b. the shared bracket, both abscissa orders -------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(9, 7, 13), (12, 12, 12)], ids=["9x7x13", "12"])
def test_plain_tables_equal_the_oracle_bitwise_in_both_abscissa_orders(api, oracle, inputs, shape):
    """The twin's lookup (csrc/cbet_node_model.h bracket, interp2) against the oracle's interp_cuda: the shipped profile
    (ascending radii) and the same profile reversed, which takes the descending branch of the clamp tests and of the
    bisection's go-low rule and interpolates every segment from its other end."""
    _, r, ne, te = inputs
    p = _params(api, shape)
    cfg = oracle.default_config(shape[0], ny=shape[1], nz=shape[2])
    tables = {}
    for order in ("ascending", "descending"):
        prof = [np.ascontiguousarray(v if order == "ascending" else v[::-1]) for v in (r, ne, te)]
        assert (prof[0][0] < prof[0][-1]) == (order == "ascending")
        got = api.target_tables(p, *prof, api.Target())
        want = oracle.node_tables(cfg, *prof)
        for what, g, w in zip(("ne3d", "kappa3d"), got, want):
            diff = g.view(np.int64) != w.view(np.int64)
            print("%s %s %s: %d of %d words differ" % (shape, order, what, int(diff.sum()), diff.size))
            assert g.shape == w.shape and not diff.any(), (order, what, np.argwhere(diff)[:5].tolist())
        tables[order] = got
    # the reversed profile is another computation, not the same one relabelled: its tables differ in the last bits
    assert any((a.view(np.int64) != d.view(np.int64)).any() for a, d in zip(tables["ascending"], tables["descending"]))


# ---- 2. independent restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [9, 17])
@pytest.mark.parametrize("lmax", [0, 1, 2])
def test_host_matches_numpy_closed_forms(api, inputs, n, lmax):
    _, r, ne, te = inputs
    p = _params(api, (n, n, n))
    c = _random_coeffs(lmax, 10 * n + lmax)
    got = api.target_tables(p, r, ne, te, api.Target(OFFSET, c))
    want = _numpy_tables(api, p, r, ne, te, OFFSET, c, lambda X, Y, Z, rho: _ylm_closed(X, Y, Z, rho)[: c.size])
    _close(got, want)
    plain = api.target_tables(p, r, ne, te, api.Target())
    assert np.abs(got[0] - plain[0]).max() > 1e-3 * plain[0].max()          # and the perturbation is not lost in the bound


@pytest.mark.parametrize("n", [9, 17])
@pytest.mark.parametrize("lmax", [2, 5, 8, 16])
def test_host_matches_numpy_scipy(api, inputs, n, lmax):
    _, r, ne, te = inputs
    p = _params(api, (n, n, n))
    c = _random_coeffs(lmax, 100 * n + lmax)
    got = api.target_tables(p, r, ne, te, api.Target(OFFSET, c))
    want = _numpy_tables(api, p, r, ne, te, OFFSET, c, lambda X, Y, Z, rho: _ylm_scipy(lmax, X, Y, Z, rho))
    _close(got, want)


# ---- 3. special nodes -----------------------------------------------------------------------------------------------
def test_node_at_the_centre_and_nodes_on_the_axis(api, inputs):
    _, r, ne, te = inputs
    n, (i0, j0, k0) = 17, (5, 9, 3)
    p = _params(api, (n, n, n))
    d = api.derive(p)
    offset = (i0 * d.dx + p.xmin, j0 * d.dy + p.ymin, k0 * d.dz + p.zmin)    # the node's own expression: s == 0 exactly
    c = _random_coeffs(2, 7)
    got = api.target_tables(p, r, ne, te, api.Target(offset, c))
    ed0, kap0 = _tables_at(api, p, r, ne, te, np.zeros(1))                    # the profile at rho' = 0
    assert got[0][i0, j0, k0] == ed0[0] == ne[0]
    assert abs(got[1][i0, j0, k0] / kap0[0] - 1.0) < 1e-14
    want = _numpy_tables(api, p, r, ne, te, offset, c, _ylm_closed)
    axis = (i0, j0, slice(None))                                              # the z axis through the target's centre
    assert np.isfinite(got[0][axis]).all() and np.isfinite(got[1][axis]).all()
    _close([g[axis] for g in got], [w[axis] for w in want])
    _close(got, want)


# ---- 4. monopole ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lmax", [0, 3])
def test_monopole_is_a_uniform_expansion(api, inputs, lmax):
    _, r, ne, te = inputs
    p, a = _params(api, (17, 17, 17)), 0.03
    c = np.zeros((lmax + 1) ** 2)
    c[0] = a * math.sqrt(4.0 * math.pi)
    got = api.target_tables(p, r, ne, te, api.Target(OFFSET, c))
    rho = _nodes(api, p, OFFSET)[3]
    _close(got, _tables_at(api, p, r, ne, te, rho / (1.0 + a)))


# ---- 5. refusals ----------------------------------------------------------------------------------------------------
def test_bad_targets_are_refused(api, inputs):
    _, r, ne, te = inputs
    p = _params(api, (9, 9, 9))

    def refused(target):
        with pytest.raises(api.CbetError) as ei:
            api.target_tables(p, r, ne, te, target)
        assert ei.value.code == api.EINVAL
        return str(ei.value)

    assert "lmax" in refused(api.Target(lmax=17))
    assert "lmax" in refused(api.Target(lmax=-1))
    assert "finite" in refused(api.Target((0.0, float("nan"), 0.0)))
    assert "finite" in refused(api.Target(coeffs=[0.0, float("inf"), 0.0, 0.0]))
    too_big = np.zeros(9)
    too_big[6] = 1.0 / math.sqrt(5.0 / (4.0 * math.pi)) * 1.0001              # |c_20| sqrt(5 / 4 pi) just above 1
    assert "below 1" in refused(api.Target(coeffs=too_big))
    too_big[6] *= 0.99                                                        # ... and just below: accepted
    api.target_tables(p, r, ne, te, api.Target(coeffs=too_big))
    out = np.zeros(9 ** 3)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))                    # noqa: E731
    t = api.Target()
    for ne3d, kap in ((None, dp(out)), (dp(out), None)):
        assert api.lib().cbet_target_tables(C.byref(p), dp(te), dp(r), dp(ne), C.byref(t), ne3d, kap) == api.EINVAL
    assert api.lib().cbet_target_tables(C.byref(p), dp(te), dp(r), dp(ne), None, dp(out), dp(out)) == api.EINVAL


def test_python_helpers(api):
    from cbet_raytracing_3d_amd import modes
    c = modes.target_coeffs(3, {(2, 0): 0.02, (3, 2): 0.01, (3, -1): -0.005})
    assert c.shape == (16,) and c[6] == 0.02 and c[14] == 0.01 and c[11] == -0.005 and np.count_nonzero(c) == 3
    with pytest.raises(ValueError):
        modes.target_coeffs(1, {(2, 0): 0.1})
    t = api.Target((1.0, 2.0, 3.0), c)
    assert t.lmax == 3 and list(t.offset) == [1.0, 2.0, 3.0] and np.array_equal(t.coeff_array(), c)
    c[6] = 9.0                                                                # the target holds its own copy
    assert t.coeffs[6] == 0.02
    with pytest.raises(ValueError):
        api.Target(coeffs=np.zeros(5))
    with pytest.raises(ValueError):
        api.Target(coeffs=np.zeros(9), lmax=3)
