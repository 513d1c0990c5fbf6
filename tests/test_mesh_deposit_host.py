"""Deposit on the hydro mesh (include/cbet_mi355x.h "deposit on the hydro mesh"), the parts that
need no device: the host twin against the independent numpy restatement of helpers/mesh_deposit_cases.py, conservation,
the link to cbet_sph_modes, padded rows, the degenerate samples, every refusal, MeshCells.from_nodes and the exports."""
import numpy as np
import pytest

from helpers import mesh_deposit_cases as D


@pytest.fixture(scope="module")
def api():
    from cbet_raytracing_3d_amd import api as a
    a.lib()   # raises if the HIP library was not built -- no fallback
    return a


def _einval(api, call):
    with pytest.raises(api.CbetError) as e:
        call()
    assert e.value.code == api.EINVAL
    return str(e.value)


@pytest.fixture(scope="module", params=list(D.CASES), ids=list(D.CASES))
def case(request, api):
    """One grid case: params, a stack of 3 seeded grids and, per kind of cells, the restatement and its sums."""
    shape, box, S = D.CASES[request.param]
    p = D.params(api, shape, box)
    g = D.grids(shape, 3, seed=11)
    out = {"p": p, "S": S, "grids": g, "shape": shape}
    for kind in D.KINDS:
        rs = D.Restatement(api, p, *D.edges(kind), D.CENTER, S)
        out[kind] = (rs, rs.deposit(g))
    return out


# ---- 1. twin against restatement, conservation -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", D.KINDS)
def test_twin_matches_restatement(api, case, kind):
    rs, (want_e, want_o) = case[kind]
    with D.cells(api, kind) as c:
        got = api.mesh_deposit_host(c, case["grids"], case["p"], case["S"])
        one = api.mesh_deposit_host(c, case["grids"][1], case["p"], case["S"])
        none = api.mesh_deposit_host(c, None, case["p"], case["S"])
    assert got[0].shape == (3,) + rs.shape and got[2].dtype == np.int64
    assert rs.counts.sum() + rs.n_outside == D.total_samples(case["p"], case["S"])
    D.check(got, (want_e, want_o, rs.counts), rs.counts, rs.n_outside, what="stack of 3")
    # a single grid is the stack's entry, bit for bit (the twin's order is fixed); counts alone: the same counts
    assert np.array_equal(one[0][0], got[0][1]) and np.array_equal(one[1][0], got[1][1]) and np.array_equal(one[2], got[2])
    assert np.array_equal(none[2], rs.counts) and not none[0].any() and not none[1].any()


@pytest.mark.parametrize("kind", D.KINDS)
def test_conservation(api, case, kind):
    rs, _ = case[kind]
    with D.cells(api, kind) as c:
        e, o, n = api.mesh_deposit_host(c, case["grids"], case["p"], case["S"])
    total = D.total_samples(case["p"], case["S"])
    for g in range(3):
        want = case["grids"][g].sum()                      # non-negative: sum |terms| is the sum itself
        # three sums of the same total in different orders: the twin's cells, their sum here, numpy's pairwise grid sum
        assert abs(e[g].sum() + o[g] - want) <= 2.0 * total * D.EPS * want


# ---- 2. S = 1, one row, one column, the shells of sph_modes -----------------------------------------------------------
def test_one_sample_per_node_is_sph_modes_shells(api, case):
    p, g = case["p"], case["grids"]
    with api.MeshCells(D.R_EDGES, center=D.CENTER) as c:
        e, o, n = api.mesh_deposit_host(c, g, p, 1)
    _, shell_energy, shell_nodes = api.sph_modes_host(g, p, D.CENTER, D.R_EDGES, 0)
    assert np.array_equal(n[:, 0, 0], shell_nodes)
    bound = 2.0 * shell_nodes * D.EPS * np.abs(shell_energy)
    assert np.all(np.abs(e[:, :, 0, 0] - shell_energy) <= bound)


# ---- 3. padded rows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", D.KINDS)
def test_padded_rows_give_the_dense_bits(api, case, kind):
    shape, p, S = case["shape"], case["p"], case["S"]
    padded = D.grids(shape, 3, seed=11, pitch=shape[2] + 2 + 5)
    assert np.isnan(padded[..., shape[2] + 2:]).all() and np.array_equal(padded[..., : shape[2] + 2], case["grids"])
    with D.cells(api, kind) as c:
        dense = api.mesh_deposit_host(c, case["grids"], p, S)
        got = api.mesh_deposit_host(c, padded, p, S)
    for a, b in zip(got, dense):
        assert np.array_equal(a, b)                        # NaN nowhere: array_equal would fail on one


# ---- 4. degenerate samples -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def on_node(api):
    """The 6x9x13 grid with the cells' centre on haloed node (3, 4, 6)."""
    shape, box, _ = D.CASES["6x9x13-S3"]
    p = D.params(api, shape, box)
    d = api.derive(p)
    node = (3, 4, 6)
    center = tuple((i - 1) * step + lo for i, step, lo in zip(node, (d.dx, d.dy, d.dz), (p.xmin, p.ymin, p.zmin)))
    return p, shape, node, center


def _single(shape, node, value=1.0):
    g = np.zeros((shape[0] + 2, shape[1] + 2, shape[2] + 2))
    g[node] = value
    return g


def test_degenerate_nodes(api, on_node):
    """S = 1: the node at the centre is counted in (shell 0, row 0, column 0); the nodes above and below it on the polar
    axis in the first and the last row, in the column that holds phi = 0 -- with edges 0.3 + 2 pi k / 9 the last one."""
    p, shape, (I, J, K), center = on_node
    nth, nph = len(D.THETA_EDGES) - 1, len(D.PHI_EDGES) - 1
    with D.cells(api, "3d", center=center) as c:
        for node, row, col in (((I, J, K), 0, 0), ((I, J, K + 2), 0, nph - 1), ((I, J, K - 2), nth - 1, nph - 1)):
            e, o, _ = api.mesh_deposit_host(c, _single(shape, node, 3.0), p, 1)
            hit = np.argwhere(e[0] != 0.0)
            assert hit.shape == (1, 3) and tuple(hit[0][1:]) == (row, col) and e[0][tuple(hit[0])] == 3.0 and o[0] == 0.0
        e, _, _ = api.mesh_deposit_host(c, _single(shape, (I, J, K)), p, 1)
        assert e[0, 0, 0, 0] == 1.0


@pytest.mark.parametrize("S", [1, 3])
def test_degenerate_samples_against_restatement(api, on_node, S):
    """The centre on a node: the S = 3 samples of that node hold the centre itself and two samples on the axis, the
    columns of nodes above and below hold more.  The restatement states the rho == 0 rule and takes the rest from arctan2."""
    p, shape, node, center = on_node
    g = D.grids(shape, 2, seed=5)
    g[:, node[0], node[1], :] += 1.0                       # the axis column and the centre node hold energy
    rs = D.Restatement(api, p, *D.edges("3d"), center, S)
    centre_samples = rs.cell[node][(S // 2,) * 3]
    assert centre_samples == 0                             # shell 0, row 0, column 0
    with D.cells(api, "3d", center=center) as c:
        got = api.mesh_deposit_host(c, g, p, S)
    want_e, want_o = rs.deposit(g)
    D.check(got, (want_e, want_o, rs.counts), rs.counts, rs.n_outside, what="centre on a node, S = %d" % S)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------
def _bad_cells():
    r, t, f = D.R_EDGES, D.THETA_EDGES, D.PHI_EDGES
    swap = lambda a, i: np.concatenate((a[:i], a[i:i + 2][::-1], a[i + 2:]))          # noqa: E731
    # strictly ascending edges whose diamond angles coincide: both wrap (d < pe[0], so + 4.0, whose spacing is 9e-16) and
    # lie 3e-17 apart as angles
    thin2 = f - 0.8
    thin2[2] = np.nextafter(thin2[1], 10.0)
    return {
        "r not ascending": dict(r_edges=swap(r, 4), theta_edges=t, phi_edges=f),
        "r repeated": dict(r_edges=np.concatenate((r[:5], r[4:])), theta_edges=t, phi_edges=f),
        "r negative": dict(r_edges=np.concatenate(([-1e-3], r[1:])), theta_edges=t, phi_edges=f),
        "r not finite": dict(r_edges=np.concatenate((r[:-1], [np.inf])), theta_edges=t, phi_edges=f),
        "theta not ascending": dict(r_edges=r, theta_edges=swap(t, 2), phi_edges=f),
        "theta does not start at 0": dict(r_edges=r, theta_edges=np.concatenate(([1e-6], t[1:])), phi_edges=f),
        "theta does not close at pi": dict(r_edges=r, theta_edges=np.concatenate((t[:-1], [3.1])), phi_edges=f),
        "phi not ascending": dict(r_edges=r, theta_edges=t, phi_edges=swap(f, 5)),
        "phi does not close at 2 pi": dict(r_edges=r, theta_edges=t, phi_edges=np.concatenate((f[:-1], [f[0] + 6.2]))),
        "phi starts below -pi": dict(r_edges=r, theta_edges=t, phi_edges=f - 0.3 - 3.2),
        "phi starts at pi": dict(r_edges=r, theta_edges=t, phi_edges=f - 0.3 + np.pi),
        "columns too thin for pe": dict(r_edges=r, theta_edges=t, phi_edges=thin2),
        "no shell": dict(r_edges=r[:1], theta_edges=t, phi_edges=f),
        "subsamples_max 0": dict(r_edges=r, theta_edges=t, phi_edges=f, subsamples_max=0),
        "subsamples_max 5": dict(r_edges=r, theta_edges=t, phi_edges=f, subsamples_max=5),
        "too many coordinates": dict(r_edges=np.linspace(0.0, 0.1, 2560 - 3 - 7 - 9 + 2), theta_edges=t, phi_edges=f),
    }


@pytest.mark.parametrize("name", list(_bad_cells()))
def test_bad_cells_are_refused(api, name):
    msg = _einval(api, lambda: api.MeshCells(center=D.CENTER, **_bad_cells()[name]))
    assert "mesh_cells" in msg


def test_most_coordinates_allowed(api):
    """nr + ntheta + nphi + 3 == CBET_MESH_MAX_COORDS is the largest accepted."""
    assert api.MESH_MAX_COORDS == 2560
    with api.MeshCells(np.linspace(0.0, 0.1, 2560 - 3 - 7 - 9 + 1), D.THETA_EDGES, D.PHI_EDGES) as c:
        assert sum(c.shape) + 3 == 2560


def test_bad_calls_are_refused(api, case):
    p, g = case["p"], case["grids"]
    with D.cells(api, "3d") as c, D.cells(api, "3d", subsamples_max=2) as c2:
        _einval(api, lambda: api.mesh_deposit_host(c, g, p, 0))
        _einval(api, lambda: api.mesh_deposit_host(c, g, p, 5))
        _einval(api, lambda: api.mesh_deposit_host(c2, g, p, 3))            # beyond the handle's subsamples_max
        api.mesh_deposit_host(c2, g, p, 2)
        _einval(api, lambda: api.mesh_deposit_host(c, np.zeros((65,) + g.shape[1:]), p, 1))
        _einval(api, lambda: api.mesh_deposit_host(c, np.zeros((0,) + g.shape[1:]), p, 1))
        api.mesh_deposit_host(c, np.zeros((64,) + g.shape[1:]), p, 1)
        L = api.lib()
        e, o, n = np.zeros((3,) + c.shape), np.zeros(3), np.zeros(c.shape, dtype=np.int64)
        args = lambda edep, ngrids, stride, ee, oo, nn: L.cbet_mesh_deposit(      # noqa: E731
            c.handle, edep, ngrids, stride, p, 1, 0, ee, oo, nn, None)
        ok = args(g.ctypes.data, 3, g[0].size, e.ctypes.data, o.ctypes.data, n.ctypes.data)
        assert ok == api.OK
        assert args(None, 3, g[0].size, e.ctypes.data, o.ctypes.data, n.ctypes.data) == api.EINVAL     # counts alone: one grid
        assert args(g.ctypes.data, 3, g[0].size - 1, e.ctypes.data, o.ctypes.data, n.ctypes.data) == api.EINVAL
        assert args(g.ctypes.data, 3, g[0].size, None, o.ctypes.data, n.ctypes.data) == api.EINVAL
        assert args(g.ctypes.data, 3, g[0].size, e.ctypes.data, o.ctypes.data, None) == api.EINVAL
        assert args(None, 1, 0, None, None, n.ctypes.data) == api.OK                                   # ... and no energy outputs
        # a host-only handle has no device tables
        assert L.cbet_mesh_deposit_device(c.handle, None, 1, 0, p, 1, 0, None, None, n.ctypes.data, None) == api.EINVAL
        assert "host-only" in L.cbet_last_error().decode()
    with pytest.raises(ValueError):
        api.mesh_deposit_host(c, g[:, :-1], p, 1)


# ---- 6. from_nodes, exports ------------------------------------------------------------------------------------------------
def test_from_nodes_edges_are_midpoints(api):
    r = 0.012 + 0.1 * np.linspace(0.0, 1.0, 9) ** 1.3
    theta = np.array([0.2, 0.9, 1.4, 2.2, 3.0])
    phi = np.array([-2.0, -1.0, 0.4, 1.1, 2.5])
    with api.MeshCells.from_nodes(r, theta, phi, center=D.CENTER) as c:
        assert c.shape == (9, 5, 5) and c.center == D.CENTER and c.column_shift == 0
        assert np.array_equal(c.r_edges[1:-1], 0.5 * (r[1:] + r[:-1]))
        assert c.r_edges[0] == r[0] - (r[1] - r[0]) / 2 and c.r_edges[-1] == r[-1] + (r[-1] - r[-2]) / 2
        assert np.array_equal(c.theta_edges[1:-1], 0.5 * (theta[1:] + theta[:-1]))
        assert c.theta_edges[0] == 0.0 and c.theta_edges[-1] == np.pi
        assert np.array_equal(c.phi_edges[1:-1], 0.5 * (phi[1:] + phi[:-1]))
        assert c.phi_edges[0] == 0.5 * ((phi[-1] - D.TWO_PI) + phi[0]) and c.phi_edges[-1] == c.phi_edges[0] + D.TWO_PI
    with api.MeshCells.from_nodes(np.array([0.001, 0.01, 0.02])) as c:           # the first edge does not go below 0
        assert c.shape == (3, 1, 1) and c.r_edges[0] == 0.0 and c.theta_edges is None and c.phi_edges is None
    # the first phi edge would lie below -pi: the same columns, named from the next edge on
    phi = np.array([-3.1, 0.0, 3.0])
    with api.MeshCells.from_nodes(r, None, phi) as c:
        assert c.shape == (9, 1, 3) and c.column_shift == 1
        assert np.array_equal(c.phi_edges[:2], 0.5 * (phi[1:] + phi[:-1])) and -np.pi <= c.phi_edges[0]
        assert abs(c.phi_edges[2] - (0.5 * (3.0 - D.TWO_PI - 3.1) + D.TWO_PI)) < 1e-15
    with pytest.raises(ValueError):
        api.MeshCells.from_nodes(np.array([0.01]))


def test_exports_and_argtypes(api):
    assert (api.MESH_DEPOSIT_AUTO, api.MESH_DEPOSIT_GLOBAL, api.MESH_DEPOSIT_LDS, api.MESH_MAX_SUBSAMPLES) == (0, 1, 2, 4)
    c = api.MeshCells(D.R_EDGES)
    c.close()
    c.close()                                              # idempotent
    assert not c.handle
