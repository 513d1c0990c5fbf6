"""Local plasma state of the gain kernels on the host (include/cbet_mi355x.h cbet_mesh_state_table):
the host twin of k_mesh_state against cbet_gain_constants for a uniform state (bitwise), against a numpy restatement for a
genuinely 3-D mesh with ion fields, its refusals, and the ctypes mirror of cbet_mesh_ions.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from helpers import mesh_cases as M
from helpers import state_cases as S


@pytest.fixture(scope="module")
def api():
    from cbet_raytracing_3d_amd import api as a
    a.lib()
    return a


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


# ---- 1. a uniform state is cbet_gain_constants' pair, bit for bit -----------------------------------------------------------
@pytest.mark.parametrize("triple", S.TRIPLES, ids=["default", "cold_z1_ti0", "corona", "hot_high_z"])
@pytest.mark.parametrize("shape", M.SHAPES, ids=M.SHAPE_IDS)
@pytest.mark.parametrize("center", [(0.0, 0.0, 0.0), M.OFFSET], ids=["centred", "offset"])
@pytest.mark.parametrize("explicit", [False, True], ids=["ions_null", "ions_arrays"])
@pytest.mark.parametrize("angles", [(1, 1), (5, 7)], ids=["1d", "5x7"])
def test_uniform_state_is_gain_constants_bitwise(api, inputs, angles, explicit, center, shape, triple):
    te_ev, ti_ev, z_ion = triple
    p = M.params(api, shape)
    gp = api.default_gain_params(te_ev=te_ev, ti_ev=ti_ev, z_ion=z_ion)
    _, cs, gc = api.gain_constants(p, gp)
    mesh = S.uniform_mesh(api, inputs, angles, center, te_ev, (ti_ev, z_ion) if explicit else None)
    table = api.mesh_state_table(p, gp, mesh, ions=explicit)
    assert table.shape == (2,) + tuple(shape)
    assert np.all(_bits(table[0]) == _bits(cs)) and np.all(_bits(table[1]) == _bits(gc))
    if explicit:                                                                # the arrays are what is read: others, another table
        other = api.mesh_state_table(p, gp, S.uniform_mesh(api, inputs, angles, center, te_ev, (ti_ev + 50.0, 2.0 * z_ion)))
        assert not np.any(_bits(other[0]) == _bits(cs)) and not np.any(_bits(other[1]) == _bits(gc))


# ---- 2. a genuinely 3-D mesh against the numpy restatement --------------------------------------------------------------
@pytest.fixture(scope="module", params=M.SHAPES, ids=M.SHAPE_IDS)
def case3d(request, api):
    p = M.params(api, request.param)
    mesh, a = S.mesh3d_ions(api)
    return p, mesh, a, M.Restatement(api, p, a["r"], a["theta"], a["phi"], a["center"])


@pytest.mark.parametrize("ions", [True, False], ids=["ti_zbar", "ions_null"])
def test_3d_mesh_matches_the_numpy_restatement(api, case3d, ions):
    p, mesh, a, R = case3d
    gp = api.default_gain_params()
    got = api.mesh_state_table(p, gp, mesh, ions=ions)
    want, top = S.restated_table(api, p, gp, R, a["te"], a["ti"] if ions else None, a["zbar"] if ions else None)
    for c, name in enumerate(("cs", "gain_const")):
        worst = float((np.abs(got[c] - want[c]) / top[c]).max())
        print("%s: max |diff| = %.3e of the largest corner-derived value (bound %.0e)" % (name, worst, M.TOL))
        assert np.all(np.abs(got[c] - want[c]) <= M.TOL * top[c]), name
    assert got[0].min() > 1e6 and got[1].min() > 0                              # cm/s; positive
    assert got[0].max() > 1.1 * got[0].min() and got[1].max() > 1.1 * got[1].min()     # a state that varies
    if ions:                                                                    # ... by a factor, and the ion fields matter
        assert got[0].max() > 1.3 * got[0].min() and got[1].max() > 1.5 * got[1].min()
        plain = api.mesh_state_table(p, gp, mesh, ions=False)
        assert np.abs(plain - got).max(axis=(1, 2, 3)).min() > 0
        assert np.abs(plain[0] / got[0] - 1.0).max() > 1e-2


@pytest.mark.parametrize("shape", M.SHAPES, ids=M.SHAPE_IDS)
def test_1d_mesh_and_its_broadcast_give_the_same_bits(api, inputs, shape):
    _, r, ne, te = inputs
    p, gp = M.params(api, shape), api.default_gain_params()
    ti, zbar = 0.5 * te, 1.0 + 2.5 * te / te.max()
    one = api.mesh_state_table(p, gp, api.Mesh(r, None, None, ne, te, None, M.OFFSET, ti=ti, zbar=zbar))
    full = lambda f: np.broadcast_to(f[:, None, None], (r.size, 5, 7))          # noqa: E731
    many = api.mesh_state_table(p, gp, api.Mesh(r, np.linspace(0.1, 3.0, 5), np.linspace(-3.0, 2.9, 7), full(ne), full(te), None,
                                                M.OFFSET, ti=full(ti), zbar=full(zbar)))
    assert np.array_equal(_bits(one), _bits(many))
    assert one[0].max() > 2.0 * one[0].min()                                    # 88 eV at the centre to ~940 eV in the corona


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------
def _good(**ions):
    r, theta, phi = np.array([0.0, 0.1, 0.2]), np.array([0.5, 1.5, 2.5]), np.array([-3.0, -1.0, 1.0, 3.0])
    f = np.ones((3, 3, 4))
    kw = dict(r=r, theta=theta, phi=phi, ne=f.copy(), te=300.0 * f, center=[0.0, 0.0, 0.0], ti=100.0 * f, zbar=3.0 * f)
    for name, (index, value) in ions.items():
        kw[name][index] = value
    return kw


BAD_IONS = {
    "ti negative": (_good(ti=((1, 2, 3), -1.0)), "ti[23]"),
    "ti nan": (_good(ti=((0, 0, 1), float("nan"))), "ti[1]"),
    "ti inf": (_good(ti=((2, 2, 3), float("inf"))), "ti[35]"),
    "zbar zero": (_good(zbar=((0, 1, 0), 0.0)), "zbar[4]"),
    "zbar negative": (_good(zbar=((1, 0, 2), -2.0)), "zbar[14]"),
    "zbar nan": (_good(zbar=((2, 0, 0), float("nan"))), "zbar[24]"),
    # cbet_mesh_check's own rules come first
    "te zero": (_good(te=((2, 2, 3), 0.0)), "te[35]"),
    "ne nan": (_good(ne=((0, 0, 1), float("nan"))), "ne[1]"),
    "r not ascending": (_good(r=(1, 0.2)), "ascending"),
    "phi a whole period": (_good(phi=(3, -3.0 + 2 * np.pi)), "period"),
}


@pytest.mark.parametrize("name", sorted(BAD_IONS))
def test_bad_ion_fields_and_bad_meshes_are_refused(api, name):
    kw, word = BAD_IONS[name]
    p, gp = M.params(api, (9, 9, 9)), api.default_gain_params()
    api.mesh_state_table(p, gp, api.Mesh(**_good()))                            # the unchanged mesh is accepted
    with pytest.raises(api.CbetError) as ei:
        api.mesh_state_table(p, gp, api.Mesh(**kw))
    assert ei.value.code == api.EINVAL and word in str(ei.value), str(ei.value)
    if word.startswith(("ti[", "zbar[")):                                       # ions=False does not read the arrays
        api.mesh_state_table(p, gp, api.Mesh(**kw), ions=False)


def test_bad_arguments_are_refused(api):
    p, gp = M.params(api, (9, 9, 9)), api.default_gain_params()
    good = api.Mesh(**_good())
    L = api.lib()
    out = np.zeros(2 * 9 ** 3)
    dp = out.ctypes.data_as(C.POINTER(C.c_double))

    def refused(rc, word):
        assert rc == api.EINVAL
        assert word in L.cbet_last_error().decode(), L.cbet_last_error()

    refused(L.cbet_mesh_state_table(C.byref(p), C.byref(gp), C.byref(good), C.byref(good.ions), None), "NULL output")
    refused(L.cbet_mesh_state_table(C.byref(p), C.byref(gp), None, None, dp), "mesh is NULL")
    refused(L.cbet_mesh_state_table(C.byref(p), None, C.byref(good), None, dp), "gain params is NULL")
    assert L.cbet_mesh_state_table(C.byref(p), C.byref(gp), C.byref(good), None, dp) == api.OK       # ions NULL is legal
    for bad in (dict(te_ev=0.0), dict(ti_ev=-1.0), dict(z_ion=0.0), dict(mi_over_me=float("nan")), dict(iaw=0.0)):
        with pytest.raises(api.CbetError) as ei:
            api.mesh_state_table(p, api.default_gain_params(**bad), good)
        assert ei.value.code == api.EINVAL and "plasma constants" in str(ei.value), bad
    m = api.Mesh(**_good())
    m.te = None
    with pytest.raises(api.CbetError) as ei:
        api.mesh_state_table(p, gp, m)
    assert ei.value.code == api.EINVAL and "NULL" in str(ei.value)
    # a wrong shape never reaches the library (which sees pointers only): api.Mesh checks ti and zbar like ne
    kw = _good()
    for name in ("ti", "zbar"):
        with pytest.raises(ValueError) as ve:
            api.Mesh(**dict(kw, **{name: np.ones((3, 3, 5))}))
        assert name in str(ve.value) and "shape" in str(ve.value)


def test_python_mesh_keeps_the_ion_fields_beside_the_struct(api):
    kw = _good()
    m = api.Mesh(**kw)
    assert C.sizeof(m) == C.sizeof(api.Mesh(kw["r"], kw["theta"], kw["phi"], kw["ne"], kw["te"]))
    assert m.ions.ti and m.ions.zbar
    kw["ti"][:] = -5.0                                                          # the mesh holds its own copies
    api.mesh_state_table(M.params(api, (9, 9, 9)), api.default_gain_params(), m)
    bare = api.Mesh(kw["r"], kw["theta"], kw["phi"], kw["ne"], kw["te"], zbar=kw["zbar"])
    assert bare.ions.ti is None and bare.ions.zbar


# ---- 4. the ctypes mirror ---------------------------------------------------------------------------------------------------
def test_mesh_ions_layout_matches_header(api):
    """The sizes of cbet_mesh_ions and of cbet_mesh, which must not have moved (test_abi_host.py asks gcc for both layouts)."""
    assert api.STRUCTS["cbet_mesh_ions"] is api.MeshIons and api.STRUCTS["cbet_mesh"] is api.Mesh
    assert C.sizeof(api.MeshIons) == 16 and C.sizeof(api.Mesh) == 104
