"""Mode spectra, host side (no GPU): the entry points exported and refusing bad arguments before touching a device;
the host cbet_sph_modes against an independent numpy restatement node by node (closed forms for l <= 2, scipy's
sph_harm_y without its (-1)^m above), on cubes and on the cases off the cube of tests/helpers/modes_shapes.py; the gfx950
listing of cbet_sph_modes.hip (cross-compiled here)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from helpers import modes_shapes as S

CSRC = os.path.join(ROOT, "cbet_raytracing_3d_amd", "csrc")


@pytest.fixture(scope="module")
def api():
    from cbet_raytracing_3d_amd import api as a
    a.lib()
    return a


def test_bad_arguments_are_refused(api):
    """Every refusal happens before any HIP call (no device here: the fake pointers are never touched)."""
    L = api.lib()
    p = api.default_params(9)
    fake = C.c_void_p(4096)
    ctr = np.zeros(3)
    good = np.linspace(0.0, 0.1, 5)

    def call(fn, edep=fake, ngrids=1, stride=0, params=p, center=ctr, edges=good, nshell=None, lmax=4, out=fake):
        e = np.ascontiguousarray(edges, dtype=np.float64)
        ns = e.size - 1 if nshell is None else nshell
        c = None if center is None else center.ctypes.data_as(C.POINTER(C.c_double))
        return fn(edep, ngrids, stride, C.byref(params), c, e.ctypes.data_as(C.POINTER(C.c_double)), ns, lmax,
                  out, out, out, None)

    for fn in (L.cbet_sph_modes_device, L.cbet_sph_modes):
        assert call(fn, lmax=33) == api.EINVAL
        assert "lmax" in L.cbet_last_error().decode()
        assert call(fn, lmax=-1) == api.EINVAL
        assert call(fn, edges=[0.0, 0.05, 0.05, 0.1]) == api.EINVAL          # not strictly increasing
        assert call(fn, edges=[0.0, 0.06, 0.04]) == api.EINVAL
        assert call(fn, edges=[-0.01, 0.05, 0.1]) == api.EINVAL             # negative
        assert call(fn, edges=[0.0, 0.05, float("nan")]) == api.EINVAL
        assert call(fn, edges=[0.0, 0.05, float("inf")]) == api.EINVAL
        assert call(fn, nshell=0) == api.EINVAL
        assert call(fn, edges=np.linspace(0.0, 0.2, 258), nshell=257) == api.EINVAL
        assert call(fn, edep=None, ngrids=2, stride=11 ** 3) == api.EINVAL   # geometry mode is one grid
        assert "geometry" in L.cbet_last_error().decode()
        assert call(fn, ngrids=0) == api.EINVAL
        assert call(fn, ngrids=65, stride=11 ** 3) == api.EINVAL
        assert call(fn, ngrids=2, stride=11 ** 3 - 1) == api.EINVAL          # grids overlap
        assert call(fn, center=None) == api.EINVAL
        assert call(fn, out=None) == api.EINVAL
        assert call(fn, params=p.copy(nx=2)) == api.EINVAL
        assert call(fn, center=np.array([0.0, np.nan, 0.0])) == api.EINVAL


# ---- numpy restatement ---------------------------------------------------------------------------------------------
def _nodes(api, p, center):
    d = api.derive(p)
    ax = [((np.arange(n + 2) - 1) * step + lo) - c
          for n, step, lo, c in ((p.nx, d.dx, p.xmin, center[0]), (p.ny, d.dy, p.ymin, center[1]), (p.nz, d.dz, p.zmin, center[2]))]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    return X, Y, Z, np.sqrt(X * X + Y * Y + Z * Z)


def _ylm_closed(X, Y, Z, r):
    """Real harmonics without the Condon-Shortley phase for l <= 2, in index order l*l + l + m."""
    pi = math.pi
    with np.errstate(divide="ignore", invalid="ignore"):
        x, y, z = (np.where(r > 0, v / r, 0.0) for v in (X, Y, Z))
    out = [np.full(r.shape, 0.5 / math.sqrt(pi))]
    k1 = math.sqrt(3.0 / (4 * pi))
    out += [k1 * y, k1 * z, k1 * x]                                              # m = -1, 0, 1
    out += [math.sqrt(15.0 / (4 * pi)) * x * y, math.sqrt(15.0 / (4 * pi)) * y * z,
            math.sqrt(5.0 / (16 * pi)) * (3 * z * z - 1.0) * (r > 0),
            math.sqrt(15.0 / (4 * pi)) * x * z, math.sqrt(15.0 / (16 * pi)) * (x * x - y * y)]
    return np.stack(out)


def _ylm_scipy(lmax, X, Y, Z, r):
    special = pytest.importorskip("scipy.special")
    with np.errstate(divide="ignore", invalid="ignore"):
        ct = np.where(r > 0, Z / r, 1.0)
    theta, phi = np.arccos(np.clip(ct, -1.0, 1.0)), np.arctan2(Y, X)
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
    out[1:, r == 0] = 0.0                                      # a node at the centre counts for Y_00 only
    out[0, r == 0] = 0.5 / math.sqrt(math.pi)
    return out


def _numpy_modes(grids, r, edges, Yc):
    nshell = len(edges) - 1
    s = np.searchsorted(edges, r, side="right") - 1
    inside = (s >= 0) & (s < nshell)
    G = grids.shape[0]
    coeffs = np.zeros((G, nshell, Yc.shape[0]))
    energy, absE = np.zeros((G, nshell)), np.zeros((G, nshell))
    nodes = np.bincount(s[inside], minlength=nshell)
    for g in range(G):
        E = grids[g][..., : r.shape[2]]
        for sh in range(nshell):
            sel = inside & (s == sh)
            coeffs[g, sh] = (Yc[:, sel] * E[sel]).sum(-1)
            energy[g, sh] = E[sel].sum()
            absE[g, sh] = np.abs(E[sel]).sum()
    return coeffs, energy, absE, nodes


CASES = [
    # n, centre, edges (None: through the corners), grids
    (9, (0.0, 0.0, 0.0), [0.0, 0.02, 0.06, 0.12, 0.2, 0.23], 2),              # a node at r = 0 (odd n, symmetric box)
    (17, (0.011, -0.007, 0.003), list(np.linspace(0.0, 0.2, 8)), 1),
    (8, (0.0, 0.0, 0.0), [0.01, 0.05, 0.08, 0.13], 1),                        # first edge > 0: the core is in no shell
]


@pytest.mark.parametrize("n,center,edges,G", CASES)
def test_host_matches_numpy_closed_forms(api, n, center, edges, G):
    p = api.default_params(n)
    X, Y, Z, r = _nodes(api, p, center)
    rng = np.random.default_rng(n)
    grids = rng.uniform(-1.0, 3.0, (G,) + r.shape) * 1e15
    coeffs, energy, nodes = api.sph_modes_host(grids if G > 1 else grids[0], p, center, edges, 2)
    want, want_e, absE, want_n = _numpy_modes(grids, r, np.asarray(edges), _ylm_closed(X, Y, Z, r))
    assert coeffs.shape == (G, len(edges) - 1, 9)
    assert np.array_equal(nodes, want_n)
    assert np.all(np.abs(coeffs - want) <= 1e-13 * absE[..., None])
    assert np.all(np.abs(energy - want_e) <= 1e-13 * absE)
    # geometry mode: E = 1
    gc, ge, gn = api.sph_modes_host(None, p, center, edges, 2)
    wc, we, wa, _ = _numpy_modes(np.ones((1,) + r.shape), r, np.asarray(edges), _ylm_closed(X, Y, Z, r))
    assert np.array_equal(gn, want_n) and np.array_equal(ge[0], want_n.astype(np.float64))
    assert np.all(np.abs(gc - wc) <= 1e-13 * wa[..., None])


@pytest.mark.parametrize("n,center,edges,G", CASES[:2])
@pytest.mark.parametrize("lmax", [8, 32])
def test_host_matches_numpy_scipy(api, n, center, edges, G, lmax):
    p = api.default_params(n)
    X, Y, Z, r = _nodes(api, p, center)
    Yc = _ylm_scipy(lmax, X, Y, Z, r)
    assert np.allclose(Yc[:9], _ylm_closed(X, Y, Z, r), rtol=0, atol=1e-13)     # the two restatements agree
    rng = np.random.default_rng(100 + n)
    grids = rng.uniform(0.0, 1.0, (G,) + r.shape) * 1e17
    coeffs, energy, nodes = api.sph_modes_host(grids, p, center, edges, lmax)
    want, want_e, absE, want_n = _numpy_modes(grids, r, np.asarray(edges), Yc)
    assert np.array_equal(nodes, want_n)
    err = np.abs(coeffs - want) / absE[..., None]
    assert err.max() <= 1e-13, err.max()
    assert np.all(np.abs(energy - want_e) <= 1e-13 * absE)


@pytest.mark.parametrize("name", S.NAMES)
def test_host_matches_numpy_off_the_cube(api, name):
    """tests/helpers/modes_shapes.py: grids with three different sides, an off-centre box, unequal spacing, a centre
    outside the box, odd and small lmax, empty shells -- three grids with values of both signs, and geometry mode."""
    _, shape, _, center, lmax = S.BY_NAME[name]
    p = S.params(api, name)
    assert (p.nx, p.ny, p.nz) == shape and len({p.nx, p.ny, p.nz}) == 3
    X, Y, Z, r = _nodes(api, p, center)
    assert r.shape == (shape[0] + 2, shape[1] + 2, shape[2] + 2)
    Yc = _ylm_scipy(lmax, X, Y, Z, r)
    nc = min(9, (lmax + 1) ** 2)
    assert np.allclose(Yc[:nc], _ylm_closed(X, Y, Z, r)[:nc], rtol=0, atol=1e-13)
    grids = S.grids(name)
    assert (grids < 0).any() and (grids > 0).any()
    coeffs, energy, nodes = api.sph_modes_host(grids, p, center, S.EDGES, lmax)
    want, want_e, absE, want_n = _numpy_modes(grids, r, S.EDGES, Yc)
    # the regime: a shell too thin to hold a node, a second empty one, and shells that do hold nodes
    assert want_n[S.THIN] == 0 and int((want_n == 0).sum()) >= 2 and int((want_n > 0).sum()) >= 2
    if name == "centre_outside":
        assert X.max() < -0.1                                   # every node, halo included, lies to one side of the centre
    else:
        assert want_n[-1] == 0 and r.max() < S.EDGES[-2]        # the last shell lies beyond every node
    assert coeffs.shape == (3, len(S.EDGES) - 1, (lmax + 1) ** 2)
    assert np.array_equal(nodes, want_n)
    err = np.abs(coeffs - want) / np.maximum(absE[..., None], 1e-300)
    print("%s: host twin vs numpy/scipy, max |da| / sum |E| = %.2e, nodes per shell %s" % (name, err.max(), want_n.tolist()))
    assert np.all(np.abs(coeffs - want) <= 1e-13 * absE[..., None])
    assert np.all(np.abs(energy - want_e) <= 1e-13 * absE)
    assert not coeffs[:, want_n == 0].any() and not energy[:, want_n == 0].any()      # an empty shell gives zeros
    gc, ge, gn = api.sph_modes_host(None, p, center, S.EDGES, lmax)
    wc, _, wa, _ = _numpy_modes(np.ones((1,) + r.shape), r, S.EDGES, Yc)
    assert np.array_equal(gn, want_n) and np.array_equal(ge[0], want_n.astype(np.float64))
    assert np.all(np.abs(gc - wc) <= 1e-13 * wa[..., None])


def test_host_padded_rows_give_the_dense_bits(api):
    p = api.default_params(11)
    rng = np.random.default_rng(7)
    dense = rng.uniform(0.0, 1.0, (2, 13, 13, 13))
    padded = np.full((2, 13, 13, 16), np.nan)           # the padding is never read
    padded[..., :13] = dense
    edges = np.linspace(0.0, 0.2, 6)
    a = api.sph_modes_host(dense, p, (0.001, 0.0, -0.002), edges, 6)
    b = api.sph_modes_host(padded, p, (0.001, 0.0, -0.002), edges, 6)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_modes_helpers():
    from cbet_raytracing_3d_amd import modes
    from cbet_raytracing_3d_amd import api as A
    assert [modes.sph_index(l, m) for l, m in ((0, 0), (1, -1), (1, 0), (1, 1), (2, -2), (4, 3))] == [0, 1, 2, 3, 4, 23]
    with pytest.raises(ValueError):
        modes.sph_index(2, 3)
    p = A.default_params(64, xmin=-0.1, ymax=0.12)
    e = modes.default_shells(p, 32)
    assert e.shape == (33,) and e[0] == 0.0 and e[-1] == 0.1 and np.allclose(np.diff(e), 0.1 / 32)
    a = np.zeros((3, 9))
    a[:, 0] = 2.0
    a[1, 2] = 1.0                        # l = 1
    a[2, 4], a[2, 8] = 3.0, 4.0          # l = 2: P_2 = 25
    P = modes.mode_power(a)
    assert np.array_equal(P[2], [4.0, 0.0, 25.0])
    s_l, s_rms = modes.nonuniformity(a)
    assert np.allclose(s_l[1], [1.0, 0.5, 0.0]) and np.allclose(s_rms, [0.0, 0.5, 2.5])
    w = np.array([0.5, 2.0, 1.0])
    assert np.allclose(modes.balance(a, w), 0.5 * a[0] + 2.0 * a[1] + a[2])


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from cbet_raytracing_3d_amd import build
    out = tmp_path_factory.mktemp("isa_sph") / "sph.s"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [build.hipcc()] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                                     "-o", str(out), os.path.join(CSRC, "cbet_sph_modes.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    text = out.read_text()
    kernels = {}
    for m in re.finditer(r"^(_ZN4cbet\S*k_sph_modes\S*):[^\n]*\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M):
        kernels[m.group(1)] = m.group(2)
    return kernels


def test_listing_no_scratch_at_lmax16_and_no_atomics(listing):
    lmax16 = {n: b for n, b in listing.items() if "ILi16E" in n}
    assert len(lmax16) == 2 and any("ILi32E" in n for n in listing)      # one grid and four grids per block; lmax 32
    for name, body in lmax16.items():
        meta = dict(re.findall(r"\.amdhsa_(\w+)\s+(\S+)", body))
        assert int(meta["private_segment_fixed_size"]) == 0, name
    for name, body in listing.items():
        ops = [l.split()[0] for l in body.splitlines() if l.startswith("\t") and not l.strip().startswith(";")]
        assert ops and not [o for o in ops if "atomic" in o], name
        assert any(o.startswith("global_store") for o in ops), name


def test_grid_layout_reads_one_grid_a_padded_grid_or_a_stack(api):
    """api.grid_layout, the one reading of a deposit array's shape (sph_modes, deposit_on_mesh and their host twins):
    (ngrids, grid_stride, params with edep_zpitch, stacked)."""
    p = api.default_params(8)
    p.edep_zpitch = 24                                      # whatever the caller's params say, the shape decides
    want = {(10, 10, 10): (1, 1000, 0, False), (10, 10, 16): (1, 1600, 16, False), (3, 10, 10, 10): (3, 1000, 0, True),
            (1, 10, 10, 10): (1, 1000, 0, True), (2, 10, 10, 16): (2, 1600, 16, True)}
    for shape, (ngrids, stride, zpitch, stacked) in want.items():
        got = api.grid_layout(shape, p)
        assert (got[0], got[1], got[2].edep_zpitch, got[3]) == (ngrids, stride, zpitch, stacked), shape
        assert got[2] is not p and (got[2].nx, got[2].nbeams) == (p.nx, p.nbeams)
    got = api.grid_layout(None, p)                          # no array: geometry mode, counts alone
    assert (got[0], got[1], got[2].edep_zpitch, got[3]) == (1, 0, 0, False)
    assert p.edep_zpitch == 24                              # the caller's params are not changed
    for shape in ((10, 10, 9), (10, 9, 10), (9, 10, 10), (10, 10), (2, 3, 10, 10, 10), (3, 10, 10, 9)):
        with pytest.raises(ValueError):
            api.grid_layout(shape, p)
    with pytest.raises(ValueError):                         # ... and through the host twin
        api.sph_modes_host(np.zeros((10, 9, 10)), api.default_params(8), (0.0, 0.0, 0.0), [0.0, 0.1], 2)
