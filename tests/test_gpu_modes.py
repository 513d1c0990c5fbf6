"""Mode spectra on the GPU (include/cbet_mi355x.h cbet_sph_modes_device): the device projection
against the host cbet_sph_modes on the real OMEGA deposit and on seeded grids off the cube (three different sides, off-centre
and unequally spaced boxes, a centre outside the box, run-time lmax below the instantiated one, empty shells), determinism
(run to run, padded rows), linearity in the beams (per-beam grids, power balance), the symmetry of the cubic lattice, and the
256^3 totals."""
import numpy as np
import pytest

from helpers import modes_shapes as S

pytestmark = pytest.mark.gpu

SURVEY_256_TOTAL = 1.0076068555e19    # SURVEY: sum of the 256^3 / 60-beam deposit
CORNER = 0.13 * 3 ** 0.5              # the default box's half-diagonal


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "the gpu tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def api():
    from cbet_raytracing_3d_amd import api as a
    a.lib()
    return a


@pytest.fixture(scope="module")
def modes():
    from cbet_raytracing_3d_amd import modes as m
    return m


def _tracer(api, inputs, n):
    from cbet_raytracing_3d_amd.tracer import RayTracer
    bn, r, ne, te = inputs
    return RayTracer(api.default_params(n), r, ne, te, beam_norm=bn)


@pytest.fixture(scope="module")
def t64(api, inputs, torch_cuda):
    tr = _tracer(api, inputs, 64)
    single, beams = tr.new_grid(), tr.new_grid(per_beam=True)
    tr.launch(single)
    tr.launch(beams)
    torch_cuda.cuda.synchronize()
    yield tr, single, beams
    tr.close()


@pytest.fixture(scope="module")
def t100(api, inputs, torch_cuda):
    tr = _tracer(api, inputs, 100)
    single = tr.new_grid()
    tr.launch(single)
    torch_cuda.cuda.synchronize()
    yield tr, single
    tr.close()


def _against_host(api, tr, grid, edges, lmax, center=(0.0, 0.0, 0.0), geometry=False):
    """Device result vs the host twin: |da| <= 1e-11 x the shell's sum |E|, shell energy 1e-13, node counts exact."""
    dc, de, dn = tr.sph_modes(grid, edges, lmax, center, geometry)
    host_grid = None if geometry else grid.cpu().numpy()
    hc, he, hn = api.sph_modes_host(host_grid, tr.params, center, edges, lmax)
    if geometry:
        absE = he
    else:
        _, absE, _ = api.sph_modes_host(np.abs(host_grid), tr.params, center, edges, 0)
    dc, de, dn = dc.cpu().numpy(), de.cpu().numpy(), dn.cpu().numpy()
    if dc.ndim == 2:
        dc, de = dc[None], de[None]
    assert dc.shape == hc.shape and de.shape == he.shape
    assert np.array_equal(dn, hn)
    assert np.all(np.abs(dc - hc) <= 1e-11 * absE[..., None]), np.max(np.abs(dc - hc) / np.maximum(absE[..., None], 1e-300))
    assert np.all(np.abs(de - he) <= 1e-13 * absE)
    assert hn.sum() > 0
    return dc, hc


def test_device_equals_host_64_single(api, modes, t64):
    tr, single, _ = t64
    shells = modes.default_shells(tr.params, 32)
    corners = np.linspace(0.0, CORNER * 1.001, 25)
    for lmax in (16, 32):
        _against_host(api, tr, single, shells, lmax)
    _against_host(api, tr, single, corners, 16)
    _against_host(api, tr, single, shells, 16, center=(0.004, -0.0025, 0.0015))
    _against_host(api, tr, single, corners, 32, center=(-0.003, 0.002, 0.001))
    _against_host(api, tr, None, shells, 16, geometry=True)
    _against_host(api, tr, None, corners, 32, geometry=True)


def test_device_equals_host_64_per_beam(api, modes, t64):
    tr, _, beams = t64
    dc, _ = _against_host(api, tr, beams, modes.default_shells(tr.params, 32), 16)
    assert dc.shape[0] == 60
    # a stack that is not a multiple of the four grids a block takes, with shells to the corners, at lmax 32
    _against_host(api, tr, beams[:7].contiguous(), np.linspace(0.0, CORNER * 1.001, 9), 32, center=(0.001, 0.0, -0.002))


def test_device_equals_host_100(api, modes, t100):
    tr, single = t100
    _against_host(api, tr, single, modes.default_shells(tr.params, 32), 16)
    _against_host(api, tr, single, np.linspace(0.0, CORNER * 1.001, 40), 32, center=(0.002, 0.003, -0.001))


# ---- off the cube (tests/helpers/modes_shapes.py; the host twin's own check of these cases is in test_modes_host.py) ----
def _worst(api, tr, dc, hc, host_grid, edges, center):
    """max |da| over the shell's sum |E| (geometry: its node count), for the printed figure."""
    if host_grid is None:
        absE = api.sph_modes_host(None, tr.params, center, edges, 0)[1]
    else:
        absE = api.sph_modes_host(np.abs(host_grid), tr.params, center, edges, 0)[1]
    full = absE > 0
    return float((np.abs(dc - hc)[full] / absE[full][:, None]).max())


def _shaped_tracer(api, inputs, name):
    """A tracer of the case's grid and box as the handle of sph_modes (nothing is traced)."""
    from cbet_raytracing_3d_amd.tracer import RayTracer
    bn, r, ne, te = inputs
    return RayTracer(S.params(api, name, nbeams=1), r, ne, te, beam_norm=bn[:1])


@pytest.fixture(scope="module", params=S.NAMES)
def shaped(request, api, inputs, torch_cuda):
    """The case's tracer and a stack of seven seeded grids of both signs."""
    name = request.param
    tr = _shaped_tracer(api, inputs, name)
    stack = torch_cuda.from_numpy(S.grids(name, 7)).cuda()
    yield name, tr, stack
    tr.close()


def test_device_equals_host_off_the_cube(api, shaped):
    """Three different sides (the node decode, `plane`), off-centre and unequally spaced boxes (node_range per axis), a
    centre outside the box, lmax 5 / 3 / 1 under <16> and 17 under <32> (odd: the middle m-group drops its second half),
    shells without a node: one grid, a stack of three (one ragged block of the four-grid kernel), a stack of seven (a full
    block and a ragged one), and geometry mode."""
    name, tr, stack = shaped
    _, shape, _, center, lmax = S.BY_NAME[name]
    assert tuple(stack.shape[1:]) == tr.grid_shape == (shape[0] + 2, shape[1] + 2, shape[2] + 2)
    assert lmax % 2 == 1
    for what, grid in (("one grid", stack[0].contiguous()), ("stack of 3", stack[:3].contiguous()), ("stack of 7", stack),
                       ("geometry", None)):
        dc, hc = _against_host(api, tr, grid, S.EDGES, lmax, center=center, geometry=grid is None)
        _, _, dn = tr.sph_modes(grid, S.EDGES, lmax, center, grid is None)
        dn = dn.cpu().numpy()
        # the regime (asserted on the host twin's cases in test_modes_host.py too): the thin shell and one more are empty
        assert dn[S.THIN] == 0 and int((dn == 0).sum()) >= 2 and int((dn > 0).sum()) >= 2
        assert not dc[:, dn == 0].any()                                       # an empty shell is written, with zeros
        print("%-15s lmax %2d %-10s: max |da - host| / sum |E| = %.2e" %
              (name, lmax, what, _worst(api, tr, dc, hc, None if grid is None else grid.cpu().numpy(), S.EDGES, center)))


def test_padded_rows_off_the_cube_give_the_dense_bits(api, inputs, torch_cuda):
    """On 12 x 7 x 70: rows padded to whole lines (nz + 2 = 72 is one already: zpitch=True is the dense grid) and to an odd
    pitch of 77 doubles, the padding NaN, against the dense grid -- bit for bit."""
    torch = torch_cuda
    name = "long_z"
    _, shape, _, center, lmax = S.BY_NAME[name]
    assert shape == (12, 7, 70)
    tr = _shaped_tracer(api, inputs, name)
    dense = torch.from_numpy(S.grids(name, 1)[0]).cuda()
    want = tr.sph_modes(dense, S.EDGES, lmax, center)
    for pitch in (True, 77):
        padded = tr.new_grid(zpitch=pitch)
        assert padded.shape[2] == (72 if pitch is True else 77)
        padded.fill_(float("nan"))
        padded[..., : dense.shape[2]] = dense
        got = tr.sph_modes(padded, S.EDGES, lmax, center)
        for x, y in zip(want, got):
            assert torch.equal(x, y)
    assert bool(want[2].sum() > 0)
    tr.close()


LMAX_SWEEP = (0, 1, 2, 3, 5, 15, 17, 31)


def test_lmax_sweep_is_a_prefix_of_lmax_32(api, modes, t64):
    """A run-time lmax below the instantiated one -- 0, 1, 2, 3, 5, 15 under <16>, 17 and 31 under <32> -- on the real 64^3
    deposit: against the host twin, and against the leading (lmax + 1)^2 columns of the lmax = 32 result (a truncated
    expansion is a prefix of the longer one), both within 1e-11 x the shell's sum |E|."""
    tr, single, _ = t64
    shells = modes.default_shells(tr.params, 32)
    host_grid = single.cpu().numpy()
    _, absE, _ = api.sph_modes_host(np.abs(host_grid), tr.params, (0.0, 0.0, 0.0), shells, 0)
    absE = absE[0]
    assert (absE > 0).sum() > 16
    a32 = tr.sph_modes(single, shells, 32)[0].cpu().numpy()
    for lmax in LMAX_SWEEP:
        dc, hc = _against_host(api, tr, single, shells, lmax)
        n = (lmax + 1) ** 2
        assert dc.shape == (1, 32, n)
        diff = np.abs(dc[0] - a32[:, :n])
        full = absE > 0
        print("lmax %2d: max |da - host| / sum |E| = %.2e, against the lmax 32 prefix %.2e" %
              (lmax, (np.abs(dc - hc)[0][full] / absE[full][:, None]).max(), (diff[full] / absE[full][:, None]).max()))
        assert np.all(diff <= 1e-11 * absE[:, None]), lmax
    assert np.abs(a32[:, 1:]).max() > 1e-6 * np.abs(a32[:, 0]).max()          # (not a spectrum of zeros beyond l = 0)


def test_bitwise_reproducible_and_padded_rows(modes, t64, torch_cuda):
    torch = torch_cuda
    tr, single, beams = t64
    shells = modes.default_shells(tr.params, 32)
    a = tr.sph_modes(single, shells, 16)
    b = tr.sph_modes(single, shells, 16)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    padded = tr.new_grid(zpitch=True)
    assert padded.shape[2] > single.shape[2]
    padded.fill_(float("nan"))                      # the padding is never read
    padded[..., : single.shape[2]] = single
    c = tr.sph_modes(padded, shells, 16)
    for x, y in zip(a, c):
        assert torch.equal(x, y)
    p1 = tr.sph_modes(beams, shells, 16)
    p2 = tr.sph_modes(beams, shells, 16)
    for x, y in zip(p1, p2):
        assert torch.equal(x, y)


def test_linear_in_the_beams(modes, t64, torch_cuda):
    torch = torch_cuda
    tr, single, beams = t64
    shells = modes.default_shells(tr.params, 32)
    a_single = tr.sph_modes(single, shells, 16)[0].cpu().numpy()
    a_beams = tr.sph_modes(beams, shells, 16)[0].cpu().numpy()
    a00 = np.abs(a_single[:, :1])
    assert np.all(np.abs(a_beams.sum(0) - a_single) <= 1e-12 * a00)
    rng = np.random.default_rng(20261016)
    w = rng.uniform(0.25, 1.75, 60)
    combined = (torch.from_numpy(w).to(beams.device).view(60, 1, 1, 1) * beams).sum(0).contiguous()
    a_comb = tr.sph_modes(combined, shells, 16)[0].cpu().numpy()
    bal = modes.balance(a_beams, w)
    assert np.all(np.abs(bal - a_comb) <= 1e-12 * np.abs(a_comb[:, :1]))
    # the torch form of balance is the same sum
    bal_t = modes.balance(torch.from_numpy(a_beams), w).numpy()
    assert np.all(np.abs(bal_t - bal) <= 1e-14 * np.abs(bal[:, :1]))


def test_swapping_x_and_y_maps_the_coefficients(modes, t64):
    tr, single, _ = t64
    shells = modes.default_shells(tr.params, 32)
    a = tr.sph_modes(single, shells, 16)[0].cpu().numpy()
    b = tr.sph_modes(single.transpose(0, 1).contiguous(), shells, 16)[0].cpu().numpy()
    want = np.empty_like(a)
    for l in range(17):
        want[:, modes.sph_index(l, 0)] = a[:, modes.sph_index(l, 0)]
        for m in range(1, l + 1):
            cm, sm = (1, 0, -1, 0)[m % 4], (0, 1, 0, -1)[m % 4]      # cos(m pi / 2), sin(m pi / 2)
            ap, an = a[:, modes.sph_index(l, m)], a[:, modes.sph_index(l, -m)]
            want[:, modes.sph_index(l, m)] = cm * ap + sm * an
            want[:, modes.sph_index(l, -m)] = sm * ap - cm * an
    assert np.all(np.abs(b - want) <= 1e-12 * np.abs(a[:, :1]))
    assert np.abs(a[:, 1:]).max() > 1e-6 * np.abs(a[:, 0]).max()     # (not a trivially symmetric deposit)


def test_geometry_floor_is_cubic(modes, t64):
    tr, _, _ = t64
    coeffs, energy, nodes = tr.sph_modes(None, modes.default_shells(tr.params, 32), 16, geometry=True)
    a = coeffs.cpu().numpy()
    assert np.array_equal(energy.cpu().numpy(), nodes.cpu().numpy().astype(np.float64))
    full = nodes.cpu().numpy() > 0
    a00 = a[full, :1]
    for l in list(range(1, 17, 2)) + [2]:
        assert np.all(np.abs(a[full, l * l:(l + 1) * (l + 1)]) <= 1e-10 * a00), l
    sigma_l, _ = modes.nonuniformity(a[full])
    assert np.all(sigma_l[len(sigma_l) // 2:, 4] > 1e-6)               # l = 4 does not vanish (outer half of the shells)


def test_totals_256(api, inputs, torch_cuda):
    tr = _tracer(api, inputs, 256)
    try:
        e = tr.new_grid()
        tr.launch(e)
        edges = np.linspace(0.0, CORNER * 1.01, 9)          # every node is in a shell
        coeffs, energy, nodes = tr.sph_modes(e, edges, 4)
        total = float(e.sum())
        got = float(energy.sum())
        assert int(nodes.sum()) == 258 ** 3
        assert abs(got - total) <= 1e-12 * total
        assert abs(got / SURVEY_256_TOTAL - 1.0) < 1e-10
        assert abs(float(coeffs[:, 0].sum()) * (4 * np.pi) ** 0.5 / total - 1.0) < 1e-12    # Y_00 = 1 / sqrt(4 pi)
    finally:
        tr.close()
