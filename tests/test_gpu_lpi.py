"""The quarter-critical LPI maps on the device (cbet_lpi.hip k_lpi_map + k_lpi_reduce) against the host
twin cbet_lpi_map_host, on the cases of helpers/lpi_cases.py -- TRACED, CROWDED with its two bands, RAMP -- and end to end at
32^3 behind a CBET solve.

The kernel and the twin run one header's statements under -ffp-contract=off, so the stack is compared BIT FOR BIT: a derived
condition, not a tolerance.  The summary's counts, maxima, max_present and argmax_cw are equal; its two sums are taken in
another order on the device and agree within the any-order bound (n - 1) 2^-53 sum |terms| per sum (tests/test_gpu_exit_arms.py's
rule for k_exit_tally).  The fields are the host-normalised ones of the twin's tests, uploaded; the twin's results are computed
once per case and shared."""
import numpy as np
import pytest

from conftest import NCPU
from helpers import gain_calls as D
from helpers import gain_worlds as W
from helpers import lpi_cases as LC
from helpers.lpi_cases import BAND, I_CW, I_SUM

pytestmark = pytest.mark.gpu

NAMES = ["traced", "crowded", "crowded_wide", "ramp"]


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


def _up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def cases(api, oracle, inputs, torch_cuda):
    """Per case: the CPU case, the twin's stack and summary, a tracer, the device fields, ne3d and Te (a tensor, or the float)."""
    torch = torch_cuda
    made = {"traced": LC.traced_case(api, oracle, inputs, NCPU), "crowded": LC.crowded_case(api, oracle, inputs, NCPU),
            "crowded_wide": LC.crowded_case(api, oracle, inputs, NCPU, wide=True), "ramp": LC.ramp_case(api)}
    out, tracers = {}, {}
    for name, c in made.items():
        key = name.split("_")[0]
        if key not in tracers:
            tracers[key] = D.tracer(inputs, c["p"], c.get("bn"), tabulate=False)
        twin, ts = api.lpi_map_host(c["fields"], c["ne3d"], c["p"], te=c["te"], band=c["band"], cone_bins=c["nbins"])
        out[name] = dict(c, tr=tracers[key], f=_up(torch, c["fields"]), dne=_up(torch, c["ne3d"]),
                         dte=c["te"] if np.isscalar(c["te"]) else _up(torch, c["te"]), twin=twin, twin_summary=ts)
    yield out
    for tr in tracers.values():
        tr.close()


def _device(c, **kw):
    args = dict(te=c["dte"], band=c["band"], cone_bins=c["nbins"], ne3d=c["dne"])
    args.update(kw)
    fields = args.pop("fields", c["f"])
    return c["tr"].lpi_map(fields, **args)


def _same_summary(got, want, terms_sum, terms_cw):
    for k in LC.COUNTS + LC.MAXIMA:
        assert got[k] == want[k], (k, got[k], want[k])
    for k, terms in (("sum_I_sum", terms_sum), ("sum_I_cw", terms_cw)):
        bound = LC.any_order_bound(terms)
        print("  %s: device %.17g twin %.17g, difference %.3e, bound %.3e" % (k, got[k], want[k], abs(got[k] - want[k]), bound))
        assert abs(got[k] - want[k]) <= bound, k


def _band_terms(c):
    band = c["twin"][BAND] > 0
    return c["twin"][I_SUM][band], c["twin"][I_CW][band]


# ---- 1. device against the host twin ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_device_matches_the_host_twin_bit_for_bit(api, torch_cuda, cases, name):
    torch = torch_cuda
    c = cases[name]
    before = c["f"].clone()
    stack, s = _device(c)
    stack2, s2 = _device(c)
    assert torch.equal(c["f"], before)                                      # the fields are read only
    assert stack.cpu().numpy().tobytes() == stack2.cpu().numpy().tobytes() and s == s2          # two calls: the same bytes
    got = stack.cpu().numpy()
    print("%s: %d band cells of %d, %d lit, max %d beams present" % (name, s["band_cells"], got[0].size, s["lit_cells"], s["max_present"]))
    assert s["band_cells"] == c["ref_summary"]["band_cells"] > 0
    assert got.tobytes() == c["twin"].tobytes()
    _same_summary(s, c["twin_summary"], *_band_terms(c))


@pytest.mark.parametrize("nbins", [1, 8, 16])
def test_cone_bins_one_eight_sixteen(api, torch_cuda, cases, nbins):
    """The three instantiations of k_lpi_map (1, up to 8, up to 16 bin sums per lane), and 5 and 11 bins inside the last two."""
    for name in ("traced", "crowded_wide"):
        c = cases[name]
        for nb in {1: (1,), 8: (8, 5), 16: (16, 11)}[nbins]:
            stack, s = _device(c, cone_bins=nb)
            twin, ts = api.lpi_map_host(c["fields"], c["ne3d"], c["p"], te=c["te"], band=c["band"], cone_bins=nb)
            assert stack.cpu().numpy().tobytes() == twin.tobytes(), (name, nb)
            band = twin[BAND] > 0
            _same_summary(s, ts, twin[I_SUM][band], twin[I_CW][band])
            if nb == 1:
                assert torch_cuda.equal(stack[I_CW], stack[I_SUM])


# ---- 2. slabs, sentinels, views ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["traced", "crowded"])
def test_slab_calls_compose(api, torch_cuda, cases, name):
    torch = torch_cuda
    c = cases[name]
    tr = c["tr"]
    cuts = W.CUTS[name]
    out = torch.full((api.LPI_NQ,) + tr.grid_shape, -7.0, dtype=torch.float64, device="cuda")
    merged = tr.new_lpi_summary()
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        before = out.clone()
        _, same = _device(c, x_lo=lo, x_hi=hi, out=out, summary=merged)
        assert same is merged
        assert torch.equal(out[:, :lo], before[:, :lo]) and torch.equal(out[:, hi:], before[:, hi:])      # other planes untouched
        assert not bool((out[:, lo:hi] == -7.0).any())                                                     # every cell of the slab written
    assert out.cpu().numpy().tobytes() == c["twin"].tobytes()
    _same_summary(api.lpi_summary_from(merged), c["twin_summary"], *_band_terms(c))
    # an empty slab changes nothing; a summary-free call writes the same stack
    _, none = _device(c, x_lo=3, x_hi=3, out=out, summary=False)
    assert none is None and out.cpu().numpy().tobytes() == c["twin"].tobytes()
    bare, none = _device(c, summary=False)
    assert none is None and torch.equal(bare, out)


def test_fields_off_a_128_byte_line(api, torch_cuda, cases):
    torch = torch_cuda
    for name in ("traced", "crowded"):
        c = cases[name]
        n = c["f"].numel()
        for off in (1, 8):
            buf = torch.zeros(n + 16, dtype=torch.float64, device="cuda")
            view = buf[off:off + n].view(c["f"].shape)
            view.copy_(c["f"])
            assert (view.data_ptr() - buf.data_ptr()) == 8 * off and buf.data_ptr() % 128 == 0
            stack, s = _device(c, fields=view)
            assert stack.cpu().numpy().tobytes() == c["twin"].tobytes(), (name, off)
            assert s == _device(c)[1]


# ---- 3. Te from the tables, a caller's ne3d, a float -------------------------------------------------------------------------
def test_te_from_the_tables_and_the_contexts_own_density(api, torch_cuda, cases, inputs):
    torch = torch_cuda
    c = cases["traced"]
    tr = c["tr"]
    with pytest.raises(ValueError, match="tabulate"):
        tr.lpi_map(c["f"], band=c["band"])
    tr.tabulate()
    te = tr.table_te()
    _, r, ne, te_profile = inputs
    want = LC.profile_te(api, c["p"], r, te_profile)
    rel = float(np.abs(te.cpu().numpy() - want).max() / np.abs(want).max())
    worst = float((np.abs(te.cpu().numpy() - want) / want).max())
    print("te from the tables against the interpolated profile: worst relative difference %.3e (of the maximum %.3e)" % (worst, rel))
    assert worst <= 1e-12
    # the default te="tables" with the context's own ne3d is the call with that tensor and that table handed in
    own_ne = torch.from_numpy(tr.node_tables()[0]).cuda()
    a, sa = tr.lpi_map(c["f"], band=c["band"])
    b, sb = tr.lpi_map(c["f"], te=te, band=c["band"], ne3d=own_ne)
    assert torch.equal(a, b) and sa == sb and sa["band_cells"] > 0
    twin, ts = api.lpi_map_host(c["fields"], own_ne.cpu().numpy(), c["p"], te=te.cpu().numpy(), band=c["band"])
    assert a.cpu().numpy().tobytes() == twin.tobytes()
    # a float: the twin's scalar path
    f, sf = _device(c, te=1500.0)
    twin, ts = api.lpi_map_host(c["fields"], c["ne3d"], c["p"], te=1500.0, band=c["band"])
    assert f.cpu().numpy().tobytes() == twin.tobytes() and sf["max_eta_cw"] == ts["max_eta_cw"]
    with pytest.raises(ValueError):
        _device(c, te="profile")
    with pytest.raises(ValueError):                     # out=: a stack of another shape is refused before the launch
        _device(c, te=1500.0, out=f[:-1].contiguous())
    mine = torch.zeros_like(f)
    assert _device(c, te=1500.0, out=mine)[0] is mine and torch.equal(mine, f)
    with pytest.raises(api.CbetError, match="te_ev"):
        _device(c, te=0.0)
    with pytest.raises(api.CbetError, match="band"):
        _device(c, band=(0.3, 0.2))
    with pytest.raises(api.CbetError, match="cone_bins"):
        _device(c, cone_bins=17)


# ---- 4. graph capture ------------------------------------------------------------------------------------------------------
def test_captured_call_replays_the_same_bytes(api, torch_cuda, cases):
    """One stream, no parallel branches: the map and its reduction, behind the copy that re-initialises the summary."""
    torch = torch_cuda
    c = cases["traced"]
    tr = c["tr"]
    eager, es = _device(c)                                                    # (also allocates the tracer's work array)
    init, summ = tr.new_lpi_summary(), tr.new_lpi_summary()
    out = torch.full_like(eager, -3.0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        summ.copy_(init)
        _device(c, out=out, summary=summ)
    out.fill_(-3.0)
    graph.replay()
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == eager.cpu().numpy().tobytes()
    assert api.lpi_summary_from(summ) == es


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------
def test_solve_then_map_then_surface_means(api, torch_cuda, inputs):
    """32^3, six beams: cbet_solve(fields=...) leaves normalised fields; their LPI map; its band means over an 8 x 16
    (theta, phi) one-shell mesh against numpy means of the stack's band cells in those bins."""
    torch = torch_cuda
    from cbet_raytracing_3d_amd import lpi
    bn_all = inputs[0]
    p = api.default_params(32, nbeams=len(W.BEAMS))
    tr = D.tracer(inputs, p, bn_all[W.BEAMS].copy())
    try:
        gp = api.default_gain_params()
        fields = tr.new_fields()
        rep = tr.cbet_solve(tr.new_grid(), gp, fields=fields)
        stack, s = tr.lpi_map(fields)
        got = stack.cpu().numpy()
        print("32^3: %d passes, summary %s" % (rep.get("passes", -1) if isinstance(rep, dict) else -1, lpi.summarize(s)))
        assert np.isfinite(got).all() and s["band_cells"] > 100 and s["lit_cells"] > 0 and s["max_eta_cw"] > 0
        d = api.derive(p)
        R = 2.0 * float(np.sqrt(3.0)) * max(abs(p.xmin), p.xmax, abs(p.ymin), p.ymax, abs(p.zmin), p.zmax)      # the halo included
        theta_edges = np.linspace(0.0, np.pi, 9)
        phi_edges = 0.05 + np.linspace(0.0, 2.0 * np.pi, 17)            # off the diagonals x = +-y, where cells sit
        cells = api.MeshCells([0.0, R], theta_edges, phi_edges, gpu=tr.gpu)
        try:
            means = lpi.surface_means(tr, stack, cells)
        finally:
            cells.close()
        count = means["cells"].cpu().numpy()
        assert count.shape == (8, 16) and float(count.sum()) == s["band_cells"]
        # numpy: every haloed cell at ((N - 1) d + min), its (theta, phi) bin, the band cells' means per bin
        ax = [(np.arange(n + 2) - 1) * dd + mn for n, dd, mn in ((p.nx, d.dx, p.xmin), (p.ny, d.dy, p.ymin), (p.nz, d.dz, p.zmin))]
        x, y, z = np.meshgrid(*ax, indexing="ij")
        rho = np.sqrt(x * x + y * y + z * z)
        th = np.arccos(np.clip(z / np.where(rho > 0, rho, 1.0), -1.0, 1.0))
        ph = np.mod(np.arctan2(y, x) - 0.05, 2.0 * np.pi)
        it = np.minimum((th / (np.pi / 8)).astype(int), 7)
        ip = np.minimum((ph / (2.0 * np.pi / 16)).astype(int), 15)
        band = got[BAND] > 0
        want_count = np.zeros((8, 16))
        np.add.at(want_count, (it[band], ip[band]), 1.0)
        assert np.array_equal(count, want_count)
        for q, name in enumerate(api.LPI_QUANTITIES):
            if q == api.LPI_BAND:
                continue
            tot = np.zeros((8, 16))
            np.add.at(tot, (it[band], ip[band]), got[q][band])
            have = means[name].cpu().numpy()
            filled = want_count > 0
            assert np.isnan(have[~filled]).all() and np.isfinite(have[filled]).all()
            want = tot[filled] / want_count[filled]
            assert (np.abs(have[filled] - want) <= 1e-12 * np.abs(want)).all(), name
    finally:
        tr.close()
