"""The pairwise exchange matrix on the device (cbet_grid_kernels.hip k_exchange_matrix + k_exchange_reduce; DESIGN.md section
18) against its host twin cbet_exchange_matrix_host, on the two grids of helpers/gain_worlds.py and three small shapes.

  TRACED  48 x 21 x 134, six beams, the oracle's traced fields.
  CROWDED 13 x 11 x 148, sixty beams, 9-54 beams per cell: runs staged whole (up to 32 present beams) and in halves.

The fields are normalised on the device by one gain_field call (pair-once, relax 1); the twin reads exactly those.  Bounds:
1e-9 of Gross_ij for the pair-once arithmetic against the ordered statements of the twin (the project's bound for that pair),
1e-12 of Gross_ij for slab calls summed against the whole (the same arithmetic, grouped differently); what must be exact is
asserted bitwise.  The limits are quantiles of a CPU reference's own pair amplitudes (saturation_cases.limits_from)."""
import numpy as np
import pytest

from conftest import NCPU
from helpers import exchange_cases as XC
from helpers import gain_calls as D
from helpers import gain_worlds as W
from helpers.gain_worlds import TOL        # here: device (pair-once arithmetic) against the host twin (ordered statements), of Gross_ij

pytestmark = pytest.mark.gpu

SLAB_BITS = 1e-12          # slab calls summed against the whole grid's call, of Gross_ij
WHICH = {"traced": "restated", "crowded": "plain"}


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


def _normalise(torch, tr, raw, gp, ne3d=None):
    """Device fields normalised by one pair-once gain update from a zero gain: (fields, gain)."""
    f, k = raw.clone(), tr.new_grid(per_beam=True)
    tr.gain_field(f, k, gp, None, ne3d=ne3d, pair_once=True)
    return f, k


@pytest.fixture(scope="module")
def worlds(api, oracle, inputs, torch_cuda):
    """Per grid: the CPU world, a tracer, the device tables, the device fields normalised once and their host copy."""
    torch = torch_cuda
    out = {}
    for name, world in (("traced", W.traced_world(api, oracle, inputs, NCPU)), ("crowded", W.crowded_world(api, oracle, inputs, NCPU))):
        tr = D.tracer(inputs, world["p"], world["bn"])
        dev = {k: _up(torch, world[k]) for k in ("raw", "flow", "state", "ne3d")}
        f, k = _normalise(torch, tr, dev["raw"], world["gp"], dev["ne3d"])
        torch.cuda.synchronize()
        out[name] = dict(world, name=name, tr=tr, dev=dev, f=f, k=k, hf=f.cpu().numpy())
    yield out
    for w in out.values():
        w["tr"].close()


def _tables(w, which):
    """(device flow, device state, host flow, host state) of a table set-up: "none"; "flow" the sphere's own table handed in
    as a caller's; "three" that flow plus the three-state pattern (kz = 1)."""
    if which == "none":
        return None, None, None, None
    if which == "flow":
        return w["dev"]["flow"], None, w["flow"], None
    return w["dev"]["flow"], w["dev"]["state"], w["flow"], w["state"]


def _limit(w, name):
    return 0.0 if name == "none" else XC.limits_of(w, WHICH[w["name"]])[name]


def _device(w, gross=True, **kw):
    return w["tr"].exchange_matrix(w["f"], w["gp"], ne3d=w["dev"]["ne3d"], gross=gross, **kw)


def _worst(got, want, gross):
    return XC.worst(got.cpu().numpy() if hasattr(got, "cpu") else got, want, gross)


# ---- 1. device against the host twin ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tables", ["none", "flow", "three"])
@pytest.mark.parametrize("grid", ["traced", "crowded"])
def test_device_matches_the_host_twin(api, torch_cuda, worlds, grid, tables):
    """Tables none / a caller's flow / flow + three-state table, each without a limit and with `half` and `all` clamped."""
    w = worlds[grid]
    tr = w["tr"]
    dflow, dstate, hflow, hstate = _tables(w, tables)
    tr.set_flow(dflow)
    tr.set_gain_state(dstate)
    try:
        for name in ("none", "half", "all"):
            dn = _limit(w, name)
            tr.set_saturation(dn)
            T, G = _device(w)
            want, gross = api.exchange_matrix_host(w["hf"], w["ne3d"], w["p"], w["gp"], flow=hflow, state=hstate, dn_max=dn)
            err, gerr = _worst(T, want, gross), _worst(G, gross, gross)
            print("%s tables %s limit %s (dn_max %.4e): device vs host twin %.3e of Gross (Gross itself %.3e); max Gross %.3e"
                  % (grid, tables, name, dn, err, gerr, gross.max()))
            assert gross.max() > 0
            assert err < TOL and gerr < TOL
    finally:
        tr.set_saturation(0.0)
        tr.set_flow(None)
        tr.set_gain_state(None)


# ---- 2. exact properties ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["traced", "crowded"])
def test_exact_properties_on_the_device(api, torch_cuda, worlds, grid):
    torch = torch_cuda
    w = worlds[grid]
    tr, f = w["tr"], w["f"]
    before = f.clone()
    T, G = _device(w)
    T2, G2 = _device(w)
    torch.cuda.synchronize()
    assert torch.equal(f, before)                                           # the fields are read only
    assert torch.equal(T, T2) and torch.equal(G, G2)                        # two calls: the same bits
    assert torch.equal(T, -T.t()) and not bool(T.diagonal().any())
    assert torch.equal(G, G.t()) and not bool(G.diagonal().any())
    assert bool((G >= T.abs()).all()) and float(G.max()) > 0
    alone = tr.exchange_matrix(f, w["gp"], ne3d=w["dev"]["ne3d"])           # without gross: the tensor alone, the same bits
    assert torch.is_tensor(alone) and torch.equal(alone, T)
    # out= and gross= as tensors are ADDED into and handed back; any other shape or dtype is refused before the launch
    mine, mine_g = torch.zeros_like(T), torch.zeros_like(G)
    got = tr.exchange_matrix(f, w["gp"], ne3d=w["dev"]["ne3d"], out=mine, gross=mine_g)
    assert got[0] is mine and got[1] is mine_g and torch.equal(mine.triu(), T.triu()) and torch.equal(mine_g.triu(), G.triu())
    for bad in (dict(out=T[:-1].contiguous()), dict(gross=G[:, :-1].contiguous()), dict(out=T.float()), dict(gross=G.t()[:, :-1])):
        with pytest.raises(ValueError):
            tr.exchange_matrix(f, w["gp"], ne3d=w["dev"]["ne3d"], **bad)
    # a view of the fields that starts 1 and 8 doubles off a 128-byte line: the aligned call's bits
    buf = torch.empty(f.numel() + 16, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 128 == 0 and f.data_ptr() % 128 == 0
    for off in (1, 8):
        view = buf[off:off + f.numel()].view(f.shape)
        view.copy_(f)
        assert view.data_ptr() % 128 == 8 * off
        Tv, Gv = tr.exchange_matrix(view, w["gp"], ne3d=w["dev"]["ne3d"], gross=True)
        assert torch.equal(Tv, T) and torch.equal(Gv, G), off
    # a pair that is never co-present gives an exact zero
    a, b = (1, 4) if grid == "traced" else (7, 41)
    assert float(G[a, b]) > 0
    cut = 20 if grid == "traced" else 7
    apart = _up(torch, XC.never_together(w["hf"], a, b, cut))
    Ta, Ga = tr.exchange_matrix(apart, w["gp"], ne3d=w["dev"]["ne3d"], gross=True)
    assert float(Ta[a, b]) == 0.0 and float(Ta[b, a]) == 0.0 and float(Ga[a, b]) == 0.0 and float(Ga[b, a]) == 0.0
    assert int((Ga > 0).sum()) == int((G > 0).sum()) - 2


# ---- 3. the row-sum identity ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["traced", "crowded"])
def test_rows_sum_to_what_the_gain_update_hands_each_beam(api, torch_cuda, worlds, grid):
    """T.sum(1) against sum over cells of ds I K, K the pair-once gain_field's from a zero gain with relax 1, everything read
    from the context's own node table (ne3d = None)."""
    torch = torch_cuda
    w = worlds[grid]
    tr = w["tr"]
    f, k = _normalise(torch, tr, w["dev"]["raw"], w["gp"])
    T, G = tr.exchange_matrix(f, w["gp"], gross=True)
    ds = _up(torch, w[WHICH[grid]].ds.reshape(tr.grid_shape))
    want = (ds[None] * f[0] * k).sum(dim=(1, 2, 3))
    err = float(((T.sum(dim=1) - want).abs() / G.sum(dim=1)).max())
    print("%s: device row sums vs sum ds I K of the pair-once gain update %.3e of sum_j Gross_ij" % (grid, err))
    assert float(G.sum()) > 0 and err < TOL


# ---- 4. slabs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["traced", "crowded"])
def test_slab_calls_add_up_to_the_whole(api, torch_cuda, worlds, grid):
    torch = torch_cuda
    w = worlds[grid]
    tr = w["tr"]
    nb, hx = w["p"].nbeams, tr.grid_shape[0]
    T, G = _device(w)
    out = torch.zeros((nb, nb), dtype=torch.float64, device="cuda")
    gross = torch.zeros_like(out)
    cuts = [(lo, min(hi, hx)) for lo, hi in XC.SLABS + [(22, hx)] if lo < hx]
    for lo, hi in cuts:
        o, g = _device(w, gross=gross, out=out, x_lo=lo, x_hi=hi)
        assert o is out and g is gross
    Gh = G.cpu().numpy()
    err, gerr = _worst(out, T.cpu().numpy(), Gh), _worst(gross, Gh, Gh)
    print("%s: device slabs %s summed vs the whole %.3e of Gross (Gross itself %.3e)" % (grid, cuts, err, gerr))
    assert err < SLAB_BITS and gerr < SLAB_BITS
    assert torch.equal(out, -out.t()) and torch.equal(gross, gross.t()) and not bool(out.diagonal().any())
    before, gbefore = out.clone(), gross.clone()
    _device(w, gross=gross, out=out, x_lo=5, x_hi=5)                         # an empty slab changes nothing
    assert torch.equal(out, before) and torch.equal(gross, gbefore)
    part, pg = _device(w, x_lo=cuts[1][0], x_hi=cuts[1][1])                  # one slab against the twin on its planes
    want, wg = api.exchange_matrix_host(w["hf"], w["ne3d"], w["p"], w["gp"], hx_lo=cuts[1][0], hx_hi=cuts[1][1])
    assert _worst(part, want, wg) < TOL and _worst(pg, wg, wg) < TOL


# ---- 5. dn_max is honoured --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["traced", "crowded"])
def test_the_limit_is_honoured_and_taken_back(api, torch_cuda, worlds, grid):
    torch = torch_cuda
    w = worlds[grid]
    tr = w["tr"]
    free, gfree = _device(w)
    try:
        tr.set_saturation(_limit(w, "all"))
        T, G = _device(w)
        live = gfree > 0
        assert int(live.sum()) > 0 and bool((T.abs()[live] < free.abs()[live]).all())
        assert bool((G[live] < gfree[live]).all())
        tr.set_saturation(XC.limits_of(w, WHICH[grid])["never"])              # never reached: the bits of no limit
        never, gnever = _device(w)
        assert torch.equal(never, free) and torch.equal(gnever, gfree)
    finally:
        tr.set_saturation(0.0)
    back, gback = _device(w)
    assert torch.equal(back, free) and torch.equal(gback, gfree)


# ---- 6. small shapes --------------------------------------------------------------------------------------------------------
def _small(api, oracle, inputs, torch, shape, nb, raw):
    """Device and twin on a small grid with synthetic raw fields: (T, G, want, gross) as numpy, and the tracer's work size."""
    bn_all, r, ne, te = inputs
    bn = np.concatenate([bn_all, bn_all])[:nb]
    cfg = oracle.default_config(shape[0], nbeams=nb, ny=shape[1], nz=shape[2])
    ne3d, _ = oracle.node_tables(cfg, r, ne, te)
    p, gp = W.params(api, shape, nb), api.default_gain_params(relax=1.0)
    tr = D.tracer(inputs, p, bn)
    try:
        dne = _up(torch, ne3d)
        f, _ = _normalise(torch, tr, _up(torch, raw), gp, dne)
        before = f.clone()
        T, G = tr.exchange_matrix(f, gp, ne3d=dne, gross=True)
        torch.cuda.synchronize()
        assert torch.equal(f, before)
        want, gross = api.exchange_matrix_host(f.cpu().numpy(), ne3d, p, gp)
        return T.cpu().numpy(), G.cpu().numpy(), want, gross
    finally:
        tr.close()


def test_two_beams_and_one_beam_on_rows_shorter_than_a_run(api, oracle, inputs, torch_cuda):
    shape = (6, 9, 13)                                                       # rows of 15 cells: every run is a partial one
    raw = XC.dense_fields(2, tuple(n + 2 for n in shape), 7)
    T, G, want, gross = _small(api, oracle, inputs, torch_cuda, shape, 2, raw)
    print("6 x 9 x 13, two beams: T01 %.6e (twin %.6e), Gross %.6e" % (T[0, 1], want[0, 1], gross[0, 1]))
    assert gross[0, 1] > 0 and XC.worst(T, want, gross) < TOL and XC.worst(G, gross, gross) < TOL
    assert T[1, 0] == -T[0, 1] and T[0, 0] == 0.0 and T[1, 1] == 0.0
    T1, G1, want1, gross1 = _small(api, oracle, inputs, torch_cuda, shape, 1, raw[:, :1])
    assert T1.shape == (1, 1) and T1[0, 0] == 0.0 and G1[0, 0] == 0.0 and want1[0, 0] == 0.0 and gross1[0, 0] == 0.0


def test_sixty_four_beams_reach_the_last_triangular_index(api, oracle, inputs, torch_cuda):
    shape = (5, 4, 37)
    raw, _ = W.crowded_fields((64,) + tuple(n + 2 for n in shape))
    T, G, want, gross = _small(api, oracle, inputs, torch_cuda, shape, 64, raw)
    err, gerr = XC.worst(T, want, gross), XC.worst(G, gross, gross)
    print("5 x 4 x 37, 64 beams: device vs host twin %.3e of Gross (Gross itself %.3e); %d of 2016 pairs exchange; T[62][63] %.6e"
          % (err, gerr, (gross > 0).sum() // 2, T[62, 63]))
    assert gross[62, 63] > 0 and gross[0, 63] > 0 and (gross > 0).sum() // 2 > 1900
    assert err < TOL and gerr < TOL
    assert np.array_equal(T, -T.T) and np.array_equal(G, G.T)
