"""Wavelength detuning in the gain stage on the device (cbet_grid_kernels.hip: the DETUNE arms of k_gain_field,
k_gain_field_sym, k_pair_amplitude and k_exchange_matrix) against the numpy restatement of
helpers/gain_reference.py with the shifts of helpers/detuning_cases.py and the shifted host twin, on the two grids of
helpers/gain_worlds.py:

  TRACED  48 x 21 x 134, six beams, the oracle's traced fields.
  CROWDED 13 x 11 x 148, sixty beams, synthetic fields: 9-54 beams per cell, so a run's slots are not its beam numbers.

Sixty DISTINCT shifts (detuning_cases.shifts).  The bounds are the project's: bit for bit where both sides run the same IEEE
statements, 1e-12 of max |K| for the pair-once kernel against the ordered one, 1e-9 of max |K| against a CPU reference,
1e-9 of Gross_ij for the exchange matrix against the twin, 1e-12 of its maximum for the amplitude map.  max |K| is the
shifted reference's own unless a test says otherwise.

The slab of the slab-wise and packed cases is [9, 22) on TRACED; CROWDED has 15 planes, there it is [9, 14), as in
tests/test_gpu_saturation.py."""
import numpy as np
import pytest

from conftest import NCPU
from helpers import detuning_cases as DC
from helpers import exchange_cases as XC
from helpers import gain_calls as D
from helpers import gain_worlds as W
from helpers import saturation_cases as SC
from helpers.gain_reference import halo
from helpers.gain_worlds import CUTS, LAST_BITS, SLABS, TOL       # LAST_BITS also bounds the amplitude map, of its maximum

pytestmark = pytest.mark.gpu

KERNELS = [False, True]
KERNEL_IDS = ["ordered", "pair_once"]


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
def worlds(api, oracle, inputs, torch_cuda):
    """Per grid: the CPU world, a tracer that gets shifts (`tr`), one that never has any (`base`), the device fields."""
    out = D.device_worlds(api, oracle, inputs, torch_cuda, NCPU)
    yield out
    D.close_worlds(out)


def _clear(tr):
    tr.set_detuning()
    tr.set_saturation(0.0)
    D.select(tr)


# ---- 1. off is off --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair_once", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("grid", ["crowded", "traced"])
def test_off_is_off(api, torch_cuda, worlds, grid, pair_once):
    """set_detuning with None, with zeros and with equal values selects no shifts: no bit of either kernel's K or fields
    changes against a tracer that never had any -- whole grid, frozen call, slab, packed slab.  Then the DETUNE arm itself
    with equal non-zero values: the shifts differ only in the last beam, which is taken out of the fields, so every pair
    that is evaluated has dw = 0 exactly."""
    torch = torch_cuda
    w = worlds[grid]
    tr, base, gp, raw, slab = w["tr"], w["base"], w["gp"], w["dev"]["raw"], SLABS[grid]
    nb = w["p"].nbeams

    def calls(tracer, fields):
        """First call, frozen call on fresh energy, slab, packed slab, frozen call on the packed slab: [(what, tensor)]."""
        return D.all_calls(torch, api, tracer, fields, gp, pair_once, slab, change=False, packed_frozen=True)

    try:
        assert base.detuning() is None and tr.detuning() is None                # a new context has none
        want = calls(base, raw)
        assert float(want[1][1].abs().max()) > 1.0 and float(want[5][1].abs().max()) > 1.0
        for mode, kw in (("none", dict()), ("zeros", dict(domega=np.zeros(nb))), ("equal", dict(domega=np.full(nb, 3.3e12))),
                         ("equal wavelengths", dict(dlambda_angstrom=np.full(nb, -2.0)))):
            tr.set_detuning(**kw)
            assert tr.detuning() is None, mode
            got = calls(tr, raw)
            for (what, a), (_, b) in zip(want, got):
                assert torch.equal(a, b), (mode, what)
        last = nb - 1
        without = raw.clone()
        without[:, last] = 0.0
        want = calls(base, without)
        assert float(want[1][1].abs().max()) > 1.0
        arm = np.full(nb, 3.3e12)
        arm[last] = 0.0
        tr.set_detuning(domega=arm)
        assert np.array_equal(tr.detuning(), arm)                                # shifts are selected: the DETUNE instantiations run
        got = calls(tr, without)
        for (what, a), (_, b) in zip(want, got):
            assert torch.equal(a, b), ("the DETUNE arm with equal shifts", what)
    finally:
        _clear(tr)


# ---- 2. against the restatement, 3. storage -------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", ["none", "half"])
@pytest.mark.parametrize("tables", DC.TABLES)
@pytest.mark.parametrize("grid", ["traced", "crowded"])
def test_detuned_update_matches_the_restatement(api, torch_cuda, worlds, grid, tables, limit):
    """Both kernels with sixty distinct shifts (six on TRACED), in every table set-up of tests/test_gpu_saturation.py -- every
    FLOW x STATE combination of the kernels' instantiations --, with and without the limit `half` of the shifted reference:
    first call and frozen call on the whole grid, slab-wise updates, the packed slab."""
    torch = torch_cuda
    w = worlds[grid]
    tr, gp, raw, slab = w["tr"], w["gp"], w["dev"]["raw"], SLABS[grid]
    ref = DC.reference(w, tables)
    want = ref["K"] if limit == "none" else ref["Khalf"]
    scale = float(np.abs(ref["K"]).max())
    D.select(tr, *D.tables(api, torch, w, tables))
    tr.set_detuning(domega=ref["shift"])
    tr.set_saturation(0.0 if limit == "none" else ref["half"])
    try:
        assert np.array_equal(tr.detuning(), ref["shift"])
        got = {}
        for pair_once in KERNELS:
            f, k, ch, _, k2, _ = D.first_and_frozen(torch, tr, raw, gp, pair_once)
            parts, fields = tr.new_grid(per_beam=True), raw.clone()
            for x0, x1 in zip(CUTS[grid][:-1], CUTS[grid][1:]):
                tr.gain_field(fields, parts, gp, None, pair_once=pair_once, x_lo=x0, x_hi=x1)
            _, kp, _ = D.packed(torch, api, tr, raw, gp, pair_once, slab, change=False)
            got[pair_once] = dict(first=k.cpu().numpy(), frozen=k2.cpu().numpy(), slabs=parts.cpu().numpy(), packed=kp.cpu().numpy(),
                                  change=ch.cpu().numpy(), fields=torch.equal(fields, f), nf=f.cpu().numpy())
    finally:
        _clear(tr)
    x0, x1 = slab
    for pair_once in KERNELS:
        g = got[pair_once]
        label = "%s %s %s %s" % (grid, tables, limit, "pair-once" if pair_once else "ordered")
        errs = {k: float(np.abs(g[k] - want).max() / scale) for k in ("first", "frozen", "slabs")}
        errs["packed"] = float(np.abs(g["packed"] - want[:, x0:x1]).max() / scale)
        moved = float(np.abs(g["first"] - ref["K0"]).max() / np.abs(ref["K0"]).max())
        print("%s (max |K| %.3e): against the restatement %s; moved from the unshifted K by %.3e of its max"
              % (label, scale, {k: "%.2e" % v for k, v in errs.items()}, moved))
        assert all(e < TOL for e in errs.values()), (label, errs)
        assert moved > DC.MOVES
        assert g["fields"]                                                   # the normalisation does not see the shifts
        assert abs(g["change"][1] / np.abs(want).sum() - 1.0) < TOL
        inten = np.where(g["nf"][0] > 0, g["nf"][0], 0.0)                    # the exchange still cancels per cell
        exch, bound = np.abs((inten * g["first"]).sum(axis=0)).max(), np.abs(inten * g["first"]).sum(axis=0).max()
        assert bound > 0 and exch <= 1e-11 * bound
        # 3. storage: slab-wise updates are the whole update bit for bit; the packed slab is, for the ordered kernel (the
        # same statements per cell), and agrees to the last bits for the pair-once kernel (its runs follow the storage)
        assert np.array_equal(g["slabs"], g["first"]), label
        if pair_once:
            assert float(np.abs(g["packed"] - g["first"][:, x0:x1]).max() / scale) < LAST_BITS
        else:
            assert np.array_equal(g["packed"], g["first"][:, x0:x1])
    for k in ("first", "frozen", "slabs", "packed"):
        err = float(np.abs(got[True][k] - got[False][k]).max() / scale)
        print("%s %s %s %s: pair-once against ordered %.3e" % (grid, tables, limit, k, err))
        assert err < LAST_BITS, (k, err)


# ---- 4. physics in still plasma, 5. parallel beams ------------------------------------------------------------------------
def _two_beams(api, inputs, torch, parallel):
    """Two synthetic beams on a 12 x 10 x 37 grid (rows of 39 cells: three runs, the last of 7), crossing at a right angle or
    exactly parallel, present in most cells, absent (zero) or touched-only (negative energy) in some."""
    p = W.params(api, (12, 10, 37), 2)
    tr = D.tracer(inputs, p, inputs[0][[0, 29]])
    shape = (2,) + tr.grid_shape
    rng = np.random.default_rng(19)
    u = rng.random(shape)
    e = (rng.random(shape) * 1e3 + 1.0) * 1e11
    raw = np.zeros((4,) + shape)
    raw[0] = np.where(u < 0.8, e, np.where(u < 0.9, -e, 0.0))
    d = np.array([[1.0, 0.25, 0.5], [1.0, 0.25, 0.5]] if parallel else [[1.0, 0.25, 0.5], [-0.5, 0.0, 1.0]])
    raw[1:] = d.T.reshape(3, 2, 1, 1, 1) * (raw[0] != 0)
    return tr, torch.from_numpy(raw).cuda()


def test_red_shifted_beam_gains_in_still_plasma(api, inputs, torch_cuda):
    torch = torch_cuda
    tr, raw = _two_beams(api, inputs, torch, parallel=False)
    gp = api.default_gain_params(relax=1.0)
    p = tr.params
    try:
        tr.set_flow(torch.zeros((3, p.nx, p.ny, p.nz), dtype=torch.float64, device="cuda"))   # a caller's zero flow table
        shift = api.wavelength_shift_to_domega(p, np.array([3.0, -3.0]))     # beam 0 red, beam 1 blue
        assert shift[0] < 0 < shift[1]
        ne3d = torch.zeros((p.nx, p.ny, p.nz), dtype=torch.float64, device="cuda")
        api.moveToAndFromGPU(ne3d, tr.ctx.tables()[0], ne3d.numel() * 8, tr.gpu)
        sub = halo(ne3d.cpu().numpy()) < api.derive(p).ncrit
        assert sub.any()
        for pair_once in KERNELS:
            _, k0, _ = D.update(torch, tr, raw, gp, pair_once, change=False)
            assert not bool(k0.any())                                        # one colour, no flow: K == 0 exactly
            tr.set_detuning(domega=shift)
            f, k, _ = D.update(torch, tr, raw, gp, pair_once, change=False)
            tr.set_detuning(domega=shift[::-1].copy())
            _, ks, _ = D.update(torch, tr, raw, gp, pair_once, change=False)
            tr.set_detuning()
            nf, K, Ks = f.cpu().numpy(), k.cpu().numpy(), ks.cpu().numpy()
            both = (nf[0, 0] > 0) & (nf[0, 1] > 0) & sub
            assert both.sum() > 1000 and (~both).sum() > 100
            assert (K[0][both] > 0).all() and (K[1][both] < 0).all()         # the red beam gains, the blue one loses
            assert not K[0][~both].any() and not K[1][~both].any()
            cancel = np.abs(nf[0, 0] * K[0] + nf[0, 1] * K[1])[both] / (np.abs(nf[0, 0] * K[0]) + np.abs(nf[0, 1] * K[1]))[both]
            print("still plasma, %s: I_i K_i + I_j K_j up to %.3e of its terms; max |K| %.3e" %
                  ("pair-once" if pair_once else "ordered", cancel.max(), np.abs(K).max()))
            assert cancel.max() <= 4 * 2.0 ** -53
            if pair_once:
                assert np.abs(Ks + K).max() <= LAST_BITS * np.abs(K).max()
            else:
                assert np.array_equal(Ks, -K)                                # swapped shifts negate the ordered kernel's K bit for bit
    finally:
        tr.close()


def test_parallel_beams_of_different_colour_exchange_nothing(api, inputs, torch_cuda):
    """q = 0 exactly in every cell: the ordered kernel does not evaluate the pair, and the pair-once kernels count the beat
    frequency only where q != 0 (the leak is guarded, not bounded): exact zeros from all four kernels."""
    torch = torch_cuda
    tr, raw = _two_beams(api, inputs, torch, parallel=True)
    gp = api.default_gain_params(relax=1.0)
    try:
        for shift in (DC.shifts(2), np.array([1e-10, -1e-10]), np.array([0.0, 5e-11])):   # the scale of the tests, and of D at q = 0
            tr.set_detuning(domega=shift)
            for pair_once in KERNELS:
                f, k, _ = D.update(torch, tr, raw, gp, pair_once, change=False)
                assert not bool(k.any()), (pair_once, shift)
            assert bool((f[0] > 0).any())
            T, G = tr.exchange_matrix(f, gp, gross=True)
            assert not bool(T.any()) and not bool(G.any())
            assert not bool(tr.pair_amplitude(f, gp).any())
    finally:
        tr.close()


# ---- 6. far off resonance -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [DC.NEAR_FAR, DC.FAR], ids=["100x", "1000x"])
@pytest.mark.parametrize("grid", ["traced", "crowded"])
def test_far_off_resonance(api, torch_cuda, worlds, grid, scale):
    """Shifts of 100 x and 1000 x the scale of the other tests (helpers/detuning_cases.py on why both): the kernels agree with
    the reference within test 2's bounds of the UNSHIFTED max |K|; at 1000 x the reference has no gain left."""
    torch = torch_cuda
    w = worlds[grid]
    tr, gp, raw = w["tr"], w["gp"], w["dev"]["raw"]
    ref = DC.reference(w, False, scale)
    k0 = float(np.abs(ref["K0"]).max())
    share = float(np.abs(ref["K"]).max()) / k0
    if scale == DC.FAR:
        assert share < DC.FAR_SHARE
    tr.set_detuning(domega=ref["shift"])
    try:
        got = [D.update(torch, tr, raw, gp, pair_once, change=False)[1].cpu().numpy() for pair_once in KERNELS]
    finally:
        _clear(tr)
    errs = [float(np.abs(g - ref["K"]).max() / k0) for g in got]
    between = float(np.abs(got[1] - got[0]).max() / k0)
    print("%s, shifts of %.1e rad/s: the reference keeps %.3e of the unshifted max |K|; ordered / pair-once against it %.3e / %.3e,"
          " against each other %.3e (all of the unshifted max |K|)" % (grid, scale, share, errs[0], errs[1], between))
    assert all(e < TOL for e in errs) and between < LAST_BITS
    assert all(np.isfinite(g).all() for g in got)


# ---- 7. exchange matrix and amplitude map ---------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", ["none", "half"])
@pytest.mark.parametrize("tables", ["none", "tabled"])
@pytest.mark.parametrize("grid", ["traced", "crowded"])
def test_exchange_matrix_and_amplitude_map_with_shifts(api, torch_cuda, worlds, grid, tables, limit):
    torch = torch_cuda
    w = worlds[grid]
    tr, gp, raw = w["tr"], w["gp"], w["dev"]["raw"]
    tabled = tables == "tabled"
    ref = DC.reference(w, tabled)
    dn = 0.0 if limit == "none" else ref["half"]
    D.select(tr, *D.tables(api, torch, w, tables))
    tr.set_detuning(domega=ref["shift"])
    tr.set_saturation(dn)
    try:
        f, k, _ = D.update(torch, tr, raw, gp, True, change=False)
        T, G = tr.exchange_matrix(f, gp, gross=True)
        T2, G2 = tr.exchange_matrix(f, gp, gross=True)
        amp = tr.pair_amplitude(f, gp)
        torch.cuda.synchronize()
    finally:
        _clear(tr)
    assert torch.equal(T, T2) and torch.equal(G, G2)                         # two calls give the same bits
    nf, T, G, K = f.cpu().numpy(), T.cpu().numpy(), G.cpu().numpy(), k.cpu().numpy()
    host, hgross = api.exchange_matrix_host(nf, w["ne3d"], w["p"], gp, flow=w["shifted"] if tabled else None,
                                            state=w["state"] if tabled else None, dn_max=dn, shift=ref["shift"])
    want, gross = (ref["T"], ref["G"]) if limit == "none" else (ref["Thalf"], ref["Ghalf"])
    err, gerr = XC.worst(T, host, hgross), XC.worst(G, hgross, hgross)
    rerr = XC.worst(T, want, gross)
    ds = w[DC.restatement_key(w, tabled)].ds.reshape(nf.shape[2:])
    inten = np.where(nf[0] > 0, nf[0], 0.0)
    rows = (ds[None] * inten * K).reshape(K.shape[0], -1).sum(axis=1)        # sum ds I_i K_i of the gain update
    row_err = float((np.abs(T.sum(axis=1) - rows) / G.sum(axis=1)).max())
    a, top = amp.cpu().numpy(), float(ref["amp"].max())
    aerr = float(np.abs(a - ref["amp"]).max() / top)
    print("%s %s %s: T against the shifted twin %.3e of Gross (Gross %.3e), against the restatement %.3e; rows against sum ds I K %.3e;"
          " amplitude map against the restatement %.3e of its maximum %.4e" % (grid, tables, limit, err, gerr, rerr, row_err, aerr, top))
    assert err < TOL and gerr < TOL and rerr < TOL
    assert np.array_equal(T, -T.T) and np.array_equal(G, G.T)
    assert row_err < TOL
    assert top > 0 and aerr < LAST_BITS                                      # the amplitude is the detuned |G_ij|'s, unclamped
    plain = SC.reference(w, DC.restatement_key(w, tabled))["amp"]
    assert float(np.abs(ref["amp"] - plain).max() / top) > 1e-2              # ... and not the unshifted one


# ---- 8. the context -------------------------------------------------------------------------------------------------------
def test_context_refuses_names_and_remembers(api, torch_cuda, worlds):
    torch = torch_cuda
    w = worlds["crowded"]
    tr, gp, raw = w["tr"], w["gp"], w["dev"]["raw"]
    first, second = DC.shifts(60), DC.shifts(60)[::-1].copy()
    try:
        assert tr.detuning() is None
        tr.set_detuning(domega=first)
        assert np.array_equal(tr.detuning(), first) and np.array_equal(tr.ctx.detuning(), first)
        for bad, word in ((np.where(np.arange(60) == 7, np.nan, first), "NaN"), (np.where(np.arange(60) == 7, np.inf, first), "infinite"),
                          (first[:59], "nbeams = 59"), (np.zeros(65), "nbeams = 65"), (np.zeros(61), "nbeams = 61")):
            with pytest.raises(api.CbetError) as ei:
                tr.set_detuning(domega=bad)
            assert ei.value.code == api.EINVAL and word in str(ei.value) and "cbet_context_set_detuning" in str(ei.value)
            assert np.array_equal(tr.detuning(), first)                      # a refused call changes nothing
        with pytest.raises(ValueError):
            tr.set_detuning(dlambda_angstrom=np.zeros(60), domega=first)
        _, k1, _ = D.update(torch, tr, raw, gp, True, change=False)
        tr.set_detuning(domega=second)                                       # replaces the first for launches made after it
        assert np.array_equal(tr.detuning(), second)
        _, k2, _ = D.update(torch, tr, raw, gp, True, change=False)
        _, k1_again, _ = D.update(torch, w["base"], raw, gp, True, change=False)
        ref = DC.reference(w, False)
        scale = float(np.abs(ref["K"]).max())
        assert float(np.abs(k1.cpu().numpy() - ref["K"]).max()) < TOL * scale
        want2 = w["plain"].update(w["raw"], second)["K"][0]
        assert float(np.abs(k2.cpu().numpy() - want2).max()) < TOL * float(np.abs(want2).max())
        assert float((k2 - k1).abs().max()) > DC.MOVES * scale
        assert float(np.abs(k1_again.cpu().numpy() - ref["K0"]).max()) < TOL * float(np.abs(ref["K0"]).max())   # another context is untouched
        three = DC.three_colours(60)
        tr.set_detuning(dlambda_angstrom=three)
        assert np.array_equal(tr.detuning(), api.wavelength_shift_to_domega(tr.params, three))
        other = api.Context(tr.params, tr.gpu)                               # a context prepared for the tracer carries its shifts
        assert other.detuning() is None
        tr._prepare_plasma(tr.params, other)
        assert np.array_equal(other.detuning(), tr.detuning())
        tr.set_detuning()
        tr._prepare_plasma(tr.params, other)
        assert other.detuning() is None and tr.detuning() is None
        tr.ctx.set_detuning(first)                                           # the caller's own call on the tracer's context is kept
        tr._prepare_plasma(tr.params, tr.ctx)
        tr._prepare_plasma(tr.params, other)
        assert np.array_equal(tr.detuning(), first) and np.array_equal(other.detuning(), first)
        other.close()
    finally:
        _clear(tr)


def test_solve_loops_run_with_shifts(api, inputs, torch_cuda):
    """tests/test_gpu_cbet.py's solve (32^3, six beams, relax 1, 12 passes) with the three-colour scheme: the Python loop, the
    slab loop at one rank and the native loop with the tracer's context all see the shifts -- each differs from its own
    unshifted result, the three agree with one another as closely as without shifts (x 10) -- and the exchange matrix of the
    solve's fields afterwards differs from the unshifted solve's."""
    from conftest import parity_err
    torch = torch_cuda
    tr = D.tracer(inputs, api.default_params(32, nbeams=len(W.BEAMS)), inputs[0][W.BEAMS])
    gp = api.default_gain_params(tolerance=1e-6, max_passes=12, relax=1.0)

    def solves():
        out = {}
        fields = tr.new_fields()
        e = tr.new_grid()
        r = tr.cbet_solve(e, gp, fields=fields)
        out["python"] = (e, r["gain"])
        e = tr.new_grid()
        r = tr.cbet_solve(e, gp, slabs=True)
        out["slabs"] = (e, r["gain"])
        e = tr.new_grid()
        ws = torch.zeros(api.cbet_workspace_bytes(tr.params) // 8 + 1, dtype=torch.float64, device="cuda")
        api.cbet_solve(tr.d_te, tr.d_r, tr.d_ne, e, tr.d_bbeam_norm, tr.d_beam_norm, tr.d_pow_r, tr.d_phase_r, tr.params, gp,
                       workspace=ws, ctx=tr.ctx, stream=D.stream(torch))
        torch.cuda.synchronize()
        n = tr.params.nbeams * e.numel()
        off = (api.cbet_workspace_gain(tr.params, ws) - ws.data_ptr()) // 8
        out["native"] = (e, ws[off:off + n].view((tr.params.nbeams,) + tr.grid_shape).clone())
        return out, tr.exchange_matrix(fields, gp)

    def spread(s):
        names = list(s)
        return max(float((s[a][1] - s[b][1]).abs().max() / s[b][1].abs().max()) for i, a in enumerate(names) for b in names[i + 1:])

    try:
        plain, t_plain = solves()
        tr.set_detuning(dlambda_angstrom=DC.three_colours(len(W.BEAMS)))
        tinted, t_tinted = solves()
        for loop in plain:
            moved = float((tinted[loop][1] - plain[loop][1]).abs().max() / plain[loop][1].abs().max())
            print("32^3 %s loop, three colours: gain moved by %.3e of max |K|, edep parity against the unshifted %.3e"
                  % (loop, moved, parity_err(tinted[loop][0].cpu().numpy(), plain[loop][0].cpu().numpy())))
            assert moved > DC.MOVES
        free, held = spread(plain), spread(tinted)
        print("32^3: loops apart by %.3e of max |K| with shifts, %.3e without" % (held, free))
        assert held <= 10.0 * max(free, 2.0 ** -52)
        assert float((t_tinted - t_plain).abs().max()) > DC.MOVES * float(t_plain.abs().max())
    finally:
        tr.close()
