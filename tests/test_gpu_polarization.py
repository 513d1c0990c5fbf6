"""Polarization smoothing in the gain stage on the device (cbet_grid_kernels.hip: the POL arms of k_gain_field,
k_gain_field_sym, k_pair_amplitude and k_exchange_matrix) against the numpy restatement of
helpers/polarization_cases.py and the polarized host twin, on the grids of helpers/gain_worlds.py and the CROSSING world:

  TRACED   48 x 21 x 134, six beams, the oracle's traced fields.
  CROWDED  13 x 11 x 148, sixty beams, synthetic fields: runs, halves and quarters, ragged bricks, unaligned rows.
  CROSSING 6 x 5 x 20, three beams along +x, +y, -x: the factor is exactly 1/4 or 1/2.

Two configurations (polarization_cases.CONFIGS): plain, and with everything on -- the offset target's flow table, the
three-state table, sixty distinct shifts and, where a test clamps, a limit at the median of the smoothed reference's own pair
amplitudes.  The bounds are the project's: bit for bit where both sides run the same IEEE statements, LAST_BITS (1e-12) of
max |K| for the pair-once kernel against the ordered one, TOL (1e-9) of max |K| against the restatement and of Gross_ij against
the twin.  max |K| is the smoothed reference's own."""
import numpy as np
import pytest

from conftest import NCPU
from helpers import exchange_cases as XC
from helpers import gain_calls as D
from helpers import polarization_cases as PC
from helpers.gain_worlds import CUTS, LAST_BITS, SLABS, TOL

pytestmark = pytest.mark.gpu

KERNELS = [False, True]
KERNEL_IDS = ["ordered", "pair_once"]
GRIDS = ["traced", "crowded"]
CONFIGS = list(PC.CONFIGS)


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
    """Per grid: the CPU world, a tracer that gets a mode (`tr`), one that never has one (`base`), the device fields."""
    out = D.device_worlds(api, oracle, inputs, torch_cuda, NCPU)
    yield out
    D.close_worlds(out)


def _clear(*tracers):
    for tr in tracers:
        tr.set_polarization("aligned")
        tr.set_detuning()
        tr.set_saturation(0.0)
        D.select(tr)


def _configure(api, torch, w, tr, config, limit=None, smoothed=True):
    """A tracer in a configuration of PC.CONFIGS: its tables and shifts, the limit (None: the reference's `half` where
    everything is on, else none), the mode.  Returns the reference and the limit."""
    tables, everything = PC.CONFIGS[config]
    ref = PC.reference(w, config)
    D.select(tr, *D.tables(api, torch, w, tables))
    tr.set_detuning(domega=ref["shift"])
    if limit is None:
        limit = ref["half"] if everything else 0.0
    tr.set_saturation(limit)
    tr.set_polarization("smoothed" if smoothed else "aligned")
    return ref, limit


def _want(ref, limit):
    return ref["Khalf"] if limit > 0 else ref["K"]


# ---- 0. the context -------------------------------------------------------------------------------------------------------
def test_context_refuses_names_and_remembers(api, worlds):
    tr, base = worlds["crowded"]["tr"], worlds["crowded"]["base"]
    try:
        assert tr.polarization() == "aligned" and tr.ctx.polarization() == "aligned"          # a new context's default
        tr.set_polarization("smoothed")
        assert tr.polarization() == "smoothed" and base.polarization() == "aligned"
        for mode in (-1, 2):
            with pytest.raises(api.CbetError) as ei:
                tr.ctx.set_polarization(mode)
            assert ei.value.code == api.EINVAL and ("mode = %d" % mode) in str(ei.value)
            assert "cbet_context_set_polarization" in str(ei.value)
            assert tr.polarization() == "smoothed"                                            # a refused call changes nothing
        with pytest.raises(ValueError):
            tr.set_polarization("circular")
        assert tr.polarization() == "smoothed"
        other = api.Context(tr.params, tr.gpu)                  # a context prepared for the tracer carries its mode
        assert other.polarization() == "aligned"
        tr._prepare_plasma(tr.params, other)
        assert other.polarization() == "smoothed"
        tr.set_polarization(api.POL_ALIGNED)
        tr._prepare_plasma(tr.params, other)
        assert other.polarization() == "aligned" and tr.polarization() == "aligned"
        other.close()
    finally:
        _clear(tr)


# ---- 1. off is off --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("grid", GRIDS)
def test_off_is_off(api, torch_cuda, worlds, grid, config):
    """"smoothed", then "aligned" again: both gain kernels (first call, frozen call, slab, packed slab), the amplitude map and
    the exchange matrix give the bits of a tracer that never set a mode."""
    torch = torch_cuda
    w = worlds[grid]
    tr, base, gp, raw, slab = w["tr"], w["base"], w["gp"], w["dev"]["raw"], SLABS[grid]

    def everything_of(tracer):
        out = []
        for pair_once in KERNELS:
            out += [("%s %s" % (KERNEL_IDS[pair_once], what), t)
                    for what, t in D.all_calls(torch, api, tracer, raw, gp, pair_once, slab, change=False)]
        f = out[0][1]
        T, G = tracer.exchange_matrix(f, gp, gross=True)
        out += [("amplitude map", tracer.pair_amplitude(f, gp)), ("T", T), ("Gross", G)]
        torch.cuda.synchronize()
        return out

    try:
        _configure(api, torch, w, base, config, smoothed=False)
        want = everything_of(base)
        _configure(api, torch, w, tr, config, smoothed=True)
        assert tr.polarization() == "smoothed" and base.polarization() == "aligned"
        moved = D.update(torch, tr, raw, gp, True, change=False)[1]
        tr.set_polarization("aligned")
        assert tr.polarization() == "aligned"
        got = everything_of(tr)
    finally:
        _clear(tr, base)
    assert float(want[1][1].abs().max()) > 1.0 and float(want[-2][1].abs().max()) > 0
    assert float((moved - want[1][1]).abs().max()) > 1e-2 * float(want[1][1].abs().max())    # the mode had been on
    for (what, a), (_, b) in zip(want, got):
        assert torch.equal(a, b), (grid, config, what)


# ---- 2. the ordered kernel, 3. the pair-once kernel -----------------------------------------------------------------------
@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("grid", GRIDS)
def test_smoothed_update_matches_the_restatement(api, torch_cuda, worlds, grid, config):
    """k_gain_field and k_gain_field_sym in smoothed mode, first call and frozen call, against the restatement (per 64-cell z
    group) and against each other; slab-wise updates and the packed slab against the whole-grid result."""
    torch = torch_cuda
    w = worlds[grid]
    tr, gp, raw, slab = w["tr"], w["gp"], w["dev"]["raw"], SLABS[grid]
    got = {}
    try:
        ref, limit = _configure(api, torch, w, tr, config)
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
    want = _want(ref, limit)
    scale = float(np.abs(ref["K"]).max())
    x0, x1 = slab
    for pair_once in KERNELS:
        g = got[pair_once]
        label = "%s %s %s" % (grid, config, KERNEL_IDS[pair_once])
        errs = {k: D.group_errors(g[k], want, scale) for k in ("first", "frozen", "slabs")}
        errs["packed"] = D.group_errors(g["packed"], want[:, x0:x1], scale)
        moved = float(np.abs(g["first"] - ref["Ka"]).max() / np.abs(ref["Ka"]).max())
        print("%s (max |K| %.3e): against the restatement per z group %s; moved from the aligned unclamped K by %.3e of its max"
              % (label, scale, {k: ["%.2e" % e for e in v] for k, v in errs.items()}, moved))
        assert all(e < TOL for v in errs.values() for e in v), (label, errs)
        assert moved > 1e-2
        assert g["fields"]                                                   # the normalisation does not see the mode
        assert abs(g["change"][1] / np.abs(want).sum() - 1.0) < TOL
        # storage: slab-wise updates are the whole update bit for bit; the packed slab is, for the ordered kernel, and
        # agrees to the last bits for the pair-once kernel (its runs follow the storage) -- the existing slab tests' bounds
        assert np.array_equal(g["slabs"], g["first"]), label
        if pair_once:
            assert float(np.abs(g["packed"] - g["first"][:, x0:x1]).max() / scale) < LAST_BITS
        else:
            assert np.array_equal(g["packed"], g["first"][:, x0:x1])
    for k in ("first", "frozen", "slabs", "packed"):
        err = max(D.group_errors(got[True][k], got[False][k], scale))
        print("%s %s %s: pair-once against ordered %.3e" % (grid, config, k, err))
        assert err < LAST_BITS, (k, err)


# ---- 4. exact factors -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", sorted(PC.FACTOR))
def test_crossing_pairs_give_the_exact_factor(api, oracle, inputs, torch_cuda, pair):
    """Beams at right angles: the ordered kernel's smoothed K is 0.25 x its aligned K bit for bit, opposed beams: 0.5 x; the
    pair-once kernel agrees within LAST_BITS."""
    torch = torch_cuda
    w = PC.crossing_world(api, oracle, inputs)
    tr = D.tracer(inputs, PC.pair_params(api), w["bn"][list(pair)])
    raw = torch.from_numpy(PC.pair_raw(w, pair)).cuda()
    K = {}
    try:
        for mode in api.POLARIZATIONS:
            tr.set_polarization(mode)
            for pair_once in KERNELS:
                K[mode, pair_once] = D.update(torch, tr, raw, w["gp"], pair_once, change=False)[1].cpu().numpy()
    finally:
        tr.close()
    aligned, factor = K["aligned", False], PC.FACTOR[pair]
    live = aligned != 0
    scale = float(np.abs(aligned).max())
    print("CROSSING %s: %d non-zero aligned entries, max |K| %.6e, smallest %.3e" % (pair, live.sum(), scale, np.abs(aligned[live]).min()))
    assert live.sum() >= 100 and np.abs(aligned[live]).min() > 1e-200        # nonzero and far from the subnormal range
    assert np.array_equal(K["smoothed", False], factor * aligned)
    assert float(np.abs(K["smoothed", True] - factor * aligned).max()) < LAST_BITS * factor * scale
    assert float(np.abs(K["aligned", True] - aligned).max()) < LAST_BITS * scale


# ---- 5. a cell's exchange cancels -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", ["none", "half"])
@pytest.mark.parametrize("grid", GRIDS)
def test_a_cells_exchange_cancels_as_well_as_aligned(api, torch_cuda, worlds, grid, limit):
    """sum_i I_i K_i of a cell relative to its largest term, the worst cell: smoothed no worse than aligned on the same fields
    (x 2 for rounding), for both kernels, with and without a limit."""
    torch = torch_cuda
    w = worlds[grid]
    tr, gp, raw = w["tr"], w["gp"], w["dev"]["raw"]
    ref = PC.reference(w, "plain")
    worst = {}
    try:
        tr.set_saturation(0.0 if limit == "none" else ref["half"])
        for mode in api.POLARIZATIONS:
            tr.set_polarization(mode)
            for pair_once in KERNELS:
                f, k, _ = D.update(torch, tr, raw, gp, pair_once, change=False)
                nf, K = f.cpu().numpy(), k.cpu().numpy()
                terms = np.where(nf[0] > 0, nf[0], 0.0) * K
                largest = np.abs(terms).max(axis=0)
                on = largest > 0
                worst[mode, pair_once] = float((np.abs(terms.sum(axis=0))[on] / largest[on]).max())
                assert on.sum() > 1000
    finally:
        _clear(tr)
    for pair_once in KERNELS:
        print("%s %s %s: |sum I K| / largest term, worst cell: aligned %.3e, smoothed %.3e"
              % (grid, limit, KERNEL_IDS[pair_once], worst["aligned", pair_once], worst["smoothed", pair_once]))
        assert worst["smoothed", pair_once] <= 2.0 * worst["aligned", pair_once]


# ---- 6. the amplitude map and the clamp -----------------------------------------------------------------------------------
@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("grid", GRIDS)
def test_amplitude_map_and_clamp_see_the_smoothed_gain(api, torch_cuda, worlds, grid, config):
    """k_pair_amplitude in smoothed mode is the restatement's map of f |G_ij|; with the limit at the median SMOOTHED amplitude
    both kernels' clamped K is the restatement's: the factor sits before the clamp on the device."""
    torch = torch_cuda
    w = worlds[grid]
    tr, gp, raw = w["tr"], w["gp"], w["dev"]["raw"]
    try:
        ref, _ = _configure(api, torch, w, tr, config, limit=0.0)
        f, _, _ = D.update(torch, tr, raw, gp, True, change=False)
        amp = tr.pair_amplitude(f, gp).cpu().numpy()
        tr.set_saturation(ref["half"])
        clamped = [D.update(torch, tr, raw, gp, pair_once, change=False)[1].cpu().numpy() for pair_once in KERNELS]
        tr.set_polarization("aligned")
        aligned_amp = tr.pair_amplitude(f, gp).cpu().numpy()
    finally:
        _clear(tr)
    top, scale = float(ref["amp"].max()), float(np.abs(ref["K"]).max())
    aerr = float(np.abs(amp - ref["amp"]).max() / top)
    kerr = [float(np.abs(k - ref["Khalf"]).max() / scale) for k in clamped]
    acts = float(np.abs(ref["Khalf"] - ref["K"]).max() / scale)
    print("%s %s: amplitude map against the restatement %.3e of its maximum %.4e; clamped K (limit %.4e) ordered / pair-once %.3e / %.3e"
          " of max |K|; the limit moves the reference by %.3e" % (grid, config, aerr, top, ref["half"], kerr[0], kerr[1], acts))
    assert top > 0 and aerr < TOL
    assert all(e < TOL for e in kerr) and acts > 1e-3
    assert float(np.abs(aligned_amp - ref["amp"]).max() / top) > 1e-2        # ... and not the aligned amplitude


# ---- 7. the exchange matrix -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("grid", GRIDS)
def test_exchange_matrix_smoothed(api, torch_cuda, worlds, grid, config):
    torch = torch_cuda
    w = worlds[grid]
    tr, gp, raw = w["tr"], w["gp"], w["dev"]["raw"]
    tabled = PC.CONFIGS[config][0] == "tabled"
    try:
        ref, limit = _configure(api, torch, w, tr, config)
        f, k, _ = D.update(torch, tr, raw, gp, True, change=False)
        T, G = tr.exchange_matrix(f, gp, gross=True)
        T2, G2 = tr.exchange_matrix(f, gp, gross=True)
        tr.set_saturation(0.0)                                               # the bounds: without a limit, aligned against smoothed
        _, Gs = tr.exchange_matrix(f, gp, gross=True)
        tr.set_polarization("aligned")
        _, Ga = tr.exchange_matrix(f, gp, gross=True)
        torch.cuda.synchronize()
    finally:
        _clear(tr)
    assert torch.equal(T, T2) and torch.equal(G, G2)                         # two calls give the same bits
    nf, T, G, K, Gs, Ga = (t.cpu().numpy() for t in (f, T, G, k, Gs, Ga))
    host, hgross = api.exchange_matrix_host(nf, w["ne3d"], w["p"], gp, flow=w["shifted"] if tabled else None,
                                            state=w["state"] if tabled else None, dn_max=limit, shift=ref["shift"],
                                            polarization="smoothed")
    want, gross = (ref["Thalf"], ref["Ghalf"]) if limit > 0 else (ref["T"], ref["G"])
    err, gerr, rerr = XC.worst(T, host, hgross), XC.worst(G, hgross, hgross), XC.worst(T, want, gross)
    ds = ref["R"].ds.reshape(nf.shape[2:])
    inten = np.where(nf[0] > 0, nf[0], 0.0)
    rows = (ds[None] * inten * K).reshape(K.shape[0], -1).sum(axis=1)        # sum ds I_i K_i of the smoothed gain update
    row_err = float((np.abs(T.sum(axis=1) - rows) / G.sum(axis=1)).max())
    live = Ga > 0
    ratio = Gs[live] / Ga[live]
    print("%s %s: T against the polarized twin %.3e of Gross (Gross %.3e), against the restatement %.3e; rows against sum ds I K %.3e;"
          " Gross smoothed / aligned between %.6f and %.6f" % (grid, config, err, gerr, rerr, row_err, ratio.min(), ratio.max()))
    assert err < TOL and gerr < TOL and rerr < TOL
    assert np.array_equal(T, -T.T) and np.array_equal(G, G.T)
    assert row_err < TOL
    assert live.any() and np.array_equal(Gs[~live], Ga[~live])
    assert (Gs >= PC.LOW * Ga * (1.0 - PC.SLACK)).all() and (Gs <= PC.HIGH * Ga * (1.0 + PC.SLACK)).all()
    assert ((ratio > PC.LOW * (1.0 + 1e-6)) & (ratio < PC.HIGH * (1.0 - 1e-6))).any()


# ---- 8. the solve ---------------------------------------------------------------------------------------------------------
def test_native_solve_honours_the_mode(api, torch_cuda, worlds):
    """cbet_cbet_solve with the tracer's context in smoothed mode, two passes on TRACED, against the same two passes stepped by
    hand with smoothed gain updates (1e-7 of max |K|: the loop tests' bound, the deposits are summed atomically) -- and more
    than 1e-3 of max |K| away from the aligned solve."""
    torch = torch_cuda
    w = worlds["traced"]
    tr = w["tr"]
    gp = api.default_gain_params(tolerance=0.0, max_passes=2, relax=1.0)
    assert gp.direction_passes == 1
    nb = tr.params.nbeams

    def native():
        e = tr.new_grid()
        ws = torch.zeros(api.cbet_workspace_bytes(tr.params) // 8 + 1, dtype=torch.float64, device="cuda")
        rep = api.cbet_solve(tr.d_te, tr.d_r, tr.d_ne, e, tr.d_bbeam_norm, tr.d_beam_norm, tr.d_pow_r, tr.d_phase_r, tr.params, gp,
                             workspace=ws, ctx=tr.ctx, stream=D.stream(torch))
        torch.cuda.synchronize()
        assert rep.passes == 2
        off = (api.cbet_workspace_gain(tr.params, ws) - ws.data_ptr()) // 8
        return ws[off:off + nb * e.numel()].view((nb,) + tr.grid_shape).clone()

    try:
        aligned = native()
        tr.set_polarization("smoothed")
        smoothed = native()
        fields, gain = tr.new_fields(), tr.new_grid(per_beam=True)           # the same two passes by hand
        tr.launch_cbet(fields, gp, fields=True)
        tr.gain_field(fields, gain, gp, None, pair_once=True)
        fields[0].zero_()
        tr.launch_cbet(fields[0], gp, fields="energy", gain=gain)
        tr.gain_field(fields, gain, gp, None, pair_once=True, frozen=True)
        torch.cuda.synchronize()
    finally:
        _clear(tr)
    scale = float(smoothed.abs().max())
    err = float((smoothed - gain).abs().max()) / scale
    moved = float((smoothed - aligned).abs().max()) / float(aligned.abs().max())
    print("TRACED, two passes: native smoothed solve against the passes by hand %.3e of max |K| = %.3e; against the aligned solve %.3e"
          % (err, scale, moved))
    assert scale > 1.0 and err < 1e-7
    assert moved > 1e-3
