"""Saturation of the ion-acoustic wave in both CBET gain kernels and the amplitude map (cbet_grid_kernels.hip: the SAT arms
of k_gain_field and k_gain_field_sym, k_pair_amplitude) on the two grids of helpers/gain_worlds.py,
against the two CPU references of helpers/gain_reference.py with the limits of helpers/saturation_cases.py.

  TRACED  48 x 21 x 134, six beams, the oracle's traced fields; reference: the oracle composed per pair.
  CROWDED 13 x 11 x 148, sixty beams, synthetic fields (9-54 beams per cell: whole runs, halves, quarters); reference: the
          numpy restatement, without a table and with a caller's flow table plus the three-state table (kz = 1).

The bounds are the project's: bit for bit where both sides run the same IEEE statements, 1e-12 of max |K| for the pair-once
kernel against the ordered one, 1e-9 of max |K| against a CPU reference -- max |K| of the UNCLAMPED update.  The limits are
quantiles of the reference's own pair amplitudes (never / half / deep / all).

The slab of the slab-wise and packed cases is [9, 22) on TRACED; CROWDED has 15 planes, there it is [9, 14): the same odd lower
boundary through a two-plane brick, a plane left outside above.
On TRACED the gain is zero beyond the second 64-cell z group with or without a limit (no beam pair meets there), so "the clamp
acts in every z group" is asked of the groups in which the unclamped reference has a gain: two there, all three on CROWDED."""
import numpy as np
import pytest

from conftest import NCPU, parity_err
from helpers import gain_calls as D
from helpers import gain_worlds as W
from helpers import saturation_cases as SC
from helpers.gain_worlds import CUTS, LAST_BITS, SLABS, TOL, Z_GROUPS

pytestmark = pytest.mark.gpu

ACTS = 1e-3                # the clamp moves K by more than this, of max |K|, in every z group that has a gain
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
    """Per grid: the CPU world, a tracer that gets limits (`tr`), one that never has one (`base`), the device fields."""
    out = D.device_worlds(api, oracle, inputs, torch_cuda, NCPU)
    yield out
    D.close_worlds(out)


# ---- 0. the context's limit -----------------------------------------------------------------------------------------------
def test_setter_round_trips_and_refuses_bad_values(api, worlds):
    tr = worlds["traced"]["tr"]
    assert tr.ctx.saturation() == 0.0 and tr.saturation == 0.0           # a new context has none
    tr.set_saturation(0.0375)
    assert tr.ctx.saturation() == 0.0375 and tr.saturation == 0.0375
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(api.CbetError) as ei:
            tr.set_saturation(bad)
        assert ei.value.code == api.EINVAL and "dn_max" in str(ei.value)
        assert tr.ctx.saturation() == 0.0375 and tr.saturation == 0.0375  # a refused value changes nothing
    tr.set_saturation(0.0)
    assert tr.ctx.saturation() == 0.0
    other = api.Context(tr.params, tr.gpu)                                # a context prepared for the tracer carries its limit
    tr.set_saturation(0.25)
    tr._prepare_plasma(tr.params, other)
    assert other.saturation() == 0.25
    tr.set_saturation(0.0)
    other.close()


# ---- 1. identity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tables", ["none", "flow", "uniform", "three"])
@pytest.mark.parametrize("pair_once", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("grid", ["traced", "crowded"])
def test_a_limit_never_reached_and_a_limit_taken_back_change_no_bit(api, torch_cuda, worlds, grid, pair_once, tables):
    """The SAT instantiations with a limit 100 x the reference's largest amplitude, and the plain ones after
    set_saturation(0), against a tracer whose context never had a limit: gains and fields bit for bit -- first call, frozen
    call, slab and packed slab -- and the convergence sums to the rounding of their accumulation order."""
    torch = torch_cuda
    w = worlds[grid]
    tr, base, gp, raw, slab = w["tr"], w["base"], w["gp"], w["dev"]["raw"], SLABS[grid]
    flow, state = D.tables(api, torch, w, tables)
    never = 100.0 * max(SC.reference(w, k)["limits"]["never"] for k in (("restated", "tabled") if grid == "traced" else ("plain", "tabled")))
    D.select(base, flow, state)
    D.select(tr, flow, state)
    try:
        assert base.ctx.saturation() == 0.0
        want = D.all_calls(torch, api, base, raw, gp, pair_once, slab)
        assert float(want[1][1].abs().max()) > 1.0 and float(want[7][1].abs().max()) > 1.0
        for mode, dn in (("never", never), ("taken back", 0.0)):
            tr.set_saturation(dn)
            assert tr.ctx.saturation() == dn
            got = D.all_calls(torch, api, tr, raw, gp, pair_once, slab)
            for (what, a), (_, b) in zip(want, got):
                if what.endswith("change"):
                    x = (0, tr.grid_shape[0]) if what.split()[0] in ("first", "frozen") else slab
                    n = D.waves(tr, pair_once, *x)
                    assert bool(torch.all((a - b).abs() <= (n - 1) * 2.0 ** -53 * a.abs())), (mode, what, a.tolist(), b.tolist())
                else:
                    assert torch.equal(a, b), (mode, what)
    finally:
        tr.set_saturation(0.0)
        D.select(tr, None, None)
        D.select(base, None, None)


# ---- 2. clamped, against the references -----------------------------------------------------------------------------------
CASES = [("traced", "composed"), ("crowded", "plain"), ("crowded", "tabled")]


def _reference(w, which, name):
    """(unclamped K, clamped K, dn_max) of a case."""
    if which == "composed":
        dn = w["limits"][name]
        key = "composed_" + name
        if key not in w:
            w[key] = w["composed"].gain(dn)
        return w["ogain"], w[key], dn
    ref = SC.reference(w, which)
    return ref["K0"], ref["K"][name], ref["limits"][name]


@pytest.mark.parametrize("name", ["half", "deep"])
@pytest.mark.parametrize("grid, which", CASES, ids=["traced", "crowded", "crowded_tabled"])
def test_clamped_update_matches_the_reference(api, torch_cuda, worlds, grid, which, name):
    """Both kernels with half and with 99 % of the pairs clamped: first call and frozen call on the whole grid, slab-wise
    updates concatenated, the packed slab."""
    torch = torch_cuda
    w = worlds[grid]
    tr, gp, raw, slab = w["tr"], w["gp"], w["dev"]["raw"], SLABS[grid]
    K0, want, dn = _reference(w, which, name)
    scale = float(np.abs(K0).max())
    D.select(tr, *D.tables(api, torch, w, "tabled" if which == "tabled" else "none"))
    tr.set_saturation(dn)
    try:
        got = {}
        for pair_once in KERNELS:
            f, k, ch, _, k2, _ = D.first_and_frozen(torch, tr, raw, gp, pair_once)
            parts, fields = tr.new_grid(per_beam=True), raw.clone()
            for x0, x1 in zip(CUTS[grid][:-1], CUTS[grid][1:]):
                tr.gain_field(fields, parts, gp, None, pair_once=pair_once, x_lo=x0, x_hi=x1)
            _, kp, _ = D.packed(torch, api, tr, raw, gp, pair_once, slab)
            got[pair_once] = dict(first=k.cpu().numpy(), frozen=k2.cpu().numpy(), slabs=parts.cpu().numpy(), packed=kp.cpu().numpy(),
                                  change=ch.cpu().numpy(), fields=torch.equal(fields, f))
    finally:
        tr.set_saturation(0.0)
        D.select(tr, None, None)
    x0, x1 = slab
    for pair_once in KERNELS:
        g = got[pair_once]
        label = "%s %s %s %s" % (grid, which, name, "pair-once" if pair_once else "ordered")
        errs = {k: float(np.abs(g[k] - want).max() / scale) for k in ("first", "frozen", "slabs")}
        errs["packed"] = float(np.abs(g["packed"] - want[:, x0:x1]).max() / scale)
        moved = D.group_errors(g["first"], K0, scale)
        print("%s (dn_max %.4e, max |K| %.3e): against the reference %s; moved from the unclamped K by z group %s; sum |K| %.3e of the reference's"
              % (label, dn, scale, {k: "%.2e" % v for k, v in errs.items()}, ["%.2e" % m for m in moved],
                 abs(g["change"][1] / np.abs(want).sum() - 1.0)))
        assert all(e < TOL for e in errs.values()), (label, errs)
        assert g["fields"]                                                   # the normalisation does not see the limit
        assert abs(g["change"][1] / np.abs(want).sum() - 1.0) < TOL
        assert abs(g["change"][0] / g["change"][1] - 1.0) < 1e-12            # from zero: every |new - old| is |new|
        has_gain = [float(np.abs(K0[..., z]).max()) > ACTS * scale for z in Z_GROUPS]
        assert sum(has_gain) >= (2 if grid == "traced" else 3)
        assert all(m > ACTS for m, h in zip(moved, has_gain) if h), (label, moved)
        if not pair_once:                                                    # slabs and packed storage: the same statements per cell
            assert np.array_equal(g["slabs"], g["first"]) and np.array_equal(g["packed"], g["first"][:, x0:x1])
    for k in ("first", "frozen", "slabs", "packed"):
        err = float(np.abs(got[True][k] - got[False][k]).max() / scale)
        by_group = D.group_errors(got[True][k], got[False][k], scale)
        print("%s %s %s %s: pair-once against ordered %.3e, by z group %s" % (grid, which, name, k, err, by_group))
        assert err < LAST_BITS, (k, err)
        assert all(e < LAST_BITS for e in by_group), (k, by_group)          # each group against the WHOLE grid's max |K|


# ---- 3. properties under the clamp ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["half", "all"])
@pytest.mark.parametrize("pair_once", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("grid, which", CASES[:2], ids=["traced", "crowded"])
def test_exchange_cancels_per_cell_under_the_clamp(api, torch_cuda, worlds, grid, which, pair_once, name):
    """tests/test_gpu_gain_shapes.py test_fields_change_exchange_frozen_and_relaxed's bound on |sum_i I_i K_i|."""
    torch = torch_cuda
    w = worlds[grid]
    tr = w["tr"]
    K0, want, dn = _reference(w, which, name)
    tr.set_saturation(dn)
    try:
        f, k, _ = D.update(torch, tr, w["dev"]["raw"], w["gp"], pair_once, change=False)
    finally:
        tr.set_saturation(0.0)
    nf, K = f.cpu().numpy(), k.cpu().numpy()
    inten = np.where(nf[0] > 0, nf[0], 0.0)
    exch, bound = np.abs((inten * K).sum(axis=0)).max(), np.abs(inten * K).sum(axis=0).max()
    err = float(np.abs(K - want).max() / np.abs(K0).max())
    print("%s %s %s: exchange per cell %.3e of the largest; against the reference %.3e of max |K|" %
          (grid, name, "pair-once" if pair_once else "ordered", exch / bound, err))
    assert bound > 0 and exch <= 1e-11 * bound
    assert err < TOL


@pytest.mark.parametrize("grid, which", CASES[:2], ids=["traced", "crowded"])
def test_every_pair_clamped_forgets_the_intensity_scale(api, torch_cuda, worlds, grid, which):
    """With every pair at the limit the exchange rate is lim sqrt(Ii Ij) whatever the gain: energies x 16 (a power of two
    passes through every statement of the ordered kernel exactly) leave K as it is -- bit for bit in the ordered kernel,
    to 1e-12 of max |K| in the pair-once kernel; without a limit the same scaling multiplies K by 16 exactly."""
    torch = torch_cuda
    w = worlds[grid]
    tr, gp, raw = w["tr"], w["gp"], w["dev"]["raw"]
    K0, want, dn = _reference(w, which, "all")
    scale = float(np.abs(K0).max())
    raw16 = raw.clone()
    raw16[0] *= 16.0
    for pair_once in KERNELS:
        _, plain, _ = D.update(torch, tr, raw, gp, pair_once, change=False)
        _, plain16, _ = D.update(torch, tr, raw16, gp, pair_once, change=False)
        tr.set_saturation(dn)
        try:
            _, k, _ = D.update(torch, tr, raw, gp, pair_once, change=False)
            _, k16, _ = D.update(torch, tr, raw16, gp, pair_once, change=False)
        finally:
            tr.set_saturation(0.0)
        err = float((k16 - k).abs().max()) / scale
        print("%s %s, every pair clamped: |K(16 E) - K(E)| = %.3e of max |K|; unclamped |K(16 E) - 16 K(E)| = %.3e; against the reference %.3e"
              % (grid, "pair-once" if pair_once else "ordered", err, float((plain16 - 16.0 * plain).abs().max()) / scale,
                 float(np.abs(k.cpu().numpy() - want).max()) / scale))
        assert float(k.abs().max()) > 0 and float(np.abs(k.cpu().numpy() - want).max()) < TOL * scale
        assert float((k - plain).abs().max()) > ACTS * scale
        if pair_once:
            assert err < LAST_BITS
            assert float((plain16 - 16.0 * plain).abs().max()) < LAST_BITS * 16.0 * scale
        else:
            assert torch.equal(k16, k)
            assert torch.equal(plain16, 16.0 * plain)


# ---- 4. the amplitude map -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tables", ["none", "tabled"])
@pytest.mark.parametrize("grid", ["traced", "crowded"])
def test_amplitude_map_matches_the_reference(api, torch_cuda, worlds, grid, tables):
    """k_pair_amplitude on the whole grid and on a slab (other planes keep a sentinel), the fields untouched, the context's
    limit ignored; amp > dn_max exactly where the reference clamps some pair."""
    torch = torch_cuda
    w = worlds[grid]
    tr, gp, raw, slab = w["tr"], w["gp"], w["dev"]["raw"], SLABS[grid]
    ref = SC.reference(w, tables if tables == "tabled" else ("restated" if grid == "traced" else "plain"))
    D.select(tr, *D.tables(api, torch, w, tables))
    try:
        f, _, _ = D.update(torch, tr, raw, gp, True, change=False)          # normalised fields
        before = f.clone()
        amp = tr.pair_amplitude(f, gp)
        tr.set_saturation(ref["limits"]["half"])                            # the map is the unclamped amplitude
        limited = tr.pair_amplitude(f, gp)
        tr.set_saturation(0.0)
        part = torch.full(tr.grid_shape, -3.0, dtype=torch.float64, device="cuda")
        assert tr.pair_amplitude(f, gp, x_lo=slab[0], x_hi=slab[1], out=part) is part
        for bad in (part[1:].contiguous(), part.float(), part.transpose(0, 2)):   # another shape, dtype or layout: refused
            with pytest.raises(ValueError):
                tr.pair_amplitude(f, gp, out=bad)
        torch.cuda.synchronize()
    finally:
        tr.set_saturation(0.0)
        D.select(tr, None, None)
    assert torch.equal(f, before)
    assert torch.equal(limited, amp)
    assert torch.equal(part[slab[0]:slab[1]], amp[slab[0]:slab[1]])
    assert bool((part[:slab[0]] == -3.0).all()) and bool((part[slab[1]:] == -3.0).all())
    a, want = amp.cpu().numpy(), ref["amp"]
    top = float(want.max())
    err = float(np.abs(a - want).max() / top)
    print("%s %s: amplitude map max %.4e in %d non-zero cells, against the reference %.3e of its maximum" %
          (grid, tables, top, int((want > 0).sum()), err))
    assert top > 0 and err < LAST_BITS
    alone = ((ref["I"] > 0).sum(axis=0) < 2) | (ref["kap"] == 0)
    assert alone.any() and not a[alone].any()                               # fewer than two beams, or not sub-critical: exactly zero
    for name in ("half", "deep"):
        dn = ref["limits"][name]
        clamps = ref["top"] > dn * ref["kap"]                               # the reference clamps some pair of the cell
        near = np.abs(want / dn - 1.0) <= SC.NEAR
        assert near.sum() <= SC.NEAR_SHARE * (want > 0).sum()
        assert np.array_equal((a > dn)[~near], clamps[~near]), name
        assert 0 < clamps.sum() < clamps.size


# ---- 5. end to end --------------------------------------------------------------------------------------------------------
def _solves(torch, api, tr, gp):
    """The three loops on tr's context: {loop: (edep, gain, report values)} and the Python loop's normalised fields."""
    out = {}
    fields = tr.new_fields()
    e = tr.new_grid()
    r = tr.cbet_solve(e, gp, fields=fields)
    out["python"] = (e, r["gain"], (r["passes"], bool(r["converged"]), r["imbalance"]))
    e = tr.new_grid()
    r = tr.cbet_solve(e, gp, slabs=True)
    out["slabs"] = (e, r["gain"], (r["passes"], bool(r["converged"]), r["imbalance"]))
    e = tr.new_grid()
    ws = torch.zeros(api.cbet_workspace_bytes(tr.params) // 8 + 1, dtype=torch.float64, device="cuda")
    rep = api.cbet_solve(tr.d_te, tr.d_r, tr.d_ne, e, tr.d_bbeam_norm, tr.d_beam_norm, tr.d_pow_r, tr.d_phase_r, tr.params, gp,
                         workspace=ws, ctx=tr.ctx, stream=D.stream(torch))
    torch.cuda.synchronize()
    n = tr.params.nbeams * e.numel()
    off = (api.cbet_workspace_gain(tr.params, ws) - ws.data_ptr()) // 8
    out["native"] = (e, ws[off:off + n].view((tr.params.nbeams,) + tr.grid_shape).clone(), (rep.passes, bool(rep.converged), rep.imbalance))
    return out, fields


def _spread(solves):
    """How far the three loops are from one another: (edep parity, gain of max |gain|), the largest over the pairs."""
    names = list(solves)
    pe, pg = 0.0, 0.0
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            pe = max(pe, parity_err(solves[a][0].cpu().numpy(), solves[b][0].cpu().numpy()))
            pg = max(pg, float((solves[a][1] - solves[b][1]).abs().max() / solves[b][1].abs().max()))
    return pe, pg


def test_solve_loops_honour_the_limit(api, inputs, torch_cuda):
    """tests/test_gpu_cbet.py's solve (32^3, six beams, relax 1, 12 passes): the Python loop, the slab loop at one rank and the
    native loop with the tracer's context.  A limit never reached gives each loop its own unlimited result -- to the bound
    those tests give two runs of one loop (the deposits are atomic sums: 1e-9) -- and the median of the unclamped solve's
    amplitude map changes what is absorbed, the three loops agreeing as closely as they do without a limit (x 10)."""
    torch = torch_cuda
    bn = inputs[0]
    tr = D.tracer(inputs, api.default_params(32, nbeams=len(W.BEAMS)), bn[W.BEAMS])
    gp = api.default_gain_params(tolerance=1e-6, max_passes=12, relax=1.0)
    try:
        plain, fields = _solves(torch, api, tr, gp)
        amp = tr.pair_amplitude(fields, gp)
        nz = amp[amp > 0]
        assert nz.numel() > 1000
        median, top = float(nz.median()), float(nz.max())
        tr.set_saturation(100.0 * top)
        never, _ = _solves(torch, api, tr, gp)
        for loop in plain:
            pe = parity_err(never[loop][0].cpu().numpy(), plain[loop][0].cpu().numpy())
            pg = float((never[loop][1] - plain[loop][1]).abs().max() / plain[loop][1].abs().max())
            print("32^3 %s loop, a limit never reached: edep parity %.3e, gain %.3e of max |K|; passes, converged, imbalance %s / %s"
                  % (loop, pe, pg, never[loop][2], plain[loop][2]))
            assert pe < 1e-9 and pg < 1e-9
            assert never[loop][2][:2] == plain[loop][2][:2]
        tr.set_saturation(median)
        clamped, _ = _solves(torch, api, tr, gp)
        free, held = _spread(plain), _spread(clamped)
        absorbed = {k: float(v["python"][0].sum()) for k, v in (("plain", plain), ("clamped", clamped))}
        print("32^3, dn_max = the amplitude map's median %.4e (max %.4e): loops apart by %.3e / %.3e (edep parity / gain), unclamped %.3e / %.3e;"
              " absorbed %.6e against %.6e" % (median, top, held[0], held[1], free[0], free[1], absorbed["clamped"], absorbed["plain"]))
        for loop in clamped:
            print("32^3 %s loop, clamped: passes %d, converged %s, imbalance %.3e" % ((loop,) + clamped[loop][2]))
        assert held[0] <= 10.0 * max(free[0], 2.0 ** -52) and held[1] <= 10.0 * max(free[1], 2.0 ** -52)
        assert abs(absorbed["clamped"] / absorbed["plain"] - 1.0) > 1e-6
    finally:
        tr.close()


def test_mesh_state_solve_runs_with_a_limit(api, inputs, torch_cuda):
    """tests/test_gpu_state.py's end-to-end case (24^3, six beams, the 3-D mesh with ti and zbar, set_flow("mesh") and
    set_gain_state("mesh")) with a limit: one solve of each Python loop runs, and the limit changes its gain."""
    from helpers import state_cases as S
    tr = D.tracer(inputs, api.default_params(24, nbeams=len(W.BEAMS)), inputs[0][W.BEAMS])
    try:
        _, a = S.mesh3d_ions(api, dense=10.0)
        tr.set_plasma_mesh(a["r"], a["theta"], a["phi"], a["ne"], a["te"], a["u"], a["center"], ti=a["ti"], zbar=a["zbar"])
        tr.set_flow("mesh")
        tr.set_gain_state("mesh")
        gp = api.default_gain_params(tolerance=1e-6, max_passes=12, relax=1.0)
        fields = tr.new_fields()
        r0 = tr.cbet_solve(tr.new_grid(), gp, fields=fields)
        amp = tr.pair_amplitude(fields, gp)
        nz = amp[amp > 0]
        assert nz.numel() > 0
        tr.set_saturation(float(nz.median()))
        r1 = tr.cbet_solve(tr.new_grid(), gp)
        r2 = tr.cbet_solve(tr.new_grid(), gp, slabs=True)
        kmax = float(r0["gain"].abs().max())
        print("24^3 mesh state, dn_max = median amplitude %.4e: passes %d / %d (unlimited %d), converged %s / %s, imbalance %.3e / %.3e, "
              "max |K - K unlimited| %.3e of max |K|" % (float(nz.median()), r1["passes"], r2["passes"], r0["passes"], r1["converged"],
                                                         r2["converged"], r1["imbalance"], r2["imbalance"],
                                                         float((r1["gain"] - r0["gain"]).abs().max()) / kmax))
        assert float((r1["gain"] - r0["gain"]).abs().max()) > ACTS * kmax
    finally:
        tr.close()
