"""Laser bandwidth in the gain stage on the device (cbet_grid_kernels.hip: the BAND arms of k_gain_field, k_gain_field_sym,
k_pair_amplitude and k_exchange_matrix) against the numpy restatement of helpers/bandwidth_cases.py --
the direct double sum over line pairs, not the library's difference table -- and the banded host twin, on the grids of
helpers/gain_worlds.py, the CROSSING world of helpers/polarization_cases.py and a 32^3 six-beam solve:

  TRACED   48 x 21 x 134, six beams, the oracle's traced fields.
  CROWDED  13 x 11 x 148, sixty beams, synthetic fields: runs, halves and quarters, ragged bricks, unaligned rows.
  CROSSING 6 x 5 x 20 (haloed 8 x 7 x 22), three beams along +x, +y, -x in every sub-critical cell: the exact cases.

The sixty shifts of helpers/detuning_cases.py are on in every parity case.  The bounds are the project's: bit for bit where both
sides run the same IEEE statements, LAST_BITS (1e-12) of max |K| for the pair-once kernel against the ordered one and of its
maximum for the amplitude map, TOL (1e-9) of max |K| against the restatement and of Gross_ij against the twin and the
restatement.  max |K| is the banded reference's own.

Observed on the MI355X: ordered kernel against the restatement 4.3e-16 of max |K|, pair-once 1.7e-15, pair-once against ordered
1.6e-15; k_exchange_matrix against the banded twin 1.4e-15 of Gross_ij, against the restatement 8.4e-15; rows of T against
sum ds I_i K_i 8.9e-16; k_pair_amplitude against the restatement 6.4e-16 of its maximum; the three solve loops 3.7e-16 of max |K|
apart with lines (4.0e-16 without), 0.71 of max |K| from the solve without lines; I_i K_i + I_j K_j exactly 0 on CROSSING."""
import numpy as np
import pytest

from conftest import NCPU
from helpers import bandwidth_cases as BC
from helpers import detuning_cases as DC
from helpers import exchange_cases as XC
from helpers import gain_calls as D
from helpers import gain_worlds as W
from helpers import polarization_cases as PC
from helpers.gain_worlds import CUTS, LAST_BITS, SLABS, TOL

pytestmark = pytest.mark.gpu

KERNELS = [False, True]
KERNEL_IDS = ["ordered", "pair_once"]
GRIDS = ["traced", "crowded"]
NONE = (None, ([1.3e12], [2.0]), ([4e11, 4e11, 4e11], [1.0, 2.0, 3.0]))      # no lines, one line, equal offsets


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
    """Per grid: the CPU world, a tracer that gets a spectrum (`tr`), one that never has one (`base`), the device fields."""
    out = D.device_worlds(api, oracle, inputs, torch_cuda, NCPU)
    yield out
    D.close_worlds(out)


def _clear(*tracers):
    for tr in tracers:
        tr.set_bandwidth()
        tr.set_polarization("aligned")
        tr.set_detuning()
        tr.set_saturation(0.0)
        D.select(tr)


def _configure(api, torch, w, tr, tables, spectrum, smoothed, limit):
    """A tracer with a table set-up, the sixty shifts, a spectrum of BC.SPECTRA (None: none), a polarization mode and a limit
    ("none", or "half" of the banded reference).  Returns the reference and the limit's value."""
    ref = BC.reference(w, tables, spectrum or "five", smoothed=smoothed)
    D.select(tr, *D.tables(api, torch, w, tables))
    tr.set_detuning(domega=ref["shift"])
    tr.set_polarization("smoothed" if smoothed else "aligned")
    dn = ref["half"] if limit == "half" else 0.0
    tr.set_saturation(dn)
    if spectrum is None:
        tr.set_bandwidth()
    else:
        tr.set_bandwidth(*ref["lines"])
    return ref, dn


def _everything_of(torch, api, tracer, raw, gp, slab):
    out = []
    for pair_once in KERNELS:
        out += [("%s %s" % (KERNEL_IDS[pair_once], what), t)
                for what, t in D.all_calls(torch, api, tracer, raw, gp, pair_once, slab, change=False)]
    f = out[0][1]
    T, G = tracer.exchange_matrix(f, gp, gross=True)
    out += [("amplitude map", tracer.pair_amplitude(f, gp)), ("T", T), ("Gross", G)]
    torch.cuda.synchronize()
    return out


# ---- 0. the context -------------------------------------------------------------------------------------------------------
def test_context_remembers_replaces_and_refuses(api, torch_cuda, worlds):
    tr, base = worlds["crowded"]["tr"], worlds["crowded"]["base"]
    try:
        assert tr.bandwidth() is None and tr.ctx.bandwidth() is None                     # a new context's default
        off, wts = BC.lines("five")
        tr.set_bandwidth(off, wts)
        got = tr.bandwidth()
        assert np.array_equal(got[0], off) and np.array_equal(got[1], wts / wts.sum())    # the getter: the normalised lines
        assert base.bandwidth() is None                                                   # another context is untouched
        for bad, text in ((([0.0, np.nan], [1.0, 1.0]), "line_domega[1] is NaN"), (([0.0, 1e12], [1.0, 0.0]), "line_weight[1]"),
                          ((np.arange(9.0), np.ones(9)), "nlines = 9")):
            with pytest.raises(api.CbetError) as ei:
                tr.set_bandwidth(*bad)
            assert ei.value.code == api.EINVAL and text in str(ei.value) and "cbet_context_set_bandwidth" in str(ei.value)
            assert np.array_equal(tr.bandwidth()[0], off)                                 # a refused call changes nothing
        with pytest.raises(ValueError):
            tr.set_bandwidth(domega=off, dlambda_angstrom=[1.0, 2.0])
        off3, wts3 = BC.lines("three")
        tr.set_bandwidth(off3, wts3)                                                      # a second call replaces the first
        assert np.array_equal(tr.bandwidth()[0], off3) and np.array_equal(tr.bandwidth()[1], wts3 / wts3.sum())
        other = api.Context(tr.params, tr.gpu)                  # a context prepared for the tracer receives its spectrum ...
        assert other.bandwidth() is None
        tr._prepare_plasma(tr.params, other)
        assert np.array_equal(other.bandwidth()[0], off3) and np.array_equal(other.bandwidth()[1], wts3 / wts3.sum())
        for none in NONE:                                       # ... and loses it with the tracer's
            tr.set_bandwidth(off3, wts3)
            tr._prepare_plasma(tr.params, other)
            assert other.bandwidth() is not None
            tr.set_bandwidth(*((None,) if none is None else none))
            assert tr.bandwidth() is None
            tr._prepare_plasma(tr.params, other)
            assert other.bandwidth() is None
        tr.set_bandwidth(dlambda_angstrom=[3.0, 0.0, -3.0])
        assert np.array_equal(tr.bandwidth()[0], api.wavelength_shift_to_domega(tr.params, np.array([3.0, 0.0, -3.0])))
        assert np.array_equal(tr.bandwidth()[1], np.full(3, 1.0) / 3.0)
        other.close()
    finally:
        _clear(tr)


def test_prepared_context_adopts_all_four_beam_options(api, torch_cuda, worlds):
    """A limit, "smoothed", sixty distinct shifts and a three-line spectrum on one tracer: a context prepared for it reads all
    four back; prepared again with nothing changed it makes no set-up call (the arrays it has recorded are the very ones the
    tracer's context recorded); with the shifts and the spectrum cleared it loses both and keeps the limit and the mode."""
    tr = worlds["crowded"]["tr"]
    other = api.Context(tr.params, tr.gpu)
    try:
        shifts, (off, wts) = DC.shifts(tr.params.nbeams), BC.lines("three")
        tr.set_saturation(0.0125)
        tr.set_polarization("smoothed")
        tr.set_detuning(domega=shifts)
        tr.set_bandwidth(off, wts)
        assert other.given_beam_options() == (None, None)
        tr._prepare_plasma(tr.params, other)
        for ctx in (tr.ctx, other):
            assert ctx.saturation() == 0.0125 and ctx.polarization() == "smoothed"
            assert np.array_equal(ctx.detuning(), shifts)
            assert np.array_equal(ctx.bandwidth()[0], off) and np.array_equal(ctx.bandwidth()[1], wts / wts.sum())
        given = other.given_beam_options()
        assert given[0] is tr.ctx.given_beam_options()[0] and given[1] is tr.ctx.given_beam_options()[1]
        assert given[0] is not None and given[1] is not None
        tr._prepare_plasma(tr.params, other)                    # nothing changed: nothing is set up again
        again = other.given_beam_options()
        assert again[0] is given[0] and again[1] is given[1]
        assert again[0] is tr.ctx.given_beam_options()[0] and again[1] is tr.ctx.given_beam_options()[1]
        assert np.array_equal(other.detuning(), shifts) and np.array_equal(other.bandwidth()[0], off)
        tr.set_detuning()
        tr.set_bandwidth()
        tr._prepare_plasma(tr.params, other)
        assert other.detuning() is None and other.bandwidth() is None and other.given_beam_options() == (None, None)
        assert other.saturation() == 0.0125 and other.polarization() == "smoothed"
    finally:
        other.close()
        _clear(tr)


# ---- 1. no spectrum is no spectrum ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", [("none", False, "none"), ("tabled", True, "half")], ids=["plain", "everything"])
@pytest.mark.parametrize("grid", GRIDS)
def test_no_spectrum_changes_no_bit(api, torch_cuda, worlds, grid, config):
    """A spectrum, then none again -- set_bandwidth with None, one line or equal offsets: both gain kernels (first call, frozen
    call, slab, packed slab), the amplitude map and the exchange matrix give the bits of a tracer that never had a spectrum."""
    torch = torch_cuda
    w = worlds[grid]
    tr, base, gp, raw, slab = w["tr"], w["base"], w["gp"], w["dev"]["raw"], SLABS[grid]
    tables, smoothed, limit = config
    try:
        _configure(api, torch, w, base, tables, None, smoothed, limit)
        want = _everything_of(torch, api, base, raw, gp, slab)
        _configure(api, torch, w, tr, tables, "five", smoothed, limit)
        moved = D.update(torch, tr, raw, gp, True, change=False)[1]
        got = []
        for none in NONE:
            tr.set_bandwidth(*BC.lines("five"))
            tr.set_bandwidth(*((None,) if none is None else none))
            assert tr.bandwidth() is None
            got.append(_everything_of(torch, api, tr, raw, gp, slab))
    finally:
        _clear(tr, base)
    assert float(want[1][1].abs().max()) > 1.0 and float(want[-2][1].abs().max()) > 0
    assert float((moved - want[1][1]).abs().max()) > 1e-2 * float(want[1][1].abs().max())    # the spectrum had been on
    for result in got:
        for (what, a), (_, b) in zip(want, result):
            assert torch.equal(a, b), (grid, config, what)


# ---- 2. the gain kernels against the restatement --------------------------------------------------------------------------
@pytest.mark.parametrize("smoothed", [False, True], ids=["aligned", "smoothed"])
@pytest.mark.parametrize("limit", ["none", "half"])
@pytest.mark.parametrize("tables", BC.TABLES)
@pytest.mark.parametrize("grid", GRIDS)
def test_banded_update_matches_the_restatement(api, torch_cuda, worlds, grid, tables, limit, smoothed):
    """k_gain_field and k_gain_field_sym under the five-line spectrum (M = 10), first call and frozen call, against the
    restatement (per 64-cell z group) and against each other; slab-wise updates and the packed slab against the whole update."""
    torch = torch_cuda
    w = worlds[grid]
    tr, gp, raw, slab = w["tr"], w["gp"], w["dev"]["raw"], SLABS[grid]
    got = {}
    try:
        ref, dn = _configure(api, torch, w, tr, tables, "five", smoothed, limit)
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
    want = ref["Khalf"] if dn > 0 else ref["K"]
    scale = float(np.abs(ref["K"]).max())
    x0, x1 = slab
    label = "%s %s %s %s" % (grid, tables, limit, "smoothed" if smoothed else "aligned")
    for pair_once in KERNELS:
        g = got[pair_once]
        errs = {k: D.group_errors(g[k], want, scale) for k in ("first", "frozen", "slabs")}
        errs["packed"] = D.group_errors(g["packed"], want[:, x0:x1], scale)
        moved = float(np.abs(g["first"] - (ref["K0"] if dn == 0 else want)).max() / np.abs(ref["K0"]).max())
        print("%s %s (max |K| %.3e): against the restatement %.2e (worst z group of first / frozen / slabs / packed)"
              % (label, KERNEL_IDS[pair_once], scale, max(e for v in errs.values() for e in v)))
        assert all(e < TOL for v in errs.values() for e in v), (label, errs)
        if dn == 0:
            assert moved > BC.MOVES                                          # ... and not the K without a spectrum
        assert g["fields"]                                                   # the normalisation does not see the spectrum
        assert abs(g["change"][1] / np.abs(want).sum() - 1.0) < TOL
        inten = np.where(g["nf"][0] > 0, g["nf"][0], 0.0)                    # a cell's exchange cancels
        exch, bound = np.abs((inten * g["first"]).sum(axis=0)).max(), np.abs(inten * g["first"]).sum(axis=0).max()
        assert bound > 0 and exch <= 1e-11 * bound
        assert np.array_equal(g["slabs"], g["first"]), label                 # slab-wise updates are the whole update
        if pair_once:
            assert float(np.abs(g["packed"] - g["first"][:, x0:x1]).max() / scale) < LAST_BITS
        else:
            assert np.array_equal(g["packed"], g["first"][:, x0:x1])
    for k in ("first", "frozen", "slabs", "packed"):
        err = float(np.abs(got[True][k] - got[False][k]).max() / scale)
        print("%s %s: pair-once against ordered %.3e" % (label, k, err))
        assert err < LAST_BITS, (k, err)


# ---- 3. the exchange matrix and the amplitude map -------------------------------------------------------------------------
@pytest.mark.parametrize("smoothed", [False, True], ids=["aligned", "smoothed"])
@pytest.mark.parametrize("limit", ["none", "half"])
@pytest.mark.parametrize("tables", ["none", "tabled"], ids=["plain", "tabled"])
@pytest.mark.parametrize("grid", GRIDS)
def test_exchange_matrix_and_amplitude_map_banded(api, torch_cuda, worlds, grid, tables, limit, smoothed):
    torch = torch_cuda
    w = worlds[grid]
    tr, gp, raw = w["tr"], w["gp"], w["dev"]["raw"]
    tabled = tables == "tabled"
    try:
        ref, dn = _configure(api, torch, w, tr, tables, "five", smoothed, limit)
        f, k, _ = D.update(torch, tr, raw, gp, True, change=False)
        T, G = tr.exchange_matrix(f, gp, gross=True)
        T2, G2 = tr.exchange_matrix(f, gp, gross=True)
        amp = tr.pair_amplitude(f, gp).cpu().numpy()
        torch.cuda.synchronize()
    finally:
        _clear(tr)
    assert torch.equal(T, T2) and torch.equal(G, G2)                         # two calls give the same bits
    nf, T, G, K = (t.cpu().numpy() for t in (f, T, G, k))
    host, hgross = api.exchange_matrix_host(nf, w["ne3d"], w["p"], gp, flow=w["shifted"] if tabled else None,
                                            state=w["state"] if tabled else None, dn_max=dn, shift=ref["shift"],
                                            polarization="smoothed" if smoothed else "aligned", lines=ref["lines"])
    want, gross = (ref["Thalf"], ref["Ghalf"]) if dn > 0 else (ref["T"], ref["G"])
    err, gerr, rerr = XC.worst(T, host, hgross), XC.worst(G, hgross, hgross), XC.worst(T, want, gross)
    ds = ref["R"].ds.reshape(nf.shape[2:])
    inten = np.where(nf[0] > 0, nf[0], 0.0)
    rows = (ds[None] * inten * K).reshape(K.shape[0], -1).sum(axis=1)        # sum ds I_i K_i of the banded gain update
    row_err = float((np.abs(T.sum(axis=1) - rows) / G.sum(axis=1)).max())
    top = float(ref["amp"].max())
    aerr = float(np.abs(amp - ref["amp"]).max() / top)
    print("%s %s %s %s: T against the banded twin %.3e of Gross (Gross %.3e), against the restatement %.3e; rows against sum ds I K %.3e;"
          " amplitude map against the restatement %.3e of its maximum %.4e"
          % (grid, tables, limit, "smoothed" if smoothed else "aligned", err, gerr, rerr, row_err, aerr, top))
    assert err < TOL and gerr < TOL and rerr < TOL
    assert np.array_equal(T, -T.T) and np.array_equal(G, G.T)
    assert row_err < TOL
    assert top > 0 and aerr < LAST_BITS                                      # the amplitude of the SUMMED gain, before the clamp


@pytest.mark.parametrize("spectrum", ["three", "eight"])
def test_other_spectra_on_crowded(api, torch_cuda, worlds, spectrum):
    """Three lines (M = 3) and eight lines on a 2^40 grid (M = 7, merged differences): all four kernels on CROWDED with the
    tables, smoothed, under `half`."""
    torch = torch_cuda
    w = worlds["crowded"]
    tr, gp, raw = w["tr"], w["gp"], w["dev"]["raw"]
    try:
        ref, dn = _configure(api, torch, w, tr, "tabled", spectrum, True, "half")
        ks = [D.update(torch, tr, raw, gp, pair_once, change=False) for pair_once in KERNELS]
        f = ks[1][0]
        T, G = tr.exchange_matrix(f, gp, gross=True)
        amp = tr.pair_amplitude(f, gp).cpu().numpy()
        torch.cuda.synchronize()
    finally:
        _clear(tr)
    scale, top = float(np.abs(ref["K"]).max()), float(ref["amp"].max())
    kerr = [float(np.abs(k.cpu().numpy() - ref["Khalf"]).max() / scale) for _, k, _ in ks]
    both = float((ks[0][1] - ks[1][1]).abs().max()) / scale
    terr = XC.worst(T.cpu().numpy(), ref["Thalf"], ref["Ghalf"])
    aerr = float(np.abs(amp - ref["amp"]).max() / top)
    print("crowded %s: ordered / pair-once against the restatement %.3e / %.3e of max |K|, against each other %.3e; T %.3e of Gross;"
          " amplitude map %.3e" % (spectrum, kerr[0], kerr[1], both, terr, aerr))
    assert all(e < TOL for e in kerr) and both < LAST_BITS and terr < TOL and aerr < LAST_BITS


# ---- 3b. far off resonance -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
def test_far_off_resonance_only_the_centre_term_is_left(api, torch_cuda, worlds, grid):
    """The five-line spectrum with its offsets x 1000 (d_m >> |q| cs), the sixty shifts on: both kernels agree with the
    reference within TOL of the no-spectrum max |K|, and their K is c_0 x their own K without a spectrum to FAR_SHARE."""
    torch = torch_cuda
    w = worlds[grid]
    tr, gp, raw = w["tr"], w["gp"], w["dev"]["raw"]
    want, mono = BC.light_reference(w, "five", BC.FAR)
    c0, scale = BC.centre_weight("five"), float(np.abs(mono).max())
    try:
        tr.set_detuning(domega=DC.shifts(raw.shape[1]))
        for pair_once in KERNELS:
            tr.set_bandwidth()
            k0 = D.update(torch, tr, raw, gp, pair_once, change=False)[1].cpu().numpy()
            tr.set_bandwidth(*BC.lines("five", BC.FAR))
            k = D.update(torch, tr, raw, gp, pair_once, change=False)[1].cpu().numpy()
            err, share = float(np.abs(k - want).max() / scale), float(np.abs(k - c0 * k0).max() / scale)
            print("%s %s, offsets x %g: against the reference %.3e of the no-spectrum max |K|; |K - c_0 K0| %.3e (c_0 = %.6f)"
                  % (grid, KERNEL_IDS[pair_once], BC.FAR, err, share, c0))
            assert err < TOL and share < BC.FAR_SHARE
            assert float(np.abs(k).max() / scale) > 0.5 * c0                     # ... and the centre term IS left
    finally:
        _clear(tr)


# ---- 4. exact cases on CROSSING -------------------------------------------------------------------------------------------
def _crossing(api, oracle, inputs, torch, parallel=False):
    w = PC.crossing_world(api, oracle, inputs)
    raw = w["raw"].copy()
    if parallel:
        raw[1:, 1] = raw[1:, 0]                                              # beam 1 along beam 0 in every cell: q = 0 exactly
    return w, D.tracer(inputs, w["p"], w["bn"]), torch.from_numpy(raw).cuda()


def _all_four(torch, tr, raw, gp):
    out = []
    for pair_once in KERNELS:
        f, k, _ = D.update(torch, tr, raw, gp, pair_once, change=False)
        out.append(k)
    T, G = tr.exchange_matrix(f, gp, gross=True)
    out += [T, G, tr.pair_amplitude(f, gp)]
    torch.cuda.synchronize()
    return f, out


def test_still_plasma_without_shifts_gives_exact_zeros(api, oracle, inputs, torch_cuda):
    """A caller's zero flow table, no shifts, the five-line spectrum: N = 0, every bracket is an exact zero -- K, T, Gross and the
    amplitude map are zeros from all four kernels; with shifts the same set-up exchanges."""
    torch = torch_cuda
    w, tr, raw = _crossing(api, oracle, inputs, torch)
    p = tr.params
    try:
        tr.set_flow(torch.zeros((3, p.nx, p.ny, p.nz), dtype=torch.float64, device="cuda"))
        tr.set_bandwidth(*BC.lines("five"))
        f, out = _all_four(torch, tr, raw, w["gp"])
        assert bool((f[0] > 0).sum() >= 3 * 100)
        for t in out:
            assert not bool(t.any())
        tr.set_detuning(domega=DC.shifts(3))
        _, out = _all_four(torch, tr, raw, w["gp"])
        assert all(bool(t.any()) for t in out)
    finally:
        tr.close()


def test_parallel_beams_of_different_colour_exchange_nothing_under_a_spectrum(api, oracle, inputs, torch_cuda):
    """Beams 0 and 1 exactly parallel, of different colour, with a spectrum: exact zeros between them from all four kernels;
    the third beam still exchanges with both."""
    torch = torch_cuda
    w, tr, raw = _crossing(api, oracle, inputs, torch, parallel=True)
    try:
        tr.set_detuning(domega=DC.shifts(3))
        tr.set_bandwidth(*BC.lines("five"))
        f, (k0, k1, T, G, amp) = _all_four(torch, tr, raw, w["gp"])
        assert float(T[0, 1]) == 0.0 and float(G[0, 1]) == 0.0 and float(T[0, 2].abs()) > 0 and float(T[1, 2].abs()) > 0
        pair = torch.from_numpy(np.ascontiguousarray(raw.cpu().numpy()[:, :2])).cuda()
        tr2 = D.tracer(inputs, PC.pair_params(api), w["bn"][:2])
        try:
            tr2.set_detuning(domega=DC.shifts(3)[:2])
            tr2.set_bandwidth(*BC.lines("five"))
            f2, out = _all_four(torch, tr2, pair, w["gp"])
            assert bool((f2[0] > 0).any())
            for t in out:
                assert not bool(t.any())
        finally:
            tr2.close()
    finally:
        tr.close()


def test_swapped_shifts_negate_the_ordered_kernel_bit_for_bit(api, oracle, inputs, torch_cuda):
    """Two beams of CROSSING at right angles in still plasma under the three-line spectrum: swapping the two shifts negates the
    ordered kernel's K bit for bit (N -> -N, the brackets commute), the pair-once kernel's to the last bits; and
    I_i K_i + I_j K_j is a few ulp of its terms."""
    torch = torch_cuda
    w = PC.crossing_world(api, oracle, inputs)
    tr = D.tracer(inputs, PC.pair_params(api), w["bn"][[0, 1]])
    raw = torch.from_numpy(PC.pair_raw(w, (0, 1))).cuda()
    p = tr.params
    shift = DC.shifts(2)
    try:
        tr.set_flow(torch.zeros((3, p.nx, p.ny, p.nz), dtype=torch.float64, device="cuda"))
        tr.set_bandwidth(*BC.lines("three"))
        for pair_once in KERNELS:
            tr.set_detuning(domega=shift)
            f, k, _ = D.update(torch, tr, raw, w["gp"], pair_once, change=False)
            tr.set_detuning(domega=shift[::-1].copy())
            _, ks, _ = D.update(torch, tr, raw, w["gp"], pair_once, change=False)
            nf, K, Ks = f.cpu().numpy(), k.cpu().numpy(), ks.cpu().numpy()
            both = (nf[0, 0] > 0) & (nf[0, 1] > 0)
            assert both.sum() >= 100 and np.abs(K[0][both]).min() > 0
            cancel = np.abs(nf[0, 0] * K[0] + nf[0, 1] * K[1])[both] / (np.abs(nf[0, 0] * K[0]) + np.abs(nf[0, 1] * K[1]))[both]
            print("CROSSING (0, 1), still plasma, three lines, %s: I_i K_i + I_j K_j up to %.3e of its terms; max |K| %.3e"
                  % (KERNEL_IDS[pair_once], cancel.max(), np.abs(K).max()))
            assert cancel.max() <= 4 * 2.0 ** -53
            if pair_once:
                assert np.abs(Ks + K).max() <= LAST_BITS * np.abs(K).max()
            else:
                assert np.array_equal(Ks, -K)
    finally:
        tr.close()


# ---- 5. the solve ---------------------------------------------------------------------------------------------------------
def test_solve_loops_see_the_spectrum(api, inputs, torch_cuda):
    """tests/test_gpu_cbet.py's solve (32^3, six beams, relax 1, 12 passes) with three colours and three lines: the Python loop,
    the slab loop at one rank and the native loop with the tracer's context stay within 1e-12 of max |K| of one another, and
    each differs from its own solve without lines."""
    torch = torch_cuda
    tr = D.tracer(inputs, api.default_params(32, nbeams=len(W.BEAMS)), inputs[0][W.BEAMS])
    gp = api.default_gain_params(tolerance=1e-6, max_passes=12, relax=1.0)

    def solves():
        out = {}
        e = tr.new_grid()
        out["python"] = tr.cbet_solve(e, gp, fields=tr.new_fields())["gain"]
        e = tr.new_grid()
        out["slabs"] = tr.cbet_solve(e, gp, slabs=True)["gain"]
        e = tr.new_grid()
        ws = torch.zeros(api.cbet_workspace_bytes(tr.params) // 8 + 1, dtype=torch.float64, device="cuda")
        api.cbet_solve(tr.d_te, tr.d_r, tr.d_ne, e, tr.d_bbeam_norm, tr.d_beam_norm, tr.d_pow_r, tr.d_phase_r, tr.params, gp,
                       workspace=ws, ctx=tr.ctx, stream=D.stream(torch))
        torch.cuda.synchronize()
        n = tr.params.nbeams * e.numel()
        off = (api.cbet_workspace_gain(tr.params, ws) - ws.data_ptr()) // 8
        out["native"] = ws[off:off + n].view((tr.params.nbeams,) + tr.grid_shape).clone()
        return out

    def spread(s):
        names = list(s)
        return max(float((s[a] - s[b]).abs().max() / s[b].abs().max()) for i, a in enumerate(names) for b in names[i + 1:])

    try:
        tr.set_detuning(dlambda_angstrom=DC.three_colours(len(W.BEAMS)))
        tinted = solves()
        tr.set_bandwidth(*api.line_spectrum(tr.params, 6.0, 3))
        banded = solves()
        for loop in tinted:
            moved = float((banded[loop] - tinted[loop]).abs().max() / tinted[loop].abs().max())
            print("32^3 %s loop, three colours + three lines: gain moved by %.3e of max |K| from the solve without lines" % (loop, moved))
            assert moved > BC.MOVES
        free, held = spread(tinted), spread(banded)
        print("32^3: loops apart by %.3e of max |K| with lines, %.3e without" % (held, free))
        assert held <= 1e-12
    finally:
        tr.close()
