"""Laser bandwidth in the gain stage, the part that needs no device: the new entries of the C ABI are
exported, declared, bound and refuse bad lines before they look at the context; the numpy reference of
helpers/bandwidth_cases.py is tied to the restatements the gain stage's tests already trust and meets the conditions asked of
it alone; the difference table is what the header says; the banded host twin agrees with the reference, keeps the bits of the
polarized twin without a spectrum, and keeps the model's identities -- in Python, and as a stand-alone program under
AddressSanitizer + UndefinedBehaviorSanitizer.

Bounds: helpers/gain_worlds.TOL (1e-9) of Gross_ij between the twin and the reference; 1e-12 of max |K| between the reference's
double sum and the weighted sum of the trusted restatement's K; what must be exact is asserted bitwise.  Observed: twin against
the reference 8.3e-15 of Gross_ij at the most (CROWDED, plain, `half`, smoothed; 3.9e-15 on TRACED), where Gross_ij of twin and
reference are themselves 1.3e-14 apart; the double sum against the weighted sum of Restatement.update 2.7e-15 of max |K|."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import NCPU, ROOT
from helpers import bandwidth_cases as BC
from helpers import detuning_cases as DC
from helpers import exchange_cases as XC
from helpers import gain_worlds as W
from helpers import polarization_cases as PC
from helpers import twin_driver as TD
from helpers.gain_reference import Restatement
from helpers.gain_worlds import TOL

NAMES = ("cbet_context_set_bandwidth", "cbet_context_bandwidth", "cbet_exchange_matrix_host_banded")
CSRC = os.path.join(ROOT, "cbet_raytracing_3d_amd", "csrc")
SPECTRA = list(BC.SPECTRA)
# |K - c_0 K0| / max |K0| of the reference with the offsets x NEAR_FAR = 3: not yet at FAR_SHARE; (low, high) around the
# recorded values x 0.8 .. x 1.2, so that a drift shows -- recorded: TRACED 1.247e-1 / 8.377e-2 / 3.233e-1 (three / five / eight),
# CROWDED 1.171e-1 / 9.605e-2 / 1.360e-1; at x 1000: 2.5e-10 at the most
NEAR_FAR_SHARE = {("traced", "three"): (1.0e-1, 1.5e-1), ("traced", "five"): (6.7e-2, 1.0e-1), ("traced", "eight"): (2.6e-1, 3.9e-1),
                  ("crowded", "three"): (9.4e-2, 1.4e-1), ("crowded", "five"): (7.7e-2, 1.15e-1), ("crowded", "eight"): (1.1e-1, 1.65e-1)}


@pytest.fixture(scope="module")
def api():
    from cbet_raytracing_3d_amd import api as a
    a.lib()
    return a


def _world(w, which):
    if "xfields" not in w:
        w["xfields"], w["xI"], w["xk"] = XC.normalised(w[which], w["raw"])
    return w


@pytest.fixture(scope="module")
def traced(api, oracle, inputs):
    return _world(W.traced_world(api, oracle, inputs, NCPU), "restated")


@pytest.fixture(scope="module")
def crowded(api, oracle, inputs):
    return _world(W.crowded_world(api, oracle, inputs, NCPU), "plain")


def _error(api):
    return api.lib().cbet_last_error().decode()


def _twin(api, w, lines=None, polarization="aligned", shift=None, tabled=False, dn_max=0.0, **kw):
    return api.exchange_matrix_host(w["xfields"], w["ne3d"], w["p"], w["gp"], flow=w["shifted"] if tabled else None,
                                    state=w["state"] if tabled else None, dn_max=dn_max, shift=shift, polarization=polarization,
                                    lines=lines, **kw)


def _table(api, name, factor=1.0):
    """The difference table of a spectrum, built here by the header's rule: (c_0, d[M], c[M]).  The library exports no reader
    of its own table; test_twin_runs_the_header_statement_on_its_table ties the two together bit for bit through the twin."""
    off, wts = BC.lines(name, factor)
    p = wts / wts.sum()
    c0, d, c = 0.0, [], []
    for a in range(p.size):
        c0 = c0 + p[a] * p[a]
    for a in range(p.size):
        for b in range(a + 1, p.size):
            diff, w = abs(off[b] - off[a]), p[a] * p[b]
            if diff == 0.0:
                c0 = c0 + (w + w)
            elif diff in d:
                c[d.index(diff)] = c[d.index(diff)] + w
            else:
                d.append(diff)
                c.append(w)
    order = sorted(range(len(d)), key=lambda m: d[m])
    return c0, np.array([d[m] for m in order]), np.array([c[m] for m in order])


# ---- the reference is the trusted one without lines -----------------------------------------------------------------------
def test_reference_without_lines_is_the_polarization_reference_bit_for_bit(crowded, traced):
    """First: helpers/bandwidth_cases.update with lines=None returns polarization_cases.update's arrays, smoothed and not."""
    for w, which in ((crowded, "plain"), (crowded, "tabled"), (traced, "restated")):
        R, raw = w[which], w["raw"]
        shift = DC.shifts(raw.shape[1]) if which == "tabled" else None
        half = PC.reference(w, "plain")["half"]
        for smoothed in (False, True):
            want = PC.update(R, raw, shift, limits=[0.0, half], amplitudes=True, matrix=True, smoothed=smoothed)
            got = BC.update(R, raw, shift, None, limits=[0.0, half], amplitudes=True, matrix=True, smoothed=smoothed)
            assert sorted(got) == sorted(want)
            for key in want:
                assert np.array_equal(got[key], want[key]), (which, smoothed, key)
            assert np.abs(want["K"][0]).max() > 0 and np.abs(want["T"][0]).max() > 0
    planes = BC.update(crowded["plain"], crowded["raw"], planes=(9, 14), matrix=True)
    assert np.array_equal(planes["T"], crowded["plain"].update(crowded["raw"], planes=(9, 14), matrix=True)["T"])


@pytest.mark.parametrize("spectrum", SPECTRA)
def test_reference_is_the_weighted_sum_of_the_trusted_restatement_on_two_beams(api, crowded, spectrum):
    """On two-beam subsets of CROWDED the unclamped K of the double sum equals sum_{a, b} p_a p_b Restatement.update(raw,
    shift + (0, o_b - o_a))["K"] to 1e-12 of max |K|."""
    w = crowded
    p2 = W.params(api, W.CROWDED, 2)
    R = Restatement(api, p2, w["gp"], w["ne3d"], w["flow"])
    off, wts = BC.lines(spectrum)
    p = wts / wts.sum()
    worst = 0.0
    for pair in ((0, 1), (7, 52), (33, 59)):
        raw = np.ascontiguousarray(w["raw"][:, list(pair)])
        shift = DC.shifts(60)[list(pair)]
        got = BC.update(R, raw, shift, (off, wts))["K"][0]
        want = np.zeros_like(got)
        for a in range(p.size):
            for b in range(p.size):
                want += p[a] * p[b] * R.update(raw, shift + np.array([0.0, off[b] - off[a]]))["K"][0]
        scale = float(np.abs(want).max())
        assert scale > 0
        worst = max(worst, float(np.abs(got - want).max() / scale))
    print("%s: the double sum against the weighted sum of Restatement.update on two-beam subsets: %.3e of max |K|" % (spectrum, worst))
    assert worst < 1e-12


# ---- conditions on the reference alone ------------------------------------------------------------------------------------
@pytest.mark.parametrize("spectrum", SPECTRA)
def test_reference_moves_with_every_spectrum(crowded, traced, spectrum):
    """With the sixty shifts on, each spectrum moves the reference's K by more than 1e-2 of the no-spectrum max |K|."""
    for name, w in (("TRACED", traced), ("CROWDED", crowded)):
        K, K0 = BC.light_reference(w, spectrum, 1.0)
        scale = float(np.abs(K0).max())
        moved = float(np.abs(K - K0).max() / scale)
        print("%s %s: the spectrum moves the reference's K by %.3e of the no-spectrum max |K| = %.3e" % (name, spectrum, moved, scale))
        assert moved > BC.MOVES


@pytest.mark.parametrize("spectrum", SPECTRA)
def test_reference_far_off_resonance_keeps_the_centre_term(crowded, traced, spectrum):
    """Offsets x 1000: K is c_0 x the no-spectrum K to 1e-4 of its max; at x 3 it is not yet (the recorded values)."""
    c0 = BC.centre_weight(spectrum)
    for name, w in (("traced", traced), ("crowded", crowded)):
        share = {}
        for factor in (BC.NEAR_FAR, BC.FAR):
            K, K0 = BC.light_reference(w, spectrum, factor)
            share[factor] = float(np.abs(K - c0 * K0).max() / np.abs(K0).max())
        print("%s %s: c_0 = %.6f; |K - c_0 K0| / max |K0| at offsets x %g: %.3e, x %g: %.3e"
              % (name, spectrum, c0, BC.NEAR_FAR, share[BC.NEAR_FAR], BC.FAR, share[BC.FAR]))
        assert share[BC.FAR] < BC.FAR_SHARE
        low, high = NEAR_FAR_SHARE[name, spectrum]
        assert low < share[BC.NEAR_FAR] < high


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_declared_and_bound(api):
    header = open(os.path.join(ROOT, "include", "cbet_mi355x.h")).read()
    for name in NAMES:
        assert ("int %s(" % name) in header
    assert "#define CBET_MAX_BAND_LINES 8" in header and api.MAX_BAND_LINES == 8
    assert callable(api.Context.set_bandwidth) and callable(api.Context.bandwidth) and callable(api.line_spectrum)
    from cbet_raytracing_3d_amd.tracer import RayTracer
    assert callable(RayTracer.set_bandwidth) and callable(RayTracer.bandwidth)
    for text in ("SUMMED pair gain", "per-beam spectra", "FM (SSD phase-modulated)", "no\n * per-line depletion"):
        assert text in header, text
    model = open(os.path.join(CSRC, "cbet_gain_model.h")).read()
    assert "pair_gain_band" in model and "SUMMED pair gain" in model


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "cbet_mi355x.h"\n'
                   "int use(cbet_context *c, double *o, double *w, int *n) { return cbet_context_set_bandwidth(c, o, w, CBET_MAX_BAND_LINES, 0)"
                   " + cbet_context_bandwidth(c, o, w, n); }\n"
                   "int host(const double *f, const double *n, double *o, const cbet_params *p, const cbet_gain_params *g, const double *w)\n"
                   "{ return cbet_exchange_matrix_host_banded(f, n, o, o, 0, 2, p, g, 0, 0, 0.05, w, CBET_POL_ALIGNED, w, w, 3); }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "use.o")])


def test_setter_refuses_bad_lines_before_it_looks_at_the_context(api):
    """The lines are judged before the context: these refusals need no device, and name the offence."""
    L = api.lib()
    off, wts = np.array([0.0, 1e12, 2e12]), np.array([1.0, 2.0, 1.0])

    def call(o, w, n):
        return L.cbet_context_set_bandwidth(None, api._addr(o), api._addr(w), n, None)

    for bad, text in ((np.nan, "line_domega[1] is NaN"), (np.inf, "line_domega[1] is infinite"), (-np.inf, "line_domega[1] is infinite")):
        o = off.copy()
        o[1] = bad
        assert call(o, wts, 3) == api.EINVAL
        assert text in _error(api) and "cbet_context_set_bandwidth" in _error(api)
    for bad in (0.0, -1.0, np.nan, np.inf):
        w = wts.copy()
        w[2] = bad
        assert call(off, w, 3) == api.EINVAL
        assert "line_weight[2]" in _error(api) and "not finite and > 0" in _error(api)
    assert call(off, wts, -1) == api.EINVAL and "nlines = -1" in _error(api)
    assert call(np.zeros(9), np.ones(9), 9) == api.EINVAL and "nlines = 9 exceeds CBET_MAX_BAND_LINES = 8" in _error(api)
    assert call(off, None, 3) == api.EINVAL and "line_weight is NULL" in _error(api)
    for o, w, n in ((off, wts, 3), (None, None, 0), (off, wts, 0)):           # good lines: then the context is asked for
        assert call(o, w, n) == api.EINVAL and "NULL context" in _error(api)
    n = C.c_int(7)
    assert L.cbet_context_bandwidth(None, None, None, C.byref(n)) == api.EINVAL and n.value == 7
    with pytest.raises(ValueError):
        api.line_arrays([0.0, 1.0], [1.0])


def test_twin_refuses_bad_lines(api, crowded):
    for lines, text in ((([0.0, np.nan], [1.0, 1.0]), "line_domega[1] is NaN"), (([0.0, 1e12], [1.0, -2.0]), "line_weight[1]"),
                        ((np.zeros(9), np.ones(9)), "nlines = 9")):
        with pytest.raises(api.CbetError) as ei:
            _twin(api, crowded, lines=lines)
        assert ei.value.code == api.EINVAL and text in str(ei.value) and "cbet_exchange_matrix_host_banded" in str(ei.value)


def test_line_spectrum_is_equally_spaced_and_exact(api, crowded):
    p = crowded["p"]
    off, wts = api.line_spectrum(p, 6.0, 5)
    assert np.array_equal(off, api.wavelength_shift_to_domega(p, np.array([3.0, 1.5, 0.0, -1.5, -3.0])))
    assert off[2] == 0.0 and (np.diff(off) > 0).all() and np.array_equal(wts, np.full(5, 0.2))
    assert abs(off[0] / -BC.SCALE - 1.0) < 0.02                               # +3 Angstrom is -4.6e12 rad/s
    first_order = -api.derive(p).omega * 3e-8 / (2.0 * np.pi * 29979245800.0 / api.derive(p).omega)
    assert 1e-4 < abs(off[0] / first_order - 1.0) < 2e-3                      # the exact form, not the first-order one (dl / l0 = 8.5e-4 apart)
    off, wts = api.line_spectrum(p, 6.0, 3, shape="gaussian")
    assert abs(wts.sum() - 1.0) < 1e-15 and abs(wts[0] / wts[1] - 0.5) < 1e-15 and wts[0] == wts[2]
    assert api.line_spectrum(p, 6.0, 1)[0].tolist() == [0.0]
    for bad in (dict(nlines=0), dict(nlines=9), dict(shape="lorentzian")):
        with pytest.raises(ValueError):
            api.line_spectrum(p, 6.0, **dict(dict(nlines=3), **bad))


# ---- the difference table -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spectrum", SPECTRA)
def test_difference_table_counts_weights_and_order(spectrum):
    """The table as the header states it: M = 3, 10 and 7 entries, c_0 + 2 sum c_m = 1 to 4 ulp, sorted by d."""
    c0, d, c = _table(None, spectrum)
    assert d.size == BC.ENTRIES[spectrum]
    assert (np.diff(d) > 0).all() and (d > 0).all() and (c > 0).all()
    total = c0 + 2.0 * float(c.sum())
    print("%s: M = %d, c_0 = %.17g, c_0 + 2 sum c_m - 1 = %.3e" % (spectrum, d.size, c0, total - 1.0))
    assert abs(total - 1.0) <= 4 * np.finfo(float).eps
    assert abs(c0 - BC.centre_weight(spectrum)) <= 4 * np.finfo(float).eps
    if spectrum == "eight":
        assert np.array_equal(d, BC.STEP * np.arange(1, 8))                   # the merge: 28 pairs, 7 exact multiples


@pytest.mark.parametrize("spectrum", SPECTRA)
def test_twin_runs_the_header_statement_on_its_table(api, crowded, spectrum):
    """The library's table is the header's: on a two-beam subset with ONE present cell the twin's T is, bit for bit,
    ((ds (pref S)) I_i) I_j with S = c_0 P(N / D), S = S + c_m (P((N + d_m) / D) + P((N - d_m) / D)) over the table built here
    by the header's rule -- order of the entries, merged weights and normalisation included."""
    w = crowded
    pair = (7, 52)
    p2 = W.params(api, W.CROWDED, 2)
    R = Restatement(api, p2, w["gp"], w["ne3d"], w["flow"])
    fields, inten, k = XC.normalised(R, np.ascontiguousarray(w["raw"][:, list(pair)]))
    both = np.nonzero((inten[0] > 0) & (inten[1] > 0))[0]
    assert both.size > 20
    shift = DC.shifts(60)[list(pair)]
    c0, d, c = _table(api, spectrum)
    iaw2 = R.iaw2

    def P(eta):
        e2 = eta * eta
        return iaw2 * eta / ((e2 - 1.0) * (e2 - 1.0) + iaw2 * e2)

    checked = 0
    for cell in both[::7]:
        one = np.zeros_like(fields).reshape(4, 2, -1)
        one[:, :, cell] = fields.reshape(4, 2, -1)[:, :, cell]
        T, _ = api.exchange_matrix_host(one.reshape(fields.shape), w["ne3d"], p2, w["gp"], shift=shift, lines=BC.lines(spectrum))
        q = k[:, 1, cell] - k[:, 0, cell]
        kiaw = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
        N = (0.0 - (q[0] * R.u[0][cell] + q[1] * R.u[1][cell] + q[2] * R.u[2][cell])) + (shift[1] - shift[0])
        D = kiaw * R.cs[cell] + 1e-10
        S = c0 * P(N / D)
        for m in range(d.size):
            S = S + c[m] * (P((N + d[m]) / D) + P((N - d[m]) / D))
        want = ((R.ds[cell] * (R.pref[cell] * S)) * inten[0, cell]) * inten[1, cell]
        assert T[0, 1] == want and T[1, 0] == -want and want != 0.0, (spectrum, cell, T[0, 1], want)
        checked += 1
    assert checked >= 3


# ---- the twin without a spectrum ------------------------------------------------------------------------------------------
def test_twin_without_a_spectrum_is_the_polarized_twin_bit_for_bit(api, crowded):
    """No lines, one line, equal offsets: the bits of cbet_exchange_matrix_host_polarized called as before."""
    w = crowded
    nb = w["p"].nbeams
    half = DC.reference(w, False)["half"]
    shifts = np.ascontiguousarray(DC.shifts(nb))
    old = api.lib().cbet_exchange_matrix_host_polarized
    none = (None, ([1.3e12], [2.0]), ([4e11, 4e11, 4e11], [1.0, 2.0, 3.0]), ([], []))
    for tabled, dn, shift, pol in ((False, 0.0, None, 0), (False, 0.0, shifts, 1), (True, half, shifts, 0), (True, half, None, 1)):
        out, gross = np.zeros((nb, nb)), np.zeros((nb, nb))
        assert old(api._addr(w["xfields"]), api._addr(np.ascontiguousarray(w["ne3d"])), api._addr(out), api._addr(gross), 0,
                   w["p"].nx + 2, C.byref(w["p"]), C.byref(w["gp"]),
                   api._addr(np.ascontiguousarray(w["shifted"])) if tabled else None,
                   api._addr(np.ascontiguousarray(w["state"])) if tabled else None, dn, api._addr(shift), pol) == api.OK
        assert np.abs(out).max() > 0
        for lines in none:
            got = _twin(api, w, lines=lines, polarization=pol, shift=shift, tabled=tabled, dn_max=dn)
            assert np.array_equal(got[0], out) and np.array_equal(got[1], gross), (tabled, dn, shift is None, pol, lines)


# ---- the banded twin against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("smoothed", [False, True], ids=["aligned", "smoothed"])
@pytest.mark.parametrize("limit", ["none", "half"])
@pytest.mark.parametrize("tables", ["none", "tabled"], ids=["plain", "tabled"])
@pytest.mark.parametrize("grid", ["traced", "crowded"])
def test_banded_twin_against_the_restatement(api, traced, crowded, grid, tables, limit, smoothed):
    """The five-line spectrum (M = 10) with the sixty shifts on."""
    w = traced if grid == "traced" else crowded
    ref = BC.reference(w, tables, "five", smoothed=smoothed)
    dn = 0.0 if limit == "none" else ref["half"]
    want, gross = (ref["T"], ref["G"]) if limit == "none" else (ref["Thalf"], ref["Ghalf"])
    pol = "smoothed" if smoothed else "aligned"
    T, G = _twin(api, w, lines=ref["lines"], polarization=pol, shift=ref["shift"], tabled=tables == "tabled", dn_max=dn)
    err, gerr = XC.worst(T, want, gross), XC.worst(G, gross, gross)
    mono, _ = _twin(api, w, polarization=pol, shift=ref["shift"], tabled=tables == "tabled", dn_max=dn)
    moved = float((np.abs(T - mono)[gross > 0] / gross[gross > 0]).max())
    print("%s %s %s %s: banded twin vs the restatement %.3e of Gross (Gross itself %.3e); the spectrum moves T by up to %.3e of Gross"
          % (grid, tables, limit, pol, err, gerr, moved))
    assert err < TOL and gerr < TOL
    assert moved > 1e-2
    assert np.array_equal(T, -T.T) and not np.diag(T).any()
    assert np.array_equal(G, G.T) and (G >= np.abs(T)).all()
    rows = XC.row_sums(ref["R"], dict(I=ref["I"], K=ref["K"] if limit == "none" else ref["Khalf"]))
    assert float((np.abs(T.sum(axis=1) - rows) / G.sum(axis=1)).max()) < TOL


@pytest.mark.parametrize("spectrum", ["three", "eight"])
def test_other_spectra_against_the_restatement(api, crowded, spectrum):
    """Three lines (M = 3) and eight lines on a 2^40 grid (M = 7, merged) on CROWDED, tabled, smoothed, under `half`."""
    w = crowded
    ref = BC.reference(w, "tabled", spectrum, smoothed=True)
    T, G = _twin(api, w, lines=ref["lines"], polarization="smoothed", shift=ref["shift"], tabled=True, dn_max=ref["half"])
    err, gerr = XC.worst(T, ref["Thalf"], ref["Ghalf"]), XC.worst(G, ref["Ghalf"], ref["Ghalf"])
    print("crowded tabled half smoothed %s: banded twin vs the restatement %.3e of Gross (Gross itself %.3e)" % (spectrum, err, gerr))
    assert err < TOL and gerr < TOL and np.array_equal(T, -T.T)


# ---- identities -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spectrum", SPECTRA)
def test_still_plasma_without_shifts_exchanges_exactly_nothing(api, crowded, spectrum):
    """A zero flow table and no shifts: N = 0, every bracket is P(d / D) + P(-(d / D)) = 0: T and Gross are exact zeros."""
    w = crowded
    still = np.zeros_like(w["flow"])
    for state in (None, w["state"]):
        T, G = api.exchange_matrix_host(w["xfields"], w["ne3d"], w["p"], w["gp"], flow=still, state=state, lines=BC.lines(spectrum))
        assert not T.any() and not G.any()
    T, _ = api.exchange_matrix_host(w["xfields"], w["ne3d"], w["p"], w["gp"], flow=still, lines=BC.lines(spectrum),
                                    shift=DC.shifts(60))
    assert np.abs(T).max() > 0                                                # ... and detuning creates a resonance to smear


@pytest.mark.parametrize("spectrum", SPECTRA)
def test_negated_shifts_negate_the_still_plasma_matrix_bit_for_bit(api, crowded, spectrum):
    """In still plasma N = w_j - w_i: negated shifts negate N exactly, and with it T, with and without a limit; Gross keeps
    its bits."""
    w = crowded
    still = np.zeros_like(w["flow"])
    shift = DC.shifts(60)
    half = DC.reference(w, False)["half"]
    for dn in (0.0, half):
        for pol in ("aligned", "smoothed"):
            call = lambda s: api.exchange_matrix_host(w["xfields"], w["ne3d"], w["p"], w["gp"], flow=still, shift=s, dn_max=dn,   # noqa: E731
                                                      polarization=pol, lines=BC.lines(spectrum))
            (Tp, Gp), (Tm, Gm) = call(shift), call(-shift)
            assert np.abs(Tp).max() > 0
            assert np.array_equal(Tm, -Tp) and np.array_equal(Gm, Gp), (dn, pol)


@pytest.mark.parametrize("spectrum", SPECTRA)
def test_far_off_resonance_the_twin_keeps_the_centre_term(api, crowded, spectrum):
    """Offsets x 1000: T is c_0 x the twin's T without a spectrum to FAR_SHARE of Gross_ij -- 1/L for L equal lines."""
    w = crowded
    shift = DC.shifts(60)
    T0, G0 = _twin(api, w, shift=shift)
    T, _ = _twin(api, w, lines=BC.lines(spectrum, BC.FAR), shift=shift)
    c0 = BC.centre_weight(spectrum)
    share = XC.worst(T, c0 * T0, G0)
    print("%s, offsets x %g: |T - c_0 T0| up to %.3e of Gross_ij (c_0 = %.6f)" % (spectrum, BC.FAR, share, c0))
    assert share < BC.FAR_SHARE
    flat = ([BC.SCALE * BC.FAR * a for a in range(4)], [2.0, 2.0, 2.0, 2.0])
    Tf, _ = _twin(api, w, lines=flat, shift=shift)
    assert XC.worst(Tf, 0.25 * T0, G0) < BC.FAR_SHARE


def test_slabs_add_up_on_crowded(api, crowded):
    w = crowded
    ln, shift = BC.lines("five"), DC.shifts(60)
    T, G = _twin(api, w, lines=ln, shift=shift)
    nb = w["p"].nbeams
    out, gross = np.zeros((nb, nb)), np.zeros((nb, nb))
    for lo, hi in ((0, 9), (9, 14), (14, 15)):
        _twin(api, w, lines=ln, shift=shift, hx_lo=lo, hx_hi=hi, out=out, gross=gross)
    assert float((np.abs(out - T)[G > 0] / G[G > 0]).max()) < 1e-14
    assert float((np.abs(gross - G)[G > 0] / G[G > 0]).max()) < 1e-14


# ---- the twin as a stand-alone program under the sanitizers ---------------------------------------------------------------
DRIVER = TD.PRELUDE + r'''
// The cases of the banded twin on one world of nb beams, every beam with |k| = kmag of its cell, and nl lines.
struct Banded : World {
    explicit Banded(int beams) : World(beams, true) {}
    void run(int nl, double *checksum)
    {
        double *off = block(nl), *wts = block(nl);
        for (int a = 0; a < nl; ++a) { off[a] = 1099511627776.0 * (a - 0.5 * (nl - 1)); wts[a] = 1.0 + (a % 3); }   // a 2^40 grid: differences merge
        auto twin = [&](double *t, double *gr, const double *fl, const double *st, double dn, const double *w, int pol, int lines, int lo, int hi) {
            std::memset(t, 0, m * sizeof(double)); std::memset(gr, 0, m * sizeof(double));
            REQUIRE(cbet_exchange_matrix_host_banded(fields, ne3d, t, gr, lo, hi, &p, &g, fl, st, dn, w, pol, off, wts, lines) == CBET_OK, "%s", cbet_last_error());
        };
        for (int tables = 0; tables < 2; ++tables)
            for (double dn : {0.0, 1e-4})
                for (int shifted = 0; shifted < 2; ++shifted)
                    for (int pol : {CBET_POL_ALIGNED, CBET_POL_SMOOTHED}) {
                        const double *fl = tables ? flow : nullptr, *st = tables ? state : nullptr, *w = shifted ? shift : nullptr;
                        twin(T, G, fl, st, dn, w, pol, 0, 0, hx);             // no lines: the bits of the polarized twin
                        std::memset(T2, 0, m * sizeof(double)); std::memset(G2, 0, m * sizeof(double));
                        REQUIRE(cbet_exchange_matrix_host_polarized(fields, ne3d, T2, G2, 0, hx, &p, &g, fl, st, dn, w, pol) == CBET_OK, "%s", cbet_last_error());
                        REQUIRE(same(T, T2, m) && same(G, G2, m), "no lines is not the polarized twin (tables %d, dn_max %g, shifts %d, pol %d)", tables, dn, shifted, pol);
                        twin(T2, G2, fl, st, dn, w, pol, nl, 0, hx);
                        if (nl == 1) REQUIRE(same(T, T2, m) && same(G, G2, m), "one line is not the polarized twin");
                        for (int i = 0; i < nb; ++i)
                            for (int j = 0; j < nb; ++j) {
                                const double a = T2[i * nb + j], b = -T2[j * nb + i];
                                REQUIRE(same(&a, &b, 1) || (a == 0.0 && b == 0.0), "T[%d][%d] %a, T[%d][%d] %a", i, j, a, j, i, T2[j * nb + i]);
                                REQUIRE(G2[i * nb + j] >= std::fabs(T2[i * nb + j]), "Gross[%d][%d]", i, j);
                                *checksum += T2[i * nb + j] + G2[i * nb + j];
                            }
                        if (nb >= 2) REQUIRE(T2[1] == 0.0 && G2[1] == 0.0, "parallel beams exchange %a", T2[1]);
                    }
        twin(T2, G2, still, nullptr, 0.0, nullptr, CBET_POL_ALIGNED, nl, 0, hx);   // still plasma, no shifts: exact zeros
        for (size_t k = 0; k < m; ++k) REQUIRE(T2[k] == 0.0 && G2[k] == 0.0, "still plasma exchanges %a at entry %zu", T2[k], k);
        twin(T, G, still, state, 1e-4, shift, CBET_POL_SMOOTHED, nl, 0, hx);       // still plasma: negated shifts negate T
        twin(T2, G2, still, state, 1e-4, minus, CBET_POL_SMOOTHED, nl, 0, hx);
        for (size_t k = 0; k < m; ++k) { const double a = -T2[k]; REQUIRE((same(&a, &T[k], 1) || (a == 0.0 && T[k] == 0.0)) && same(&G2[k], &G[k], 1), "negated shifts: entry %zu", k); }
        twin(T2, G2, nullptr, nullptr, 0.0, shift, CBET_POL_SMOOTHED, nl, 2, 2);   // an empty slab
        for (size_t k = 0; k < m; ++k) REQUIRE(T2[k] == 0.0, "an empty slab wrote entry %zu", k);
        twin(T, G, flow, state, 1e-4, shift, CBET_POL_SMOOTHED, nl, 0, hx);        // slabs add up
        std::memset(T2, 0, m * sizeof(double)); std::memset(G2, 0, m * sizeof(double));
        for (int lo = 0; lo < hx; lo += 3)
            REQUIRE(cbet_exchange_matrix_host_banded(fields, ne3d, T2, G2, lo, lo + 3 < hx ? lo + 3 : hx, &p, &g, flow, state, 1e-4, shift,
                                                     CBET_POL_SMOOTHED, off, wts, nl) == CBET_OK, "%s", cbet_last_error());
        for (size_t k = 0; k < m; ++k) REQUIRE(std::fabs(T2[k] - T[k]) <= 1e-13 * G[k], "slabs: entry %zu: %a against %a", k, T2[k], T[k]);
        if (nl >= 2) {                                                              // a NaN offset, a bad weight, too many lines
            const double keep = off[nl - 1], wkeep = wts[0];
            off[nl - 1] = std::numeric_limits<double>::quiet_NaN();
            REQUIRE(cbet_exchange_matrix_host_banded(fields, ne3d, T2, G2, 0, hx, &p, &g, nullptr, nullptr, 0.0, nullptr, 0, off, wts, nl) == CBET_EINVAL, "a NaN offset passed");
            REQUIRE(std::strstr(cbet_last_error(), "is NaN"), "%s", cbet_last_error());
            off[nl - 1] = keep; wts[0] = 0.0;
            REQUIRE(cbet_exchange_matrix_host_banded(fields, ne3d, T2, G2, 0, hx, &p, &g, nullptr, nullptr, 0.0, nullptr, 0, off, wts, nl) == CBET_EINVAL, "a zero weight passed");
            wts[0] = wkeep;
        }
        REQUIRE(cbet_exchange_matrix_host_banded(fields, ne3d, T2, G2, 0, hx, &p, &g, nullptr, nullptr, 0.0, nullptr, 0, off, wts, CBET_MAX_BAND_LINES + 1) == CBET_EINVAL, "nine lines passed");
        std::free(off); std::free(wts);
    }
};

int main()
{
    double checksum = 0.0;
    for (int nb : {1, 2, 7, 64})
        for (int nl : {1, 2, 8}) Banded(nb).run(nl, &checksum);
    std::printf("banded twin ok: checksum %.17g\n", checksum);
    return 0;
}
'''


def test_banded_twin_is_clean_under_asan_ubsan(tmp_path):
    """The twin with the argument builder and the table builder it shares with the kernels and the context
    (cbet_exchange_host.cpp) and the host arithmetic (cbet_params.cpp) compiled with the sanitizers into a program of their
    own, no HIP library on the link line: 1, 2, 7 and 64 beams x 1, 2 and 8 lines, heap blocks of exactly their size, a parallel
    pair, a NaN offset; nothing is loaded into Python."""
    out = TD.run_driver(tmp_path, DRIVER)
    assert "banded twin ok" in out and "checksum" in out
