"""Polarization smoothing in the gain stage, the part that needs no device: the new entries of the C
ABI are exported, declared, bound and refuse bad arguments, the numpy reference of helpers/polarization_cases.py is tied to the
restatement the gain stage's tests already trust, and the polarized host twin of the exchange matrix agrees with that
reference, keeps the bits of the aligned twin with the mode off and gives the exact factors 1/4 and 1/2 on the CROSSING world
-- in Python, and as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer.

Bounds: helpers/gain_worlds.TOL (1e-9) of Gross_ij between the twin and the reference; what must be exact is asserted
bitwise.  Observed: 1.2e-14 of Gross_ij at the most (CROWDED with everything on; 2.8e-15 on TRACED), where Gross_ij of twin
and reference are themselves 1.2e-14 apart."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import NCPU, ROOT
from helpers import detuning_cases as DC
from helpers import exchange_cases as XC
from helpers import gain_worlds as W
from helpers import polarization_cases as PC
from helpers import twin_driver as TD
from helpers.gain_reference import Restatement
from helpers.gain_worlds import TOL

NAMES = ("cbet_context_set_polarization", "cbet_context_polarization", "cbet_exchange_matrix_host_polarized")
CSRC = os.path.join(ROOT, "cbet_raytracing_3d_amd", "csrc")


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


@pytest.fixture(scope="module")
def crossing(api, oracle, inputs):
    return PC.crossing_world(api, oracle, inputs)


def _error(api):
    return api.lib().cbet_last_error().decode()


def _twin(api, w, polarization="smoothed", shift=None, tabled=False, dn_max=0.0, **kw):
    return api.exchange_matrix_host(w["xfields"], w["ne3d"], w["p"], w["gp"], flow=w["shifted"] if tabled else None,
                                    state=w["state"] if tabled else None, dn_max=dn_max, shift=shift, polarization=polarization, **kw)


# ---- the reference is the trusted one with the factor off -----------------------------------------------------------------
def test_reference_with_the_factor_off_is_the_restatement_bit_for_bit(crowded, traced):
    """First: helpers/polarization_cases.update with smoothed=False returns Restatement.update's arrays."""
    for w, which in ((crowded, "plain"), (crowded, "tabled"), (traced, "restated")):
        R, raw = w[which], w["raw"]
        shift = DC.shifts(raw.shape[1]) if which == "tabled" else None
        half = PC.reference(w, "plain")["half"]
        want = R.update(raw, shift, limits=[0.0, half], amplitudes=True, matrix=True)
        got = PC.update(R, raw, shift, limits=[0.0, half], amplitudes=True, matrix=True, smoothed=False)
        assert sorted(got) == sorted(want)
        for key in want:
            assert np.array_equal(got[key], want[key]), (which, key)
        assert np.abs(want["K"][0]).max() > 0 and np.abs(want["T"][0]).max() > 0
    planes = PC.update(crowded["plain"], crowded["raw"], planes=(9, 14), matrix=True, smoothed=False)
    assert np.array_equal(planes["T"], crowded["plain"].update(crowded["raw"], planes=(9, 14), matrix=True)["T"])


def test_reference_factor_lies_between_a_quarter_and_a_half(crowded, traced):
    for name, w in (("TRACED", traced), ("CROWDED", crowded)):
        for config in PC.CONFIGS:
            ref = PC.reference(w, config)
            scale = float(np.abs(ref["Ka"]).max())
            moved = float(np.abs(ref["K"] - ref["Ka"]).max() / scale)
            print("%s %s: smoothing moves the reference's K by %.3e of max |K| = %.3e; max |K| smoothed %.3e; `half` = %.4e"
                  % (name, config, moved, scale, float(np.abs(ref["K"]).max()), ref["half"]))
            assert moved > 1e-2
            assert np.array_equal(ref["T"], -ref["T"].T)
            assert float(np.abs(ref["Khalf"] - ref["K"]).max() / scale) > 1e-3      # the limit acts on the smoothed gain


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_declared_and_bound(api):
    header = open(os.path.join(ROOT, "include", "cbet_mi355x.h")).read()
    for name in NAMES:
        assert ("int %s(" % name) in header
    assert "#define CBET_POL_ALIGNED 0" in header and "#define CBET_POL_SMOOTHED 1" in header
    assert (api.POL_ALIGNED, api.POL_SMOOTHED) == (0, 1) and api.POLARIZATIONS == ("aligned", "smoothed")
    assert callable(api.Context.set_polarization) and callable(api.Context.polarization)
    from cbet_raytracing_3d_amd.tracer import RayTracer
    assert callable(RayTracer.set_polarization) and callable(RayTracer.polarization)
    assert "polarization smoothing" in header and "BEFORE the saturation clamp" in header and "(e_i . e_j)^2" in header
    model = open(os.path.join(CSRC, "cbet_gain_model.h")).read()
    assert "pair_smoothing" in model and "BEFORE the clamp" in model


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "cbet_mi355x.h"\n'
                   "int use(cbet_context *c, int *m) { return cbet_context_set_polarization(c, CBET_POL_SMOOTHED) + cbet_context_polarization(c, m); }\n"
                   "int host(const double *f, const double *n, double *o, const cbet_params *p, const cbet_gain_params *g, const double *w)\n"
                   "{ return cbet_exchange_matrix_host_polarized(f, n, o, o, 0, 2, p, g, 0, 0, 0.05, w, CBET_POL_ALIGNED); }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "use.o")])


def test_setter_refuses_unknown_modes_and_a_null_context(api):
    """The mode is judged before the context: these refusals need no device."""
    L = api.lib()
    for mode in (-1, 2):
        assert L.cbet_context_set_polarization(None, mode) == api.EINVAL
        assert ("mode = %d" % mode) in _error(api) and "cbet_context_set_polarization" in _error(api)
    for mode in (api.POL_ALIGNED, api.POL_SMOOTHED):
        assert L.cbet_context_set_polarization(None, mode) == api.EINVAL
        assert "NULL context" in _error(api) and "cbet_context_set_polarization" in _error(api)
    out = C.c_int(7)
    assert L.cbet_context_polarization(None, C.byref(out)) == api.EINVAL and out.value == 7
    with pytest.raises(ValueError):
        api.polarization_mode("circular")
    assert api.polarization_mode("smoothed") == 1 and api.polarization_mode("aligned") == 0 and api.polarization_mode(1) == 1


def test_twin_refuses_an_unknown_mode(api, crowded):
    for mode in (-1, 2):
        with pytest.raises(api.CbetError) as ei:
            _twin(api, crowded, polarization=mode)
        assert ei.value.code == api.EINVAL and ("pol = %d" % mode) in str(ei.value)


# ---- the twin, aligned ----------------------------------------------------------------------------------------------------
def test_aligned_twin_is_the_shifted_twin_bit_for_bit(api, crowded):
    """pol = 0 through the new entry against cbet_exchange_matrix_host_shifted called as before: with and without shifts, and
    with a limit."""
    w = crowded
    nb = w["p"].nbeams
    half = DC.reference(w, False)["half"]
    shifts = np.ascontiguousarray(DC.shifts(nb))
    old = api.lib().cbet_exchange_matrix_host_shifted
    for tabled, dn, shift in ((False, 0.0, None), (False, 0.0, shifts), (False, half, None), (True, half, shifts)):
        out, gross = np.zeros((nb, nb)), np.zeros((nb, nb))
        assert old(api._addr(w["xfields"]), api._addr(np.ascontiguousarray(w["ne3d"])), api._addr(out), api._addr(gross), 0,
                   w["p"].nx + 2, C.byref(w["p"]), C.byref(w["gp"]),
                   api._addr(np.ascontiguousarray(w["shifted"])) if tabled else None,
                   api._addr(np.ascontiguousarray(w["state"])) if tabled else None, dn, api._addr(shift)) == api.OK
        assert np.abs(out).max() > 0
        for mode in ("aligned", api.POL_ALIGNED):
            got = _twin(api, w, polarization=mode, shift=shift, tabled=tabled, dn_max=dn)
            assert np.array_equal(got[0], out) and np.array_equal(got[1], gross), (tabled, dn, shift is None)


# ---- the twin, smoothed ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", ["none", "half"])
@pytest.mark.parametrize("config", list(PC.CONFIGS))
@pytest.mark.parametrize("grid", ["traced", "crowded"])
def test_smoothed_twin_against_the_restatement(api, traced, crowded, grid, config, limit):
    """`everything`: the offset target's flow table, the three-state table, sixty distinct shifts; `half`: a limit too."""
    w = traced if grid == "traced" else crowded
    ref = PC.reference(w, config)
    tabled = PC.CONFIGS[config][0] == "tabled"
    dn = 0.0 if limit == "none" else ref["half"]
    want, gross = (ref["T"], ref["G"]) if limit == "none" else (ref["Thalf"], ref["Ghalf"])
    T, G = _twin(api, w, shift=ref["shift"], tabled=tabled, dn_max=dn)
    err, gerr = XC.worst(T, want, gross), XC.worst(G, gross, gross)
    aligned, _ = _twin(api, w, polarization="aligned", shift=ref["shift"], tabled=tabled, dn_max=dn)
    moved = float((np.abs(T - aligned)[gross > 0] / gross[gross > 0]).max())
    print("%s %s %s: smoothed twin vs the restatement %.3e of Gross (Gross itself %.3e); smoothing moves T by up to %.3e of Gross"
          % (grid, config, limit, err, gerr, moved))
    assert err < TOL and gerr < TOL
    assert moved > 1e-2
    assert np.array_equal(T, -T.T) and not np.diag(T).any()
    assert np.array_equal(G, G.T) and (G >= np.abs(T)).all()
    rows = XC.row_sums(ref["R"], dict(I=ref["I"], K=ref["K"] if limit == "none" else ref["Khalf"]))
    assert float((np.abs(T.sum(axis=1) - rows) / G.sum(axis=1)).max()) < TOL


# ---- exact factors --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", sorted(PC.FACTOR))
def test_crossing_pairs_give_the_exact_factor(api, crossing, pair):
    """Beams at right angles: 0.25 x the aligned T and Gross, bit for bit; opposed beams: 0.5 x."""
    w = crossing
    p2 = PC.pair_params(api)
    R = Restatement(api, p2, w["gp"], w["ne3d"], api.flow_table(p2, w["gp"], None))
    fields, inten, k = XC.normalised(R, PC.pair_raw(w, pair))
    on = inten[0] > 0
    assert on.sum() == w["present"].sum() and np.array_equal(inten[0], inten[1])
    kmag = R.kmag[on]
    a, b = pair
    for beam, slot in ((a, 0), (b, 1)):                                     # k = +-kmag on one axis exactly
        axis, sign = int(np.nonzero(PC.DIRECTIONS[beam])[0][0]), PC.DIRECTIONS[beam].sum()
        assert np.array_equal(k[axis, slot][on], sign * kmag)
        assert not k[[c for c in range(3) if c != axis], slot].any()
    call = lambda mode: api.exchange_matrix_host(fields, w["ne3d"], p2, w["gp"], polarization=mode)      # noqa: E731
    (Ta, Ga), (Ts, Gs) = call("aligned"), call("smoothed")
    print("CROSSING %s: aligned T %.6e, Gross %.6e; smoothed / aligned %.17g" % (pair, Ta[0, 1], Ga[0, 1], Ts[0, 1] / Ta[0, 1]))
    assert abs(Ta[0, 1]) > 1e-200 and Ga[0, 1] > 1e-200                     # nonzero and far from the subnormal range
    assert np.array_equal(Ts, PC.FACTOR[pair] * Ta) and np.array_equal(Gs, PC.FACTOR[pair] * Ga)
    ref = PC.update(R, None, normalised=(inten, k), matrix=True)
    assert XC.worst(Ts, ref["T"][0], ref["G"][0]) < TOL


# ---- bounds and identities ------------------------------------------------------------------------------------------------
def test_bounds_antisymmetry_and_slabs_on_crowded(api, crowded):
    w = crowded
    Ta, Ga = _twin(api, w, polarization="aligned")
    Ts, Gs = _twin(api, w)
    live = Ga > 0
    assert live.sum() > 1000
    assert (Gs >= PC.LOW * Ga * (1.0 - PC.SLACK)).all() and (Gs <= PC.HIGH * Ga * (1.0 + PC.SLACK)).all()
    ratio = Gs[live] / Ga[live]
    print("CROWDED: Gross smoothed / aligned between %.6f and %.6f" % (ratio.min(), ratio.max()))
    assert ((ratio > PC.LOW * (1.0 + 1e-6)) & (ratio < PC.HIGH * (1.0 - 1e-6))).any()     # some element strictly inside
    assert np.array_equal(Gs[~live], Ga[~live])
    assert np.array_equal(Ts, -Ts.T) and not np.diag(Ts).any()
    nb = w["p"].nbeams
    out, gross = np.zeros((nb, nb)), np.zeros((nb, nb))
    for lo, hi in ((0, 9), (9, 14), (14, 15)):
        _twin(api, w, hx_lo=lo, hx_hi=hi, out=out, gross=gross)
    assert float((np.abs(out - Ts)[Gs > 0] / Gs[Gs > 0]).max()) < 1e-14
    assert float((np.abs(gross - Gs)[Gs > 0] / Gs[Gs > 0]).max()) < 1e-14


# ---- the twin as a stand-alone program under the sanitizers ---------------------------------------------------------------
DRIVER = TD.PRELUDE + r'''
// The cases of the polarized twin on one world of nb beams, every beam with |k| = kmag of its cell.
struct Polarized : World {
    explicit Polarized(int beams) : World(beams, true) {}
    void run(double *checksum)
    {
        auto twin = [&](double *t, double *gr, const double *fl, const double *st, double dn, const double *w, int pol, int lo, int hi) {
            std::memset(t, 0, m * sizeof(double)); std::memset(gr, 0, m * sizeof(double));
            REQUIRE(cbet_exchange_matrix_host_polarized(fields, ne3d, t, gr, lo, hi, &p, &g, fl, st, dn, w, pol) == CBET_OK, "%s", cbet_last_error());
        };
        for (int tables = 0; tables < 2; ++tables)
            for (double dn : {0.0, 1e-4})
                for (int shifted = 0; shifted < 2; ++shifted) {
                    const double *fl = tables ? flow : nullptr, *st = tables ? state : nullptr, *w = shifted ? shift : nullptr;
                    twin(T, G, fl, st, dn, w, CBET_POL_ALIGNED, 0, hx);       // aligned: the bits of the shifted twin
                    std::memset(T2, 0, m * sizeof(double)); std::memset(G2, 0, m * sizeof(double));
                    REQUIRE(cbet_exchange_matrix_host_shifted(fields, ne3d, T2, G2, 0, hx, &p, &g, fl, st, dn, w) == CBET_OK, "%s", cbet_last_error());
                    REQUIRE(same(T, T2, m) && same(G, G2, m), "pol = 0 is not the shifted twin (tables %d, dn_max %g, shifts %d)", tables, dn, shifted);
                    twin(T2, G2, fl, st, dn, w, CBET_POL_SMOOTHED, 0, hx);
                    for (int i = 0; i < nb; ++i)
                        for (int j = 0; j < nb; ++j) {
                            const double a = T2[i * nb + j], b = -T2[j * nb + i];
                            REQUIRE(same(&a, &b, 1) || (a == 0.0 && b == 0.0), "T[%d][%d] %a, T[%d][%d] %a", i, j, a, j, i, T2[j * nb + i]);
                            REQUIRE(G2[i * nb + j] >= std::fabs(T2[i * nb + j]), "Gross[%d][%d]", i, j);
                            if (dn == 0.0) {                                  // without a limit: 1/4 <= Gross smoothed / aligned <= 1/2
                                REQUIRE(G2[i * nb + j] >= 0.25 * G[i * nb + j] * (1.0 - 1e-12), "Gross[%d][%d] below a quarter", i, j);
                                REQUIRE(G2[i * nb + j] <= 0.5 * G[i * nb + j] * (1.0 + 1e-12), "Gross[%d][%d] above a half", i, j);
                            }
                            *checksum += T2[i * nb + j] + G2[i * nb + j];
                        }
                    if (nb >= 2) REQUIRE(T2[1] == 0.0 && G2[1] == 0.0, "parallel beams exchange %a", T2[1]);
                }
        twin(T2, G2, nullptr, nullptr, 0.0, shift, CBET_POL_SMOOTHED, 2, 2);   // an empty slab
        for (size_t k = 0; k < m; ++k) REQUIRE(T2[k] == 0.0, "an empty slab wrote entry %zu", k);
        twin(T, G, flow, state, 1e-4, shift, CBET_POL_SMOOTHED, 0, hx);        // slabs add up
        std::memset(T2, 0, m * sizeof(double)); std::memset(G2, 0, m * sizeof(double));
        for (int lo = 0; lo < hx; lo += 3)
            REQUIRE(cbet_exchange_matrix_host_polarized(fields, ne3d, T2, G2, lo, lo + 3 < hx ? lo + 3 : hx, &p, &g, flow, state, 1e-4, shift,
                                                        CBET_POL_SMOOTHED) == CBET_OK, "%s", cbet_last_error());
        for (size_t k = 0; k < m; ++k) REQUIRE(std::fabs(T2[k] - T[k]) <= 1e-13 * G[k], "slabs: entry %zu: %a against %a", k, T2[k], T[k]);
        for (int pol : {-1, 2}) {
            REQUIRE(cbet_exchange_matrix_host_polarized(fields, ne3d, T2, G2, 0, hx, &p, &g, nullptr, nullptr, 0.0, nullptr, pol) == CBET_EINVAL, "mode %d passed", pol);
            REQUIRE(std::strstr(cbet_last_error(), "pol = "), "%s", cbet_last_error());
        }
    }
};

int main()
{
    double checksum = 0.0;
    for (int nb : {1, 2, 7, 64}) Polarized(nb).run(&checksum);
    std::printf("polarized twin ok: checksum %.17g\n", checksum);
    return 0;
}
'''


def test_polarized_twin_is_clean_under_asan_ubsan(tmp_path):
    """The twin with the argument builder it shares with the kernels (cbet_exchange_host.cpp) and the host arithmetic
    (cbet_params.cpp) compiled with the sanitizers into a program of their own, no HIP library on the link line, over a small
    grid with and without tables, shifts and a limit; nothing is loaded into Python."""
    out = TD.run_driver(tmp_path, DRIVER)
    assert "polarized twin ok" in out and "checksum" in out
