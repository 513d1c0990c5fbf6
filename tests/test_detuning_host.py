"""Wavelength detuning in the gain stage, the part that needs no device: the new entries of the C ABI
are exported, declared and refuse bad arguments, the wavelength conversion is the exact one, the CPU reference of
tests/test_gpu_detuning.py (helpers/gain_reference.py with the shifts of helpers/detuning_cases.py) meets the conditions asked of it alone, and the shifted host twin of
the exchange matrix agrees with that reference and keeps its exact identities -- in Python, and as a stand-alone program
under AddressSanitizer + UndefinedBehaviorSanitizer.

Bounds: 1e-12 of Gross_ij between the twin and the reference, tests/test_exchange_host.py's for the unshifted twin; what must
be exact is asserted bitwise."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import NCPU, ROOT
from helpers import detuning_cases as DC
from helpers import exchange_cases as XC
from helpers import gain_worlds as W
from helpers import saturation_cases as SC
from helpers import twin_driver as TD
from helpers.gain_worlds import LAST_BITS         # here of Gross_ij: tests/test_exchange_host.py's bound

NAMES = ("cbet_context_set_detuning", "cbet_context_detuning", "cbet_exchange_matrix_host_shifted")
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


def _error(api):
    return api.lib().cbet_last_error().decode()


def _twin(api, w, shift=None, tabled=False, dn_max=0.0, flow=None, **kw):
    if flow is None and tabled:
        flow = w["shifted"]
    return api.exchange_matrix_host(w["xfields"], w["ne3d"], w["p"], w["gp"], flow=flow, state=w["state"] if tabled else None,
                                    dn_max=dn_max, shift=shift, **kw)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_declared_and_bound(api):
    header = open(os.path.join(ROOT, "include", "cbet_mi355x.h")).read()
    for name in NAMES:
        assert ("int %s(" % name) in header
    assert callable(api.Context.set_detuning) and callable(api.Context.detuning) and callable(api.wavelength_shift_to_domega)
    from cbet_raytracing_3d_amd.tracer import RayTracer
    assert callable(RayTracer.set_detuning) and callable(RayTracer.detuning)
    assert "wavelength detuning" in header and "Manley-Rowe" in header and "not capturable" in header
    model = open(os.path.join(CSRC, "cbet_gain_model.h")).read()
    assert "Manley-Rowe" in model and "nominal wavelength" in model


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "cbet_mi355x.h"\n'
                   "int use(cbet_context *c, const double *w, double *o, int *n) { return cbet_context_set_detuning(c, w, 60, 0) + cbet_context_detuning(c, o, n); }\n"
                   "int host(const double *f, const double *n, double *o, const cbet_params *p, const cbet_gain_params *g, const double *w)\n"
                   "{ return cbet_exchange_matrix_host_shifted(f, n, o, o, 0, 2, p, g, 0, 0, 0.05, w); }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "use.o")])


@pytest.mark.parametrize("value, word", [(math.nan, "NaN"), (math.inf, "infinite"), (-math.inf, "infinite")])
def test_setter_refuses_bad_shifts_and_names_the_offence(api, value, word):
    """The values are judged before the context: the refusal does not need a device."""
    w = np.zeros(60)
    w[41] = value
    assert api.lib().cbet_context_set_detuning(None, w.ctypes.data, 60, None) == api.EINVAL
    assert word in _error(api) and "domega[41]" in _error(api)


def test_setter_refuses_bad_counts_and_a_null_context(api):
    w = DC.shifts(60)
    big = np.zeros(65)
    assert api.lib().cbet_context_set_detuning(None, big.ctypes.data, 65, None) == api.EINVAL
    assert "nbeams = 65" in _error(api) and "CBET_MAX_CBET_BEAMS" in _error(api)
    assert api.lib().cbet_context_set_detuning(None, w.ctypes.data, 0, None) == api.EINVAL and "nbeams = 0" in _error(api)
    assert api.lib().cbet_context_set_detuning(None, w.ctypes.data, 60, None) == api.EINVAL and "NULL context" in _error(api)
    assert api.lib().cbet_context_set_detuning(None, None, 0, None) == api.EINVAL and "NULL context" in _error(api)
    out, n = np.full(64, 7.0), C.c_int(5)
    assert api.lib().cbet_context_detuning(None, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n)) == api.EINVAL
    assert n.value == 5 and (out == 7.0).all()


def test_twin_refuses_a_shift_that_is_not_finite(api, crowded):
    w = DC.shifts(60)
    w[13] = math.nan
    with pytest.raises(api.CbetError) as ei:
        _twin(api, crowded, shift=w)
    assert ei.value.code == api.EINVAL and "shift[13]" in str(ei.value)
    with pytest.raises(ValueError):
        _twin(api, crowded, shift=np.zeros(59))


# ---- the conversion -------------------------------------------------------------------------------------------------------
def test_wavelength_conversion_is_the_exact_one(api):
    p = api.default_params(64)
    omega = api.derive(p).omega
    c = 29979245800.0
    lam0 = 2.0 * math.pi * c / omega
    assert abs(lam0 - 351e-7) < 1e-9                                        # 351 nm
    dl = np.array([-3.0, 0.0, 3.0, 0.5, -10.0, 40.0])
    got = api.wavelength_shift_to_domega(p, dl)
    want = np.array([float(np.longdouble(2.0) * np.longdouble(math.pi) * c / (np.longdouble(lam0) + np.longdouble(d) * 1e-8)
                           - np.longdouble(omega)) for d in dl])
    first_order = -omega * dl * 1e-8 / lam0
    print("d omega for %s Angstrom: %s rad/s; against 2 pi c / lambda %.3e rad/s; the first-order form is off by %.3e"
          % (dl.tolist(), got.tolist(), np.abs(got - want).max(), np.abs(first_order - want).max()))
    # omega' - omega cancels eleven bits of omega' = 5.4e15 (ulp 1 rad/s): a few rad/s, 1e-12 of the shifts the tests use
    assert np.abs(got - want).max() <= 4.0
    assert got[1] == 0.0 and got[2] < 0.0 < got[0]                          # red is down
    assert abs(got[0] / DC.SCALE - 1.0) < 0.01                              # +-3 Angstrom is the scale of the tests' shifts
    assert np.abs(first_order - want).max() > 1e6 * np.abs(got - want).max()
    assert api.wavelength_shift_to_domega(p, 3.0) == got[2]                 # a scalar


# ---- conditions on the reference alone ------------------------------------------------------------------------------------
def test_shifts_are_distinct_and_move_the_reference(traced, crowded):
    w = DC.shifts(60)
    assert np.unique(w).size == 60 and np.abs(w).max() <= DC.SCALE and abs(w.sum()) < 1e-3
    for name, world in (("TRACED", traced), ("CROWDED", crowded)):
        for tabled in ("none", "three", "tabled"):
            ref = DC.reference(world, tabled)
            scale = float(np.abs(ref["K0"]).max())
            moved = float(np.abs(ref["K"] - ref["K0"]).max() / scale)
            print("%s%s: the shifts (scale %.2e rad/s) move the reference's K by %.3e of max |K| = %.3e; `half` = %.4e"
                  % (name, "" if tabled == "none" else " " + tabled, DC.SCALE, moved, scale, ref["half"]))
            assert moved > DC.MOVES
            assert float(np.abs(ref["Khalf"] - ref["K"]).max() / scale) > 1e-3          # the limit acts on the shifted gain


def test_reference_without_shifts_is_the_saturation_tests_reference(crowded):
    R = crowded["plain"]
    again = R.update(crowded["raw"])
    assert np.array_equal(again["K"][0], SC.reference(crowded, "plain")["K0"])
    equal = R.update(crowded["raw"], np.full(60, 1.7e12))
    assert np.array_equal(equal["K"][0], again["K"][0])                     # only differences enter


def test_far_off_resonance_the_reference_has_no_gain(traced, crowded):
    """helpers/detuning_cases.py on the scale: 1000 x the tests' shifts; at 100 x the reference is not below the bound yet and
    keeps its recorded share."""
    for name, world in (("TRACED", traced), ("CROWDED", crowded)):
        near = DC.reference(world, False, DC.NEAR_FAR)
        ref = DC.reference(world, False, DC.FAR)
        scale = np.abs(ref["K0"]).max()
        share = float(np.abs(ref["K"]).max() / scale)
        print("%s: shifts of %.1e rad/s leave max |K| = %.3e of the unshifted; of %.1e rad/s: %.3e"
              % (name, DC.FAR, share, DC.NEAR_FAR, float(np.abs(near["K"]).max() / scale)))
        assert share < DC.FAR_SHARE
        assert float(np.abs(near["K"]).max() / scale) < DC.NEAR_FAR_SHARE[name.lower()]


def test_reference_exchange_cancels_and_red_gains(crowded):
    ref = DC.reference(crowded, False)
    exch, bound = np.abs((ref["I"] * ref["K"]).sum(axis=0)).max(), np.abs(ref["I"] * ref["K"]).sum(axis=0).max()
    assert exch <= 1e-11 * bound
    assert np.array_equal(ref["T"], -ref["T"].T)


# ---- the shifted twin -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", ["none", "half"])
@pytest.mark.parametrize("tabled", [False, True], ids=["plain", "tabled"])
@pytest.mark.parametrize("grid", ["traced", "crowded"])
def test_shifted_twin_against_the_restatement(api, traced, crowded, grid, tabled, limit):
    w = traced if grid == "traced" else crowded
    ref = DC.reference(w, tabled)
    dn = 0.0 if limit == "none" else ref["half"]
    want, gross = (ref["T"], ref["G"]) if limit == "none" else (ref["Thalf"], ref["Ghalf"])
    T, G = _twin(api, w, shift=ref["shift"], tabled=tabled, dn_max=dn)
    err, gerr = XC.worst(T, want, gross), XC.worst(G, gross, gross)
    plain, _ = _twin(api, w, tabled=tabled, dn_max=dn)
    moved = float((np.abs(T - plain)[gross > 0] / gross[gross > 0]).max())
    print("%s %s %s: shifted twin vs the restatement %.3e of Gross (Gross itself %.3e); the shifts move T by up to %.3e of Gross"
          % (grid, "tabled" if tabled else "plain", limit, err, gerr, moved))
    assert err < LAST_BITS and gerr < LAST_BITS
    assert moved > 1e-2
    assert np.array_equal(T, -T.T) and not np.diag(T).any()                 # antisymmetric
    assert np.array_equal(G, G.T) and (G >= np.abs(T)).all()
    rows = XC.row_sums(w[DC.restatement_key(w, tabled)], dict(I=ref["I"], K=ref["K"] if limit == "none" else ref["Khalf"]))
    assert float((np.abs(T.sum(axis=1) - rows) / G.sum(axis=1)).max()) < LAST_BITS


def test_equal_shifts_are_no_shifts_bit_for_bit(api, traced, crowded):
    for w in (traced, crowded):
        nb = w["p"].nbeams
        half = DC.reference(w, False)["half"]
        for tabled, dn in ((False, 0.0), (True, 0.0), (False, half)):
            none = _twin(api, w, tabled=tabled, dn_max=dn)
            old = api.lib().cbet_exchange_matrix_host                        # the entry that keeps its signature
            out, gross = np.zeros((nb, nb)), np.zeros((nb, nb))
            assert old(api._addr(w["xfields"]), api._addr(np.ascontiguousarray(w["ne3d"])), api._addr(out), api._addr(gross), 0,
                       w["p"].nx + 2, C.byref(w["p"]), C.byref(w["gp"]),
                       api._addr(np.ascontiguousarray(w["shifted"])) if tabled else None,
                       api._addr(np.ascontiguousarray(w["state"])) if tabled else None, dn) == api.OK
            assert np.array_equal(out, none[0]) and np.array_equal(gross, none[1])
            for value in (4.6e12, -1.25e11, 0.0):
                got = _twin(api, w, shift=np.full(nb, value), tabled=tabled, dn_max=dn)
                assert np.array_equal(got[0], none[0]) and np.array_equal(got[1], none[1]), (tabled, dn, value)


def test_negated_shifts_in_still_plasma_negate_the_matrix_bit_for_bit(api, traced, crowded):
    for w in (traced, crowded):
        p = w["p"]
        still = np.zeros((3, p.nx, p.ny, p.nz))
        shift = DC.shifts(p.nbeams)
        for dn in (0.0, DC.reference(w, False)["half"]):
            a = _twin(api, w, shift=shift, flow=still, dn_max=dn)
            b = _twin(api, w, shift=-shift, flow=still, dn_max=dn)
            assert np.abs(a[0]).max() > 0
            assert np.array_equal(b[0], -a[0]) and np.array_equal(b[1], a[1])
            zero = _twin(api, w, flow=still, dn_max=dn)                      # no flow, one colour: nothing is exchanged
            assert not zero[0].any() and not zero[1].any()
        red = int(np.argmin(shift))                                          # the reddest beam gains from everyone it meets
        T, G = _twin(api, w, shift=shift, flow=still)
        met = G[red] > 0
        assert met.sum() >= 1 and (T[red][met] > 0).all()


def test_slabs_of_the_shifted_twin_add_up(api, crowded):
    ref = DC.reference(crowded, False)
    T, G = _twin(api, crowded, shift=ref["shift"])
    nb = crowded["p"].nbeams
    out, gross = np.zeros((nb, nb)), np.zeros((nb, nb))
    for lo, hi in ((0, 9), (9, 14), (14, 15)):
        _twin(api, crowded, shift=ref["shift"], hx_lo=lo, hx_hi=hi, out=out, gross=gross)
    assert float((np.abs(out - T)[G > 0] / G[G > 0]).max()) < 1e-14


# ---- the twin as a stand-alone program under the sanitizers ---------------------------------------------------------------
DRIVER = TD.PRELUDE + r'''
// The cases of the shifted twin on one world of nb beams (|k| = 0.8 k0 everywhere).
struct Shifted : World {
    explicit Shifted(int beams) : World(beams, false) {}
    void run(double *checksum)
    {
        double *equal = block(nb);
        for (int b = 0; b < nb; ++b) equal[b] = 3.3e12;
        auto twin = [&](double *t, double *gr, const double *fl, const double *st, double dn, const double *w, int lo, int hi) {
            std::memset(t, 0, m * sizeof(double)); std::memset(gr, 0, m * sizeof(double));
            REQUIRE(cbet_exchange_matrix_host_shifted(fields, ne3d, t, gr, lo, hi, &p, &g, fl, st, dn, w) == CBET_OK, "%s", cbet_last_error());
        };
        for (int tables = 0; tables < 2; ++tables)
            for (double dn : {0.0, 1e-4}) {
                const double *fl = tables ? flow : nullptr, *st = tables ? state : nullptr;
                twin(T, G, fl, st, dn, shift, 0, hx);
                for (int i = 0; i < nb; ++i)
                    for (int j = 0; j < nb; ++j) {
                        const double a = T[i * nb + j], b = -T[j * nb + i];
                        REQUIRE(same(&a, &b, 1) || (a == 0.0 && b == 0.0), "T[%d][%d] %a, T[%d][%d] %a", i, j, T[i * nb + j], j, i, T[j * nb + i]);
                        REQUIRE(G[i * nb + j] >= std::fabs(T[i * nb + j]), "Gross[%d][%d]", i, j);
                        *checksum += T[i * nb + j] + G[i * nb + j];
                    }
                if (nb >= 2) REQUIRE(T[1] == 0.0 && G[1] == 0.0, "parallel beams of different colour exchange %a", T[1]);
                twin(T, G, fl, st, dn, nullptr, 0, hx);             // one colour: NULL and equal shifts give the same bits
                twin(T2, G2, fl, st, dn, equal, 0, hx);
                REQUIRE(same(T, T2, m) && same(G, G2, m), "equal shifts change a bit (tables %d, dn_max %g)", tables, dn);
                std::memset(T2, 0, m * sizeof(double)); std::memset(G2, 0, m * sizeof(double));
                REQUIRE(cbet_exchange_matrix_host(fields, ne3d, T2, G2, 0, hx, &p, &g, fl, st, dn) == CBET_OK, "%s", cbet_last_error());
                REQUIRE(same(T, T2, m) && same(G, G2, m), "cbet_exchange_matrix_host is not the shifted twin with NULL");
            }
        twin(T, G, still, nullptr, 0.0, shift, 0, hx);              // still plasma: negated shifts negate T
        twin(T2, G2, still, nullptr, 0.0, minus, 0, hx);
        for (size_t k = 0; k < m; ++k) REQUIRE(T2[k] == -T[k] && G2[k] == G[k], "entry %zu: %a against %a", k, T2[k], T[k]);
        twin(T2, G2, still, nullptr, 0.0, shift, 2, 2);             // an empty slab
        for (size_t k = 0; k < m; ++k) REQUIRE(T2[k] == 0.0, "an empty slab wrote entry %zu", k);
        if (nb >= 2) {
            shift[nb - 1] = NAN;
            REQUIRE(cbet_exchange_matrix_host_shifted(fields, ne3d, T2, G2, 0, hx, &p, &g, nullptr, nullptr, 0.0, shift) == CBET_EINVAL, "a NaN shift passed");
            REQUIRE(std::strstr(cbet_last_error(), "shift["), "%s", cbet_last_error());
        }
        std::free(equal);
    }
};

int main()
{
    double checksum = 0.0;
    for (int nb : {1, 2, 7, 64}) Shifted(nb).run(&checksum);
    std::printf("shifted twin ok: checksum %.17g\n", checksum);
    return 0;
}
'''


def test_shifted_twin_is_clean_under_asan_ubsan(tmp_path):
    """The twin with the argument builder it shares with the kernels (cbet_exchange_host.cpp) and the host arithmetic
    (cbet_params.cpp) compiled with the sanitizers into a program of their own, no HIP library on the link line; nothing is
    loaded into Python."""
    out = TD.run_driver(tmp_path, DRIVER)
    assert "shifted twin ok" in out and "checksum" in out


def test_shifts_to_domega_takes_one_of_the_two(api):
    """tracer.shifts_to_domega, the one reading of "wavelength shifts or frequency shifts" (set_detuning, set_bandwidth,
    backscatter_gain): both given raises, neither given raises where one is required and is None (off) where not, a NaN or
    infinite wavelength shift raises, and the conversion is api.wavelength_shift_to_domega's."""
    from cbet_raytracing_3d_amd.tracer import shifts_to_domega
    p = api.default_params(8)
    dl = np.array([-3.0, 0.0, 0.5, 7.0])
    with pytest.raises(ValueError, match="caller"):
        shifts_to_domega(p, "caller", dl, np.zeros(4), False)
    with pytest.raises(ValueError, match="caller"):
        shifts_to_domega(p, "caller", dl, np.zeros(4), True)
    with pytest.raises(ValueError, match="caller"):
        shifts_to_domega(p, "caller", None, None, True)
    assert shifts_to_domega(p, "caller", None, None, False) is None
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="caller"):
            shifts_to_domega(p, "caller", [0.0, bad], None, False)
    assert np.array_equal(shifts_to_domega(p, "caller", dl, None, True), api.wavelength_shift_to_domega(p, dl))
    assert shifts_to_domega(p, "caller", 2.0, None, False) == api.wavelength_shift_to_domega(p, 2.0)
    given = np.array([1e12, -2e12])
    assert shifts_to_domega(p, "caller", None, given, True) is given          # frequency shifts pass as they are
