"""The pairwise exchange matrix, the part that needs no device: the new entries of the C ABI are
exported, declared and refuse bad arguments, and the host twin cbet_exchange_matrix_host -- the reference of the device path
in tests/test_gpu_exchange_matrix.py -- agrees with two CPU references that share no line with the library
(helpers/exchange_cases.py) on the two grids of helpers/gain_worlds.py:

  TRACED  48 x 21 x 134, six beams, the oracle's traced fields: the oracle composed per pair, and the numpy pair loop.
  CROWDED 13 x 11 x 148, sixty beams, 9-54 beams per cell, super-critical nodes, touched-but-absent entries: the numpy pair
          loop, plain and "tabled" (shifted flow + three-state table).

Bounds: 1e-12 of Gross_ij between the ordered statements and a reference, the project's standing one; what must be exact
is asserted bitwise."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import NCPU, ROOT
from helpers import exchange_cases as XC
from helpers import gain_worlds as W
from helpers import saturation_cases as SC
from helpers.gain_worlds import LAST_BITS         # here of Gross_ij (row sums: of sum_j Gross_ij)

SLAB_BITS = 1e-14          # slabs against the whole: the same compensated sums, cut in three
NAMES = ("cbet_exchange_matrix_work_bytes", "cbet_exchange_matrix", "cbet_exchange_matrix_host")


@pytest.fixture(scope="module")
def api():
    from cbet_raytracing_3d_amd import api as a
    a.lib()
    return a


@pytest.fixture(scope="module")
def traced(api, oracle, inputs):
    w = W.traced_world(api, oracle, inputs, NCPU)
    if "xfields" not in w:
        w["xfields"], w["xI"], w["xk"] = XC.normalised(w["restated"], w["ofields"])
    return w


@pytest.fixture(scope="module")
def crowded(api, oracle, inputs):
    w = W.crowded_world(api, oracle, inputs, NCPU)
    if "xfields" not in w:
        w["xfields"], w["xI"], w["xk"] = XC.normalised(w["plain"], w["raw"])
    return w


def _error(api):
    return api.lib().cbet_last_error().decode()


def _twin(api, w, fields=None, tabled=False, dn_max=0.0, **kw):
    return api.exchange_matrix_host(w["xfields"] if fields is None else fields, w["ne3d"], w["p"], w["gp"],
                                    flow=w["shifted"] if tabled else None, state=w["state"] if tabled else None, dn_max=dn_max, **kw)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_declared_and_bound(api):
    header = open(os.path.join(ROOT, "include", "cbet_mi355x.h")).read()
    for name in NAMES:
        assert ("%s(" % name) in header
    assert callable(api.exchange_matrix) and callable(api.exchange_matrix_host) and callable(api.exchange_matrix_work_bytes)
    from cbet_raytracing_3d_amd.tracer import RayTracer
    assert callable(RayTracer.exchange_matrix)
    assert "pairwise exchange matrix" in header and "CBET_EXCHANGE_MAX_GROUPS" in header


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "cbet_mi355x.h"\n'
                   "int dev(const double *f, double *o, void *w, const cbet_params *p, const cbet_gain_params *g, cbet_context *c)\n"
                   "{ return cbet_exchange_matrix_work_bytes(p) ? cbet_exchange_matrix(f, 0, o, 0, w, 0, 2, p, g, c, 0) : 0; }\n"
                   "int host(const double *f, const double *n, double *o, const cbet_params *p, const cbet_gain_params *g)\n"
                   "{ return cbet_exchange_matrix_host(f, n, o, o, 0, 2, p, g, 0, 0, 0.05); }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "use.o")])


def test_work_bytes_follow_the_grid_and_the_beam_count(api):
    cap = 768                                                               # CBET_EXCHANGE_MAX_GROUPS
    for shape, nb in (((6, 9, 13), 2), ((6, 9, 13), 1), ((13, 11, 148), 60), ((48, 21, 134), 6), ((5, 4, 37), 64), ((256, 256, 256), 60)):
        p = W.params(api, shape, nb)
        rows = (shape[0] + 2) * (shape[1] + 2)
        assert api.exchange_matrix_work_bytes(p) == min(rows, cap) * 2 * (nb * (nb - 1) // 2) * 8, (shape, nb)
    assert api.exchange_matrix_work_bytes(W.params(api, (5, 4, 37), 65)) == 0
    assert api.lib().cbet_exchange_matrix_work_bytes(None) == 0


def test_device_entry_refuses_bad_arguments_and_names_them(api):
    """The arguments are judged before the context: the refusals do not need a device."""
    p, g = api.default_params(16), api.default_gain_params()
    call = lambda f, o, w, lo, hi, pp=p, gg=g: api.lib().cbet_exchange_matrix(f, None, o, None, w, lo, hi, C.byref(pp), C.byref(gg), None, None)  # noqa: E731
    assert call(None, 8, 8, 0, 18) == api.EINVAL and "fields is NULL" in _error(api)
    assert call(8, None, 8, 0, 18) == api.EINVAL and "out is NULL" in _error(api)
    assert call(8, 8, None, 0, 18) == api.EINVAL and "work is NULL" in _error(api)
    for lo, hi in ((-1, 4), (0, 19), (5, 4)):
        assert call(8, 8, 8, lo, hi) == api.EINVAL and "slab [%d,%d)" % (lo, hi) in _error(api)
    assert call(8, 8, 8, 0, 18, pp=api.default_params(16, nbeams=65)) == api.EINVAL
    assert "nbeams = 65" in _error(api) and "CBET_MAX_CBET_BEAMS" in _error(api)
    assert call(8, 8, 8, 0, 18) == api.EINVAL and "NULL context" in _error(api)          # every argument fine but the context
    assert call(8, 8, 8, 0, 18, gg=api.default_gain_params(iaw=-1.0)) == api.EINVAL and "NULL context" not in _error(api)
    assert api.lib().cbet_exchange_matrix(8, None, 8, None, 8, 0, 18, None, C.byref(g), None, None) == api.EINVAL


def test_host_twin_refuses_bad_arguments_and_names_them(api):
    p, g = W.params(api, (6, 9, 13), 2), api.default_gain_params()
    f, n, o = np.zeros((4, 2, 8, 11, 15)), np.zeros((6, 9, 13)), np.zeros((2, 2))
    call = lambda ff, nn, oo, lo, hi, pp=p, dn=0.0: api.lib().cbet_exchange_matrix_host(  # noqa: E731
        api._addr(ff), api._addr(nn), api._addr(oo), None, lo, hi, C.byref(pp), C.byref(g), None, None, dn)
    assert call(None, n, o, 0, 8) == api.EINVAL and "fields is NULL" in _error(api)
    assert call(f, None, o, 0, 8) == api.EINVAL and "ne3d is NULL" in _error(api)
    assert call(f, n, None, 0, 8) == api.EINVAL and "out is NULL" in _error(api)
    for lo, hi in ((-1, 4), (0, 9), (5, 4)):
        assert call(f, n, o, lo, hi) == api.EINVAL and "slab [%d,%d)" % (lo, hi) in _error(api)
    for dn in (-1.0, float("nan"), float("inf")):
        assert call(f, n, o, 0, 8, dn=dn) == api.EINVAL and "dn_max" in _error(api)
    assert call(f, n, o, 0, 8, pp=W.params(api, (6, 9, 13), 65)) == api.EINVAL and "nbeams = 65" in _error(api)
    assert call(f, n, o, 0, 8) == api.OK and not o.any()                                 # empty fields: zeros
    one = W.params(api, (6, 9, 13), 1)
    assert call(np.ones((4, 1, 8, 11, 15)), n, np.zeros((1, 1)), 0, 8, pp=one) == api.OK  # one beam: nothing to do


# ---- TRACED: two references -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["none", "half", "all"])
def test_traced_twin_against_the_oracle_composed_per_pair(api, traced, name):
    dn = 0.0 if name == "none" else traced["limits"][name]
    want, gross = XC.composed_matrix(traced["composed"], dn)
    T, G = _twin(api, traced, dn_max=dn)
    err, gerr = XC.worst(T, want, gross), XC.worst(G, gross, gross)
    print("TRACED %s (dn_max %.4e): twin vs the oracle composed per pair %.3e of Gross (Gross itself %.3e); max Gross %.3e, max |T| %.3e"
          % (name, dn, err, gerr, gross.max(), np.abs(want).max()))
    assert gross.max() > 0 and (gross > 0).sum() == 30
    assert err < LAST_BITS and gerr < LAST_BITS


@pytest.mark.parametrize("name", ["none", "half", "all"])
def test_traced_twin_against_the_numpy_pair_loop(api, traced, name):
    dn = 0.0 if name == "none" else XC.limits_of(traced, "restated")[name]
    want, gross = XC.pairwise_matrix(traced["restated"], traced["xI"], traced["xk"], dn)
    T, G = _twin(api, traced, dn_max=dn)
    err, gerr = XC.worst(T, want, gross), XC.worst(G, gross, gross)
    print("TRACED %s (dn_max %.4e): twin vs the numpy pair loop %.3e of Gross (Gross itself %.3e)" % (name, dn, err, gerr))
    assert err < LAST_BITS and gerr < LAST_BITS
    if name == "all":                                                       # every exchanging pair is clamped: |T| shrinks
        free, _ = _twin(api, traced)
        assert (np.abs(T)[gross > 0] < np.abs(free)[gross > 0]).all()


# ---- CROWDED ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["none", "half"])
@pytest.mark.parametrize("which", ["plain", "tabled"])
def test_crowded_twin_against_the_numpy_pair_loop(api, crowded, which, name):
    dn = 0.0 if name == "none" else XC.limits_of(crowded, which)[name]
    want, gross = XC.pairwise_matrix(crowded[which], crowded["xI"], crowded["xk"], dn)
    T, G = _twin(api, crowded, tabled=which == "tabled", dn_max=dn)
    err, gerr = XC.worst(T, want, gross), XC.worst(G, gross, gross)
    print("CROWDED %s %s (dn_max %.4e): twin vs the numpy pair loop %.3e of Gross (Gross itself %.3e); %d of 1770 pairs exchange"
          % (which, name, dn, err, gerr, (gross > 0).sum() // 2))
    assert (gross > 0).sum() == 60 * 59                                     # every pair meets somewhere
    assert err < LAST_BITS and gerr < LAST_BITS
    sub = crowded[which].sub.reshape(crowded[which].grid)
    assert not sub.all()                                                    # super-critical cells are part of the case


# ---- exact properties -------------------------------------------------------------------------------------------------------
def test_exact_properties_of_the_twin(api, crowded):
    limits = XC.limits_of(crowded, "plain")
    T, G = _twin(api, crowded)
    again = _twin(api, crowded)
    assert np.array_equal(T, again[0]) and np.array_equal(G, again[1])     # deterministic
    for t, g in ((T, G), _twin(api, crowded, dn_max=limits["half"])):
        assert np.array_equal(t, -t.T) and not np.diag(t).any()
        assert np.array_equal(g, g.T) and not np.diag(g).any()
        assert (g >= np.abs(t)).all()
    never = _twin(api, crowded, dn_max=limits["never"])                     # a limit never reached: the bits of none
    assert np.array_equal(never[0], T) and np.array_equal(never[1], G)
    a, b = 7, 41
    assert G[a, b] > 0
    t, g = _twin(api, crowded, fields=XC.never_together(crowded["xfields"], a, b, 7))
    assert t[a, b] == 0.0 and t[b, a] == 0.0 and g[a, b] == 0.0 and g[b, a] == 0.0
    assert np.count_nonzero(g) == 60 * 59 - 2                               # ... and only that pair


def test_rows_sum_to_what_the_gain_update_hands_each_beam(api, traced, crowded):
    for label, w, which in (("TRACED", traced, "restated"), ("CROWDED", crowded, "plain"), ("CROWDED tabled", crowded, "tabled")):
        R = w[which]
        ref = SC.reference(w, which)
        want = XC.row_sums(R, dict(I=ref["I"], K=ref["K0"]))
        T, G = _twin(api, w, tabled=which == "tabled")
        err = float((np.abs(T.sum(axis=1) - want) / G.sum(axis=1)).max())
        print("%s: row sums vs sum ds I K0 of the restatement %.3e of sum_j Gross_ij" % (label, err))
        assert err < LAST_BITS
        for name in ("half", "all"):                                        # ... and under the clamp
            Tc, Gc = _twin(api, w, tabled=which == "tabled", dn_max=ref["limits"][name])
            wantc = XC.row_sums(R, dict(I=ref["I"], K=ref["K"][name]))
            errc = float((np.abs(Tc.sum(axis=1) - wantc) / Gc.sum(axis=1)).max())
            print("%s %s: row sums %.3e" % (label, name, errc))
            assert errc < LAST_BITS


def test_slabs_add_up_to_the_whole(api, traced, crowded):
    for label, w in (("TRACED", traced), ("CROWDED", crowded)):
        T, G = _twin(api, w)
        nb, hx = w["p"].nbeams, w["p"].nx + 2
        out, gross = np.zeros((nb, nb)), np.zeros((nb, nb))
        cuts = [s for s in XC.SLABS + [(22, hx)] if s[0] < hx]
        cuts = [(lo, min(hi, hx)) for lo, hi in cuts]
        for lo, hi in cuts:
            o, g = _twin(api, w, hx_lo=lo, hx_hi=hi, out=out, gross=gross)
            assert o is out and g is gross
        err = float((np.abs(out - T)[G > 0] / G[G > 0]).max())
        print("%s: slabs %s summed vs the whole %.3e of Gross" % (label, cuts, err))
        assert err < SLAB_BITS and float((np.abs(gross - G)[G > 0] / G[G > 0]).max()) < SLAB_BITS
        assert np.array_equal(out, -out.T) and np.array_equal(gross, gross.T)
        before = out.copy()
        _twin(api, w, hx_lo=5, hx_hi=5, out=out, gross=gross)                # an empty slab changes nothing
        assert np.array_equal(out, before)
        part, _ = _twin(api, w, hx_lo=cuts[1][0], hx_hi=cuts[1][1])          # one slab against the reference on its planes
        want, wg = XC.pairwise_matrix(w["restated" if label == "TRACED" else "plain"], w["xI"], w["xk"], planes=cuts[1])
        assert XC.worst(part, want, wg) < LAST_BITS
