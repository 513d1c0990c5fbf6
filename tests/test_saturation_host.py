"""Saturation of the ion-acoustic wave in the gain kernels, the part that needs no device: the new
entries of the C ABI are exported, declared and refuse bad arguments, and the two CPU references of
tests/test_gpu_saturation.py (helpers/gain_reference.py, with the limits of helpers/saturation_cases.py) agree with the oracle and with each other before any kernel is
measured against them.  A context cannot be created without a device: the setter's round trip is in the GPU tests."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import NCPU, ROOT
from helpers import gain_worlds as W
from helpers import saturation_cases as SC
from helpers.gain_worlds import LAST_BITS         # here of max |K|: two CPU formulations of the same update


@pytest.fixture(scope="module")
def api():
    from cbet_raytracing_3d_amd import api as a
    a.lib()
    return a


@pytest.fixture(scope="module")
def traced(api, oracle, inputs):
    return W.traced_world(api, oracle, inputs, NCPU)


@pytest.fixture(scope="module")
def crowded(api, oracle, inputs):
    return W.crowded_world(api, oracle, inputs, NCPU)


def _error(api):
    return api.lib().cbet_last_error().decode()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_declared_and_bound(api):
    header = open(os.path.join(ROOT, "include", "cbet_mi355x.h")).read()
    for name in ("cbet_context_set_saturation", "cbet_context_saturation", "cbet_pair_amplitude"):
        assert ("int %s(" % name) in header
    assert callable(api.Context.set_saturation) and callable(api.Context.saturation) and callable(api.pair_amplitude)
    from cbet_raytracing_3d_amd.tracer import RayTracer
    assert callable(RayTracer.set_saturation) and callable(RayTracer.pair_amplitude)
    assert "saturation of the ion-acoustic wave" in header


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "cbet_mi355x.h"\n'
                   "int use(cbet_context *c, double *o) { return cbet_context_set_saturation(c, 0.05) + cbet_context_saturation(c, o); }\n"
                   "int map(const double *f, double *a, const cbet_params *p, const cbet_gain_params *g, cbet_context *c)\n"
                   "{ return cbet_pair_amplitude(f, 0, a, 0, 2, p, g, c, 0); }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "use.o")])


@pytest.mark.parametrize("value, word", [(-1.0, "negative"), (-1e-300, "negative"), (math.nan, "NaN"), (math.inf, "infinite"),
                                         (-math.inf, "infinite")])
def test_setter_refuses_bad_values_and_names_the_offence(api, value, word):
    """The value is judged before the context: the refusal does not need a device."""
    assert api.lib().cbet_context_set_saturation(None, value) == api.EINVAL
    assert word in _error(api) and "dn_max" in _error(api)


def test_setter_and_getter_refuse_a_null_context(api):
    assert api.lib().cbet_context_set_saturation(None, 0.05) == api.EINVAL and "NULL context" in _error(api)
    assert api.lib().cbet_context_set_saturation(None, 0.0) == api.EINVAL
    out = C.c_double(7.0)
    assert api.lib().cbet_context_saturation(None, C.byref(out)) == api.EINVAL and out.value == 7.0


def test_pair_amplitude_refuses_null_pointers_and_bad_slabs(api):
    p, g = api.default_params(16), api.default_gain_params()
    call = lambda f, a, lo, hi, pp=p, gg=g: api.lib().cbet_pair_amplitude(f, None, a, lo, hi, C.byref(pp), C.byref(gg), None, None)  # noqa: E731
    assert call(None, 8, 0, 18) == api.EINVAL and "fields is NULL" in _error(api)
    assert call(8, None, 0, 18) == api.EINVAL and "amp is NULL" in _error(api)
    for lo, hi in ((-1, 4), (0, 19), (5, 4)):
        assert call(8, 8, lo, hi) == api.EINVAL and "slab [%d,%d)" % (lo, hi) in _error(api)
    assert call(8, 8, 0, 18) == api.EINVAL and "NULL context" in _error(api)          # every argument fine but the context
    assert call(8, 8, 0, 18, gg=api.default_gain_params(iaw=-1.0)) == api.EINVAL and "NULL context" not in _error(api)
    assert api.lib().cbet_pair_amplitude(8, None, 8, 0, 18, None, C.byref(g), None, None) == api.EINVAL


# ---- the references -------------------------------------------------------------------------------------------------------
def test_composition_without_a_clamp_is_the_oracles_whole_field_run(traced):
    K = traced["composed"].gain(0.0)
    err = float(np.abs(K - traced["ogain"]).max() / traced["scale"])
    print("TRACED: composed per pair vs the oracle's whole-field run %.3e of max |K| = %.3e" % (err, traced["scale"]))
    assert traced["scale"] > 1.0 and err < LAST_BITS


def test_restatement_without_a_clamp_is_the_oracle_on_both_grids(traced, crowded):
    for name, world, which in (("TRACED", traced, "restated"), ("CROWDED", crowded, "plain")):
        ref = SC.reference(world, which)
        err = float(np.abs(ref["K0"] - world["ogain"]).max() / world["scale"])
        print("%s: restatement vs oracle %.3e of max |K| = %.3e" % (name, err, world["scale"]))
        assert world["scale"] > 1.0 and err < LAST_BITS


@pytest.mark.parametrize("name", ["half", "deep", "all"])
def test_the_two_references_agree_under_the_clamp(traced, name):
    """TRACED, the limits of the composed reference: its clamped gain against the restatement's, and the amplitudes too."""
    dn = traced["limits"][name]
    want = traced["composed"].gain(dn)
    got = traced["restated"].update(traced["ofields"], limits=[dn])["K"][0]
    err = float(np.abs(got - want).max() / traced["scale"])
    moved = float(np.abs(want - traced["ogain"]).max() / traced["scale"])
    print("TRACED %s (dn_max %.4e): restatement vs composition %.3e of max |K|; the clamp moves K by %.3e" % (name, dn, err, moved))
    assert err < LAST_BITS
    assert moved > 1e-3
    ref = SC.reference(traced, "restated")
    a, b = np.sort(ref["amps"][ref["amps"] > 0]), np.sort(traced["amps"][traced["amps"] > 0])    # the pairs that exchange something
    assert a.size == b.size > 50000 and np.abs(a - b).max() <= 1e-9 * b.max()


def test_limits_clamp_the_share_their_names_say(traced, crowded):
    for label, amps, limits in (("TRACED composed", traced["amps"], traced["limits"]),
                                ("TRACED restated", SC.reference(traced, "restated")["amps"], SC.reference(traced, "restated")["limits"]),
                                ("TRACED tabled", SC.reference(traced, "tabled")["amps"], SC.reference(traced, "tabled")["limits"]),
                                ("CROWDED plain", SC.reference(crowded, "plain")["amps"], SC.reference(crowded, "plain")["limits"]),
                                ("CROWDED tabled", SC.reference(crowded, "tabled")["amps"], SC.reference(crowded, "tabled")["limits"])):
        shares = SC.check_shares(amps, limits)
        print("%s: %d evaluated pairs, amplitudes %.3e .. %.3e, limits %s, clamped shares %s" %
              (label, amps.size, amps[amps > 0].min(), amps.max(), {k: "%.4e" % v for k, v in limits.items()}, shares))
        assert limits["all"] < limits["deep"] < limits["half"] < limits["never"]


def test_few_cells_sit_on_the_limit(traced, crowded):
    """The amplitude map's "clamps here or not" comparison leaves out cells within 1e-9 of the limit: at most 0.1 % of the
    non-zero cells, for `half` and `deep` of every reference map the GPU test uses."""
    for label, world, which in (("TRACED", traced, "restated"), ("TRACED tabled", traced, "tabled"),
                                ("CROWDED", crowded, "plain"), ("CROWDED tabled", crowded, "tabled")):
        ref = SC.reference(world, which)
        for name in ("half", "deep"):
            share = SC.near_share(ref["amp"], ref["limits"][name])
            over = float((ref["amp"] > ref["limits"][name]).mean())
            print("%s %s: %.2e of the non-zero cells within 1e-9 of the limit; %.3f of all cells above it" % (label, name, share, over))
            assert share <= SC.NEAR_SHARE
            assert 0.0 < over < 1.0


def test_clamp_keeps_the_exchange_and_forgets_the_intensity_scale(crowded):
    """Two properties the GPU tests ask of the kernels, of the reference first: the per-cell exchange cancels under the clamp,
    and with every pair clamped K does not depend on the scale of the energies (without a limit it scales with it)."""
    ref = SC.reference(crowded, "plain")
    inten = ref["I"]
    for name in ("half", "all"):
        K = ref["K"][name]
        exch, bound = np.abs((inten * K).sum(axis=0)).max(), np.abs(inten * K).sum(axis=0).max()
        print("CROWDED %s: exchange per cell %.3e of the largest" % (name, exch / bound))
        assert exch <= 1e-11 * bound
    raw16 = crowded["raw"].copy()
    raw16[0] *= 16.0
    both = crowded["plain"].update(raw16, limits=[0.0, ref["limits"]["all"]])["K"]
    assert np.array_equal(both[0], 16.0 * ref["K0"])
    assert np.abs(both[1] - ref["K"]["all"]).max() <= LAST_BITS * crowded["scale"]
