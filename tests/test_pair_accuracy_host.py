"""Per-pair accuracy of the gain stage ("Per-pair accuracy"), the part that needs no device.

  1. The fixture tests/golden/pair_accuracy.npz is what helpers/pair_cases.py's 200-bit model gives today, bit for bit, from the
     constants api.derive gives today; the cases hold what the GPU test relies on (the run classes of world B, the clamped share).
  2. c_ref: the worst error of the IEEE ordered statements -- helpers/gain_reference.Restatement and the numpy statements of
     helpers/polarization_cases.py / bandwidth_cases.py, on the fixture's inputs with I = E / ds formed in numpy -- against the
     model, in units of 2^-53 S, per options set over every entry with an evaluated pair.  Printed, finite, and no larger than the
     recorded pair_cases.C_REF the device bound 4 x ceil(c_ref) is derived from.
  3. Teeth: an emulation of the pair-once kernels' pair function (pair_gain_fast, cbet_grid_kernels.hip) -- every fused operation
     exact and rounded once, the hardware estimates replaced by the exact value times (1 + d), |d| <= 2^-23 -- stays inside the
     device bound, and each of three mutants that lack one step (the square root's correction, the reciprocal's Newton step,
     the quotient's correction) exceeds 4 x the bound on some case.

Measured here (units of 2^-53 S; worlds A / B): see pair_cases.C_REF and the table in DESIGN.md section 9."""
import math
import os

import mpmath
import numpy as np
import pytest

from conftest import GOLDEN
from helpers import bandwidth_cases as BC
from helpers import pair_cases as PA
from helpers import polarization_cases as PC
from helpers.gain_reference import Restatement


@pytest.fixture(scope="module")
def api():
    from cbet_raytracing_3d_amd import api as a
    a.lib()
    return a


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "pair_accuracy.npz")))


def _params(api, world):
    p = api.default_params(PA.SHAPE[0], nbeams=PA.NBEAMS[world])
    p.ny, p.nz = PA.SHAPE[1], PA.SHAPE[2]
    return p


# ---- 1. the fixture -------------------------------------------------------------------------------------------------------
def test_fixture_is_the_model_bit_for_bit(api, fx):
    import sys
    sys.path.insert(0, GOLDEN)
    try:
        import make_pair_golden as M
    finally:
        sys.path.remove(GOLDEN)
    consts = M.derived_constants(api)
    assert PA.constants(fx) == consts                                        # api.derive gives the fixture's constants
    # the reference: the model on the fixture's own inputs, every array of the fixture bit for bit
    inp = PA.inputs_of(fx)
    fresh = PA.pack(inp, consts, PA.model(inp, consts))
    assert sorted(fresh) == sorted(fx)
    for key in fresh:
        a, b = np.asarray(fresh[key]), fx[key]
        assert a.dtype == b.dtype and a.shape == b.shape, key
        assert a.tobytes() == b.tobytes(), key
    # the inputs: the designed cases as build_inputs makes them today -- the case of every node exactly; the doubles to 1e-12 of
    # themselves, since cos, sin and pow of another libm may differ in the last bit and the fixture's are the ones that count
    # (the flow to 1e-5: it is built from q = k_j - k_i, which at a crossing angle of 1e-9 magnifies a last bit of k 1e7 times)
    built = PA.build_inputs(consts)
    for key in ("angle", "eta", "construction", "frac", "kind"):
        assert np.array_equal(built[key], inp[key]), key
    for key in ("ne3d", "flow", "state", "E", "k"):
        assert np.allclose(built[key], inp[key], rtol=1e-5 if key == "flow" else 1e-12, atol=0.0), key
    assert os.path.getsize(os.path.join(GOLDEN, "pair_accuracy.npz")) < 2 ** 20


def test_cases_hold_what_the_device_test_relies_on(fx):
    inp = PA.inputs_of(fx)
    kind = fx["kind"]
    assert kind.size == PA.NODES == 1776
    zero = np.isin(kind, (2, 3, 4)).sum()
    assert 0 < zero <= 0.15 * PA.NODES
    crossed = kind == 0
    for ai in range(len(PA.ANGLES)):                                         # every combination that matters occurs
        for ei in range(len(PA.ETAS)):
            assert {int(c) for c in fx["construction"][crossed & (fx["angle"] == ai) & (fx["eta"] == ei)]} == {0, 1, 2}
    for name, count in (("eta", len(PA.ETAS)), ("angle", len(PA.ANGLES)), ("construction", 3)):
        for v in range(count):
            assert {int(f) for f in fx["frac"][crossed & (fx[name] == v)]} == set(range(len(PA.FRACS))), (name, v)
    for world in PA.WORLDS:
        raw = PA.fields(inp, world)
        assert raw.shape == (4, PA.NBEAMS[world]) + PA.GRID == (4, PA.NBEAMS[world], 6, 5, 150)
        present = raw[0] != 0
        assert not present[:, [0, -1]].any() and not present[:, :, [0, -1]].any() and not present[..., [0, -1]].any()   # the halo
        assert (raw[0] < 0).any()
        per_cell = (raw[0] > 0).sum(0)[1:-1, 1:-1, 1:-1]
        assert per_cell.max() == (2 if world == "A" else 3)
        share = fx["share_" + world]
        print("world %s: limits %s clamp %s of the present pairs" % (world, fx["sat_" + world], share))
        assert ((share >= 0.4) & (share <= 0.6)).all()
        print("world %s: clamped pairs one rounding can unclamp or flip, which keep the eta term of S: %s" % (world, fx["soft_" + world]))
        assert (fx["soft_" + world] <= 10).all()                             # a handful of ~800 (A) and ~2500 (B) clamped pairs
    classes = PA.run_classes(PA.fields(inp, "B"))
    print("world B: 16-cell windows beyond the first 64 cells with <= 20, 21 - 40, > 40 present beams: %s" % classes)
    assert min(classes) >= 10
    e = np.abs(inp["E"][inp["E"] != 0])
    assert e.min() < 1e9 and e.max() > 1e13                                  # six decades


# ---- 2. c_ref -------------------------------------------------------------------------------------------------------------
def ieee_statements(api, fx, world, option):
    """K [nbeams, 6, 5, 150] of the ordered IEEE statements in numpy for a world and options set of the fixture."""
    inp = PA.inputs_of(fx)
    p, gp = _params(api, world), api.default_gain_params(relax=1.0)
    assert gp.iaw == PA.constants(fx)["iaw"]
    R = Restatement(api, p, gp, inp["ne3d"], inp["flow"], cs=inp["state"][0], gc=inp["state"][1])
    raw = PA.fields(inp, world)
    nb = raw.shape[1]
    E, k = raw[0].reshape(nb, -1), raw[1:4].reshape(3, nb, -1)
    inten = np.where(R.sub & (E > 0), E / np.where(R.sub, R.ds, 1.0), 0.0)
    detune, pol, band, sat = PA.OPTIONS[option]
    shift = PA.shifts(world) if detune else None
    limits = [float(fx["sat_" + world][list(PA.CLAMPS).index(option)])] if sat else (0.0,)
    with np.errstate(all="ignore"):
        if band:
            out = BC.update(R, None, shift, (fx["line_offsets"], fx["line_weights"]), limits=limits, normalised=(inten, k), smoothed=pol)
        elif pol:
            out = PC.update(R, None, shift, limits=limits, normalised=(inten, k))
        else:
            out = R.update(None, shift, limits=limits, normalised=(inten, k))
    return out["K"][0]


def worst_units(fx, world, option, K):
    """(worst u, its haloed index) over the entries with an evaluated pair; entries with S = 0 must be exact and the rest of the
    grid exactly zero."""
    hi, lo, S, live = PA.reference(fx, world, option)
    assert np.array_equal(K[~live], np.zeros((~live).sum()))                 # -0.0 == 0.0: the sign bit is ignored
    err = PA.errors(K, hi, lo)
    exact = live & (S == 0)
    assert (err[exact] == 0).all()
    u = np.where(live & (S > 0), err / np.where(S > 0, PA.UNIT * S, 1.0), 0.0)
    at = np.unravel_index(np.argmax(u), u.shape)
    return float(u[at]), at


def test_c_ref_of_the_ieee_statements(api, fx):
    measured = {}
    for option in PA.ORDER:
        per_world = []
        for world in PA.WORLDS:
            u, at = worst_units(fx, world, option, ieee_statements(api, fx, world, option))
            per_world.append(u)
            print("c_ref %-8s world %s: %.3f units at beam %d, %s" % (option, world, u, at[0], PA.describe(fx, at[1:])))
        measured[option] = max(per_world)
        assert math.isfinite(measured[option])
    print("c_ref per options set: %s" % {o: round(v, 3) for o, v in measured.items()})
    for option in PA.ORDER:                                                  # the device bound stands on the recorded figure
        assert math.ceil(measured[option]) <= math.ceil(PA.C_REF[option]), (option, measured[option])


# ---- 3. teeth -------------------------------------------------------------------------------------------------------------
class FastPair:
    """pair_gain_fast (plain and DETUNE forms) in Python floats: every fma exact and rounded once (mpmath at 400 bits, then
    float()), the rsq / rcp estimates the exact value times (1 + d).  drop: the step a mutant lacks."""

    def __init__(self, seed, drop=None):
        self.mp = mpmath.mp.clone()
        self.mp.prec = 400
        self.rng = np.random.default_rng(seed)
        self.drop = drop

    def fma(self, a, b, c):
        f = self.mp.mpf
        return float(f(a) * f(b) + f(c))

    def estimate(self, exact):
        return float(exact * self.mp.mpf(1.0 + float(self.rng.uniform(-1.0, 1.0)) * 2.0 ** -23))

    def gain(self, ki, kj, u, cs, iaw2, pref_iaw2, dw=None):
        fma, f = self.fma, self.mp.mpf
        qx, qy, qz = kj[0] - ki[0], kj[1] - ki[1], kj[2] - ki[2]
        q2raw = fma(qz, qz, fma(qy, qy, qx * qx))
        q2 = max(q2raw, 1e-280)
        dot = fma(qz, u[2], fma(qy, u[1], qx * u[0]))
        N = -dot if dw is None else (dw if q2raw > 0.0 else 0.0) - dot
        r0 = self.estimate(1 / self.mp.sqrt(f(q2)))
        gq, hq = q2 * r0, 0.5 * r0
        e = fma(-hq, gq, 0.5)
        gq, hq = fma(gq, e, gq), fma(hq, e, hq)
        if self.drop != "sqrt":
            gq = fma(fma(-gq, gq, q2), hq, gq)
        D = fma(gq, cs, 1e-10)
        N2, D2 = N * N, D * D
        t = N2 - D2
        den = fma(t, t, (iaw2 * N2) * D2)
        num = ((pref_iaw2 * N) * D) * D2
        y = self.estimate(1 / f(den))
        if self.drop != "newton":
            y = fma(fma(-den, y, 1.0), y, y)
        qt = num * y
        return qt if self.drop == "quotient" else fma(fma(-den, qt, num), y, qt)


def emulated(api, fx, option, drop=None):
    """World A's K [2, 6, 5, 150] with the pair function emulated: the cell's factors and I = E / ds as the kernels' IEEE
    statements form them, K_0 = g I_1 and K_1 = -(g I_0)."""
    inp = PA.inputs_of(fx)
    p, gp = _params(api, "A"), api.default_gain_params(relax=1.0)
    R = Restatement(api, p, gp, inp["ne3d"], inp["flow"], cs=inp["state"][0], gc=inp["state"][1])
    raw = PA.fields(inp, "A").reshape(4, 2, -1)
    dw = float(PA.DW) if PA.OPTIONS[option][0] else None
    fast = FastPair(20261021, drop)
    K = np.zeros((2, raw.shape[2]))
    for cell in np.nonzero(R.sub & (raw[0, 0] > 0) & (raw[0, 1] > 0))[0]:
        I0, I1 = raw[0, 0, cell] / R.ds[cell], raw[0, 1, cell] / R.ds[cell]
        g = fast.gain([float(x) for x in raw[1:, 0, cell]], [float(x) for x in raw[1:, 1, cell]], [float(c[cell]) for c in R.u],
                      float(R.cs[cell]), R.iaw2, float(R.pref[cell] * R.iaw2), dw)
        K[0, cell], K[1, cell] = g * I1, -(g * I0)
    return K.reshape((2,) + PA.GRID)


@pytest.mark.parametrize("option", ["plain", "detune"])
def test_emulated_pair_function_and_its_mutants(api, fx, option):
    bound = PA.bound(option)
    u, at = worst_units(fx, "A", option, emulated(api, fx, option))
    print("%s: faithful emulation %.3f units (bound %d) at %s" % (option, u, bound, PA.describe(fx, at[1:])))
    assert u <= bound
    for drop in ("sqrt", "newton", "quotient"):
        hi, lo, S, live = PA.reference(fx, "A", option)
        K = emulated(api, fx, option, drop)
        on = live & (S > 0)
        units = np.where(on, PA.errors(K, hi, lo) / np.where(on, PA.UNIT * S, 1.0), 0.0)
        at = np.unravel_index(np.argmax(units), units.shape)
        print("%s: without the %s step %.1f units (%d cases beyond 4 x the bound = %d) at %s"
              % (option, drop, units[at], (units > 4 * bound).sum(), 4 * bound, PA.describe(fx, at[1:])))
        assert units[at] > 4 * bound, (option, drop)
