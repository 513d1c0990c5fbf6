"""The cases of tests/test_detuning_host.py and tests/test_gpu_detuning.py (wavelength detuning in the gain stage, DESIGN.md
section 19): the shifts, and the reference they give.  The reference is the numpy restatement of helpers/gain_reference.py,
whose pair loop takes per-beam shifts as the beat frequency in the resonance,

    eta_ij = ((0.0 - q . u) + (w_j - w_i)) / (|q| cs + 1e-10),        q = k_j - k_i,

on the two worlds of helpers/gain_worlds.py (TRACED 48 x 21 x 134 with six traced beams, CROWDED 13 x 11 x 148 with sixty
synthetic ones).

The shifts.  w_b = SCALE ((37 b mod 60) - 29.5) / 30 rad/s: sixty DISTINCT values (37 and 60 are coprime) between -SCALE and
+SCALE, so that a slot / beam mix-up cannot pass.  SCALE = 4.6e12 rad/s is the scale of +-3 Angstrom at 351 nm
(omega = 5.37e15 rad/s, d omega = omega dl / l = 4.6e12) and of |q| cs (|q| ~ 1e5 / cm, cs ~ 3e7 cm/s).  The condition the
tests ask of the reference alone -- its K with these shifts differs from its K without by more than 1e-2 of max |K| on both
worlds -- holds at this scale (tests/test_detuning_host.py asserts it and prints the figures), so it was not enlarged.

Far off resonance: max |K| of the reference below FAR_SHARE = 1e-4 of its unshifted value.  With these sixty values
neighbouring colours are only SCALE / 30 apart, and at NEAR_FAR = 100 SCALE the reference is not there yet: 2.7e-4 on TRACED,
1.9e-1 on CROWDED (NEAR_FAR_SHARE holds these figures with a margin; 3e-5 / 3e-2 at 200 SCALE, 8e-6 / 8e-3 at 300 SCALE).  As
with the condition above, the scale is enlarged until the REFERENCE meets the bound -- FAR = 1000 SCALE: 2.1e-7 on TRACED,
6.2e-6 on CROWDED -- and the kernels are compared with the reference at both scales.

Tables.  The set-ups of helpers/gain_calls.tables and the restatement each is compared with: "none", "flow" (the sphere's
own flow table handed in as a caller's) and "uniform" (that plus a state table holding the scalars) -> the world's restatement
without tables; "three" (the sphere's flow plus the three-state table) -> a restatement of its own, built here; "tabled" (the
offset target's flow plus the three-state table) -> the world's `tabled`."""
import numpy as np

from helpers import saturation_cases as SC
from helpers.gain_reference import Restatement

SCALE = 4.6e12
NEAR_FAR = 100.0 * SCALE
FAR = 1000.0 * SCALE
MOVES = 1e-2               # the shifts move the reference's K by more than this, of max |K|
FAR_SHARE = 1e-4           # max |K| far off resonance, of the unshifted max |K|
NEAR_FAR_SHARE = {"traced": 3e-4, "crowded": 0.2}      # ... at NEAR_FAR: the recorded 2.7e-4 and 1.9e-1, so that a drift shows
TABLES = ["none", "flow", "uniform", "three", "tabled"]


def shifts(nbeams, scale=SCALE):
    """w_b = scale ((37 b mod 60) - 29.5) / 30 for b < nbeams: distinct values."""
    b = np.arange(nbeams)
    return scale * (((37 * b) % 60) - 29.5) / 30.0


def three_colours(nbeams, angstrom=3.0):
    """Wavelength shifts (-a, 0, +a) Angstrom by beam index mod 3."""
    return angstrom * ((np.arange(nbeams) % 3) - 1.0)


def restatement_key(world, tables):
    """The name, in the world, of the restatement a table set-up is compared with (TABLES; True / False = "tabled" / "none").
    "three" is built on first use: the sphere's own flow with the world's three-state table."""
    if tables is True or tables == "tabled":
        return "tabled"
    if tables == "three":
        if "three" not in world:
            from cbet_raytracing_3d_amd import api
            world["three"] = Restatement(api, world["p"], world["gp"], world["ne3d"], world["flow"], cs=world["state"][0],
                                         gc=world["state"][1])
        return "three"
    assert tables in (False, "none", "flow", "uniform"), tables
    return "restated" if "restated" in world else "plain"


def reference(world, tables=False, scale=SCALE):
    """The shifted restatement of a world, cached in it: dict(shift, K0 the UNSHIFTED unclamped K, K the shifted unclamped K,
    Khalf the shifted K under `half`, half = the median of the shifted reference's own pair amplitudes
    (saturation_cases.limits_from), amp / top / kap / I, T / G and Thalf / Ghalf the exchange matrices)."""
    which = restatement_key(world, tables)
    key = "detuned_%s_%g" % (which, scale)
    if key not in world:
        R, raw = world[which], world["raw"]
        nb = raw.shape[1]
        w_b = shifts(nb, scale)
        first = R.update(raw, w_b, amplitudes=True)
        half = SC.limits_from(first["amps"])["half"]
        both = R.update(raw, w_b, limits=[0.0, half], matrix=True)
        world[key] = dict(shift=w_b, K0=SC.reference(world, which)["K0"], K=both["K"][0], Khalf=both["K"][1], half=half,
                          amp=first["amp"], top=first["top"], kap=first["kap"], I=first["I"], T=both["T"][0], G=both["G"][0],
                          Thalf=both["T"][1], Ghalf=both["G"][1])
    return world[key]
