"""The cases of tests/test_detuning_host.py and tests/test_gpu_detuning.py (wavelength detuning in the gain stage, DESIGN.md
section 19): the numpy restatement of helpers/saturation_cases.py with the beat frequency in the resonance,

    eta_ij = ((0.0 - q . u) + (w_j - w_i)) / (|q| cs + 1e-10),        q = k_j - k_i,

on the two worlds of that module (TRACED 48 x 21 x 134 with six traced beams, CROWDED 13 x 11 x 148 with sixty synthetic
ones).  It is built on saturation_cases.Restatement's cell quantities (pref, kap, u, cs, ds, normalise) and shares no line
with the library.

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

Tables.  The set-ups of tests/test_gpu_saturation.py and the restatement each is compared with: "none", "flow" (the sphere's
own flow table handed in as a caller's) and "uniform" (that plus a state table holding the scalars) -> the world's restatement
without tables; "three" (the sphere's flow plus the three-state table) -> a restatement of its own, built here; "tabled" (the
offset target's flow plus the three-state table) -> the world's `tabled`."""
import numpy as np

from helpers import saturation_cases as SC

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


def update(R, raw, shift=None, limits=(0.0,), amplitudes=False, matrix=False, normalised=None):
    """saturation_cases.Restatement.update with the beat frequency: one update from a zero gain with relax = 1 for each limit
    of `limits` (0 = none).  shift: [nb] rad/s or None.  dict(K [limits, nb, grid], amp [grid] the unclamped amplitude map,
    top [grid], I [nb, grid], kap [grid], amps 1-D over the evaluated pairs if asked; matrix=True: T and Gross
    [limits, nb, nb] of the pairwise exchange too).  normalised = (I, k): take these instead of normalising `raw`."""
    inten, k = R.normalise(raw) if normalised is None else normalised
    nb, n = inten.shape
    w_b = np.zeros(nb) if shift is None else np.asarray(shift, dtype=np.float64)
    K = np.zeros((len(limits), nb, n))
    T, G = np.zeros((len(limits), nb, nb)), np.zeros((len(limits), nb, nb))
    top = np.zeros(n)
    amps = []
    for i in range(nb - 1):
        at = np.nonzero(inten[i] > 0)[0]
        if at.size == 0:
            continue
        Ii, Ij = inten[i, at], inten[i + 1:, at]
        q = k[:, i + 1:, at] - k[:, i:i + 1, at]
        kiaw = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
        ok = (Ij > 0) & (kiaw > 0)
        dw = (w_b[i + 1:] - w_b[i])[:, None]
        eta = ((0.0 - (q[0] * R.u[0][at] + q[1] * R.u[1][at] + q[2] * R.u[2][at])) + dw) / (np.where(ok, kiaw, 1.0) * R.cs[at] + 1e-10)
        e2 = eta * eta
        P = R.iaw2 * eta / ((e2 - 1.0) * (e2 - 1.0) + R.iaw2 * e2)
        gain = np.where(ok, R.pref[at] * P, 0.0)
        w = np.abs(gain) * np.sqrt(Ii * Ij)
        top[at] = np.maximum(top[at], w.max(axis=0))
        if amplitudes:
            amps.append((w / R.kap[at])[ok])
        for m, dn_max in enumerate(limits):
            Gc = gain
            if dn_max > 0:
                lim = dn_max * R.kap[at]
                Gc = gain * np.where(w > lim, lim / np.where(w > 0, w, 1.0), 1.0)
            K[m][i, at] += (Gc * Ij).sum(axis=0)
            K[m][i + 1:, at] -= Gc * Ii
            if matrix:
                x = R.ds[at] * Gc * Ii * Ij
                T[m, i, i + 1:] = x.sum(axis=1)
                G[m, i, i + 1:] = np.abs(x).sum(axis=1)
    amp = np.where(R.kap > 0, top / np.where(R.kap > 0, R.kap, 1.0), 0.0)
    out = dict(K=K.reshape((len(limits), nb) + R.grid), amp=amp.reshape(R.grid), top=top.reshape(R.grid),
               I=inten.reshape((nb,) + R.grid), kap=R.kap.reshape(R.grid))
    if amplitudes:
        out["amps"] = np.concatenate(amps)
    if matrix:
        out["T"], out["G"] = T - np.transpose(T, (0, 2, 1)), G + np.transpose(G, (0, 2, 1))
    return out


def restatement_key(world, tables):
    """The name, in the world, of the restatement a table set-up is compared with (TABLES; True / False = "tabled" / "none").
    "three" is built on first use: the sphere's own flow with the world's three-state table."""
    if tables is True or tables == "tabled":
        return "tabled"
    if tables == "three":
        if "three" not in world:
            from cbet_raytracing_3d_amd import api
            world["three"] = SC.Restatement(api, world["p"], world["gp"], world["ne3d"], world["flow"], cs=world["state"][0],
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
        R, raw = world[which], world.get("raw", world.get("ofields"))
        nb = raw.shape[1]
        w_b = shifts(nb, scale)
        first = update(R, raw, w_b, amplitudes=True)
        half = SC.limits_from(first["amps"])["half"]
        both = update(R, raw, w_b, limits=[0.0, half], matrix=True)
        world[key] = dict(shift=w_b, K0=SC.reference(world, which)["K0"], K=both["K"][0], Khalf=both["K"][1], half=half,
                          amp=first["amp"], top=first["top"], kap=first["kap"], I=first["I"], T=both["T"][0], G=both["G"][0],
                          Thalf=both["T"][1], Ghalf=both["G"][1])
    return world[key]
