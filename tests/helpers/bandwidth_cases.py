"""The cases of tests/test_bandwidth_host.py and tests/test_gpu_bandwidth.py (laser bandwidth in the gain stage, DESIGN.md
section 21): the spectra, and the reference.

The reference.  `update` below is a numpy restatement of the pair loop written beside helpers/polarization_cases.update and
sharing no line with the library.  It takes the LINES (offsets o_a, weights p_a normalised by their sum) and forms the direct
double sum over line pairs,

    g = pref sum_a sum_b p_a p_b P(((0.0 - q . u) + (w_j - w_i) + (o_b - o_a)) / (|q| cs + 1e-10)),

L^2 resonances per beam pair -- NOT the difference table the library collapses the sum onto, so it checks the collapse
independently.  Then the factor f where `smoothed` and the clamp, as polarization_cases.update.  With lines=None it returns
polarization_cases.update's arrays bit for bit (tests/test_bandwidth_host.py asserts that first, and on two-beam subsets that
its K is the weighted sum of Restatement.update's K at the shifts moved by every line pair's offset difference).

The spectra.  Offsets at the scale of helpers/detuning_cases.SCALE = 4.6e12 rad/s (+-3 Angstrom at 351 nm, and |q| cs):

  three   three lines at SCALE (-1, 0.2, 1), weights 1/4, 1/2, 1/4: unequally spaced, M = 3 differences.
  five    five lines at SCALE (-1, -0.61, 0.07, 0.37, 1), weights (1, 2, 4, 3, 1.5) / 11.5: unequally spaced, unequal weights,
          M = 10 and nothing merges.
  eight   eight lines spaced by exactly 2^40 rad/s (1.0995e12; offsets (a - 3.5) 2^40), weights (1, 2, 3, 4, 4, 3, 2, 1) / 20:
          every difference is an exact multiple of 2^40, M = 7: the merge is exercised.

Conditions on the reference alone (tests/test_bandwidth_host.py asserts them and prints the figures): with the sixty shifts of
detuning_cases on, each spectrum moves K by more than MOVES = 1e-2 of the no-spectrum max |K| on both worlds -- that holds at
this scale, so no spectrum was enlarged; with the offsets x FAR the reference's K is within FAR_SHARE = 1e-4 of
c_0 x the no-spectrum K (relative to its max), and the value at NEAR_FAR is asserted too (NEAR_FAR_SHARE), so that a drift shows."""
import numpy as np

from helpers import detuning_cases as DC
from helpers import saturation_cases as SC

SCALE = DC.SCALE
STEP = 2.0 ** 40
SPECTRA = {
    "three": (SCALE * np.array([-1.0, 0.2, 1.0]), np.array([0.25, 0.5, 0.25])),
    "five": (SCALE * np.array([-1.0, -0.61, 0.07, 0.37, 1.0]), np.array([1.0, 2.0, 4.0, 3.0, 1.5])),
    "eight": (STEP * (np.arange(8) - 3.5), np.array([1.0, 2.0, 3.0, 4.0, 4.0, 3.0, 2.0, 1.0])),
}
ENTRIES = {"three": 3, "five": 10, "eight": 7}           # M of each spectrum's difference table
MOVES = 1e-2               # a spectrum moves the reference's K by more than this, of the no-spectrum max |K|
FAR = 1000.0               # offsets x FAR: only the centre term is left ...
FAR_SHARE = 1e-4           # ... K within this of c_0 x the no-spectrum K, of its max
NEAR_FAR = 3.0             # ... and not yet at this factor (NEAR_FAR_SHARE: bounds around the recorded values)
TABLES = DC.TABLES


def lines(name, factor=1.0):
    """(offsets x factor, weights as given -- not normalised: the library and the reference normalise)."""
    off, wts = SPECTRA[name]
    return off * factor, wts.copy()


def centre_weight(name):
    """c_0 = sum p_a^2 of a spectrum, in plain numpy (compared to a few ulp, not bitwise)."""
    p = SPECTRA[name][1] / SPECTRA[name][1].sum()
    return float((p * p).sum())


def update(R, raw, shift=None, lines=None, limits=(0.0,), amplitudes=False, matrix=False, normalised=None, planes=None, smoothed=False):
    """polarization_cases.update's contract (one update from a zero gain with relax = 1 for each limit of `limits`), the pair
    gain summed over all line pairs of `lines` = (offsets, weights).  R: a gain_reference.Restatement, for its cell arrays."""
    inten, k = R.normalise(raw) if normalised is None else normalised
    nb, n = inten.shape
    w_b = np.zeros(nb) if shift is None else np.asarray(shift, dtype=np.float64)
    if lines is not None:
        offs = np.asarray(lines[0], dtype=np.float64)
        p = np.asarray(lines[1], dtype=np.float64) / np.asarray(lines[1], dtype=np.float64).sum()
    inside = None
    if planes is not None:
        inside = np.zeros(R.grid, dtype=bool)
        inside[planes[0]:planes[1]] = True
        inside = inside.reshape(-1)
    K = np.zeros((len(limits), nb, n))
    T, G = np.zeros((len(limits), nb, nb)), np.zeros((len(limits), nb, nb))
    top = np.zeros(n)
    amps = []
    for i in range(nb - 1):
        at = np.nonzero(inten[i] > 0 if inside is None else (inten[i] > 0) & inside)[0]
        if at.size == 0:
            continue
        Ii, Ij = inten[i, at], inten[i + 1:, at]
        ki, kj = k[:, i:i + 1, at], k[:, i + 1:, at]
        q = kj - ki
        kiaw = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
        ok = (Ij > 0) & (kiaw > 0)
        dw = (w_b[i + 1:] - w_b[i])[:, None]
        num = (0.0 - (q[0] * R.u[0][at] + q[1] * R.u[1][at] + q[2] * R.u[2][at])) + dw
        den = np.where(ok, kiaw, 1.0) * R.cs[at] + 1e-10
        if lines is None:
            eta = num / den
            e2 = eta * eta
            P = R.iaw2 * eta / ((e2 - 1.0) * (e2 - 1.0) + R.iaw2 * e2)
        else:
            P = np.zeros_like(num)
            for a in range(offs.size):
                for b in range(offs.size):
                    eta = (num + (offs[b] - offs[a])) / den
                    e2 = eta * eta
                    P += (p[a] * p[b]) * (R.iaw2 * eta / ((e2 - 1.0) * (e2 - 1.0) + R.iaw2 * e2))
        gain = np.where(ok, R.pref[at] * P, 0.0)
        if smoothed:
            kmag = R.kmag[at]
            cth = ((ki[0] * kj[0] + ki[1] * kj[1]) + ki[2] * kj[2]) / (kmag * kmag)
            f = 0.25 * (1.0 + cth * cth)
            gain = np.where(ok, gain * f, 0.0)
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


def reference(world, tables, spectrum, smoothed=False, factor=1.0, shifted=True):
    """The banded restatement of a world, cached in it, for a table set-up of TABLES, a spectrum of SPECTRA (offsets x factor)
    and a polarization mode, with the shifts of detuning_cases on (shifted) or none: dict(shift, lines, K0 the unclamped K
    WITHOUT a spectrum in the same configuration, K the unclamped banded K, half = the median of the banded reference's own
    pair amplitudes, Khalf the K under it, amp / I / kap, T / G and Thalf / Ghalf the exchange matrices, R the restatement)."""
    which = DC.restatement_key(world, tables)
    key = "banded_%s_%s_%d_%g_%d" % (which, spectrum, smoothed, factor, shifted)
    if key not in world:
        R, raw = world[which], world["raw"]
        w_b = DC.shifts(raw.shape[1]) if shifted else None
        ln = lines(spectrum, factor)
        normalised = R.normalise(raw)
        first = update(R, raw, w_b, ln, amplitudes=True, normalised=normalised, smoothed=smoothed)
        half = SC.limits_from(first["amps"])["half"]
        both = update(R, raw, w_b, ln, limits=[0.0, half], matrix=True, normalised=normalised, smoothed=smoothed)
        mono = update(R, raw, w_b, None, normalised=normalised, smoothed=smoothed)
        world[key] = dict(shift=w_b, lines=ln, K0=mono["K"][0], K=both["K"][0], Khalf=both["K"][1], half=half, amp=first["amp"],
                          I=first["I"], kap=first["kap"], T=both["T"][0], G=both["G"][0], Thalf=both["T"][1], Ghalf=both["G"][1],
                          R=R)
    return world[key]


def light_reference(world, spectrum, factor):
    """The unclamped banded K alone (plain tables, aligned, shifts on), for the conditions on the reference: (K, K0)."""
    key = "banded_light_%s_%g" % (spectrum, factor)
    if key not in world:
        R, raw = world[DC.restatement_key(world, "none")], world["raw"]
        w_b = DC.shifts(raw.shape[1])
        normalised = R.normalise(raw)
        world[key] = (update(R, raw, w_b, lines(spectrum, factor), normalised=normalised)["K"][0],
                      update(R, raw, w_b, None, normalised=normalised)["K"][0])
    return world[key]
