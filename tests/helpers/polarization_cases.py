"""The cases of tests/test_polarization_host.py and tests/test_gpu_polarization.py (polarization smoothing in the gain stage,
DESIGN.md section 20): the reference, and the CROSSING world.

The reference.  `update` below is a numpy restatement of the pair loop with the polarization factor, written beside
helpers/gain_reference.py's Restatement.update and sharing no line with the library: the same normalised (I, k), prefactor,
eta with shifts, limits, T and Gross, and in front of the clamp

    cth = ((k_i.x k_j.x + k_i.y k_j.y) + k_i.z k_j.z) / (kmag kmag),    f = 0.25 (1.0 + cth cth),    g = (pref P(eta)) f

with kmag = k0 sqrt(eps), the cell's.  With smoothed=False it returns Restatement.update's arrays bit for bit
(tests/test_polarization_host.py asserts that first), which ties it to the reference the gain stage's tests already trust.

`reference(world, tables, everything)` caches in a world of helpers/gain_worlds.py the smoothed update: plain, or with
everything on -- the shifts of helpers/detuning_cases.py and a limit at the median of the SMOOTHED reference's own pair
amplitudes (`half`), on the restatement the table set-up is compared with.

CROSSING.  6 x 5 x 20 nodes on the default profile with its radial flow, three beams present in every sub-critical cell with
the same positive energy and the directions (1, 0, 0), (0, 1, 0), (-1, 0, 0).  The normalisation gives k = +-kmag on one axis
exactly (kmag (1 / 1)), so cth is exactly 0 for the pairs (0, 1) and (1, 2) and exactly -1 for (0, 2): f is exactly 1/4 and
1/2, powers of two, and the ordered statements of the smoothed mode give 0.25 x and 0.5 x the aligned bits."""
import numpy as np

from helpers import detuning_cases as DC
from helpers import gain_worlds as W
from helpers import saturation_cases as SC
from helpers.gain_reference import Restatement

CROSSING = (6, 5, 20)
DIRECTIONS = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])
FACTOR = {(0, 1): 0.25, (1, 2): 0.25, (0, 2): 0.5}       # the exact f of CROSSING's pairs
ENERGY = 3.0e13                                          # every present entry of CROSSING, of the order of real deposits
LOW, HIGH = 0.25, 0.5                                    # the bounds of f
SLACK = 1e-12                                            # ... on sums of products rounded a few ulp apart


def update(R, raw, shift=None, limits=(0.0,), amplitudes=False, matrix=False, normalised=None, planes=None, smoothed=True):
    """Restatement.update's contract (one update from a zero gain with relax = 1 for each limit of `limits`), the pair gain
    times f where `smoothed`.  R: a gain_reference.Restatement, for its cell arrays only."""
    inten, k = R.normalise(raw) if normalised is None else normalised
    nb, n = inten.shape
    w_b = np.zeros(nb) if shift is None else np.asarray(shift, dtype=np.float64)
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
        eta = ((0.0 - (q[0] * R.u[0][at] + q[1] * R.u[1][at] + q[2] * R.u[2][at])) + dw) / (np.where(ok, kiaw, 1.0) * R.cs[at] + 1e-10)
        e2 = eta * eta
        P = R.iaw2 * eta / ((e2 - 1.0) * (e2 - 1.0) + R.iaw2 * e2)
        gain = np.where(ok, R.pref[at] * P, 0.0)
        if smoothed:                                     # beam i is present in every cell of `at`: eps > 0, kmag > 0 there
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


# the two configurations of the tests: (tables of helpers/gain_calls.tables, everything on)
CONFIGS = {"plain": ("none", False), "everything": ("tabled", True)}


def reference(world, config):
    """The smoothed restatement of a world in a configuration of CONFIGS, cached in the world: dict(shift [nb] or None, K the
    smoothed unclamped K, Ka the ALIGNED unclamped K of the same configuration, half = the median of the smoothed reference's
    own pair amplitudes, Khalf the smoothed K under it, amp / I / kap, T / G and Thalf / Ghalf the exchange matrices, R the
    restatement used)."""
    tables, everything = CONFIGS[config]
    key = "smoothed_" + config
    if key not in world:
        R, raw = world[DC.restatement_key(world, tables)], world["raw"]
        w_b = DC.shifts(raw.shape[1]) if everything else None
        first = update(R, raw, w_b, amplitudes=True)
        half = SC.limits_from(first["amps"])["half"]
        both = update(R, raw, w_b, limits=[0.0, half], matrix=True)
        aligned = R.update(raw, w_b)
        world[key] = dict(shift=w_b, K=both["K"][0], Ka=aligned["K"][0], Khalf=both["K"][1], half=half, amp=first["amp"],
                          I=first["I"], kap=first["kap"], T=both["T"][0], G=both["G"][0], Thalf=both["T"][1], Ghalf=both["G"][1],
                          R=R)
    return world[key]


_cache = {}


def crossing_world(api, oracle, inputs):
    """CROSSING: dict(p, gp, ne3d, raw [4, 3, 8, 7, 22], present [8, 7, 22] the sub-critical cells, bn the three beams'
    normals); pair_params / pair_raw give the two-beam subset of a pair (a, b) of its beams."""
    if "crossing" not in _cache:
        bn_all, r, ne, te = inputs
        cfg = oracle.default_config(CROSSING[0], nbeams=3, ny=CROSSING[1], nz=CROSSING[2])
        grid = oracle.grid_shape(cfg)
        assert grid == (8, 7, 22)
        ne3d, _ = oracle.node_tables(cfg, r, ne, te)
        p = W.params(api, CROSSING, 3)
        gp = api.default_gain_params(relax=1.0)
        idx = [np.clip(np.arange(n + 2) - 1, 0, n - 1) for n in CROSSING]
        present = (ne3d < api.derive(p).ncrit)[np.ix_(*idx)]
        assert present.sum() >= 100                      # the regime: sub-critical cells to exchange in
        raw = np.zeros((4, 3) + grid)
        for b in range(3):
            raw[0, b] = np.where(present, ENERGY, 0.0)
            for c in range(3):
                raw[1 + c, b] = np.where(present, DIRECTIONS[b, c], 0.0)
        _cache["crossing"] = dict(p=p, gp=gp, ne3d=ne3d, raw=raw, present=present, bn=bn_all[:3].copy())
    return _cache["crossing"]


def pair_params(api):
    """The parameters of a two-beam subset of CROSSING."""
    return W.params(api, CROSSING, 2)


def pair_raw(world, a_b):
    """The raw fields [4, 2, grid] of beams a and b of CROSSING alone."""
    return np.ascontiguousarray(world["raw"][:, list(a_b)])
