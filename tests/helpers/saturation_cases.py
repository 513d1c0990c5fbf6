"""The cases of tests/test_saturation_host.py and tests/test_gpu_saturation.py (saturation of the ion-acoustic wave in the gain
kernels): what is about limits.  The two grids are those of helpers/gain_worlds.py, the two CPU references
of the clamped update (the oracle composed per pair, the numpy restatement) those of helpers/gain_reference.py.

The limits of the tests are quantiles of a REFERENCE's own unclamped pair amplitudes (limits_from), never of the library's."""
import numpy as np

NEAR = 1e-9            # cells whose amplitude is this close (relative) to the limit are left out of the "clamps or not" comparison
NEAR_SHARE = 1e-3      # ... and may be this share of the non-zero cells at the most


def limits_from(amps):
    """The four limits of the tests from a reference's unclamped pair amplitudes (1-D, one entry per evaluated pair).  The
    quantiles are taken over the pairs that exchange something.  The composed reference knows a pair by its energies alone and
    so lists, with amplitude zero, the cells in which one beam has energy but no direction (it is absent to the model: about
    a third of the traced fields' entries) or the two beams are parallel; a zero has nothing to clamp."""
    pos = amps[amps > 0]
    return dict(never=100.0 * float(pos.max()), half=float(np.median(pos)), deep=float(np.percentile(pos, 1.0)),
                all=0.5 * float(pos.min()))


def clamped_share(amps, dn_max):
    """Share of the pairs that exchange something whose amplitude lies above the limit."""
    pos = amps[amps > 0]
    return float((pos > dn_max).mean())


WANT_SHARE = dict(never=0.0, half=0.5, deep=0.99, all=1.0)


def check_shares(amps, limits, slack=1e-3):
    """The reference's clamped share is what the limit's name says (ties and the quantile's interpolation: `slack`)."""
    shares = {name: clamped_share(amps, limits[name]) for name in WANT_SHARE}
    for name, want in WANT_SHARE.items():
        exact = name in ("never", "all")
        assert (shares[name] == want) if exact else (abs(shares[name] - want) <= slack), (name, shares[name])
    return shares


def near_share(amp_map, dn_max):
    """Share of the non-zero cells of an amplitude map that lie within NEAR (relative) of the limit."""
    nz = amp_map[amp_map > 0]
    return float((np.abs(nz / dn_max - 1.0) <= NEAR).mean())


def reference(world, which, names=("half", "deep", "all")):
    """A restatement's unclamped update with its pair amplitudes, its limits, and the clamped updates for `names`: cached in
    the world under `which` ("plain" / "tabled", or "restated" on TRACED)."""
    key = "ref_" + which
    if key not in world:
        R, raw = world[which], world["raw"]
        first = R.update(raw, amplitudes=True)
        limits = limits_from(first["amps"])
        clamped = R.update(raw, limits=[limits[n] for n in names])
        world[key] = dict(K0=first["K"][0], amp=first["amp"], top=first["top"], kap=first["kap"], I=first["I"], amps=first["amps"],
                          limits=limits, K={n: clamped["K"][m] for m, n in enumerate(names)})
    return world[key]
