"""Cases for the arms of the exit pass that a trace of the shipped plasma does not reach:
seeded gain fields in three regimes of the gain exponent, the long box whose y beams run out of steps, synthetic exit
records for the two reductions, and the long-double references of those reductions, written from the column and bin
definitions of include/cbet_mi355x.h.

Everything here is numpy and the CPU oracle; the GPU tests (test_gpu_exit_arms.py) and the CPU tests of the regimes
(test_exit_oracle.py) both draw from it.
"""
import numpy as np

from helpers import config_matrix as M

LAUNCHED, CUTOFF, ESCAPED, TIMEOUT = 1, 2, 4, 8       # include/cbet_mi355x.h CBET_RAY_*
EPS = 2.0 ** -53                                      # unit roundoff of fp64

# ---- the ragged grid of the per-ray gain tests ----------------------------------------------------------------------
RAGGED = M.Entry("ragged_20x17x25", n=20, ny=17, nz=25)      # sXh, sYh and the z pitch all differ; beams M.B4

SERIES_SWITCH = 0.03125      # |x| below which a wave whose live lanes all satisfy it takes the short series

# Amplitudes A of the three gain fields, gain[b][node] uniform in [-A, A] (1/cm), seed GAIN_SEED + index.  x = K ds with
# ds ~ 0.005 cm on the ragged grid; K is the deposit-weighted sum of eight node values (the weights of a ray that has
# left the grid, or lost its cell after a far jump, extrapolate, so |K| can exceed A).  Chosen on the oracle;
# test_exit_oracle.py asserts each regime:
#   small   : max |x| over all ray-steps < 1/32, so every wave takes the short series;
#   mixed   : some ray-steps have |x| >= 1/32, none reaches max_exponent = 1.  The two entries of the configuration
#             matrix the field is re-run on have their own amplitude: box_small's far-jump rays gather with weights of
#             tens, and its steps are a quarter as long;
#   clamped : the clamp engages.  The clamp is brought down to the field (max_exponent = 1/16, gain_params) rather than
#             the field up to the clamp: at max_exponent = 1 a clamped field multiplies a ray's energy by up to e per
#             step, some rays end 1e7 .. 1e11 times their launch energy, and a comparison to 1e-9 of uray0 would then
#             ask for more than fp64 holds.  Doubling max_exponent changes `gained` of nearly every ray.
# In "mixed" and "clamped" no ray's energy or gain exceeds 1e4 uray0 (asserted on the oracle).
GAIN_SEED = 20261018
GAIN_FIELDS = ("small", "mixed", "clamped")
GAIN_AMPLITUDE = {"small": 2.0, "mixed": 60.0, "clamped": 60.0}
MIXED_AMPLITUDE = {"box_small": 5.0, "strided_5": 60.0}
GAIN_MAX_EXPONENT = {"small": 1.0, "mixed": 1.0, "clamped": 0.0625}
MIXED_ENTRIES = (RAGGED, M.BY_NAME["box_small"], M.BY_NAME["strided_5"])


def gain_field(name, entry=RAGGED):
    """The seeded gain field `name` for `entry`'s grid: float64 [nbeams][nx+2][ny+2][nz+2]."""
    rng = np.random.default_rng(GAIN_SEED + GAIN_FIELDS.index(name))
    a = GAIN_AMPLITUDE[name]
    if entry is not RAGGED:
        assert name == "mixed"
        a = MIXED_AMPLITUDE[entry.name]
    return rng.uniform(-a, a, size=(entry.nbeams(), entry.n + 2, entry.ny + 2, entry.nz + 2))


def oracle_gain_config(oracle, name, **kw):
    return oracle.gain_default(max_exponent=kw.pop("max_exponent", GAIN_MAX_EXPONENT[name]), **kw)


def oracle_exits(oracle, entry, inputs, gain=None, gain_cfg=None, ne=None, beams=None):
    """Every live ray of `beams` (default: all) of `entry` through cbet_oracle_ray_exit, node tables from the profile:
    (ids [R], records float64 [len(beams)][R][13], columns oracle.EXIT_FIELDS)."""
    bn, r, ne0, te = inputs
    cfg, bt = entry.config(oracle), entry.beam_table(bn)
    ne3d, kap = oracle.node_tables(cfg, r, ne0 if ne is None else ne, te)
    g = oracle.gain_default() if gain_cfg is None else gain_cfg
    ids = M.live_ids(oracle, cfg, bt)
    beams = list(range(cfg.nbeams)) if beams is None else list(beams)
    if gain is not None:
        gain = np.ascontiguousarray(gain, dtype=np.float64)
    out = np.zeros((len(beams), len(ids), len(oracle.EXIT_FIELDS)))
    for k, b in enumerate(beams):
        for j, i in enumerate(ids):
            out[k, j] = oracle.ray_exit(cfg, g, bt, ne3d, kap, gain, int(b), int(i))
    return np.asarray(ids), out


# ---- the long box: rays that run out of steps ----------------------------------------------------------------------
# 24^3 nodes, y from -0.8 to 0.8 cm, the six axis beams, vacuum: dt follows min(dx, dz), so nt = 96 steps of half an x
# cell cross 0.54 cm -- the +-y beams' rays, launched 0.1 cm from the origin, are still inside after nt steps and nothing
# absorbs them; the four other beams' rays leave through the near faces.
LONG_BOX = M.Entry("long_box_y", n=24, beams=M.AXIS_BEAMS, overrides=dict(ymin=-0.8, ymax=0.8))
LONG_BOX_NT = 96
LONG_BOX_LIVE = 124
LONG_BOX_Y_BEAMS = (2, 3)
LONG_BOX_OTHER_BEAMS = (0, 1, 4, 5)


# ---- synthetic records ----------------------------------------------------------------------------------------------
def exit_dtype():
    from cbet_raytracing_3d_amd import api
    return api.EXIT_DTYPE


def tally_records(nbeams, L, seed=20261018):
    """[nbeams][L] records for cbet_exit_tally: uray0 log-uniform over 1e-3 .. 1e12, gained of both signs (above -uray0),
    uray uniform in [0, uray0 + gained], status cycling through all 16 combinations of the four bits in a seeded order."""
    rng = np.random.default_rng(seed + 1000 * nbeams + L)
    rec = np.zeros((nbeams, L), dtype=exit_dtype())
    n = nbeams * L
    uray0 = 10.0 ** rng.uniform(-3.0, 12.0, size=n)
    gained = uray0 * rng.uniform(-0.9, 2.0, size=n)
    uray = (uray0 + gained) * rng.uniform(0.0, 1.0, size=n)
    status = (np.arange(n) + rng.integers(16)) % 16
    status = status[rng.permutation(n)] if n >= 16 else rng.integers(0, 16, size=n)
    for name in ("x", "y", "z", "vx", "vy", "vz"):
        rec[name] = rng.normal(size=n).reshape(nbeams, L)
    rec["uray0"], rec["gained"], rec["uray"] = (a.reshape(nbeams, L) for a in (uray0, gained, uray))
    rec["steps"] = rng.integers(1, 1000, size=n).reshape(nbeams, L)
    rec["status"] = status.reshape(nbeams, L)
    return rec


def tally_reference(rec):
    """(want, bound), long double [nbeams][8]: the columns of include/cbet_mi355x.h (CBET_TALLY_*) and, for columns
    0..5, the bound (L - 1) 2^-53 sum |terms| that holds for a sum of L terms in ANY order; columns 6, 7 are exact.

    The header's rule: only LAUNCHED records count; each of them is booked once, in `escaped` if ESCAPED is set, else in
    `stranded` if CUTOFF is set, else in `unfinished`."""
    ld = np.longdouble
    nb, L = rec.shape
    want = np.zeros((nb, 8), dtype=ld)
    mag = np.zeros((nb, 8), dtype=ld)
    st = rec["status"]
    launched = (st & LAUNCHED) != 0
    esc = launched & ((st & ESCAPED) != 0)
    cut = launched & ~esc & ((st & CUTOFF) != 0)
    rest = launched & ~esc & ~cut
    u0, g, u = (rec[k].astype(ld) for k in ("uray0", "gained", "uray"))
    absorbed = (rec["uray0"] + rec["gained"]) - rec["uray"]      # the column's term is this fp64 expression
    terms = [np.where(launched, u0, 0), np.where(launched, g, 0), np.where(launched, absorbed.astype(ld), 0),
             np.where(esc, u, 0), np.where(cut, u, 0), np.where(rest, u, 0)]
    for c, t in enumerate(terms):
        t = t.astype(ld)
        want[:, c] = t.sum(axis=1)
        mag[:, c] = np.abs(t).sum(axis=1)
    want[:, 6] = launched.sum(axis=1)
    want[:, 7] = esc.sum(axis=1)
    bound = (L - 1) * ld(EPS) * mag
    return want, bound


C_LIGHT = 29979245800.0


def farfield_exact_records():
    """Hand-made records for cbet_farfield and where the header's formula puts each: (records, [(index, it_of, ip_of)])
    with it_of / ip_of functions of (ntheta, nphi), or None for a record that must contribute nothing.  Energies are
    distinct powers of two, so any subset sums exactly and a histogram names the records it holds."""
    c = C_LIGHT
    both = LAUNCHED | ESCAPED
    half = lambda n: n // 2                   # floor(n / 2): atan2 = +-0 gives (0 + pi) / (2 pi) * nphi = nphi / 2
    first = lambda n: 0
    last = lambda n: n - 1
    cases = [
        # the poles: 1 - vz/|v| = 0 -> it = 0;  = 2 -> ntheta, clamped to ntheta - 1.  atan2(+-0, +-0), IEEE 754 / C11
        # F.10.1.4: atan2(+0, +0) = +0, atan2(-0, +0) = -0, atan2(+0, -0) = +pi, atan2(-0, -0) = -pi
        ((+0.0, +0.0, +c), both, first, half),
        ((+0.0, -0.0, +c), both, first, half),
        ((-0.0, +0.0, +c), both, first, last),      # (pi + pi) / (2 pi) * nphi = nphi -> clamped
        ((-0.0, -0.0, +c), both, first, first),     # (-pi + pi) = 0 -> bin 0
        ((+0.0, +0.0, -c), both, last, half),
        ((-0.0, +0.0, -c), both, last, last),
        ((-0.0, -0.0, -c), both, last, first),
        # the -x seam: atan2(+0, -c) = +pi -> nphi - 1, atan2(-0, -c) = -pi -> 0;  vz = 0 -> it = floor(ntheta / 2)
        ((-c, +0.0, 0.0), both, half, last),
        ((-c, -0.0, 0.0), both, half, first),
        # no direction: vz/|v| = 0/0 = NaN -> the polar coordinate is NaN -> bin 0;  atan2(+0, +0) = 0 -> nphi / 2
        ((0.0, 0.0, 0.0), both, first, half),
        # +x for orientation: atan2(0, c) = 0 -> nphi / 2 (pi / (2 pi) is 0.5 exactly, so even an even nphi is safe; +-y
        # would sit on the edges 3 nphi / 4 and nphi / 4 with a rounded quotient)
        ((c, 0.0, 0.0), both, half, half),
        # status bits beyond the two do not matter
        ((c, 0.0, 0.0), both | CUTOFF, half, half),
        ((c, 0.0, 0.0), both | TIMEOUT | CUTOFF, half, half),
        # records that contribute nothing
        ((c, 0.0, 0.0), ESCAPED, None, None),
        ((c, 0.0, 0.0), ESCAPED | CUTOFF | TIMEOUT, None, None),
        ((c, 0.0, 0.0), LAUNCHED, None, None),
        ((c, 0.0, 0.0), LAUNCHED | CUTOFF, None, None),
        ((c, 0.0, 0.0), LAUNCHED | TIMEOUT, None, None),
        ((0.0, 0.0, 0.0), 0, None, None),
    ]
    rec = np.zeros(len(cases), dtype=exit_dtype())
    where = []
    for k, (v, status, it_of, ip_of) in enumerate(cases):
        rec[k]["vx"], rec[k]["vy"], rec[k]["vz"] = v
        rec[k]["status"] = status
        rec[k]["uray"] = 2.0 ** k
        rec[k]["uray0"] = 2.0 ** (k + 1)
        where.append((k, it_of, ip_of))
    # an all-zero record's uray is zero too
    rec[-1]["uray"] = rec[-1]["uray0"] = 0.0
    return rec, where


def farfield_bulk_records(n, ntheta, nphi, seed=20261018, margin=1e-9):
    """n records with seeded random directions, none within `margin` of a bin edge in either coordinate of
    api.farfield_bins (redrawn until so), energies log-uniform over six decades, three in four launched and escaped."""
    from cbet_raytracing_3d_amd import api
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v *= C_LIGHT * rng.uniform(0.3, 1.0, size=(n, 1)) / np.linalg.norm(v, axis=1, keepdims=True)
    for _ in range(100):
        ct, cp = api.farfield_bins(v[:, 0], v[:, 1], v[:, 2], ntheta, nphi)
        bad = (np.abs(ct - np.round(ct)) < margin) | (np.abs(cp - np.round(cp)) < margin)
        if not bad.any():
            break
        w = rng.normal(size=(int(bad.sum()), 3))
        v[bad] = w * (C_LIGHT * 0.5 / np.linalg.norm(w, axis=1, keepdims=True))
    else:
        raise AssertionError("could not draw directions clear of the bin edges")
    rec = np.zeros(n, dtype=exit_dtype())
    rec["vx"], rec["vy"], rec["vz"] = v.T
    rec["uray"] = 10.0 ** rng.uniform(3.0, 9.0, size=n)
    rec["uray0"] = 2.0 * rec["uray"]
    rec["status"] = np.where(rng.integers(4, size=n) > 0, LAUNCHED | ESCAPED,
                             rng.choice([0, LAUNCHED, ESCAPED, LAUNCHED | CUTOFF, LAUNCHED | TIMEOUT], size=n))
    return rec


def farfield_reference(rec, ntheta, nphi):
    """(want, bound, count): long double [ntheta][nphi] histogram of the header's formula with bins from
    api.farfield_bins, the per-bin bound (m - 1) 2^-53 sum |terms| for the m terms of a bin in any order, and m."""
    from cbet_raytracing_3d_amd import api
    ld = np.longdouble
    r = rec[(rec["status"] & (LAUNCHED | ESCAPED)) == (LAUNCHED | ESCAPED)]
    with np.errstate(invalid="ignore", divide="ignore"):
        ct, cp = api.farfield_bins(r["vx"], r["vy"], r["vz"], ntheta, nphi)

    def idx(c, n):       # min(n - 1, floor(c)); a coordinate that is not > 0 (NaN included) is bin 0
        return np.minimum(np.floor(np.where(c > 0.0, c, 0.0)), n - 1).astype(np.int64)

    it, ip = idx(ct, ntheta), idx(cp, nphi)
    want = np.zeros((ntheta, nphi), dtype=ld)
    mag = np.zeros((ntheta, nphi), dtype=ld)
    count = np.zeros((ntheta, nphi), dtype=np.int64)
    np.add.at(want, (it, ip), r["uray"].astype(ld))
    np.add.at(mag, (it, ip), np.abs(r["uray"]).astype(ld))
    np.add.at(count, (it, ip), 1)
    bound = np.maximum(count - 1, 0) * ld(EPS) * mag
    return want, bound, count
