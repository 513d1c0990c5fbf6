"""The cases of tests/test_lpi_host.py and tests/test_gpu_lpi.py (the quarter-critical LPI maps) and their
CPU reference: lpi_reference, a numpy restatement of the model written from the TEXT of csrc/cbet_lpi_model.h -- vectorised over
the cells, a plain loop over the beams in increasing order (never np.sum over the beam axis: that sums pairwise), sharing no
line with the library.

  TRACED   gain_worlds.traced_world: 48 x 21 x 134, six beams, the oracle's traced fields normalised by
           gain_reference.Restatement (the host path of the exchange matrix's tests), Te per node from the oracle's own
           (ne3d, kappa3d), band (0.20, 0.25), 8 cone bins: every arm of the bin logic runs.
  CROWDED  gain_worlds.crowded_world: 13 x 11 x 148, sixty beams, touched-but-absent and untouched entries, super-critical
           nodes, ragged bricks, rows off a 128-byte line; band (0.15, 0.25), and once more with the band (0.0, 0.999).
  RAMP     9 x 7 x 40, a caller's ne3d = n0 exp(-(z - zmin) / L), three synthetic beams: L_n = dz / sinh(dz / L) at interior
           nodes, two beams mirrored about z in one bin, a third antiparallel to the gradient in the last bin.

Each builder asserts its regime on the CPU and caches its case for the session."""
import numpy as np

from helpers import exchange_cases as XC
from helpers import gain_worlds as W
from helpers.gain_reference import KC, halo

EC, ME = 1.60217662e-19, 9.10938356e-31
NQ = 7
BAND, I_SUM, I_CW, I_MAX, LN, ETA_SUM, ETA_CW = range(NQ)
EDGE = 1e-9                # a present beam's (1 - mu) NB / 2 this close to an integer: its bin may differ between two roundings
COUNTS = ("band_cells", "lit_cells", "above_max", "above_cw", "above_sum", "max_present", "argmax_cw")
MAXIMA = ("max_eta_max", "max_eta_cw", "max_eta_sum")
SUMS = ("sum_I_sum", "sum_I_cw")


def lambda_um(api, p):
    return 2.0 * np.pi * KC / api.derive(p).omega * 1e4


def _axis_gradient(ne, axis, d):
    n = ne.shape[axis]
    if n < 3:
        return np.zeros_like(ne)
    a = np.moveaxis(ne, axis, 0)
    g = np.empty_like(a)
    g[1:-1] = (a[2:] - a[:-2]) / (2.0 * d)
    g[0] = (a[2] - a[0]) / (2.0 * d)
    g[-1] = (a[-1] - a[-3]) / (2.0 * d)
    return np.moveaxis(g, 0, axis)


def lpi_reference(api, p, fields, ne3d, te, band=(0.20, 0.25), cone_bins=8, planes=None):
    """(stack [7, grid], summary dict, near [grid]) of normalised fields [4, nb, grid]; te: a float or a node array, eV;
    planes = (lo, hi): those x planes only, zeros elsewhere.  near: cells with a present beam within EDGE of a bin edge."""
    d = api.derive(p)
    ne3d = np.asarray(ne3d, dtype=np.float64)
    grid = (p.nx + 2, p.ny + 2, p.nz + 2)
    gx, gy, gz = (_axis_gradient(ne3d, ax, dd) for ax, dd in ((0, d.dx), (1, d.dy), (2, d.dz)))
    gn = np.sqrt(gx * gx + gy * gy + gz * gz)
    with np.errstate(divide="ignore", invalid="ignore"):
        Ln = np.where(gn == 0, 0.0, ne3d / gn)
        te = np.full(ne3d.shape, float(te)) if np.isscalar(te) else np.asarray(te, dtype=np.float64)
        T = np.where((te > 0) & (Ln != 0), ((Ln * 1e4) * lambda_um(api, p)) / (81.86 * (te * 1e-3)), 0.0)
    ne, gx, gy, gz, gn, Ln, T = (halo(a) for a in (ne3d, gx, gy, gz, gn, Ln, T))
    frac = ne / d.ncrit
    inband = (band[0] <= frac) & (frac <= band[1])
    if planes is not None:
        keep = np.zeros(grid, dtype=bool)
        keep[planes[0]:planes[1]] = True
        inband &= keep
    Isum, Imax, npres = np.zeros(grid), np.zeros(grid), np.zeros(grid, dtype=np.int64)
    bins = np.zeros((cone_bins,) + grid)
    near = np.zeros(grid, dtype=bool)
    for b in range(p.nbeams):                                     # beams in increasing order, every sum in that order
        I, kx, ky, kz = (fields[c, b] for c in range(4))
        kn = np.sqrt(kx * kx + ky * ky + kz * kz)
        pres = inband & (I > 0) & (kn > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            mu = np.where(gn != 0, ((kx * gx + ky * gy) + kz * gz) / (kn * gn), 1.0)
        mu = np.where(pres, np.clip(mu, -1.0, 1.0), 1.0)
        t = (1.0 - mu) * (0.5 * cone_bins)
        which = np.minimum(cone_bins - 1, t.astype(np.int64))
        near |= pres & (np.abs(t - np.rint(t)) < EDGE)
        Isum = np.where(pres, Isum + I, Isum)
        Imax = np.where(pres & (I > Imax), I, Imax)
        npres += pres
        for q in range(cone_bins):
            sel = pres & (which == q)
            bins[q] = np.where(sel, bins[q] + I, bins[q])
    Icw = bins.max(axis=0)
    eta = lambda x: (x * 1e-14) * T                               # noqa: E731
    stack = np.stack([inband.astype(np.float64), Isum, Icw, Imax, Ln, eta(Isum), eta(Icw)])
    stack[1:] = np.where(inband, stack[1:], 0.0)
    cells = np.flatnonzero(inband.reshape(-1))
    flat = lambda a: a.reshape(-1)[cells]                         # noqa: E731
    ecw, esum, emax = flat(stack[ETA_CW]), flat(stack[ETA_SUM]), flat(eta(Imax))
    summary = dict(band_cells=int(cells.size), lit_cells=int((flat(npres) >= 1).sum()),
                   above_max=int((emax >= 1).sum()), above_cw=int((ecw >= 1).sum()), above_sum=int((esum >= 1).sum()),
                   argmax_cw=int(cells[np.argmax(ecw)]) if cells.size else -1,
                   max_eta_max=float(emax.max()) if cells.size else 0.0, max_eta_cw=float(ecw.max()) if cells.size else 0.0,
                   max_eta_sum=float(esum.max()) if cells.size else 0.0,
                   sum_I_sum=float(flat(stack[I_SUM]).sum()), sum_I_cw=float(flat(stack[I_CW]).sum()),
                   max_present=int(flat(npres).max()) if cells.size else 0)
    return stack, summary, near & inband


def any_order_bound(terms):
    """The bound on the difference of two sums of the same n non-negative terms taken in any two orders: each is within
    (n - 1) 2^-53 sum |terms| of the exact sum (tests/test_gpu_exit_arms.py's rule for k_exit_tally), so twice that apart."""
    terms = np.asarray(terms, dtype=np.float64).reshape(-1)
    return 2.0 * max(terms.size - 1, 0) * 2.0 ** -53 * float(np.abs(terms).sum())


def table_te(api, p, ne3d, kap3d):
    """Te (eV) per node from (ne3d, kappa3d): cbet_node_model.h's kappa() inverted, as RayTracer.table_te does on the device."""
    d = api.derive(p)
    live = (ne3d > 0) & (kap3d > 0)
    x = (5.2e-4 * 1e6) * ne3d * ne3d * (EC * EC / ME) * d.dt / (d.ncrit * np.where(live, kap3d, 1.0))
    return np.where(live, x ** (2.0 / 3.0), 0.0)


def profile_te(api, p, r, te):
    """The Te profile interpolated linearly at every node's radius (the end values beyond the profile's ends), [nx, ny, nz]: what
    the tabulation puts into kappa3d's formula at a node of the spherical target about the origin."""
    x, y, z = api.node_coordinates(p)
    rho = np.sqrt(x * x + y * y + z * z)
    r, te = np.asarray(r, dtype=np.float64), np.asarray(te, dtype=np.float64)
    if r[0] > r[-1]:
        r, te = r[::-1], te[::-1]
    assert (np.diff(r) > 0).all()
    return np.interp(rho, r, te)


_cache = {}


def _case(name, p, fields, ne3d, te, band, nbins):
    return dict(name=name, p=p, fields=np.ascontiguousarray(fields), ne3d=np.ascontiguousarray(ne3d), te=te, band=band, nbins=nbins)


def _with_reference(api, c):
    c["ref"], c["ref_summary"], c["near"] = lpi_reference(api, c["p"], c["fields"], c["ne3d"], c["te"], c["band"], c["nbins"])
    return c


def traced_case(api, oracle, inputs, nthreads):
    if "traced" not in _cache:
        w = W.traced_world(api, oracle, inputs, nthreads)
        if "xfields" not in w:
            w["xfields"], w["xI"], w["xk"] = XC.normalised(w["restated"], w["ofields"])
        _, r, ne, te = inputs
        ne3d, kap3d = oracle.node_tables(w["cfg"], r, ne, te)
        assert np.array_equal(ne3d, w["ne3d"])
        c = _with_reference(api, _case("traced", w["p"], w["xfields"], ne3d, table_te(api, w["p"], ne3d, kap3d), (0.20, 0.25), 8))
        c["bn"] = w["bn"]
        s, ref = c["ref_summary"], c["ref"]
        inb = ref[BAND] > 0
        npres = (c["fields"][0] > 0).sum(axis=0)[inb]
        # the regime: a populated band where beams overlap, every arm of the bin logic taken, no beam on a bin edge
        assert s["band_cells"] >= 800 and (npres >= 2).sum() >= 800 and (npres >= 3).sum() >= 500, s
        assert int((ref[I_CW][inb] < ref[I_SUM][inb]).sum()) >= 500
        assert int((ref[I_CW][inb] > ref[I_MAX][inb]).sum()) >= 100
        assert int((ref[I_CW][inb] == ref[I_SUM][inb]).sum()) >= 10
        assert not c["near"].any()
        assert _bins_used(api, c) == set(range(8))
        te_band, ln_band = halo(c["te"])[inb], ref[LN][inb]
        assert 600 < te_band.min() and te_band.max() < 900 and 100e-4 < ln_band.min() and ln_band.max() < 300e-4
        _cache["traced"] = c
    return _cache["traced"]


def _bins_used(api, c):
    """The cone bins that hold a present beam in some band cell."""
    d = api.derive(c["p"])
    gx, gy, gz = (halo(_axis_gradient(c["ne3d"], ax, dd)) for ax, dd in ((0, d.dx), (1, d.dy), (2, d.dz)))
    gn = np.sqrt(gx * gx + gy * gy + gz * gz)
    inb = c["ref"][BAND] > 0
    used = set()
    for b in range(c["p"].nbeams):
        I, kx, ky, kz = (c["fields"][x, b] for x in range(4))
        kn = np.sqrt(kx * kx + ky * ky + kz * kz)
        lit = inb & (I > 0) & (kn > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            mu = np.clip(np.where(gn != 0, ((kx * gx + ky * gy) + kz * gz) / (kn * gn), 1.0), -1.0, 1.0)
        which = np.minimum(c["nbins"] - 1, ((1.0 - mu[lit]) * (0.5 * c["nbins"])).astype(np.int64))
        used |= set(int(q) for q in np.unique(which))
    return used


def crowded_case(api, oracle, inputs, nthreads, wide=False):
    """CROWDED with the band (0.15, 0.25): 488 band cells, all in the planes 5 .. 9, 10 to 30 beams present in each.  The cells
    with 40 and more beams and the sub-critical cells without any lie outside that band on this grid (the planes from 10 on and
    below 5), so wide=True is the same case with the band (0.0, 0.999) -- every sub-critical cell -- which holds both."""
    name = "crowded_wide" if wide else "crowded"
    if name not in _cache:
        w = W.crowded_world(api, oracle, inputs, nthreads)
        if "xfields" not in w:
            w["xfields"], w["xI"], w["xk"] = XC.normalised(w["plain"], w["raw"])
        _, r, ne, te = inputs
        ne3d, kap3d = oracle.node_tables(w["cfg"], r, ne, te)
        assert np.array_equal(ne3d, w["ne3d"])
        band = (0.0, 0.999) if wide else (0.15, 0.25)
        c = _with_reference(api, _case(name, w["p"], w["xfields"], ne3d, table_te(api, w["p"], ne3d, kap3d), band, 8))
        c["bn"] = w["bn"]
        inb = c["ref"][BAND] > 0
        npres = (c["fields"][0] > 0).sum(axis=0)[inb]
        assert c["ref_summary"]["band_cells"] >= 400 and npres.max() >= 25, (c["ref_summary"], npres.max(), npres.min())
        if wide:
            assert npres.max() >= 40 and npres.min() == 0 and not inb.all()       # crowded cells, empty ones, super-critical ones
            assert c["ref_summary"]["lit_cells"] < c["ref_summary"]["band_cells"]
        assert int(c["near"].sum()) <= 0.01 * c["ref_summary"]["band_cells"]
        _cache[name] = c
    return _cache[name]


RAMP = (9, 7, 40)
RAMP_BAND = (0.10, 0.30)
RAMP_I = (2e14, 1e14, 1.5e14)


def ramp_case(api):
    """ne = 0.4 ncrit exp(-(z - zmin) / L), L = 12 dz, uniform in x and y; beams 0 and 1 at (+-0.6, 0, -0.8) |k|, beam 2 along +z,
    antiparallel to the gradient (which points to -z); beam 2 alone in plane 3, no beam in plane 4; Te = 2 keV."""
    if "ramp" not in _cache:
        p = W.params(api, RAMP, 3)
        d = api.derive(p)
        L = 12.0 * d.dz
        z = np.arange(p.nz) * d.dz
        ne3d = np.broadcast_to(0.4 * d.ncrit * np.exp(-z / L), RAMP).copy()
        grid = (p.nx + 2, p.ny + 2, p.nz + 2)
        kmag = 1.5e5
        fields = np.zeros((4, 3) + grid)
        for b, (I, dirn) in enumerate(zip(RAMP_I, ((0.6, 0.0, -0.8), (-0.6, 0.0, -0.8), (0.0, 0.0, 1.0)))):
            fields[0, b] = I
            for x in range(3):
                fields[1 + x, b] = kmag * dirn[x]
        fields[:, :2, 3] = 0.0
        fields[:, :, 4] = 0.0
        c = _with_reference(api, _case("ramp", p, fields, ne3d, 2000.0, RAMP_BAND, 8))
        c["L"], c["dz"] = L, d.dz
        # beam 2 has mu = -1 exactly: (1 - mu) NB / 2 = NB, an integer, and min() puts it into bin NB - 1 whatever the rounding
        # of its neighbours would do -- no cell of this case is left out of a comparison
        c["near"][:] = False
        assert c["ref_summary"]["band_cells"] >= 10 * grid[0] * grid[1]
        _cache["ramp"] = c
    return _cache["ramp"]
