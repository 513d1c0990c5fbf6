"""The cases of tests/test_saturation_host.py and tests/test_gpu_saturation.py (saturation of the ion-acoustic wave in the gain
kernels): the two grids of tests/test_gpu_gain_shapes.py, and two CPU references of the clamped update
that do not share a line with the library.

  Composed: the unchanged oracle.gain_field run once per unordered beam pair with every other beam's fields zeroed gives
      K_i^(ij) = G_ij I_j per cell; the amplitude follows from it and the deposited energies alone (in one cell the intensity is
      the energy over a common factor), the clamped K_i is the sum of the scaled pieces.
  Restatement: normalisation, prefactor, eta, P, clamp and amplitude map in numpy over flattened cells, the flow from
      api.flow_table, cs and gain_const from api.gain_constants or per node.

The limits of the tests are quantiles of a REFERENCE's own unclamped pair amplitudes (limits_from), never of the library's."""
import numpy as np

from helpers import state_cases as S

KC = 29979245800.0
BEAMS = [0, 16, 29, 38, 47, 55]
TRACED, CROWDED = S.TRACED, S.CROWDED
SLAB = (9, 22)
NEAR = 1e-9            # cells whose amplitude is this close (relative) to the limit are left out of the "clamps or not" comparison
NEAR_SHARE = 1e-3      # ... and may be this share of the non-zero cells at the most


def halo(node_array):
    """A node array [nx, ny, nz] on the haloed cells: cell (hi, hj, hk) reads node (hi - 1, hj - 1, hk - 1), clamped."""
    idx = [np.clip(np.arange(n + 2) - 1, 0, n - 1) for n in node_array.shape]
    return node_array[np.ix_(*idx)]


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


# ---- reference 1: the oracle, composed per pair ---------------------------------------------------------------------------
class Composed:
    """oracle.gain_field once per unordered pair (relax = 1, the other beams' fields zeroed): pieces[(i, j)] = K_i^(ij)."""

    def __init__(self, oracle, cfg, og, ofields, ne3d, kap, nthreads=1):
        nb = cfg.nbeams
        self.nb, self.E, self.kap = nb, ofields[0], kap
        self.pieces = {}
        for i in range(nb):
            for j in range(i + 1, nb):
                two = np.zeros_like(ofields)
                two[:, [i, j]] = ofields[:, [i, j]]
                g, _ = oracle.gain_field(cfg, og, two, ne3d, relax=1.0, nthreads=nthreads)
                self.pieces[(i, j)], self.pieces[(j, i)] = g[i].copy(), g[j].copy()

    def w(self, i, j):
        """|G_ij| sqrt(Ii Ij) = |K_i^(ij)| sqrt(E_i / E_j) where both beams are present, 0 elsewhere."""
        Ei, Ej = self.E[i], self.E[j]
        both = (Ei > 0) & (Ej > 0)
        return np.where(both, np.abs(self.pieces[(i, j)]) * np.sqrt(np.where(both, Ei, 0.0) / np.where(both, Ej, 1.0)), 0.0)

    def evaluated(self, i, j):
        """The cells in which the pair is evaluated: both present, sub-critical (kap > 0 there), a gain defined."""
        return (self.E[i] > 0) & (self.E[j] > 0) & (self.kap > 0)

    def amplitudes(self):
        """Unclamped amplitudes of the evaluated pairs, i < j: 1-D."""
        out = []
        for i in range(self.nb):
            for j in range(i + 1, self.nb):
                out.append((self.w(i, j) / np.where(self.kap > 0, self.kap, 1.0))[self.evaluated(i, j)])
        return np.concatenate(out)

    def gain(self, dn_max=0.0):
        """K_i = sum_j K_i^(ij) min(1, lim / w_ij), j increasing; dn_max = 0: no clamp."""
        K = np.zeros((self.nb,) + self.E.shape[1:])
        lim = dn_max * self.kap
        for i in range(self.nb):
            for j in range(self.nb):
                if j == i:
                    continue
                piece = self.pieces[(i, j)]
                if dn_max > 0:
                    w = self.w(i, j)
                    piece = piece * np.where(w > lim, lim / np.where(w > 0, w, 1.0), 1.0)
                K[i] += piece
        return K


def kappa_cells(api, p, ne3d):
    """kap = ((0.5 k0) frac) / sqrt(eps) on the haloed cells from a node table of ne; 0 at and above critical density."""
    d = api.derive(p)
    frac = halo(np.asarray(ne3d)) / d.ncrit
    eps = 1.0 - frac
    sub = eps > 0
    return np.where(sub, ((0.5 * (d.omega / KC)) * frac) / np.sqrt(np.where(sub, eps, 1.0)), 0.0)


# ---- reference 2: the numpy restatement -----------------------------------------------------------------------------------
class Restatement:
    """The gain update over flattened haloed cells.  flow: [3, nx, ny, nz]; cs, gc: None = api.gain_constants', or node
    arrays [nx, ny, nz]."""

    def __init__(self, api, p, gp, ne3d, flow, cs=None, gc=None):
        d = api.derive(p)
        _, cs0, gc0 = api.gain_constants(p, gp)
        flat = lambda a: halo(np.asarray(a, dtype=np.float64)).reshape(-1)        # noqa: E731
        self.grid = (p.nx + 2, p.ny + 2, p.nz + 2)
        frac = flat(ne3d) / d.ncrit
        eps = 1.0 - frac
        self.sub = eps > 0
        rt = np.where(self.sub, np.sqrt(np.where(self.sub, eps, 1.0)), 0.0)
        k0 = d.omega / KC
        self.kmag, self.ds = k0 * rt, (KC * rt) * d.dt
        self.u = [flat(flow[c]) for c in range(3)]
        self.cs = np.full(frac.shape, cs0) if cs is None else flat(cs)
        gcs = np.full(frac.shape, gc0) if gc is None else flat(gc)
        one = np.where(self.sub, rt, 1.0)
        self.pref = np.where(self.sub, gcs * frac * (1.0 / gp.iaw) / one, 0.0)
        self.kap = np.where(self.sub, ((0.5 * k0) * frac) / one, 0.0)
        self.iaw2 = gp.iaw * gp.iaw

    def normalise(self, raw):
        """(E, Dx, Dy, Dz) [4, nb, ...] -> I [nb, cells], k [3, nb, cells]."""
        nb = raw.shape[1]
        E, D = raw[0].reshape(nb, -1), raw[1:4].reshape(3, nb, -1)
        dn = np.sqrt(D[0] * D[0] + D[1] * D[1] + D[2] * D[2])
        ok = self.sub & (dn > 0)
        inten = np.where(ok & (E > 0), E / np.where(self.sub, self.ds, 1.0), 0.0)
        k = np.where(ok, self.kmag * (D / np.where(dn > 0, dn, 1.0)), 0.0)
        return inten, k

    def update(self, raw, limits=(0.0,), amplitudes=False):
        """One update from a zero gain with relax = 1 for each limit of `limits` (0 = none): dict(K [limits, nb, grid],
        amp [grid] the unclamped amplitude map, top [grid] the largest w of a cell, amps 1-D over the evaluated pairs if asked,
        I [nb, grid])."""
        inten, k = self.normalise(raw)
        nb, n = inten.shape
        K = np.zeros((len(limits), nb, n))
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
            eta = (0.0 - (q[0] * self.u[0][at] + q[1] * self.u[1][at] + q[2] * self.u[2][at])) / (np.where(ok, kiaw, 1.0) * self.cs[at] + 1e-10)
            e2 = eta * eta
            P = self.iaw2 * eta / ((e2 - 1.0) * (e2 - 1.0) + self.iaw2 * e2)
            G = np.where(ok, self.pref[at] * P, 0.0)
            w = np.abs(G) * np.sqrt(Ii * Ij)
            top[at] = np.maximum(top[at], w.max(axis=0))
            if amplitudes:
                amps.append((w / self.kap[at])[ok])
            for m, dn_max in enumerate(limits):
                Gc = G
                if dn_max > 0:
                    lim = dn_max * self.kap[at]
                    Gc = G * np.where(w > lim, lim / np.where(w > 0, w, 1.0), 1.0)
                Km = K[m]
                Km[i, at] += (Gc * Ij).sum(axis=0)
                Km[i + 1:, at] -= Gc * Ii
        amp = np.where(self.kap > 0, top / np.where(self.kap > 0, self.kap, 1.0), 0.0)
        out = dict(K=K.reshape((len(limits), nb) + self.grid), amp=amp.reshape(self.grid), top=top.reshape(self.grid),
                   I=inten.reshape((nb,) + self.grid), kap=self.kap.reshape(self.grid))
        if amplitudes:
            out["amps"] = np.concatenate(amps)
        return out


# ---- the two worlds, built once per session -------------------------------------------------------------------------------
_cache = {}


def params(api, shape, nbeams):
    p = api.default_params(shape[0], nbeams=nbeams)
    p.ny, p.nz = shape[1], shape[2]
    return p


def three_states(api, p, gp, shape, kz=1):
    """The three-state node table of helpers/state_cases (node_pattern with kz): [2, nx, ny, nz] of (cs, gain_const)."""
    consts = []
    for st in S.STATES:
        g = api.default_gain_params(relax=gp.relax, **st)
        consts.append(api.gain_constants(p, g)[1:])
    which = S.node_pattern(shape, kz)
    return np.stack([np.choose(which, [c[0] for c in consts]), np.choose(which, [c[1] for c in consts])])


def traced_world(api, oracle, inputs, nthreads):
    """TRACED: the oracle's traced fields of six beams, its whole-field gain, the composed reference and its limits."""
    if "traced" not in _cache:
        bn_all, r, ne, te = inputs
        bn = bn_all[BEAMS].copy()
        cfg = oracle.default_config(TRACED[0], nbeams=len(BEAMS), ny=TRACED[1], nz=TRACED[2])
        ne3d, kap3d = oracle.node_tables(cfg, r, ne, te)
        og = oracle.gain_default()
        ofields = np.stack([oracle.trace_cbet(cfg, og, bn, ne3d, kap3d, quantity=q, per_beam=True, nthreads=nthreads)[0]
                            for q in (1, 2, 3, 4)])
        ogain, _ = oracle.gain_field(cfg, og, ofields, ne3d, relax=1.0, nthreads=nthreads)
        p = params(api, TRACED, len(BEAMS))
        gp = api.default_gain_params(relax=1.0)
        comp = Composed(oracle, cfg, og, ofields, ne3d, kappa_cells(api, p, ne3d), nthreads)
        amps = comp.amplitudes()
        flow = api.flow_table(p, gp, None)
        state = three_states(api, p, gp, TRACED, kz=1)
        shifted = api.flow_table(p, gp, api.Target((20e-4, 0.0, -15e-4)))
        _cache["traced"] = dict(flow=flow, shifted=shifted, state=state, restated=Restatement(api, p, gp, ne3d, flow),
                                tabled=Restatement(api, p, gp, ne3d, shifted, cs=state[0], gc=state[1]), raw=ofields,
                                bn=bn, cfg=cfg, og=og, ne3d=ne3d, ofields=ofields, ogain=ogain, scale=float(np.abs(ogain).max()),
                                p=p, gp=gp, composed=comp, amps=amps, limits=limits_from(amps))
    return _cache["traced"]


def crowded_world(api, oracle, inputs, nthreads):
    """CROWDED: sixty beams' synthetic fields, the oracle's whole-field gain, the restatement without a table and with a
    caller's flow table plus the three-state table (kz = 1), each with its own limits."""
    if "crowded" not in _cache:
        bn, r, ne, te = inputs
        cfg = oracle.default_config(CROWDED[0], nbeams=60, ny=CROWDED[1], nz=CROWDED[2])
        ne3d, _ = oracle.node_tables(cfg, r, ne, te)
        p = params(api, CROWDED, 60)
        gp = api.default_gain_params(relax=1.0)
        raw, present = S.crowded_fields((60,) + (CROWDED[0] + 2, CROWDED[1] + 2, CROWDED[2] + 2))
        ogain, _ = oracle.gain_field(cfg, oracle.gain_default(), raw, ne3d, relax=1.0, nthreads=nthreads)
        flow = api.flow_table(p, gp, None)
        state = three_states(api, p, gp, CROWDED, kz=1)
        shifted = api.flow_table(p, gp, api.Target((20e-4, 0.0, -15e-4)))
        plain = Restatement(api, p, gp, ne3d, flow)
        tabled = Restatement(api, p, gp, ne3d, shifted, cs=state[0], gc=state[1])
        _cache["crowded"] = dict(bn=bn, cfg=cfg, ne3d=ne3d, raw=raw, ogain=ogain, scale=float(np.abs(ogain).max()), p=p, gp=gp,
                                 flow=flow, shifted=shifted, state=state, plain=plain, tabled=tabled)
    return _cache["crowded"]


def reference(world, which, names=("half", "deep", "all")):
    """A restatement's unclamped update with its pair amplitudes, its limits, and the clamped updates for `names`: cached in
    the world under `which` ("plain" / "tabled", or "restated" on TRACED)."""
    key = "ref_" + which
    if key not in world:
        R, raw = world[which], world.get("raw", world.get("ofields"))
        first = R.update(raw, amplitudes=True)
        limits = limits_from(first["amps"])
        clamped = R.update(raw, limits=[limits[n] for n in names])
        world[key] = dict(K0=first["K"][0], amp=first["amp"], top=first["top"], kap=first["kap"], I=first["I"], amps=first["amps"],
                          limits=limits, K={n: clamped["K"][m] for m, n in enumerate(names)})
    return world[key]
