"""The two CPU references of the gain update that the tests of the gain stage judge the kernels by (saturation, exchange matrix,
detuning, local state: DESIGN.md sections 16 to 19).  Neither shares a line with the library.

  Composed: the unchanged oracle.gain_field run once per unordered beam pair with every other beam's fields zeroed gives
      K_i^(ij) = G_ij I_j per cell; the amplitude follows from it and the deposited energies alone (in one cell the intensity is
      the energy over a common factor), the clamped K_i is the sum of the scaled pieces.
  Restatement: normalisation, prefactor, eta, P, clamp, amplitude map and exchange matrix in numpy over flattened cells, the
      flow from api.flow_table, cs and gain_const from api.gain_constants or per node.  Its `update` is the one pair loop of the
      tests: per-beam frequency shifts put the beat frequency into the resonance,

          eta_ij = ((0.0 - q . u) + (w_j - w_i)) / (|q| cs + 1e-10),        q = k_j - k_i,

      a list of limits clamps the ion-acoustic amplitude, `matrix` adds T[i][j] = sum over cells of ds g_ij I_i I_j and
      Gross[i][j] = the sum of the magnitudes, `planes` keeps the loop to a range of x planes."""
import numpy as np

KC = 29979245800.0


def halo(node_array):
    """A node array [nx, ny, nz] on the haloed cells: cell (hi, hj, hk) reads node (hi - 1, hj - 1, hk - 1), clamped."""
    idx = [np.clip(np.arange(n + 2) - 1, 0, n - 1) for n in node_array.shape]
    return node_array[np.ix_(*idx)]


def kappa_cells(api, p, ne3d):
    """kap = ((0.5 k0) frac) / sqrt(eps) on the haloed cells from a node table of ne; 0 at and above critical density."""
    d = api.derive(p)
    frac = halo(np.asarray(ne3d)) / d.ncrit
    eps = 1.0 - frac
    sub = eps > 0
    return np.where(sub, ((0.5 * (d.omega / KC)) * frac) / np.sqrt(np.where(sub, eps, 1.0)), 0.0)


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

    def update(self, raw, shift=None, limits=(0.0,), amplitudes=False, matrix=False, normalised=None, planes=None):
        """One update from a zero gain with relax = 1 for each limit of `limits` (0 = none).  shift: [nb] rad/s, None = no
        shifts.  normalised = (I, k): take these instead of normalising `raw`.  planes = (lo, hi): those x planes only.
        dict(K [limits, nb, grid], amp [grid] the unclamped amplitude map, top [grid] the largest w of a cell, I [nb, grid],
        kap [grid]; amplitudes=True: amps, 1-D over the evaluated pairs; matrix=True: T and G (Gross) [limits, nb, nb] of the
        pairwise exchange).  The statements of the loop follow the library's operation order."""
        inten, k = self.normalise(raw) if normalised is None else normalised
        nb, n = inten.shape
        w_b = np.zeros(nb) if shift is None else np.asarray(shift, dtype=np.float64)
        inside = None
        if planes is not None:
            inside = np.zeros(self.grid, dtype=bool)
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
            q = k[:, i + 1:, at] - k[:, i:i + 1, at]
            kiaw = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
            ok = (Ij > 0) & (kiaw > 0)
            dw = (w_b[i + 1:] - w_b[i])[:, None]
            eta = ((0.0 - (q[0] * self.u[0][at] + q[1] * self.u[1][at] + q[2] * self.u[2][at])) + dw) / (np.where(ok, kiaw, 1.0) * self.cs[at] + 1e-10)
            e2 = eta * eta
            P = self.iaw2 * eta / ((e2 - 1.0) * (e2 - 1.0) + self.iaw2 * e2)
            gain = np.where(ok, self.pref[at] * P, 0.0)
            w = np.abs(gain) * np.sqrt(Ii * Ij)
            top[at] = np.maximum(top[at], w.max(axis=0))
            if amplitudes:
                amps.append((w / self.kap[at])[ok])
            for m, dn_max in enumerate(limits):
                Gc = gain
                if dn_max > 0:
                    lim = dn_max * self.kap[at]
                    Gc = gain * np.where(w > lim, lim / np.where(w > 0, w, 1.0), 1.0)
                K[m][i, at] += (Gc * Ij).sum(axis=0)
                K[m][i + 1:, at] -= Gc * Ii
                if matrix:
                    x = self.ds[at] * Gc * Ii * Ij
                    T[m, i, i + 1:] = x.sum(axis=1)
                    G[m, i, i + 1:] = np.abs(x).sum(axis=1)
        amp = np.where(self.kap > 0, top / np.where(self.kap > 0, self.kap, 1.0), 0.0)
        out = dict(K=K.reshape((len(limits), nb) + self.grid), amp=amp.reshape(self.grid), top=top.reshape(self.grid),
                   I=inten.reshape((nb,) + self.grid), kap=self.kap.reshape(self.grid))
        if amplitudes:
            out["amps"] = np.concatenate(amps)
        if matrix:
            out["T"], out["G"] = T - np.transpose(T, (0, 2, 1)), G + np.transpose(G, (0, 2, 1))
        return out
