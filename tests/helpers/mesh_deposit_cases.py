"""The cases of tests/test_mesh_deposit_host.py and tests/test_gpu_mesh_deposit.py (deposit on the hydro mesh, DESIGN.md
section 15) and a numpy restatement of the contract in include/cbet_mi355x.h, formulated differently from the library:
the cell of a sample from its true angles -- arctan2 for theta and for phi, searchsorted on the edges themselves, no
cosine or diamond-angle table -- and the sums with np.add.at.

Two formulations of a binning agree exactly only where no sample sits on an edge, so the restatement asserts its own
precondition: no sample of a case lies within MARGIN (relative for r, radians for the angles) of an edge; the roundings of
either formulation are ~1e-15.  The cases below were chosen so that this holds.

Bounds.  A sum of n fp64 terms taken in ANY order (any tree) differs from the exact sum by at most (n - 1) 2^-53 sum|terms|
(tests/helpers/exit_cases.py uses the same bound for the tally).  Two such sums of the same terms therefore differ by at
most 2 (n - 1) 2^-53 sum|terms|; the tests allow 2 n 2^-53 sum|terms| per cell, n = the cell's samples.  The device books
a run of k samples of one node as one term (E inv) k: one rounding in place of k - 1 additions, inside the same bound.
sum|terms| is itself a computed sum (relative error <= n 2^-53); the slack 2 * 2^-53 sum|terms| between 2 (n - 1) and 2 n
covers that for every n < 9e7."""
import numpy as np

EPS = 2.0 ** -53
MARGIN = 1e-9
TWO_PI = 6.283185307179586
CENTER = (0.0031, -0.0017, 0.0023)
R_EDGES = 0.11 * (np.arange(12) / 11.0) ** 1.3
THETA_EDGES = np.pi * (np.arange(8) / 7.0) ** 1.1
PHI_EDGES = 0.3 + 2.0 * np.pi * np.arange(10) / 9.0
BOX_A = ((-0.05, 0.06), (-0.07, 0.05), (-0.06, 0.065))
BOX_B = ((-0.06, 0.06), (-0.05, 0.055), (-0.07, 0.07))
# name: (grid, box, S)
CASES = {
    "9x14x21-S2": ((9, 14, 21), BOX_A, 2),
    "12x7x70-S1": ((12, 7, 70), BOX_B, 1),
    "6x9x13-S3": ((6, 9, 13), BOX_B, 3),
    "7x20x11-S4": ((7, 20, 11), BOX_B, 4),
}
BIG = ((104, 101, 103), BOX_B, 1)       # 1,081,912 haloed nodes and more: the kernel's grid-stride loop turns
KINDS = ("1d", "2d", "3d")


def edges(kind):
    """(r_edges, theta_edges, phi_edges) of the 11x1x1, 11x7x1 and 11x7x9 cells."""
    return (R_EDGES, None if kind == "1d" else THETA_EDGES, PHI_EDGES if kind == "3d" else None)


def params(api, shape, box):
    p = api.default_params(shape[0])
    p.ny, p.nz = shape[1], shape[2]
    (p.xmin, p.xmax), (p.ymin, p.ymax), (p.zmin, p.zmax) = box
    return p


def cells(api, kind, center=CENTER, gpu=None, **kw):
    return api.MeshCells(*edges(kind), center=center, gpu=gpu, **kw)


def grids(shape, ngrids, seed, pitch=None):
    """[ngrids, nx+2, ny+2, row] seeded, non-negative, about 40 % exact zeros; pitch: row length, NaN beyond nz + 2."""
    rng = np.random.default_rng(seed)
    full = (ngrids, shape[0] + 2, shape[1] + 2, shape[2] + 2)
    g = rng.uniform(0.0, 1.0, full) * (rng.uniform(0.0, 1.0, full) < 0.6)
    if pitch is None:
        return g
    out = np.full(full[:3] + (pitch,), np.nan)
    out[..., : shape[2] + 2] = g
    return out


def samples(api, p, center, S):
    """The coordinates of every sample relative to the centre, [nx+2, ny+2, nz+2, S, S, S] each, by the header's
    statements (numpy's elementwise fp64 operations are the library's)."""
    d = api.derive(p)
    off = np.array([(2 * a + 1 - S) / (2.0 * S) for a in range(S)])
    ax = []
    for n, step, lo, o in ((p.nx, d.dx, p.xmin, center[0]), (p.ny, d.dy, p.ymin, center[1]), (p.nz, d.dz, p.zmin, center[2])):
        node = (np.arange(n + 2) - 1) * step + lo
        ax.append((node[:, None] + off[None, :] * step) - o)                       # [n+2, S]
    sx = ax[0][:, None, None, :, None, None]
    sy = ax[1][None, :, None, None, :, None]
    sz = ax[2][None, None, :, None, None, :]
    return np.broadcast_arrays(sx, sy, sz)


def _margin(values, edge_list, relative_to=None):
    gap = np.min(np.abs(values[..., None] - np.asarray(edge_list)), axis=-1)
    return gap / relative_to if relative_to is not None else gap


class Restatement:
    """Cell of every sample of grid `p` for the cells (r_edges, theta_edges, phi_edges) about `center`, S sub-samples per
    axis.  cell: flat index into [nr, ntheta, nphi], -1 outside every shell.  The header's degenerate rule for rho == 0
    (row 0, column 0) is stated here too; arctan2 gives the others (0 on the axis, 0 / pi at the poles)."""

    def __init__(self, api, p, r_edges, theta_edges, phi_edges, center, S):
        sx, sy, sz = samples(api, p, center, S)
        rho = np.sqrt(sx * sx + sy * sy + sz * sz)
        self.S, self.shape = S, (len(r_edges) - 1, 1 if theta_edges is None else len(theta_edges) - 1,
                                 1 if phi_edges is None else len(phi_edges) - 1)
        nr, nth, nph = self.shape
        m = np.searchsorted(r_edges, rho, side="right") - 1
        inside = (m >= 0) & (m < nr)
        live = rho > 0
        assert _margin(rho[live], r_edges, rho[live]).min() > MARGIN, "a sample lies on an r edge"
        row = np.zeros(rho.shape, dtype=np.int64)
        if nth > 1:
            theta = np.arctan2(np.sqrt(sx * sx + sy * sy), sz)
            assert _margin(theta[live], theta_edges[1:-1]).min() > MARGIN, "a sample lies on a theta edge"
            row = np.searchsorted(theta_edges[1:-1], theta, side="right")
        col = np.zeros(rho.shape, dtype=np.int64)
        if nph > 1:
            phi = np.arctan2(sy, sx)
            phi = np.where(phi < phi_edges[0], phi + TWO_PI, phi)
            assert _margin(phi[live], phi_edges).min() > MARGIN, "a sample lies on a phi edge"
            col = np.searchsorted(phi_edges[:nph], phi, side="right") - 1
        row, col = np.where(live, row, 0), np.where(live, col, 0)
        self.cell = np.where(inside, (np.clip(m, 0, nr - 1) * nth + row) * nph + col, -1)
        self.ncell = nr * nth * nph
        self.counts = np.bincount(self.cell[inside], minlength=self.ncell).reshape(self.shape)
        self.n_outside = int((~inside).sum())

    def deposit(self, grid):
        """(cell_energy [G, nr, ntheta, nphi], outside [G]) of grids [G, nx+2, ny+2, >= nz+2]."""
        nz2 = self.cell.shape[2]
        inv = 1.0 / (self.S * self.S * self.S)
        energy, outside = np.zeros((grid.shape[0], self.ncell + 1)), None
        slot = np.where(self.cell >= 0, self.cell, self.ncell).reshape(-1)      # the last slot: outside
        for g in range(grid.shape[0]):
            terms = np.broadcast_to((grid[g, :, :, :nz2] * inv)[..., None, None, None], self.cell.shape)
            np.add.at(energy[g], slot, terms.reshape(-1))
        outside = energy[:, -1].copy()
        return energy[:, :-1].reshape((grid.shape[0],) + self.shape), outside


def bounds(counts, n_outside, mag_energy, mag_outside):
    """The any-order bounds of the docstring: per cell and for `outside`."""
    return 2.0 * counts * EPS * mag_energy, 2.0 * n_outside * EPS * mag_outside


def total_samples(p, S):
    return (p.nx + 2) * (p.ny + 2) * (p.nz + 2) * S ** 3


def check(got, want, counts_want, n_outside, mag=None, what=""):
    """got / want: (cell_energy [G, ...], outside [G], cell_samples).  Counts exactly, energies within the bounds, whose
    sum|terms| is mag = (cell_energy, outside) of the |grid| (default: want's, for non-negative grids)."""
    mag_e, mag_o = (np.abs(want[0]), np.abs(want[1])) if mag is None else mag
    assert np.array_equal(got[2], counts_want), what + ": cell_samples differ"
    be, bo = bounds(counts_want, n_outside, mag_e, mag_o)
    err_e, err_o = np.abs(got[0] - want[0]), np.abs(got[1] - want[1])
    assert np.all(err_e <= be), "%s: cell_energy off by %g at most, bound %g there" % (
        what, err_e.max(), be.reshape(-1)[np.argmax((err_e - be).reshape(-1)) % be.size])
    assert np.all(err_o <= bo), "%s: outside off by %s, bound %s" % (what, err_o, bo)
