"""The cases of tests/test_exchange_host.py and tests/test_gpu_exchange_matrix.py (the pairwise exchange matrix, DESIGN.md
section 18): two CPU references of T[i][j] = sum over cells of ds g_ij I_i I_j and of Gross[i][j] = the sum of the magnitudes
that do not share a line with the library, on the worlds of helpers/gain_worlds.py.

  composed_matrix: T_ij = sum over cells of E_i K_i^(ij), K_i^(ij) the pieces of gain_reference.Composed -- the unchanged
      oracle run pair by pair; E_i = ds I_i is the deposited energy, so nothing of the normalisation is restated.
  pairwise_matrix: the pair loop of gain_reference.Restatement.update over normalised fields with matrix=True, one row of the
      matrix at a time.

normalised(): the fields a gain update leaves, from Restatement.normalise -- what both the host twin and pairwise_matrix read."""
import numpy as np

from helpers import saturation_cases as SC
from helpers.gain_worlds import SLABS as _SLABS

SLABS = [(0, 9), _SLABS["traced"]]          # and (22, nx + 2): the three slabs of the tests


def normalised(R, raw):
    """(fields [4, nb, grid] = (I, kx, ky, kz), I [nb, cells], k [3, nb, cells]) of raw fields (E, Dx, Dy, Dz)."""
    inten, k = R.normalise(raw)
    nb = inten.shape[0]
    fields = np.concatenate([inten[None], k]).reshape((4, nb) + R.grid)
    return np.ascontiguousarray(fields), inten, k


def _antisymmetric(T, G):
    return T - T.T, G + G.T


def pairwise_matrix(R, inten, k, dn_max=0.0, planes=None):
    """(T, Gross) of normalised fields by Restatement R's pair loop; planes = (lo, hi): those x planes only."""
    out = R.update(None, limits=[dn_max], matrix=True, normalised=(inten, k), planes=planes)
    return out["T"][0], out["G"][0]


def composed_matrix(comp, dn_max=0.0):
    """(T, Gross) from gain_reference.Composed: sum over cells of E_i K_i^(ij), the piece scaled by the clamp's factor."""
    nb = comp.nb
    T, G = np.zeros((nb, nb)), np.zeros((nb, nb))
    lim = dn_max * comp.kap
    for i in range(nb):
        for j in range(i + 1, nb):
            piece = comp.pieces[(i, j)]
            if dn_max > 0:
                w = comp.w(i, j)
                piece = piece * np.where(w > lim, lim / np.where(w > 0, w, 1.0), 1.0)
            x = np.where(comp.E[i] > 0, comp.E[i], 0.0) * piece
            T[i, j], G[i, j] = x.sum(), np.abs(x).sum()
    return _antisymmetric(T, G)


def row_sums(R, update):
    """sum over cells of ds I_i K_i for an update of Restatement.update (its K [nb, grid] and I [nb, grid])."""
    nb = update["I"].shape[0]
    return (R.ds[None] * update["I"].reshape(nb, -1) * update["K"].reshape(nb, -1)).sum(axis=1)


def never_together(fields, a, b, cut):
    """A copy of normalised fields in which beams a and b never share a cell: a is absent from the planes below `cut`, b from
    the others."""
    out = fields.copy()
    out[:, a, :cut] = 0.0
    out[:, b, cut:] = 0.0
    return out


def worst(got, want, gross):
    """max over the pairs of |got - want| / Gross (pairs that never exchange anything must agree exactly)."""
    live = gross > 0
    assert np.array_equal(got[~live], want[~live])
    return float((np.abs(got - want)[live] / gross[live]).max()) if live.any() else 0.0


def dense_fields(nb, grid, seed):
    """Synthetic raw fields [4, nb, grid] for the small shapes: each beam is present in ~70 % of the cells, touched but absent
    (negative energy) in ~10 %, untouched elsewhere; energies of the order of real deposits."""
    rng = np.random.default_rng(seed)
    shape = (nb,) + tuple(grid)
    u = rng.random(shape)
    e = (rng.random(shape) * 1e3 + 1.0) * 1e11
    raw = np.zeros((4,) + shape)
    raw[0] = np.where(u < 0.7, e, np.where(u < 0.8, -e, 0.0))
    raw[1:] = (rng.random((3,) + shape) - 0.5) * (raw[0] != 0)
    return raw


def limits_of(world, which):
    """The limits of a world's restatement `which` (saturation_cases.limits_from of ITS unclamped pair amplitudes)."""
    return SC.reference(world, which)["limits"]
