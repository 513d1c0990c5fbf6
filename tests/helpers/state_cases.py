"""The cases of tests/test_state_host.py and tests/test_gpu_state.py (local plasma state of the gain kernels, DESIGN.md section
16): ion fields for the meshes of helpers/mesh_cases.py, a numpy restatement of the state model formulated differently from
the library (helpers/mesh_cases.Restatement's brackets and eight-corner sum, the physics in cgs with the temperatures in
kelvin), the crowded synthetic field generator of tests/test_gpu_gain_shapes.py and the three-state node pattern of the gain
kernels' tests."""
import numpy as np

from helpers import mesh_cases as M

EV_K = 11604.5052                            # def.cuh:103, as the library has it
ESTAT, KB, C_CGS = 4.80320427e-10, 1.3806485279e-16, 29979245800.0
CROWDED = (13, 11, 148)                      # haloed 15 x 13 x 150: rows of 150 cells, three 64-cell state groups, the last of 22
TRACED = (48, 21, 134)
Z_GROUPS = (slice(0, 64), slice(64, 128), slice(128, None))
# (te_ev, ti_ev, z_ion): a corona, a cold dense shell, a hot mid-Z spot -- 8 x apart in te_ev
STATES = [dict(te_ev=2000.0, ti_ev=1000.0, z_ion=3.1), dict(te_ev=250.0, ti_ev=90.0, z_ion=2.2),
          dict(te_ev=900.0, ti_ev=1300.0, z_ion=5.3)]
TRIPLES = [(2000.0, 1000.0, 3.1), (88.0, 0.0, 1.0), (940.0, 470.0, 3.5), (3500.0, 5200.0, 13.0)]


def uniform_mesh(api, inputs, angles, center, te_ev, ions=None):
    """helpers/mesh_cases.profile_mesh with te = te_ev everywhere; ions = (ti_ev, z_ion): explicit arrays holding them."""
    _, r, ne, _ = inputs
    nth, nph = angles
    theta = None if nth == 1 else np.linspace(0.1, 3.0, nth)
    phi = None if nph == 1 else np.linspace(-3.0, 2.9, nph)
    full = lambda v: np.full((r.size, nth, nph), v)                             # noqa: E731
    ti, zbar = (None, None) if ions is None else (full(ions[0]), full(ions[1]))
    return api.Mesh(r, theta, phi, np.broadcast_to(ne[:, None, None], (r.size, nth, nph)), full(te_ev), None, center,
                    ti=ti, zbar=zbar)


def ions3d(arrays, seed=5):
    """Smooth-times-noise ti (eV) and zbar on mesh_cases.mesh3d's nodes: (ti, zbar)."""
    rng = np.random.default_rng(seed)
    R, T, P = np.meshgrid(arrays["r"], arrays["theta"], arrays["phi"], indexing="ij")
    noise = lambda: 1.0 + 0.05 * rng.uniform(-1.0, 1.0, R.shape)               # noqa: E731
    ti = (120.0 + 900.0 * R + 40.0 * np.cos(T) * np.cos(P)) * noise()
    zbar = (3.5 - 8.0 * R + 0.4 * np.sin(T) * np.sin(P + 0.3)) * noise()
    return ti, zbar


def mesh3d_ions(api, center=M.OFFSET, dense=1.0):
    """mesh_cases.mesh3d with ions3d's fields (dense: the density's factor): (mesh, arrays with "ti" and "zbar")."""
    _, a = M.mesh3d(api, center)
    a["ne"] = dense * a["ne"]
    a["ti"], a["zbar"] = ions3d(a)
    return api.Mesh(a["r"], a["theta"], a["phi"], a["ne"], a["te"], a["u"], a["center"], ti=a["ti"], zbar=a["zbar"]), a


def model(api, p, gp, te, ti, z):
    """(cs, gain_const) of the header's model in another formulation: the temperatures in kelvin first, the ion term
    as 3 Ti / Z beside Te, one quotient for the constant."""
    omega = api.derive(p).omega
    tk, ik = np.asarray(te) * EV_K, np.asarray(ti) * EV_K
    gc = (ESTAT ** 2 * 8.0 * np.pi * 1.0e7) / (4.0e3 * M.K_ME * C_CGS ** 2 * omega * KB * (tk + 3.0 * ik / z))
    cs = 100.0 * np.sqrt(M.K_EC * KB * (z * tk + 3.0 * ik) / (KB * EV_K * gp.mi_over_me * M.K_ME))
    return cs, gc


def restated_table(api, p, gp, R, te, ti, zbar):
    """The state table [2, nx, ny, nz] from interpolated Te, Ti, Z (R: a mesh_cases.Restatement; ti / zbar None: the gain
    parameters'), and per component the largest value the model gives at any of the node's eight corners."""
    fields = [te, np.full(np.shape(te), gp.ti_ev) if ti is None else ti, np.full(np.shape(te), gp.z_ion) if zbar is None else zbar]
    cs, gc = model(api, p, gp, *[R.value(f)[0] for f in fields])
    corner = model(api, p, gp, *[R.corners(f)[0] for f in fields])
    return np.stack([cs, gc]), np.stack([np.abs(c).max(axis=(0, 1, 2)) for c in corner])


def crowded_fields(shape):
    """tests/test_gpu_gain_shapes.py's generator: up to ~54 of 60 beams per cell, energies of the order of real deposits
    (x 1e11), touched-but-absent (negative) and untouched entries: (fields [4, 60, ...], present mask)."""
    rng = np.random.default_rng(20261018)
    u = rng.random(shape)
    row = rng.random(shape[:3] + (1,))                          # a beam crosses a z-row or not
    x = np.arange(shape[1]).reshape(1, -1, 1, 1)
    density = np.where(x < 5, 0.15, np.where(x < 10, 0.45, 0.9))
    present = (row < density) & (u < 0.8)
    touched_only = (row < density + 0.03) & ~present & (u < 0.9)
    e = (rng.random(shape) * 1e3 + 1.0) * 1e11
    raw = np.zeros((4,) + shape)
    raw[0] = np.where(present, e, np.where(touched_only, -e, 0.0))
    raw[1:] = (rng.random((3,) + shape) - 0.5) * (raw[0] != 0)
    return raw, present


def node_pattern(shape, kz=3):
    """Which of the three STATES node (i, j, k) has: (i + 2 j + kz k) % 3.  kz = 3 is the pattern as the feature's request
    words it; 3 k is a multiple of 3, so that one varies with i and j only.  kz = 1 is the pattern the request describes: the
    state changes from cell to cell along z, inside every 16-cell run and every 64-cell group.  The tests run both."""
    i, j, k = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    return (i + 2 * j + kz * k) % 3


def cell_pattern(shape, kz=3):
    """The same for the haloed cells: cell (hi, hj, hk) takes the state of node (hi - 1, hj - 1, hk - 1), clamped."""
    idx = [np.clip(np.arange(n + 2) - 1, 0, n - 1) for n in shape]
    return node_pattern(shape, kz)[np.ix_(*idx)]
