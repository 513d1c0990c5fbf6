"""The cases of tests/test_state_host.py and tests/test_gpu_state.py (local plasma state of the gain kernels, DESIGN.md section
16): ion fields for the meshes of helpers/mesh_cases.py, a numpy restatement of the state model formulated differently from
the library (helpers/mesh_cases.Restatement's brackets and eight-corner sum, the physics in cgs with the temperatures in
kelvin).  The crowded grid, its field generator and the three-state node pattern of the gain kernels' tests are in
helpers/gain_worlds.py."""
import numpy as np

from helpers import mesh_cases as M

EV_K = 11604.5052                            # def.cuh:103, as the library has it
ESTAT, KB, C_CGS = 4.80320427e-10, 1.3806485279e-16, 29979245800.0
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
