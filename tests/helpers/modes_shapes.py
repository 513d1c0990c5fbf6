"""Mode-spectrum cases off the cube, shared by tests/test_modes_host.py (host twin against numpy / scipy) and
tests/test_gpu_modes.py (device against the host twin): three different sides, off-centre and unequally spaced boxes, a
centre outside the box, run-time lmax below the instantiated one (odd ones among them), and shells that hold no node."""
import numpy as np

# first edge > 0 (the core is in no shell), a shell too thin to hold a node ([0.03, 0.0300001)), one beyond every node of
# a box around its centre ([0.5, 0.9))
EDGES = np.array([0.01, 0.03, 0.0300001, 0.08, 0.13, 0.2, 0.5, 0.9])
THIN = 1                    # index of the thin shell

# name, (nx, ny, nz), box overrides, centre, lmax
CASES = [
    ("off_centre_box", (9, 14, 21), dict(xmin=-0.10, xmax=0.16, ymin=-0.15, ymax=0.11, zmin=-0.12, zmax=0.14),
     (0.011, -0.007, 0.003), 5),
    ("long_z", (12, 7, 70), {}, (0.0, 0.0, 0.0), 17),
    ("thin_y", (7, 20, 11), dict(ymin=-0.04, ymax=0.04), (0.002, 0.001, -0.003), 3),
    ("centre_outside", (6, 9, 13), {}, (0.3, 0.0, 0.0), 1),
]
NAMES = [c[0] for c in CASES]
BY_NAME = {c[0]: c for c in CASES}


def params(api, name, **overrides):
    _, (nx, ny, nz), box, _, _ = BY_NAME[name]
    p = api.default_params(nx, **dict(box, **overrides))
    p.ny, p.nz = ny, nz
    return p


def grids(name, count=3):
    """`count` haloed grids with values of both signs, seeded by the case."""
    _, (nx, ny, nz), _, _, _ = BY_NAME[name]
    rng = np.random.default_rng(20261018 + NAMES.index(name))
    return rng.uniform(-1.0, 3.0, (count, nx + 2, ny + 2, nz + 2)) * 1e15
