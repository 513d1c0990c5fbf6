"""The meshes of tests/test_mesh_host.py and tests/test_gpu_mesh.py (hydro-mesh plasma) and a numpy
restatement of the model in include/cbet_mi355x.h, formulated differently from the library: brackets by searchsorted,
clamps by clipping the weights to [0, 1], the period by one extra phi column, the interpolation as an eight-corner sum."""
import numpy as np

UM = 1e-4                                   # cm
OFFSET = (20 * UM, -35 * UM, 10 * UM)
SHAPES = [(24, 24, 24), (20, 17, 25)]
SHAPE_IDS = ["24", "20x17x25"]
K_EC, K_ME = 1.60217662e-19, 9.10938356e-31  # def.cuh:63-64, as the library has them
TWO_PI = 6.283185307179586
TOL = 1e-12                                 # two formulations of one quantity


def params(api, shape, nbeams=4):
    p = api.default_params(shape[0], nbeams=nbeams)
    p.ny, p.nz = shape[1], shape[2]
    return p


def ramp(api, p, gp, r):
    """The gain kernels' radial flow speed at radii r (cbet_tabulate_flow's statements in numpy)."""
    cs = api.gain_constants(p, gp)[1]
    t = np.clip((r - gp.mach_r0) / (gp.mach_r1 - gp.mach_r0), 0.0, 1.0)
    return (gp.mach_0 + (gp.mach_1 - gp.mach_0) * t) * cs


def profile_mesh(api, inputs, angles, center=(0.0, 0.0, 0.0)):
    """Item 1: the s83177 profile as a mesh, alone (angles = (1, 1)) or broadcast over ntheta x nphi angles; its velocity
    is angle-independent too (the default ramp in ur, fractions of it in uth and uph)."""
    _, r, ne, te = inputs
    nth, nph = angles
    theta = None if nth == 1 else np.linspace(0.1, 3.0, nth)
    phi = None if nph == 1 else np.linspace(-3.0, 2.9, nph)
    full = lambda f: np.broadcast_to(f[:, None, None], (r.size, nth, nph))      # noqa: E731
    ur = ramp(api, params(api, SHAPES[0]), api.default_gain_params(), r)
    return api.Mesh(r, theta, phi, full(ne), full(te), (full(ur), full(0.1 * ur), full(-0.05 * ur)), center)


def mesh3d(api, center=OFFSET, seed=3, velocity=True):
    """Item 2: 37 x 9 x 14, all three coordinates non-uniform; theta cell-centred (both polar caps clamp), r[0] > 0 and
    r[last] = 0.17 cm inside the grid's corner radius 0.225 cm (both radial clamps occur), phi from -3.0 to 3.0 (the wrap
    bracket is 0.28 rad wide).  Fields: smooth, positive, times seeded noise of 5 %.  Returns (mesh, arrays)."""
    rng = np.random.default_rng(seed)
    nr, nth, nph = 37, 9, 14
    r = 0.012 + (0.17 - 0.012) * np.linspace(0.0, 1.0, nr) ** 1.3
    edges = np.pi * np.linspace(0.0, 1.0, nth + 1) ** 1.2
    theta = 0.5 * (edges[1:] + edges[:-1])
    phi = -3.0 + 6.0 * (np.linspace(0.0, 1.0, nph) ** 0.9)
    R, T, P = np.meshgrid(r, theta, phi, indexing="ij")
    wobble = 1.0 + 0.3 * np.cos(T) + 0.2 * np.sin(T) * np.cos(P - 0.4)
    noise = lambda: 1.0 + 0.05 * rng.uniform(-1.0, 1.0, R.shape)               # noqa: E731
    ne = 4e21 * np.exp(-R / 0.04) * wobble * noise()
    te = (300.0 + 2000.0 * R + 100.0 * np.sin(T) * np.sin(2 * P)) * noise()
    u = None
    if velocity:
        u = (3e7 * (R / 0.1) * wobble * noise(), 5e6 * np.sin(2 * T) * noise(), 4e6 * np.cos(P) * np.sin(T) * noise())
    arrays = dict(r=r, theta=theta, phi=phi, ne=ne, te=te, u=u, center=center)
    return api.Mesh(r, theta, phi, ne, te, u, center), arrays


class Restatement:
    """The model at every node of the grid `p`, for a mesh given as arrays (theta / phi None: no dependence)."""

    def __init__(self, api, p, r, theta, phi, center):
        d = api.derive(p)
        ax = [(np.arange(n) * step + lo) - o for n, step, lo, o in
              ((p.nx, d.dx, p.xmin, center[0]), (p.ny, d.dy, p.ymin, center[1]), (p.nz, d.dz, p.zmin, center[2]))]
        X, Y, Z = np.meshgrid(*ax, indexing="ij")
        self.X, self.Y, self.Z = X, Y, Z
        self.rho, self.rxy = np.sqrt(X * X + Y * Y + Z * Z), np.sqrt(X * X + Y * Y)
        self.dt, self.ncrit = d.dt, d.ncrit
        self.m, self.wr = self._bracket(np.asarray(r), self.rho)
        self.below, self.above = self.rho <= r[0], self.rho >= r[-1]
        if theta is None:
            self.j, self.wt = np.zeros(X.shape, int), np.zeros(X.shape)
            self.cap_lo = self.cap_hi = np.zeros(X.shape, bool)
        else:
            th = np.arctan2(self.rxy, Z)
            self.j, self.wt = self._bracket(np.asarray(theta), th)
            self.cap_lo, self.cap_hi = th <= theta[0], th >= theta[-1]
        if phi is None:
            self.k, self.wp = np.zeros(X.shape, int), np.zeros(X.shape)
            self.wrap = np.zeros(X.shape, bool)
        else:
            ph = np.arctan2(Y, X)
            ph = np.where(ph < phi[0], ph + TWO_PI, ph)
            self.k, self.wp = self._bracket(np.append(phi, phi[0] + TWO_PI), ph)      # one period more
            self.wrap = self.k == len(phi) - 1
        self.interior = ~(self.below | self.above | self.cap_lo | self.cap_hi | self.wrap)

    @staticmethod
    def _bracket(x, xp):
        if len(x) == 1:
            return np.zeros(xp.shape, int), np.zeros(xp.shape)
        i = np.clip(np.searchsorted(x, xp, side="right") - 1, 0, len(x) - 2)
        return i, np.clip((xp - x[i]) / (x[i + 1] - x[i]), 0.0, 1.0)

    def corners(self, f):
        """The eight corner values [2, 2, 2, nx, ny, nz] and their weights of a field [nr, ntheta, nphi]."""
        f = np.asarray(f, dtype=np.float64)
        f = np.concatenate([f, f[:, :, :1]], axis=2)                            # the extra column: phi[0] + 2 pi
        f = np.concatenate([f, f[:, -1:, :]], axis=1) if f.shape[1] == 1 else f  # (so that j + 1 exists when ntheta == 1)
        vals, wts = np.empty((2, 2, 2) + self.rho.shape), np.empty((2, 2, 2) + self.rho.shape)
        for a in (0, 1):
            for b in (0, 1):
                for c in (0, 1):
                    vals[a, b, c] = f[self.m + a, self.j + b, self.k + c]
                    wts[a, b, c] = (self.wr if a else 1 - self.wr) * (self.wt if b else 1 - self.wt) * (self.wp if c else 1 - self.wp)
        return vals, wts

    def value(self, f):
        """(the interpolated field, the largest |corner| per node)."""
        vals, wts = self.corners(f)
        return (vals * wts).sum(axis=(0, 1, 2)), np.abs(vals).max(axis=(0, 1, 2))

    def tables(self, ne, te):
        """(ne3d, kappa3d, bound on |ne3d error|, bound on |kappa3d error|) for TOL of the corner values in ne and Te:
        kappa = C ed^2 etemp^-1.5, so |d kappa| <= kappa (2 |d ed| / ed + 1.5 |d etemp| / etemp)."""
        ed, ne_top = self.value(ne)
        etemp, te_top = self.value(te)
        eta = 5.2e-5 * 10.0 / (etemp * np.sqrt(etemp))
        nuei = (1e6 * ed * (K_EC * K_EC) / K_ME) * eta
        kap = ed / self.ncrit * nuei * self.dt
        return ed, kap, TOL * ne_top, kap * TOL * (2.0 * ne_top / ed + 1.5 * te_top / etemp)

    def flow(self, ur, uth, uph):
        """[3, nx, ny, nz]: the interpolated components turned with the node's direction; (c1, s1) = (1, 0) on the axis,
        zero at the centre."""
        zero = np.zeros(self.rho.shape)
        u = [zero if f is None else self.value(f)[0] for f in (ur, uth, uph)]
        with np.errstate(divide="ignore", invalid="ignore"):
            ct, st = self.Z / self.rho, self.rxy / self.rho
            c1, s1 = np.where(self.rxy > 0, self.X / self.rxy, 1.0), np.where(self.rxy > 0, self.Y / self.rxy, 0.0)
        h = u[0] * st + u[1] * ct
        out = np.stack([h * c1 - u[2] * s1, h * s1 + u[2] * c1, u[0] * ct - u[1] * st])
        out[:, self.rho == 0] = 0.0
        return out
