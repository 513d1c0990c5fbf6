"""The cases of tests/test_backscatter_host.py and tests/test_gpu_backscatter.py (backscatter SBS gain spectra along rays,
DESIGN.md section 24) and their CPU reference: sbs_reference, a numpy restatement of the model written from the TEXT of the
section -- a plain loop over the items, vectorised over an item's steps, the sum taken in step order -- sharing no line with
the library.

  RAGGED    helpers/exit_cases.RAGGED: 20 x 17 x 25 nodes, four beams, 426 live rays per beam of 11 .. 59 steps through the
            shipped plasma: strides sXh, sYh and the z pitch all differ.
  LONG_BOX  helpers/exit_cases.LONG_BOX: 24^3 nodes, y from -0.8 to 0.8 cm, the six axis beams, here WITH the shipped plasma
            (the path tests run it in vacuum): 124 live rays per beam.

oracle_world builds a world's stride-1 path records from the CPU oracle's ray_path once per session."""
import numpy as np

from helpers import config_matrix as M
from helpers import exit_cases as X
from helpers.gain_reference import KC

SEED = 20261021
STEP = 2.0 ** 38          # rad/s: the scans below are multiples of it; |k_iaw| cs is ~ 1e12 .. 6e12 rad/s on these rays

# the scans of the tests, in rad/s (negative = red): one shift, five (a partially filled NS = 8), eight, sixteen
SCANS = {1: [-8.0 * STEP], 5: [STEP * s for s in (-24.0, -12.0, -6.0, 0.0, 6.0)],
         8: [STEP * (s - 20.0) for s in range(0, 24, 3)], 16: [STEP * (2.0 * s - 26.0) for s in range(16)]}


def synthetic_fields(entry, seed=SEED):
    """Normalised-looking fields [4, nbeams, grid]: intensities uniform in (0, 1e15) W/cm^2 with one cell in seven at zero
    (a beam absent from the cell); the direction components are random and never read by the model."""
    rng = np.random.default_rng(seed)
    shape = (4, entry.nbeams(), entry.n + 2, entry.ny + 2, entry.nz + 2)
    f = rng.uniform(-1.0, 1.0, size=shape)
    f[0] = np.where(rng.integers(7, size=shape[1:]) == 0, 0.0, rng.uniform(0.0, 1e15, size=shape[1:]))
    return f


def path_records(api, entry_params, derived, lps, paths):
    """Stride-1 path records of oracle paths, as cbet_trace_paths lays them out: (samples [capacity, nitems] of
    api.PATH_DTYPE, turns [nitems] of api.TURN_DTYPE), capacity = 1 + the longest path.  steps and status as
    test_gpu_paths._oracle_status derives them; the closest-approach members stay zero (the twin does not read them)."""
    p, d = entry_params, derived
    n = len(paths)
    cap = 1 + max(len(path) for path in paths)
    S = np.zeros((cap, n), dtype=api.PATH_DTYPE)
    T = np.zeros(n, dtype=api.TURN_DTYPE)
    lo = (p.xmin - (d.dx / 2.0), p.ymin - (d.dy / 2.0), p.zmin - (d.dz / 2.0))
    hi = (p.xmax + (d.dx / 2.0), p.ymax + (d.dy / 2.0), p.zmax + (d.dz / 2.0))
    for k, (lp, path) in enumerate(zip(lps, paths)):
        m = len(path)
        S["x"][0, k], S["y"][0, k], S["z"][0, k], S["uray"][0, k] = lp
        S["x"][1:m + 1, k], S["y"][1:m + 1, k], S["z"][1:m + 1, k] = path[:, 0], path[:, 1], path[:, 2]
        S["ci"][1:m + 1, k], S["cj"][1:m + 1, k], S["ck"][1:m + 1, k] = (path[:, c].astype(np.int32) for c in (3, 4, 5))
        S["absorbed"][1:m + 1, k], S["uray"][1:m + 1, k] = path[:, 6], path[:, 7]
        S["step"][:m + 1, k] = np.arange(m + 1)
        x, y, z, u = path[-1, 0], path[-1, 1], path[-1, 2], path[-1, 7]
        cut = u <= 0.05 * lp[3]
        out = x < lo[0] or x > hi[0] or y < lo[1] or y > hi[1] or z < lo[2] or z > hi[2]
        status = X.LAUNCHED | (X.CUTOFF if cut else 0) | (X.ESCAPED if out else 0)
        if not (cut or out):
            status |= X.TIMEOUT
        T["steps"][k], T["status"][k], T["nsamples"][k] = m, status, m + 1
    return S, T


_cache = {}


def oracle_world(api, oracle, inputs, entry, every=1):
    """The world of `entry` on the CPU oracle, cached: params, derived, ne3d, the item list (every `every`-th live ray of every
    beam, beam by beam), the stride-1 records of the oracle's paths, and synthetic fields."""
    key = (entry.name, every)
    if key not in _cache:
        bn, r, ne, te = inputs
        cfg, bt = entry.config(oracle), entry.beam_table(bn)
        p = entry.params(api)
        d = api.derive(p)
        ids = np.asarray(M.live_ids(oracle, cfg, bt))[::every]
        beams = np.repeat(np.arange(cfg.nbeams, dtype=np.int32), len(ids))
        raynums = np.tile(ids.astype(np.int32), cfg.nbeams)
        lps, paths = [], []
        for b, i in zip(beams, raynums):
            live, lp = oracle.launch_point(cfg, bt, int(b), int(i))
            assert live
            lps.append(lp)
            paths.append(oracle.ray_path(cfg, bt, r, ne, te, int(b), int(i)))
        S, T = path_records(api, p, d, lps, paths)
        ne3d, _ = oracle.node_tables(cfg, r, ne, te)
        _cache[key] = dict(entry=entry, p=p, d=d, cfg=cfg, bt=bt, beams=beams, raynums=raynums, S=S, T=T, ne3d=ne3d,
                           fields=synthetic_fields(entry))
    return _cache[key]


def state_table(api, p, gp):
    """A [2, nx, ny, nz] state table (cs, gain_const) that varies from node to node: the scalars of gp times a smooth factor."""
    _, cs, gc = api.gain_constants(p, gp)
    i, j, k = np.meshgrid(np.arange(p.nx), np.arange(p.ny), np.arange(p.nz), indexing="ij")
    w = 1.0 + 0.3 * np.sin(0.7 * i + 0.4 * j - 0.5 * k)
    return np.stack([cs * w, gc * (2.0 - w)])


def flow_table(p, seed=SEED + 1):
    """A [3, nx, ny, nz] flow table that is no radial ramp: a few 1e7 cm/s, random per node."""
    return np.random.default_rng(seed).uniform(-4e7, 4e7, size=(3, p.nx, p.ny, p.nz))


def sbs_reference(api, p, gp, S, T, beams, fields, ne3d, shifts, flow=None, state=None, smoothed=False):
    """gamma [nshift, nitems] of DESIGN.md section 24, restated in numpy from its text."""
    d = api.derive(p)
    _, cs0, gc0 = api.gain_constants(p, gp)
    qs = ((2.0 * (d.omega / KC)) / KC) / d.dt
    iaw2 = gp.iaw * gp.iaw
    shifts = np.asarray(shifts, dtype=np.float64)
    x, y, z = api.node_coordinates(p)
    if flow is None:                                         # the closed-form Mach ramp about the origin
        rr = np.sqrt(x * x + y * y + z * z)
        t = np.clip((rr - gp.mach_r0) / (gp.mach_r1 - gp.mach_r0), 0.0, 1.0)
        um = (gp.mach_0 + (gp.mach_1 - gp.mach_0) * t) * cs0
        with np.errstate(divide="ignore", invalid="ignore"):
            flow = np.stack([np.where(rr > 0, um * (c / rr), 0.0) for c in (x, y, z)])
    cs = np.full(ne3d.shape, cs0) if state is None else state[0]
    gc = np.full(ne3d.shape, gc0) if state is None else state[1]
    frac = ne3d / d.ncrit
    eps = 1.0 - frac
    with np.errstate(divide="ignore", invalid="ignore"):
        pref = np.where(eps > 0, gc * frac * (1.0 / gp.iaw) / np.sqrt(np.where(eps > 0, eps, 1.0)), 0.0)
    gamma = np.zeros((len(shifts), len(beams)))
    for k in range(len(beams)):
        if T["status"][k] == 0:
            continue
        n = int(T["nsamples"][k]) - 1
        pos = np.stack([S[c][:n + 1, k] for c in ("x", "y", "z")], axis=1)
        dd = pos[1:] - pos[:-1]
        ds = np.sqrt((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2])
        node = (S["ci"][1:n + 1, k], S["cj"][1:n + 1, k], S["ck"][1:n + 1, k])
        q = qs * dd
        kiaw = np.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2])
        qu = q[:, 0] * flow[0][node] + q[:, 1] * flow[1][node] + q[:, 2] * flow[2][node]
        I = fields[0, beams[k], node[0] + 1, node[1] + 1, node[2] + 1]
        for m, delta in enumerate(shifts):
            eta = ((0.0 - qu) + (0.0 - delta)) / (kiaw * cs[node] + 1e-10)
            e2 = eta * eta
            g = pref[node] * (iaw2 * eta / ((e2 - 1.0) * (e2 - 1.0) + iaw2 * e2))
            if smoothed:
                g = g * 0.5
            term = np.where(ds == 0.0, 0.0, (g * I) * ds)
            gamma[m, k] = np.cumsum(term)[-1] if n else 0.0  # cumsum: in step order
    return gamma
