"""The two worlds of the gain stage's tests and the constants that go with them, each defined here once.

  TRACED  48 x 21 x 134, six beams, the oracle's traced fields: haloed 50 x 23 x 136 -- a ragged last brick in y, whole bricks
          in z, three 64-cell state groups per row, planes of 23 * 136 doubles.
  CROWDED 13 x 11 x 148, sixty beams, synthetic crowded fields: haloed 15 x 13 x 150 -- odd in x, ragged bricks in y and z,
          rows that start off a 128-byte line, the last state group holds 22 cells, the halves and quarters arms in runs
          beyond the first group, touched-but-absent and untouched entries, super-critical nodes.

traced_world / crowded_world build a world's CPU side once per session and assert the regime every user relies on.  A cached
world is read-only apart from the caches that helpers keep in it under names of their own (saturation_cases.reference,
detuning_cases.reference, the host tests' normalised fields).  Device tracers are not part of a world: every test module makes
its own, because the tests switch flow, state, limit and shifts on them."""
import numpy as np

from helpers.gain_reference import Composed, Restatement, kappa_cells
from helpers.saturation_cases import limits_from

TOL = 1e-9                 # against a CPU reference or the oracle, of max |K| (tests/test_gpu_cbet.py's bound); of Gross_ij
LAST_BITS = 1e-12          # two formulations of one quantity, pair-once against ordered kernel: of max |K|, or of Gross_ij
TRACED = (48, 21, 134)
CROWDED = (13, 11, 148)                      # haloed 15 x 13 x 150: rows of 150 cells, three 64-cell state groups, the last of 22
BEAMS = [0, 16, 29, 38, 47, 55]              # the six beams of tests/test_gpu_cbet.py
OFFSET = (20e-4, 0.0, -15e-4)                # the offset target of tests/test_gpu_flow.py's oracle comparisons, cm
# hk of the pair-once kernel's 64-cell state groups (up to a row's shift of 0 or 8 cells on these grids)
Z_GROUPS = (slice(0, 64), slice(64, 128), slice(128, None))
# the slab of the slab-wise and packed cases: CROWDED has 15 planes, there it is [9, 14) -- the same odd lower boundary through a
# two-plane brick, a plane left outside above -- and the cuts of the slab-wise updates, odd boundaries through the bricks
SLABS = {"traced": (9, 22), "crowded": (9, 14)}
CUTS = {"traced": [0, 1, 12, 13, 29, 50], "crowded": [0, 1, 6, 9, 14, 15]}
# (te_ev, ti_ev, z_ion): a corona, a cold dense shell, a hot mid-Z spot -- 8 x apart in te_ev
STATES = [dict(te_ev=2000.0, ti_ev=1000.0, z_ion=3.1), dict(te_ev=250.0, ti_ev=90.0, z_ion=2.2),
          dict(te_ev=900.0, ti_ev=1300.0, z_ion=5.3)]


def params(api, shape, nbeams):
    p = api.default_params(shape[0], nbeams=nbeams)
    p.ny, p.nz = shape[1], shape[2]
    return p


def crowded_fields(shape):
    """Up to ~54 of 60 beams per cell, energies of the order of real deposits (x 1e11), touched-but-absent (negative) and
    untouched entries: (fields [4, 60, ...], present mask)."""
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


def three_states(api, p, gp, shape, kz=1):
    """The three-state node table (node_pattern with kz): [2, nx, ny, nz] of (cs, gain_const)."""
    consts = []
    for st in STATES:
        g = api.default_gain_params(relax=gp.relax, **st)
        consts.append(api.gain_constants(p, g)[1:])
    which = node_pattern(shape, kz)
    return np.stack([np.choose(which, [c[0] for c in consts]), np.choose(which, [c[1] for c in consts])])


# ---- the two worlds, built once per session -------------------------------------------------------------------------------
_cache = {}


def _tables(api, p, gp, shape, ne3d):
    """What both worlds hold beside their fields: the sphere's flow table, the offset target's, the three-state table
    (kz = 1), and the restatement without tables and with the last two."""
    flow = api.flow_table(p, gp, None)
    state = three_states(api, p, gp, shape, kz=1)
    shifted = api.flow_table(p, gp, api.Target(OFFSET))
    return dict(flow=flow, shifted=shifted, state=state, plain=Restatement(api, p, gp, ne3d, flow),
                tabled=Restatement(api, p, gp, ne3d, shifted, cs=state[0], gc=state[1]))


def traced_world(api, oracle, inputs, nthreads):
    """TRACED: the oracle's traced fields of six beams (`ofields`, and `raw`), its whole-field gain, the composed reference and
    its limits, the restatement without tables (`restated`) and with (`tabled`)."""
    if "traced" not in _cache:
        bn_all, r, ne, te = inputs
        bn = bn_all[BEAMS].copy()
        cfg = oracle.default_config(TRACED[0], nbeams=len(BEAMS), ny=TRACED[1], nz=TRACED[2])
        assert oracle.grid_shape(cfg) == (50, 23, 136)
        ne3d, kap3d = oracle.node_tables(cfg, r, ne, te)
        og = oracle.gain_default()
        ofields = np.stack([oracle.trace_cbet(cfg, og, bn, ne3d, kap3d, quantity=q, per_beam=True, nthreads=nthreads)[0]
                            for q in (1, 2, 3, 4)])
        ogain, _ = oracle.gain_field(cfg, og, ofields, ne3d, relax=1.0, nthreads=nthreads)
        scale = float(np.abs(ogain).max())
        # the regime: a non-trivial gain (1/cm), and most of it beyond the first 64 cells of its z-row
        assert scale > 1.0
        assert int((ogain[..., 64:] != 0).sum()) >= 10000
        assert all(np.abs(ogain[..., z]).max() > 1e-3 * scale for z in Z_GROUPS[:2])
        p = params(api, TRACED, len(BEAMS))
        gp = api.default_gain_params(relax=1.0)
        comp = Composed(oracle, cfg, og, ofields, ne3d, kappa_cells(api, p, ne3d), nthreads)
        amps = comp.amplitudes()
        tables = _tables(api, p, gp, TRACED, ne3d)
        tables["restated"] = tables.pop("plain")
        _cache["traced"] = dict(tables, raw=ofields, bn=bn, cfg=cfg, og=og, ne3d=ne3d, ofields=ofields, ogain=ogain, scale=scale,
                                p=p, gp=gp, composed=comp, amps=amps, limits=limits_from(amps))
    return _cache["traced"]


def crowded_world(api, oracle, inputs, nthreads):
    """CROWDED: sixty beams' synthetic fields, the oracle's whole-field gain, the restatement without a table (`plain`) and
    with a caller's flow table plus the three-state table (`tabled`); `classes`: the 16-cell runs beyond the first 64 cells
    that hold up to 20, up to 40 and more beams."""
    if "crowded" not in _cache:
        bn, r, ne, te = inputs
        cfg = oracle.default_config(CROWDED[0], nbeams=60, ny=CROWDED[1], nz=CROWDED[2])
        grid = oracle.grid_shape(cfg)
        assert grid == (15, 13, 150)
        assert grid[2] % 16 != 0                     # rows of 150 doubles: most start off a 128-byte line
        ne3d, _ = oracle.node_tables(cfg, r, ne, te)
        p = params(api, CROWDED, 60)
        gp = api.default_gain_params(relax=1.0)
        raw, present = crowded_fields((60,) + grid)
        assert (raw[0] < 0).any() and (raw[0] == 0).any()
        windows = np.stack([present[..., z0:z0 + 16].any(-1).sum(0) for z0 in range(64, grid[2], 16)])
        classes = [int((windows <= 20).sum()), int(((windows > 20) & (windows <= 40)).sum()), int((windows > 40).sum())]
        assert min(classes) >= 50, classes           # whole runs, halves and quarters, all beyond the first 64 cells
        assert (ne3d >= api.derive(p).ncrit).any()   # the eps <= 0 arm runs
        ogain, _ = oracle.gain_field(cfg, oracle.gain_default(), raw, ne3d, relax=1.0, nthreads=nthreads)
        scale = float(np.abs(ogain).max())
        assert scale > 1.0
        assert all(np.abs(ogain[..., z]).max() > 1e-3 * scale for z in Z_GROUPS)         # something in all three groups
        _cache["crowded"] = dict(_tables(api, p, gp, CROWDED, ne3d), bn=bn, cfg=cfg, ne3d=ne3d, raw=raw, ogain=ogain, scale=scale,
                                 classes=classes, p=p, gp=gp)
    return _cache["crowded"]
