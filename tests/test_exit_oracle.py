"""cbet_oracle_ray_exit -- the per-ray exit record of the CPU oracle that the GPU tests of the exit pass's arms compare
with (test_gpu_exit_arms.py) -- tied to the oracle functions the suite already trusts, and the regimes of the cases in
helpers/exit_cases.py asserted on the oracle: a gain field or a box that stops reaching its regime fails here, without
a GPU."""
import numpy as np
import pytest

from conftest import NCPU
from helpers import config_matrix as M
from helpers import exit_cases as X

EPS = X.EPS


@pytest.fixture(scope="module")
def ragged_plain(oracle, inputs):
    return X.oracle_exits(oracle, X.RAGGED, inputs)


def test_ray_exit_without_gain_is_ray_path(oracle, inputs, ragged_plain):
    """gain = NULL, node tables from node_tables: every live ray of the 4 beams at 20x17x25 against ray_path's last row.
    ray_path looks the profile up at a node's radius where ray_exit reads the table node_tables made from the same
    expression at the same radius (sqrt of the same three squares in the same order), and the absorption factor
    ((ed / ncrit * nuei) * dt) * uray is the same four operations in the same order either way: the two go through the
    same arithmetic statement by statement, so position and energy are compared bit for bit."""
    bn, r, ne, te = inputs
    cfg, bt = X.RAGGED.config(oracle), X.RAGGED.beam_table(bn)
    d = oracle.derive(cfg)
    ids, rec = ragged_plain
    assert rec.shape[:2] == (4, len(ids)) and len(ids) > 300
    lo = (cfg.xmin - (d.dx / 2.0), cfg.ymin - (d.dy / 2.0), cfg.zmin - (d.dz / 2.0))
    hi = (cfg.xmax + (d.dx / 2.0), cfg.ymax + (d.dy / 2.0), cfg.zmax + (d.dz / 2.0))
    seen = set()
    for b in range(cfg.nbeams):
        for j, i in enumerate(ids):
            e = dict(zip(oracle.EXIT_FIELDS, rec[b, j]))
            path = oracle.ray_path(cfg, bt, r, ne, te, b, int(i))
            live, lp = oracle.launch_point(cfg, bt, b, int(i))
            assert live and len(path) > 0
            x, y, z, uray = path[-1, 0], path[-1, 1], path[-1, 2], path[-1, 7]
            assert (e["x"], e["y"], e["z"], e["uray"], e["uray0"]) == (x, y, z, uray, lp[3]), (b, i)
            assert e["steps"] == len(path)
            cut = uray <= 0.05 * lp[3]                     # the rule of test_gpu_exits._check_against_oracle
            out = x < lo[0] or x > hi[0] or y < lo[1] or y > hi[1] or z < lo[2] or z > hi[2]
            status = X.LAUNCHED | (X.CUTOFF if cut else 0) | (X.ESCAPED if out else 0)
            if not (cut or out):
                assert len(path) == d.nt
                status = X.LAUNCHED | X.TIMEOUT
            assert e["status"] == status, (b, i)
            seen.add(status)
            prev = path[-2, :3] if len(path) > 1 else lp[:3]
            v = (path[-1, :3] - prev) / d.dt
            assert np.abs(np.array([e["vx"], e["vy"], e["vz"]]) - v).max() <= 1e-9 * np.linalg.norm(v)
            assert e["gained"] == 0.0 and e["x_max"] == 0.0 and e["x_min"] == 0.0
    assert {X.LAUNCHED | X.CUTOFF, X.LAUNCHED | X.ESCAPED} <= seen
    # a culled ray: all zeros
    culled = [i for i in range(d.nrays) if not oracle.launch_point(cfg, bt, 0, i)[0]]
    ne3d, kap = oracle.node_tables(cfg, r, ne, te)
    assert culled and not oracle.ray_exit(cfg, oracle.gain_default(), bt, ne3d, kap, None, 0, culled[0]).any()


@pytest.mark.parametrize("name", X.GAIN_FIELDS)
def test_ray_exit_sums_are_trace_cbet(oracle, inputs, name):
    """With a gain: per beam, sum of `gained` = trace_cbet's beam_gain, sum of (uray0 + gained - uray) = the sum of its
    deposit grid, sum of steps = its step count.  Only the summation order differs (the ray loop is the same code), so the
    bound is n_rays 2^-53 sum |terms| -- for the deposit, whose sum has 8 terms per step, sum |grid terms| stands in."""
    bn, r, ne, te = inputs
    cfg, bt = X.RAGGED.config(oracle), X.RAGGED.beam_table(bn)
    gain = X.gain_field(name)
    g = X.oracle_gain_config(oracle, name)
    ids, rec = X.oracle_exits(oracle, X.RAGGED, inputs, gain=gain, gain_cfg=g)
    ne3d, kap = oracle.node_tables(cfg, r, ne, te)
    dep, steps, bg = oracle.trace_cbet(cfg, g, bt, ne3d, kap, gain=gain, quantity=0, per_beam=True, nthreads=NCPU)
    f = {k: rec[..., c] for c, k in enumerate(oracle.EXIT_FIELDS)}
    n = len(ids)
    ld = np.longdouble
    gained = f["gained"].astype(ld).sum(axis=1)
    bound = n * EPS * np.abs(f["gained"]).sum(axis=1)
    assert np.all(np.abs(gained - bg) <= bound), (gained - bg, bound)
    absorbed = ((f["uray0"] + f["gained"]) - f["uray"]).astype(ld).sum(axis=1)
    dsum = dep.astype(ld).sum(axis=(1, 2, 3))
    bound = n * EPS * np.maximum(np.abs(dep).sum(axis=(1, 2, 3)), np.abs(absorbed))
    print("%s: absorbed vs deposit, fraction of the bound %.3f" % (name, float((np.abs(absorbed - dsum) / bound).max())))
    assert np.all(np.abs(absorbed - dsum) <= bound), (absorbed - dsum, bound)
    assert int(f["steps"].sum()) == steps
    assert np.abs(f["gained"]).max() > 0


def _regime(oracle, inputs, name, entry):
    gain = X.gain_field(name, entry)
    g = X.oracle_gain_config(oracle, name)
    ids, rec = X.oracle_exits(oracle, entry, inputs, gain=gain, gain_cfg=g)
    return gain, g, {k: rec[..., c] for c, k in enumerate(oracle.EXIT_FIELDS)}


def test_regime_small(oracle, inputs):
    _, g, f = _regime(oracle, inputs, "small", X.RAGGED)
    assert 0.0 < f["x_max"].max() < X.SERIES_SWITCH            # no ray-step reaches 1/32: every wave takes the short series
    assert np.abs(f["gained"]).max() > 0.0


@pytest.mark.parametrize("entry", X.MIXED_ENTRIES, ids=lambda e: e.name)
def test_regime_mixed(oracle, inputs, entry):
    _, g, f = _regime(oracle, inputs, "mixed", entry)
    assert (f["x_max"] >= X.SERIES_SWITCH).any()               # some ray-steps take the long series ...
    assert (f["x_min"] < X.SERIES_SWITCH).any()                # ... some could take the short one ...
    assert f["x_max"].max() < g.max_exponent                   # ... and none reaches the clamp
    assert (np.abs(f["gained"]) / f["uray0"]).max() > 1e-3
    # the energy stays within a few decades of the launch energy: the 1e-9 uray0 bound of the GPU test leaves fp64 room
    assert (np.maximum(np.abs(f["gained"]), f["uray"]) / f["uray0"]).max() < 1e4


def test_regime_clamped(oracle, inputs):
    gain, g, f = _regime(oracle, inputs, "clamped", X.RAGGED)
    assert f["x_max"].max() > g.max_exponent
    g2 = X.oracle_gain_config(oracle, "clamped", max_exponent=2.0 * g.max_exponent)
    _, rec2 = X.oracle_exits(oracle, X.RAGGED, inputs, gain=gain, gain_cfg=g2)
    changed = np.abs(rec2[..., 8] - f["gained"]) > 1e-6 * np.abs(f["gained"])
    print("clamped: %.1f %% of the rays change with the clamp doubled" % (100.0 * changed.mean()))
    assert changed.mean() >= 0.05
    assert (np.abs(f["gained"]) / f["uray0"]).max() > 1e-3
    assert (np.maximum(np.abs(f["gained"]), f["uray"]) / f["uray0"]).max() < 1e4


def test_regime_long_box(oracle, inputs):
    """The long box: nt = 96, 124 live rays per beam; every ray of the two y beams ends with neither stop condition
    after nt steps, every ray of the four other beams escapes -- from ray_exit and from ray_path."""
    bn, r, ne, te = inputs
    vac = np.zeros_like(ne)
    entry = X.LONG_BOX
    cfg, bt = entry.config(oracle), entry.beam_table(bn)
    d = oracle.derive(cfg)
    assert d.nt == X.LONG_BOX_NT and cfg.nbeams == 6
    ids, rec = X.oracle_exits(oracle, entry, inputs, ne=vac)
    assert len(ids) == X.LONG_BOX_LIVE
    status, steps = rec[..., 10], rec[..., 9]
    for b in X.LONG_BOX_Y_BEAMS:
        assert np.all(status[b] == (X.LAUNCHED | X.TIMEOUT)) and np.all(steps[b] == d.nt)
        assert np.array_equal(rec[b, :, 6], rec[b, :, 7]) and not rec[b, :, 8].any()
    for b in X.LONG_BOX_OTHER_BEAMS:
        assert np.all(status[b] == (X.LAUNCHED | X.ESCAPED)) and np.all(steps[b] < d.nt)
    hi_y, lo_y = cfg.ymax + d.dy / 2.0, cfg.ymin - d.dy / 2.0
    for b in range(cfg.nbeams):
        for j, i in enumerate(ids):
            path = oracle.ray_path(cfg, bt, r, vac, te, b, int(i))
            assert len(path) == steps[b, j] and tuple(path[-1, :3]) == tuple(rec[b, j, :3])
            if b in X.LONG_BOX_Y_BEAMS:
                assert lo_y <= path[-1, 1] <= hi_y and path[-1, 7] == rec[b, j, 7]
