"""The run-time knobs of cbet_params as one table of configurations: Courant multiplier, box extents, launch rule
(max_threads / threads_per_block) and the caller's beam table -- everything the default configuration never moves.

Each entry names the regime it exists for and carries a cheap CPU-side assertion of that regime (`regime`), computed
from the oracle's ray paths of a seeded sample of rays, so an entry that silently stops reaching its regime fails.
The host tests, the GPU parity tests, the exit / CBET tests and the bounds-audited twin all draw from this table.

    f = (pos - min) / d,  g = max over axes |f - cell|        (cell = columns 3..5 of oracle.ray_path)

The nearest-node update looks one cell either way with a half-width of 0.5001, so a step with g >= 1.5 cannot be
followed: the reference keeps the old cell and the ray's cell no longer tracks its position ("far jump", "lost").
"""
import ctypes as C
import json
import os

import numpy as np

FAR = 1.4998          # |f - cell| from which the nearest-node update cannot follow (issue's threshold)
SAMPLE = 240          # rays sampled per entry for the regime statistics
B4 = (0, 17, 33, 58)  # rows of the OMEGA-60 table used unless an entry brings its own beams

AXIS_BEAMS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
_DIAG = np.array([[1, 1, 1], [-1, 1, -1], [1, -1, 0], [0, 1, 1]], dtype=np.float64)
DIAG_BEAMS = _DIAG / np.linalg.norm(_DIAG, axis=1, keepdims=True)

NT_EDGE = 65535       # the window kernel's 16-bit per-wave step counters: nt >= 65536 is refused


def courant_for_nt(nx, nt):
    """A Courant multiplier for which derive().nt == nt: nt = (int)((1 / c) * nx * 2.0)."""
    return (2.0 * nx) / (nt + 0.5)


class Entry:
    def __init__(self, name, n=48, ny=None, nz=None, beams=None, overrides=None, regime=None, far_jump=False,
                 heavy=False):
        self.name, self.n = name, n
        self.ny, self.nz = (n if ny is None else ny), (n if nz is None else nz)
        self._beams = beams                   # None: B4 rows of the OMEGA table; tuple of ints: those rows; array: as is
        self.overrides = dict(overrides or {})
        self.regime = regime                  # regime(stats) -> None, asserts
        self.far_jump = far_jump              # deposit weights of both signs cancel: signs compared above a floor only
        self.heavy = heavy                    # minutes on the CPU oracle's ray paths: no path sample, regime from derive()

    def __repr__(self):
        return self.name

    def beam_table(self, bn):
        b = self._beams
        if b is None:
            b = B4
        if isinstance(b, tuple):
            return np.ascontiguousarray(np.asarray(bn)[list(b)], dtype=np.float64)
        return np.ascontiguousarray(b, dtype=np.float64).copy()

    def nbeams(self):
        b = B4 if self._beams is None else self._beams
        return len(b)

    def _apply(self, obj, extra):
        obj.ny, obj.nz = self.ny, self.nz
        obj.nbeams = self.nbeams()
        for k, v in self.overrides.items():
            setattr(obj, k, v)
        for k, v in extra.items():
            setattr(obj, k, v)
        return obj

    def params(self, api, **extra):
        """api.default_params(n) with this entry's overrides (and the caller's, e.g. kernel_variant)."""
        return self._apply(api.default_params(self.n), extra)

    def config(self, oracle, **extra):
        """oracle.default_config(n) with the same overrides."""
        return self._apply(oracle.default_config(self.n), extra)


# ---- regime statistics ------------------------------------------------------------------------------------------------
def live_ids(oracle, cfg, bt, beam=0):
    """{i : id_is_traced(i) and launch_point(i) live}: the reference's ray set of one beam (the same for every beam)."""
    L = oracle.lib()
    d = oracle.derive(cfg)
    return [i for i in range(d.nrays)
            if L.cbet_oracle_id_is_traced(C.byref(cfg), i) and oracle.launch_point(cfg, bt, beam, i)[0]]


def regime_stats(oracle, entry, inputs, sample=SAMPLE, seed=20261016):
    """Statistics of a seeded sample of rays of `entry`, from the oracle alone."""
    bn, r, ne, te = inputs
    cfg, bt = entry.config(oracle), entry.beam_table(bn)
    d = oracle.derive(cfg)
    ids = live_ids(oracle, cfg, bt)
    st = dict(entry=entry.name, nt=d.nt, nindices=d.nindices, grid_y=d.grid_y, nrays=d.nrays, nlive=len(ids),
              ntraced=sum(1 for i in range(d.nrays) if oracle.lib().cbet_oracle_id_is_traced(C.byref(cfg), i)),
              nlive_all=sum(1 for i in range(d.nrays) if oracle.launch_point(cfg, bt, 0, i)[0]),
              dx=d.dx, dy=d.dy, dz=d.dz, dt=d.dt, unit_beams=bool(np.allclose(np.linalg.norm(bt, axis=1), 1.0, atol=1e-8)))
    if entry.heavy:
        return st
    rng = np.random.default_rng(seed)
    lo = np.array([cfg.xmin, cfg.ymin, cfg.zmin])
    hi = np.array([cfg.xmax, cfg.ymax, cfg.zmax])
    dd = np.array([d.dx, d.dy, d.dz])
    steps = far_steps = rays_far = outside = 0
    gmax = 0.0
    move_max = np.zeros(3)                 # largest single-step move per axis, in cells
    cell_axes = set()                      # axes along which the sampled rays' cell ever changed
    for _ in range(sample):
        b, i = int(rng.integers(cfg.nbeams)), int(ids[int(rng.integers(len(ids)))])
        _, lp = oracle.launch_point(cfg, bt, b, i)
        outside += bool(np.any(lp[:3] < lo - dd / 2) or np.any(lp[:3] > hi + dd / 2))
        path = oracle.ray_path(cfg, bt, r, ne, te, b, i)
        assert len(path) > 0 and np.isfinite(path).all(), (entry.name, b, i)
        f = (path[:, :3] - lo) / dd
        g = np.abs(f - path[:, 3:6]).max(axis=1)
        far = g >= FAR
        steps += len(path)
        far_steps += int(far.sum())
        rays_far += bool(far.any())
        gmax = max(gmax, float(g.max()))
        pos = np.vstack([lp[:3], path[:, :3]])
        move_max = np.maximum(move_max, (np.abs(np.diff(pos, axis=0)) / dd).max(axis=0))
        for a in range(3):
            if np.ptp(path[:, 3 + a]) > 0:
                cell_axes.add(a)
    st.update(sample=sample, steps=steps, far_frac=far_steps / max(1, steps), rays_far=rays_far, outside=outside,
              gmax=gmax, move_max=move_max.tolist(), cell_axes=sorted(cell_axes))
    return st


# ---- the regimes, as assertions on those statistics --------------------------------------------------------------------
def _no_jump(st):
    assert st["rays_far"] == 0 and st["far_frac"] == 0.0, st


def _default_rule(st):
    assert st["nindices"] == 1 and st["nlive"] == st["nlive_all"], st      # one pass, no live ray left out


def _r_courant_025(st):
    _no_jump(st)
    _default_rule(st)
    assert st["nt"] == 384, st


def _r_courant_10(st):
    _no_jump(st)
    assert st["gmax"] > 1.0, st            # offsets of more than a cell appear (rays past a face keep the face's cell)


def _r_courant_13(st):
    assert 0.2 * st["sample"] < st["rays_far"] < 0.8 * st["sample"], st      # a mix of tracked and lost rays


def _r_courant_16(st):
    assert st["far_frac"] > 0.5 and st["rays_far"] > 0.9 * st["sample"], st


def _r_courant_25(st):
    assert st["far_frac"] > 0.9 and st["rays_far"] == st["sample"], st


def _r_off_centre(st):
    _no_jump(st)
    _default_rule(st)


def _r_box_small(st):
    assert st["outside"] > 0.25 * st["sample"] and st["rays_far"] > 0.25 * st["sample"], st


def _r_box_large(st):
    _no_jump(st)
    assert st["outside"] == 0 and st["grid_y"] == 5, st


def _r_thin(axis):
    def check(st):
        assert st["outside"] > 0.25 * st["sample"], st
        d = [st["dx"], st["dy"], st["dz"]]
        assert d[axis] == min(d) and d[axis] < 0.5 * max(d), st
    return check


def _r_tall_y(st):
    assert st["dy"] < st["dx"] / 3 and st["dx"] == st["dz"], st      # dt follows min(dx, dz): 0.5 dx / dy > 1.5 cells in y
    assert st["move_max"][1] > 1.5 and st["rays_far"] > 0, st


def _r_axis_beams(st):
    _no_jump(st)
    assert st["unit_beams"], st


def _r_diag_beams(st):
    _no_jump(st)
    assert st["unit_beams"], st


def _r_strided_2(st):
    assert st["nindices"] == 2 and st["grid_y"] == 11, st
    _no_jump(st)


def _r_strided_5(st):
    assert st["nindices"] == 5 and st["grid_y"] == 10, st
    _no_jump(st)


def _r_truncated(st):
    assert st["nindices"] == 1 and st["grid_y"] == 4, st
    assert st["nlive_all"] - st["nlive"] == 153, st            # live rays the truncating grid_y never visits


def _r_tpb_7(st):
    assert st["nindices"] == 1 and st["nlive"] == st["nlive_all"] == 3486, st


def _r_long_nt(st):
    assert st["nt"] == NT_EDGE, st


ENTRIES = [
    Entry("courant_0.25", overrides=dict(courant_mult=0.25), regime=_r_courant_025),
    Entry("courant_1.0", overrides=dict(courant_mult=1.0), regime=_r_courant_10),
    Entry("courant_1.3", overrides=dict(courant_mult=1.3), regime=_r_courant_13, far_jump=True),
    Entry("courant_1.6", overrides=dict(courant_mult=1.6), regime=_r_courant_16, far_jump=True),
    Entry("courant_2.5", overrides=dict(courant_mult=2.5), regime=_r_courant_25, far_jump=True),
    Entry("courant_2.5_n96", n=96, overrides=dict(courant_mult=2.5), regime=_r_courant_25, far_jump=True),
    Entry("box_off_centre", overrides=dict(xmin=-0.10, xmax=0.16, ymin=-0.15, ymax=0.11, zmin=-0.12, zmax=0.14),
          regime=_r_off_centre),
    Entry("box_small", overrides=dict(xmin=-0.08, xmax=0.08, ymin=-0.08, ymax=0.08, zmin=-0.08, zmax=0.08),
          regime=_r_box_small, far_jump=True),
    Entry("box_large", overrides=dict(xmin=-0.25, xmax=0.25, ymin=-0.25, ymax=0.25, zmin=-0.25, zmax=0.25),
          regime=_r_box_large),
    Entry("box_thin_y", overrides=dict(ymin=-0.04, ymax=0.04), regime=_r_thin(1), far_jump=True),
    Entry("box_thin_x", overrides=dict(xmin=-0.05, xmax=0.05), regime=_r_thin(0), far_jump=True),
    Entry("box_thin_z", overrides=dict(zmin=-0.05, zmax=0.05), regime=_r_thin(2), far_jump=True),
    Entry("tall_y", n=20, ny=80, nz=20, regime=_r_tall_y, far_jump=True),
    Entry("axis_beams", beams=AXIS_BEAMS, regime=_r_axis_beams),
    Entry("diag_beams", beams=DIAG_BEAMS, regime=_r_diag_beams),
    Entry("strided_2", overrides=dict(max_threads=4 * 3000), regime=_r_strided_2),
    Entry("strided_5", overrides=dict(max_threads=4 * 1000, threads_per_block=96), regime=_r_strided_5),
    Entry("truncated", overrides=dict(threads_per_block=1000), regime=_r_truncated),
    Entry("tpb_7", overrides=dict(threads_per_block=7), regime=_r_tpb_7),
    Entry("long_nt", n=24, beams=(3,), overrides=dict(courant_mult=courant_for_nt(24, NT_EDGE)), regime=_r_long_nt,
          heavy=True),
]
BY_NAME = {e.name: e for e in ENTRIES}
NAMES = [e.name for e in ENTRIES]

# the step counts of the reference's own kernel source, compiled as host C++ and run on every light entry
# (tests/golden/reference_kat.json, written by tests/golden/make_reference_golden.py; tests/test_reference_pin.py holds
# the file to the live binaries and to the oracle).  Tests compare with the oracle's count at run time and pin these on
# top; the heavy entry (long_nt) has no recorded count.
with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "reference_kat.json")) as _f:
    _KAT = json.load(_f)["cases"]
PINNED_STEPS = {e.name: _KAT[e.name]["ray_steps"] for e in ENTRIES if not e.heavy}
assert len(PINNED_STEPS) == 19 and PINNED_STEPS["courant_1.3"] == 410101 and PINNED_STEPS["diag_beams"] == 880381

EXTRAS = ("courant_1.6", "box_small", "axis_beams", "strided_5")     # wide index, per beam, padded rows, shards
EXIT_ENTRIES = ("courant_1.6", "box_small", "box_thin_y", "axis_beams", "strided_5")
CBET_ENTRIES = ("courant_1.6", "box_off_centre", "box_small", "axis_beams")


def oracle_trace(oracle, entry, inputs, nthreads=8, **kw):
    bn, r, ne, te = inputs
    return oracle.trace(entry.config(oracle), entry.beam_table(bn), r, ne, te, nthreads=nthreads, **kw)
