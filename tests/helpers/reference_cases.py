"""The cases on which the reference's own kernel source, compiled as host C++ (oracle/ref_build.py), is run and compared
with the oracle, with the committed fixtures made from it (tests/golden/make_reference_golden.py) and, through those,
with the HIP kernels.  One binary per case: the reference's knobs are compile-time constants.

  * every non-heavy entry of config_matrix.ENTRIES, with the entry's own beam table;
  * exit_cases.RAGGED's grid (20 x 17 x 25) with all 60 OMEGA beams;
  * the extra axes the GPU suite moves: rays_per_zone 3 on 40 x 48 x 36 (test_nonuniform_grid_and_rays_per_zone),
    rays_per_zone 6 on 24^3, profiles of 2, 64 and 2048 rows (test_analytic_profile_of_other_lengths), BASELINE config 1
    (uniform plasma, absorption off, 64^3; test_config1_uniform_plasma_properties) and the s83177 profile reversed, which
    takes the descending branch of interp_cuda, on the ragged grid;
  * the default 64^3 and 100^3 of SURVEY.md 8(c).

NOT here: config_matrix's `long_nt`.  It is one beam at nt = 65535, minutes of serial CPU per run, and exists for the
window kernel's 16-bit step counters, not for a generalisation of the reference's constants.

Every case is cheap except default_64 and default_100 (about 10 s and 40 s of one core each).
"""
import numpy as np

from helpers import config_matrix as M
from helpers import exit_cases as X

S83177 = "s83177"


class Case:
    def __init__(self, name, n, ny=None, nz=None, beams=None, overrides=None, profile=S83177, far_jump=False,
                 full_grid=False):
        self.name, self.n = name, n
        self.ny, self.nz = (n if ny is None else ny), (n if nz is None else nz)
        self._beams = beams               # tuple of ints: rows of the OMEGA table; array: as is
        self.overrides = dict(overrides or {})
        self.profile_name = profile
        self.far_jump = far_jump          # deposit weights of both signs cancel (config_matrix.Entry.far_jump)
        self.full_grid = full_grid        # the whole grid of a single-threaded reference run is a committed fixture

    def __repr__(self):
        return self.name

    def beam_table(self, bn):
        if isinstance(self._beams, tuple):
            return np.ascontiguousarray(np.asarray(bn)[list(self._beams)], dtype=np.float64)
        return np.ascontiguousarray(self._beams, dtype=np.float64).copy()

    def _apply(self, obj, extra):
        obj.ny, obj.nz = self.ny, self.nz
        obj.nbeams = len(self._beams)
        for k, v in self.overrides.items():
            setattr(obj, k, v)
        for k, v in extra.items():
            setattr(obj, k, v)
        return obj

    def config(self, oracle, **extra):
        return self._apply(oracle.default_config(self.n), extra)

    def params(self, api, **extra):
        return self._apply(api.default_params(self.n), extra)

    def profile(self, oracle, inputs):
        """(r, ne, te) of this case, nprofile rows each."""
        _, r, ne, te = inputs
        cfg = self.config(oracle)
        if self.profile_name == S83177:
            out = r, ne, te
        elif self.profile_name == "descending":
            out = tuple(np.ascontiguousarray(v[::-1]) for v in (r, ne, te))
        elif self.profile_name == "uniform":          # BASELINE config 1
            out = r, np.full(len(r), 0.1 * oracle.derive(cfg).ncrit), np.full(len(r), 2000.0)
        else:                                         # SURVEY 8(d)'s analytic stand-in, as the GPU test builds it
            assert self.profile_name == "analytic"
            ncrit = oracle.derive(cfg).ncrit
            ra = np.linspace(0.0, 0.3, cfg.nprofile)
            nea = ncrit * (np.array([0.9, 0.0]) if cfg.nprofile == 2 else np.exp(-(ra - 0.035) / 0.01))
            out = ra, nea, 500.0 + 6000.0 * ra
        assert all(len(v) == cfg.nprofile for v in out), self.name
        return tuple(np.ascontiguousarray(v, dtype=np.float64) for v in out)


def _from_entry(e, name=None, beams=None):
    b = e._beams if beams is None else beams
    return Case(name or e.name, e.n, e.ny, e.nz, beams=(M.B4 if b is None else b), overrides=e.overrides,
                far_jump=e.far_jump)


ANALYTIC_BEAMS = (2, 14, 33, 47, 58)
ALL60 = tuple(range(60))

CASES = [_from_entry(e) for e in M.ENTRIES if not e.heavy]       # long_nt stays out (see above)
CASES += [
    _from_entry(X.RAGGED, name="ragged_60", beams=ALL60),
    Case("rpz3_40x48x36", 40, 48, 36, beams=(1, 12, 33, 58), overrides=dict(rays_per_zone=3)),
    Case("rpz6_24", 24, beams=M.B4, overrides=dict(rays_per_zone=6), full_grid=True),
    Case("nprofile_2", 40, beams=ANALYTIC_BEAMS, overrides=dict(nprofile=2), profile="analytic"),
    Case("nprofile_64", 40, beams=ANALYTIC_BEAMS, overrides=dict(nprofile=64), profile="analytic"),
    Case("nprofile_2048", 40, beams=ANALYTIC_BEAMS, overrides=dict(nprofile=2048), profile="analytic"),
    Case("config1_64", 64, beams=(0, 30), overrides=dict(absorption=0), profile="uniform"),
    Case("descending_20x17x25", 20, 17, 25, beams=M.B4, profile="descending", full_grid=True),
    Case("default_64", 64, beams=ALL60),
    Case("default_100", 100, beams=ALL60),
]
BY_NAME = {c.name: c for c in CASES}
BY_NAME["tall_y"].full_grid = BY_NAME["ragged_60"].full_grid = True
NAMES = [c.name for c in CASES]
FULL_GRID = [c.name for c in CASES if c.full_grid]       # tall_y, ragged_60, rpz6_24, descending_20x17x25
assert len(BY_NAME) == len(CASES) and "long_nt" not in BY_NAME and len(FULL_GRID) == 4


# ---- running a case ----------------------------------------------------------------------------------------------------
def run_reference(ref_build, oracle, case, inputs, workdir, threads=1):
    """Runs oracle/_ref/<case>/run.  Returns dict(grid, steps_per_beam, phase_r, pow_r, consts)."""
    import os
    import subprocess
    cfg, bt = case.config(oracle), case.beam_table(inputs[0])
    d = os.path.join(str(workdir), case.name)
    os.makedirs(d, exist_ok=True)
    paths = [os.path.join(d, f) for f in ("profile.bin", "beams.bin", "grid.bin", "side.bin")]
    np.concatenate(case.profile(oracle, inputs)).tofile(paths[0])
    bt.tofile(paths[1])
    subprocess.run([ref_build.binary(case.name)] + paths + [str(threads)], check=True, timeout=600)
    grid = np.fromfile(paths[2], dtype=np.float64).reshape(oracle.grid_shape(cfg))
    side = open(paths[3], "rb").read()
    nb = int(np.frombuffer(side, dtype=np.int64, count=1)[0])
    assert nb == cfg.nbeams and len(side) == 8 * (1 + nb + 2 * oracle.NPHASE + 3)
    tail = np.frombuffer(side, dtype=np.float64, offset=8 * (1 + nb))
    os.remove(paths[2])
    return dict(grid=grid, steps_per_beam=np.frombuffer(side, dtype=np.int64, count=nb, offset=8).copy(),
                phase_r=tail[:oracle.NPHASE].copy(), pow_r=tail[oracle.NPHASE:2 * oracle.NPHASE].copy(),
                consts=tail[2 * oracle.NPHASE:].copy())


def kat(grid, steps_per_beam):
    """The known answers of one run, as reference_kat.json records them (Python floats print round-trip exact)."""
    g = np.asarray(grid)
    return dict(ray_steps=int(np.sum(steps_per_beam)), steps_per_beam=[int(s) for s in steps_per_beam],
                sum=float(g.sum()), max=float(g.max()), nonzero=int(np.count_nonzero(g)), negative=int((g < 0).sum()),
                sum_per_x_plane=[float(v) for v in g.sum(axis=(1, 2))])
