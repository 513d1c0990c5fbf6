"""The arms of the trace kernel's step loop that its branch hints move out of line (cbet_trace_window.hip, CBET_USUAL /
CBET_RARE / CBET_SELDOM) still run and still compute the oracle's grid.

The calm step is the fall-through of every wave-uniform branch of the loop; everything else -- the face-aware relocation,
the non-negative offsets, the window arm with its plane write-backs, box B, lanes outside both boxes, rays that end,
rays that run out of steps -- is laid out behind the loop.  These runs reach every one of those arms in the plain and
in the generic (wide-index) instantiation, each with the window statistics on: the grid agrees with the oracle cell by
cell at the project's 1e-9, the ray-step count is the oracle's, and the window counters say that the cold blocks ran.
That the inputs reach the arms the counters cannot see (faces, the sliver of non-negative offsets, the three ways a ray
ends) is checked on the oracle's ray paths, without a GPU."""
import numpy as np
import pytest

from conftest import NCPU, parity_err
from helpers import config_matrix as M
from helpers import exit_cases as X

PARITY_TOL = 1e-9
N40 = M.Entry("n40_three_beams", n=40, beams=(0, 17, 42))      # the shapes of test_patch_orders_trace_the_same_rays
THIN = 0.01     # the long box with the plasma thinned a hundredfold: the +-y beams' rays cross it almost straight and
                # run out of steps (nt = 96), the others leave through the near faces; what is absorbed is still non-zero
CASES = {"n40": (N40, 1.0), "long_box": (X.LONG_BOX, 1.0), "long_box_thin": (X.LONG_BOX, THIN)}
RAY_DEEP_LO = 6  # cbet_relocate.h kRelocateDeep: a cell below it, or above n - 3, is not deep inside the grid


@pytest.fixture(scope="module")
def references(oracle, inputs):
    """case -> (grid, ray-steps) of the oracle, computed once."""
    bn, r, ne, te = inputs
    out = {}
    for name, (entry, thin) in CASES.items():
        out[name] = oracle.trace(entry.config(oracle), entry.beam_table(bn), r, ne * thin, te, nthreads=NCPU)
    return out


def test_inputs_reach_the_cold_arms(oracle, inputs, references):
    """On the oracle's ray paths: steps near a face and steps deep inside, steps with a non-negative offset (the 1e-4
    wide sliver behind `all_negative`), rays that end by energy, by leaving the grid and by running out of steps."""
    from cbet_raytracing_3d_amd import api
    bn, r, ne, te = inputs
    seen = {}
    for name, (entry, thin) in CASES.items():
        cfg, bt = entry.config(oracle), entry.beam_table(bn)
        d = oracle.derive(cfg)
        lo, dd = np.array([cfg.xmin, cfg.ymin, cfg.zmin]), np.array([d.dx, d.dy, d.dz])
        nn = np.array([cfg.nx, cfg.ny, cfg.nz])
        ids = M.live_ids(oracle, cfg, bt)
        rng = np.random.default_rng(20261019)
        st = dict(near=0, deep=0, sliver=0, steps=0)
        for _ in range(150):
            b, i = int(rng.integers(cfg.nbeams)), int(ids[int(rng.integers(len(ids)))])
            path = oracle.ray_path(cfg, bt, r, ne * thin, te, b, i)
            cell = path[:, 3:6]
            off = (path[:, :3] - lo) / dd - cell - 0.5
            near = ((cell < RAY_DEEP_LO) | (cell > nn - 3)).any(axis=1)
            st["near"] += int(near.sum())
            st["deep"] += int((~near).sum())
            st["sliver"] += int((off >= 0).any(axis=1).sum())
            st["steps"] += len(path)
        ids_o, rec = X.oracle_exits(oracle, entry, inputs, ne=ne * thin)
        status = rec[..., oracle.EXIT_FIELDS.index("status")].astype(int)
        st["cutoff"] = int(((status & api.RAY_CUTOFF) != 0).sum())
        st["escaped"] = int(((status & api.RAY_ESCAPED) != 0).sum())
        st["timeout"] = int(((status & api.RAY_TIMEOUT) != 0).sum())
        assert rec[..., oracle.EXIT_FIELDS.index("steps")].sum() == references[name][1]
        seen[name] = st
        print(name, st)
    assert all(s["near"] > 0 for s in seen.values())
    assert seen["n40"]["deep"] > 0 and seen["n40"]["sliver"] > 0
    assert seen["n40"]["cutoff"] > 0 and seen["n40"]["escaped"] > 0
    assert seen["long_box"]["escaped"] > 0
    # the long box, thin: every ray of the +-y beams runs out of steps, every other ray leaves through a face
    per_beam = len(M.live_ids(oracle, X.LONG_BOX.config(oracle), X.LONG_BOX.beam_table(bn)))
    assert seen["long_box_thin"]["timeout"] == len(X.LONG_BOX_Y_BEAMS) * per_beam
    assert seen["long_box_thin"]["escaped"] == len(X.LONG_BOX_OTHER_BEAMS) * per_beam
    assert np.count_nonzero(references["long_box_thin"][0]) > 0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "the gpu tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def api():
    from cbet_raytracing_3d_amd import api as a
    a.lib()
    return a


WINDOW_COUNTERS = ("wave_steps", "wave_steps_miss", "wave_steps_wide", "slabs_retired", "lds_evictions", "global_atomics")


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_cold_arms_run_and_deposit_the_oracles_grid(api, oracle, inputs, references, torch_cuda, case):
    from cbet_raytracing_3d_amd.tracer import RayTracer
    bn, r, ne, te = inputs
    entry, thin = CASES[case]
    want, steps = references[case]
    tr = RayTracer(entry.params(api), r, ne * thin, te, beam_norm=entry.beam_table(bn))
    counted = []
    for wide in (0, 1):     # k_trace_window<16, false, 0, true> and <16, true, 0, true>
        e = tr.new_grid()
        tr.counters(reset=True)
        tr.launch(e, force_wide_index=wide, stats=True)
        c = tr.counters(reset=True)
        err = parity_err(e.cpu().numpy(), want)
        counted.append({k: int(getattr(c, k)) for k in WINDOW_COUNTERS})
        print(case, "wide index" if wide else "plain", "parity %.2e" % err, "ray-steps", c.ray_steps, counted[-1])
        assert c.ray_steps == steps, (case, wide)
        assert err < PARITY_TOL, (case, wide, err)
    tr.close()
    # the windows follow the rays' cells, which are the oracle's in both instantiations: the same counts
    assert counted[0] == counted[1]
    got = counted[0]
    assert got["wave_steps"] > 0 and got["slabs_retired"] > 0            # the window arm, planes written back
    # (the long box's other window counters are printed, not required: whether a beam of 124 rays fans out far enough to need
    # box B cannot be told without running it, and in the thinned plasma the rays go straight and never leave box A; the arms
    # the counters cannot see are checked on the oracle's paths in test_inputs_reach_the_cold_arms)
    if case == "n40":
        # bundles that fan out behind the turning point: lanes adopted by box B, lanes outside both boxes
        assert got["wave_steps_wide"] > 0 and got["wave_steps_miss"] > 0 and got["lds_evictions"] > 0
