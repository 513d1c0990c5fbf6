"""The trace kernel when every ray runs out of steps: nothing leaves the LDS boxes because a ray ended.

One +y beam on 24^3 nodes whose y extent is stretched to +-0.8 cm (helpers/exit_cases.py's long box): the step length
follows min(dx, dz), so after nt = 96 steps every ray is still inside the grid -- no ray leaves, none is cut off (the
plasma is the shipped profile thinned to a tenth: 8 % of the light is absorbed).  The deposit reaches the grid by two
routes only: the planes that leave box A while it follows the bundle along y (retire_planes in the window arm), and
whatever the boxes -- A, and B where it is live -- still hold when the step count runs out, which goes out through
flush_box at the end of the kernel together with every lane's pending sums.  The two routes are not told apart here; the
grid is held to the oracle and to the rays' own energy loss.
"""
import numpy as np
import pytest

from conftest import NCPU, parity_err
from helpers import config_matrix as M

pytestmark = pytest.mark.gpu

ENTRY = M.Entry("flush_long_y", n=24, beams=np.array([[0.0, 1.0, 0.0]]), overrides=dict(ymin=-0.8, ymax=0.8))
NE_SCALE = 0.1
NT, LIVE = 96, 124
LAUNCHED, TIMEOUT = 1, 8      # include/cbet_mi355x.h CBET_RAY_*


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


def test_rays_that_run_out_of_steps_leave_their_whole_deposit_in_the_grid(api, oracle, inputs, torch_cuda):
    from cbet_raytracing_3d_amd.tracer import RayTracer
    bn, r, ne, te = inputs
    thin = ne * NE_SCALE
    bt = ENTRY.beam_table(bn)
    tr = RayTracer(ENTRY.params(api), r, thin, te, beam_norm=bt)
    assert tr.derived.nt == NT
    # every ray runs out of steps (the exit pass: each ray's final state)
    rec = tr.trace_exits(tr.new_exits()).cpu().numpy().copy().view(api.EXIT_DTYPE)[..., 0]
    live = rec[0][tr.ray_ids() >= 0]
    assert len(live) == LIVE
    assert np.all(live["status"] == (LAUNCHED | TIMEOUT)) and np.all(live["steps"] == NT)
    absorbed = float((live["uray0"].astype(np.longdouble) - live["uray"].astype(np.longdouble)).sum())
    assert absorbed > 0.05 * float(live["uray0"].sum())
    # ... and what they lost is in the grid
    e = tr.new_grid()
    tr.counters(reset=True)
    tr.launch(e)
    c = tr.counters(reset=True)
    e = e.cpu().numpy()
    oe, osteps = oracle.trace(ENTRY.config(oracle), bt.copy(), r, thin, te, nthreads=NCPU)
    assert c.ray_steps == osteps == LIVE * NT
    print("flush: parity err %.2e, grid sum / absorbed - 1 = %.2e" % (parity_err(e, oe), float(e.sum()) / absorbed - 1.0))
    assert parity_err(e, oe) < 1e-9
    assert np.array_equal(e == 0, oe == 0)
    assert abs(float(e.astype(np.longdouble).sum()) - absorbed) <= 1e-12 * absorbed
    tr.close()
