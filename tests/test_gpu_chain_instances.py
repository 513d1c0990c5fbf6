"""The sixteen trace-kernel instantiations -- eight without the window statistics, eight with --, one launch each on a small
ragged grid.

cbet_trace_window.hip pins instructions around the record gather in every instantiation; the
listing rules of tests/test_isa_chain.py say where they stand, this file that each body still computes what it did:
plain, gain hooks, energy field (all WZ = 16) and the fused four-component pass (WZ = 8), each compiled-in and generic
(forced through the wide-index flag, as tests/test_gpu_parity.py and tests/test_gpu_cbet.py reach it), and each of those
again as the counting instantiation (cbet_params.window_stats = 1; `stats=True` for the plain launch).  The grid is
20 x 17 x 25 with two beams: no axis a multiple of a box extent, every bundle near a face for part of its life.
References and tolerances are those files': kernel_variant 1 cell by cell with equal step counts for the plain trace
(PARITY_TOL), the CPU model for the CBET quantities (TOL)."""
import numpy as np
import pytest

from conftest import NCPU, parity_err
from test_gpu_cbet import TOL
from test_gpu_parity import PARITY_TOL

pytestmark = pytest.mark.gpu

NX, NY, NZ = 20, 17, 25
BEAMS = [0, 16]
# (generic, stats); the cases without statistics keep the ids they had
INSTANCES = [pytest.param(False, False, id="False"), pytest.param(True, False, id="True"),
             pytest.param(False, True, id="False-stats"), pytest.param(True, True, id="True-stats")]


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


def _params(api, **kw):
    p = api.default_params(NX, nbeams=len(BEAMS), **kw)
    p.ny, p.nz = NY, NZ
    return p


@pytest.fixture(scope="module")
def case(api, oracle, inputs, torch_cuda):
    """The four tracers ((generic, stats): compiled-in or generic, without or with the window statistics) and every
    reference, computed once."""
    from cbet_raytracing_3d_amd.tracer import RayTracer
    bn, r, ne, te = inputs
    bt = bn[BEAMS].copy()
    tracers = {(g, s): RayTracer(_params(api, force_wide_index=int(g), window_stats=int(s)), r, ne, te, beam_norm=bt)
               for g in (False, True) for s in (False, True)}
    for tr in tracers.values():
        tr.tabulate()
    cfg = oracle.default_config(NX, nbeams=len(BEAMS))
    cfg.ny, cfg.nz = NY, NZ
    og = oracle.gain_default()
    ne3d, kap = oracle.node_tables(cfg, r, ne, te)
    gain = np.random.default_rng(48).uniform(-60.0, 60.0, size=(len(BEAMS),) + tracers[False, False].grid_shape)
    ofields = np.stack([oracle.trace_cbet(cfg, og, bt, ne3d, kap, gain=gain, quantity=q, per_beam=True, nthreads=NCPU)[0]
                        for q in (1, 2, 3, 4)])
    oe, osteps, obg = oracle.trace_cbet(cfg, og, bt, ne3d, kap, gain=gain, nthreads=NCPU)
    # the plain trace's reference: kernel_variant 1 (one global atomic per node and step)
    tr = tracers[False, False]
    e1 = tr.new_grid()
    tr.counters(reset=True)
    tr.launch(e1, kernel_variant=1)
    steps1 = tr.counters(reset=True).ray_steps
    yield dict(tracers=tracers, cfg=cfg, bt=bt, r=r, ne=ne, te=te, gain=gain, d_gain=torch_cuda.from_numpy(gain).cuda(),
               gp=api.default_gain_params(relax=1.0), ofields=ofields, oe=oe, osteps=osteps, obg=obg,
               e1=e1.cpu().numpy(), steps1=steps1)
    for tr in tracers.values():
        tr.close()


def test_launch_moves_box_a_and_ends_rays_inside_the_grid(api, oracle, case, torch_cuda):
    """What the eight launches below exercise.  On the oracle's ray paths (CPU): some ray ends inside the exit planes --
    absorbed, not escaped -- and some bundle holds a ray that crosses more cells along x or y than box A is wide, so
    that box cannot rest.  On the GPU, the window statistics of the same launch: planes or bricks were retired."""
    tr, cfg = case["tracers"][False, False], case["cfg"]
    p, d = tr.params, tr.derived
    lo = np.array([p.xmin - d.dx / 2.0, p.ymin - d.dy / 2.0, p.zmin - d.dz / 2.0])
    hi = np.array([p.xmax + d.dx / 2.0, p.ymax + d.dy / 2.0, p.zmax + d.dz / 2.0])
    bundles = api.live_ray_list(p).reshape(-1, 64)
    ended_inside, restless = 0, 0
    for b in range(len(BEAMS)):
        for ids in bundles:
            spans = []
            for k in ids[ids >= 0]:
                path = oracle.ray_path(cfg, case["bt"], case["r"], case["ne"], case["te"], b, int(k))
                assert 0 < len(path) <= d.nt
                if len(path) < d.nt and (path[-1, :3] >= lo).all() and (path[-1, :3] <= hi).all():
                    ended_inside += 1
                cells = path[:, 3:5]
                spans.append((cells.max(0) - cells.min(0)).max())
            restless += 1 if max(spans) >= 8 else 0
    assert ended_inside > 0 and restless > 0, (ended_inside, restless)
    e = tr.new_grid()
    tr.counters(reset=True)
    tr.launch(e, kernel_variant=3, stats=True)
    c = tr.counters(reset=True)
    print("window statistics: %d wave-steps, %d planes/bricks retired, %d wave-steps with box B live; oracle: %d rays end inside, "
          "%d restless bundles" % (c.wave_steps, c.slabs_retired, c.wave_steps_wide, ended_inside, restless))
    assert c.ray_steps == case["steps1"] and c.slabs_retired > 0


@pytest.mark.parametrize("generic,stats", INSTANCES)
def test_plain_trace(case, torch_cuda, generic, stats):
    tr = case["tracers"][False, False]
    e = tr.new_grid()
    tr.counters(reset=True)
    tr.launch(e, kernel_variant=3, force_wide_index=1 if generic else 0, stats=stats)
    c = tr.counters(reset=True)
    assert c.ray_steps == case["steps1"] > 0
    if stats:
        assert c.wave_steps > 0 and c.slabs_retired > 0
    else:
        assert c.global_atomics == 0 and c.wave_steps == 0      # (not the counting instantiation)
    err = parity_err(e.cpu().numpy(), case["e1"])
    print("plain, generic %d, stats %d: %d ray-steps, %d wave-steps, %d planes/bricks retired, err %.3e"
          % (generic, stats, c.ray_steps, c.wave_steps, c.slabs_retired, err))
    assert err < PARITY_TOL


@pytest.mark.parametrize("generic,stats", INSTANCES)
def test_gain_hooks(case, torch_cuda, generic, stats):
    tr = case["tracers"][generic, stats]
    e = tr.new_grid()
    bg = torch_cuda.zeros(len(BEAMS), dtype=torch_cuda.float64, device="cuda")
    tr.counters(reset=True)
    tr.launch_cbet(e, case["gp"], gain=case["d_gain"], beam_gain=bg)
    c = tr.counters(reset=True)
    err = parity_err(e.cpu().numpy(), case["oe"])
    err_bg = float(np.abs(bg.cpu().numpy() - case["obg"]).max() / np.abs(case["obg"]).max())
    print("gain hooks, generic %d, stats %d: %d ray-steps, edep %.3e, beam gain %.3e" % (generic, stats, c.ray_steps, err, err_bg))
    assert c.ray_steps == case["osteps"]
    assert (c.wave_steps > 0) == stats                          # (the counting instantiation, or not)
    assert err < TOL and err_bg < TOL


@pytest.mark.parametrize("generic,stats", INSTANCES)
def test_energy_field(case, torch_cuda, generic, stats):
    tr = case["tracers"][generic, stats]
    fe = tr.new_fields()
    tr.counters(reset=True)
    tr.launch_cbet(fe[0], case["gp"], fields="energy", gain=case["d_gain"])
    c = tr.counters(reset=True)
    fe = fe.cpu().numpy()
    err = max(parity_err(fe[0, b], case["ofields"][0, b]) for b in range(len(BEAMS)))
    print("energy field, generic %d, stats %d: %d ray-steps, err %.3e" % (generic, stats, c.ray_steps, err))
    assert c.ray_steps == case["osteps"] and not fe[1:].any()
    assert (c.wave_steps > 0) == stats                          # (the counting instantiation, or not)
    assert err < TOL


@pytest.mark.parametrize("generic,stats", INSTANCES)
def test_four_component_pass(case, torch_cuda, generic, stats):
    tr = case["tracers"][generic, stats]
    f = tr.new_fields()
    tr.counters(reset=True)
    tr.launch_cbet(f, case["gp"], fields=True, gain=case["d_gain"])
    c = tr.counters(reset=True)
    f = f.cpu().numpy()
    err = max(parity_err(f[q, b], case["ofields"][q, b]) for q in range(4) for b in range(len(BEAMS)))
    print("four components, generic %d, stats %d: %d ray-steps, err %.3e" % (generic, stats, c.ray_steps, err))
    assert c.ray_steps == case["osteps"]
    assert (c.wave_steps > 0) == stats                          # (the counting instantiation, or not)
    assert err < TOL
