"""The shipped trace kernel's face handling, axis by axis.

Near a face the kernel steps with the closed-form relocation and compares the exit planes; deep inside it updates the
cell in place and compares nothing.  Which of the two a wave does is decided per AXIS (a three-bit mask, DESIGN.md
section 4.3): an axis of 14 nodes can never be deep (the origin of the 8-wide deposit box would have to be >= 7 and
<= n - 9), an axis of 48 nodes can, so the eight grids below reach every value of the mask.  Each is traced by the
shipped kernel and by kernel_variant 1, which shares no window or relocation code with it, and both are held to the CPU
oracle: cell by cell at the parity tests' 1e-9, equal ray-step and ray counts.
"""
import numpy as np
import pytest

from conftest import NCPU, parity_err

pytestmark = pytest.mark.gpu

PARITY_TOL = 1e-9          # tests/test_gpu_parity.py's bound for the same comparison
DEEP, NEVER = 48, 14
GRIDS = [(DEEP, DEEP, DEEP), (NEVER, DEEP, DEEP), (DEEP, NEVER, DEEP), (DEEP, DEEP, NEVER), (NEVER, NEVER, DEEP),
         (NEVER, DEEP, NEVER), (DEEP, NEVER, NEVER), (NEVER, NEVER, NEVER)]


def face_beams(bn):
    """Four rows of the beam table that point most nearly along +x, -x, y and z: their rays cross the grid along
    different axes and leave through different faces."""
    bn = np.asarray(bn)
    picks = []
    for k in (int(np.argmax(bn[:, 0])), int(np.argmin(bn[:, 0])), int(np.argmax(np.abs(bn[:, 1]))), int(np.argmax(np.abs(bn[:, 2])))):
        if k not in picks:
            picks.append(k)
    k = 0
    while len(picks) < 4:      # (cannot happen with the OMEGA table: the four directions are distinct rows)
        if k not in picks:
            picks.append(k)
        k += 1
    return picks


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


def _tracer(api, inputs, shape, beams):
    from cbet_raytracing_3d_amd.tracer import RayTracer
    bn, r, ne, te = inputs
    p = api.default_params(shape[0], nbeams=len(beams))
    p.ny, p.nz = shape[1], shape[2]
    return RayTracer(p, r, ne, te, beam_norm=bn[beams])


def _config(oracle, shape, beams):
    cfg = oracle.default_config(shape[0], nbeams=len(beams))
    cfg.ny, cfg.nz = shape[1], shape[2]
    return cfg


def _run(tr, grid, **kw):
    tr.counters(reset=True)
    tr.launch(grid, **kw)
    return grid.cpu().numpy(), tr.counters(reset=True)


@pytest.mark.parametrize("shape", GRIDS, ids=["x".join(map(str, s)) for s in GRIDS])
def test_every_axis_mask_against_variant_1_and_the_oracle(api, oracle, inputs, torch_cuda, shape):
    bn, r, ne, te = inputs
    beams = face_beams(bn)
    assert len(set(beams)) == 4
    tr = _tracer(api, inputs, shape, beams)
    e0, c0 = _run(tr, tr.new_grid(), kernel_variant=0)
    e1, c1 = _run(tr, tr.new_grid(), kernel_variant=1)
    oe, osteps = oracle.trace(_config(oracle, shape, beams), bn[beams].copy(), r, ne, te, nthreads=NCPU)
    print("%s beams %s: %d ray-steps, shipped vs variant 1 %.2e, shipped vs oracle %.2e" %
          (shape, beams, c0.ray_steps, parity_err(e0, e1), parity_err(e0, oe)))
    assert c0.ray_steps == c1.ray_steps == osteps and osteps > 0
    assert c0.rays_traced == c1.rays_traced == 4 * tr.derived.nlive_rays
    assert parity_err(e0, oe) < PARITY_TOL        # the oracle decides what is right ...
    assert parity_err(e1, oe) < PARITY_TOL
    assert parity_err(e0, e1) < PARITY_TOL        # ... and the two kernels agree cell by cell
    assert np.array_equal(e0 == 0, oe == 0)
    tr.close()


def test_padded_rows_equal_dense_rows(api, oracle, inputs, torch_cuda):
    """48^3 into a grid whose rows are padded to whole 64-byte lines (cbet_params.edep_zpitch) and into dense rows: the
    write-backs' row arithmetic with both pitches."""
    bn, r, ne, te = inputs
    beams = face_beams(bn)
    shape = (DEEP, DEEP, DEEP)
    tr = _tracer(api, inputs, shape, beams)
    dense, cd = _run(tr, tr.new_grid())
    pad = tr.new_grid(zpitch=True)
    assert pad.shape[2] > shape[2] + 2
    padded, cp = _run(tr, pad)
    oe, osteps = oracle.trace(_config(oracle, shape, beams), bn[beams].copy(), r, ne, te, nthreads=NCPU)
    assert cd.ray_steps == cp.ray_steps == osteps
    assert not padded[..., shape[2] + 2:].any()                   # nothing lands in the padding
    assert parity_err(padded[..., :shape[2] + 2], oe) < PARITY_TOL
    assert parity_err(dense, oe) < PARITY_TOL
    tr.close()


def _cbet_setup(api, oracle, inputs, shape, beams):
    bn, r, ne, te = inputs
    tr = _tracer(api, inputs, shape, beams)
    tr.tabulate()
    cfg = _config(oracle, shape, beams)
    ne3d, kap = oracle.node_tables(cfg, r, ne, te)
    return tr, cfg, ne3d, kap


def test_gain_hooks_on_a_grid_that_is_never_deep_along_x(api, oracle, inputs, torch_cuda):
    """The gain-hook instantiation on 14 x 48 x 48 against the CPU model, at tests/test_gpu_cbet.py's bound."""
    bn, r, ne, te = inputs
    beams, shape = face_beams(bn), (NEVER, DEEP, DEEP)
    tr, cfg, ne3d, kap = _cbet_setup(api, oracle, inputs, shape, beams)
    gain = np.random.default_rng(20261019).uniform(-40.0, 40.0, size=(len(beams),) + tuple(n + 2 for n in shape))
    e = tr.new_grid()
    bg = torch_cuda.zeros(len(beams), dtype=torch_cuda.float64, device="cuda")
    tr.counters(reset=True)
    tr.launch_cbet(e, api.default_gain_params(), gain=torch_cuda.from_numpy(gain).cuda(), beam_gain=bg)
    c = tr.counters(reset=True)
    oe, osteps, obg = oracle.trace_cbet(cfg, oracle.gain_default(), bn[beams].copy(), ne3d, kap, gain=gain, nthreads=NCPU)
    assert c.ray_steps == osteps
    assert parity_err(e.cpu().numpy(), oe) < 1e-9
    assert np.abs(bg.cpu().numpy() - obg).max() < 1e-9 * np.abs(obg).max()
    assert np.abs(obg).max() > 0
    tr.close()


def test_field_pass_on_a_grid_that_is_never_deep_along_y(api, oracle, inputs, torch_cuda):
    """The fused four-component field pass on 48 x 14 x 48 against the oracle's four single-quantity passes, the
    cross-check of tests/test_gpu_cbet.py::test_field_pass_matches_oracle."""
    bn, r, ne, te = inputs
    beams, shape = face_beams(bn), (DEEP, NEVER, DEEP)
    tr, cfg, ne3d, kap = _cbet_setup(api, oracle, inputs, shape, beams)
    f = tr.new_fields()
    tr.counters(reset=True)
    tr.launch_cbet(f, api.default_gain_params(), fields=True)
    c = tr.counters(reset=True)
    f = f.cpu().numpy()
    og = oracle.gain_default()
    for q in range(4):
        of, osteps = oracle.trace_cbet(cfg, og, bn[beams].copy(), ne3d, kap, quantity=q + 1, per_beam=True, nthreads=NCPU)[:2]
        assert c.ray_steps == osteps
        for b in range(len(beams)):
            assert parity_err(f[q, b], of[b]) < 1e-9, (q, b)
    tr.close()
