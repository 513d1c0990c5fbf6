"""Perturbed targets on the device (include/cbet_mi355x.h cbet_tabulate_target): k_tabulate_target
against its host twin (bitwise), the zero target against cbet_tabulate_plasma / cbet_prepare_plasma, and the traces that
run on the perturbed tables -- launch(), the pipeline, the exit pass, a captured graph -- against the oracle's node-table
tracer fed with the host twin's tables."""
import numpy as np
import pytest

from conftest import NCPU, parity_err
from helpers.device_tables import context_tables as _download

PARITY_TOL = 1e-9          # the project's bound on the SURVEY 8(c) metric (tests/test_gpu_parity.py)
UM = 1e-4                  # cm
OFFSET = (20 * UM, -35 * UM, 10 * UM)
BEAMS = [1, 16, 29, 38, 47, 55]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "the gpu tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def api():
    from cbet_raytracing_3d_amd import api as a
    a.lib()   # raises if the HIP library was not built -- no fallback
    return a


def _random_coeffs(lmax, seed, total=0.05):
    c = np.random.default_rng(seed).standard_normal((lmax + 1) ** 2)
    return c * (total / np.abs(c).sum())


def _tracer(api, inputs, shape, beams):
    from cbet_raytracing_3d_amd.tracer import RayTracer
    bn, r, ne, te = inputs
    p = api.default_params(shape[0], nbeams=len(beams))
    p.ny, p.nz = shape[1], shape[2]
    return RayTracer(p, r, ne, te, beam_norm=bn[beams])


# ---- 6. device = host twin, bitwise -----------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(40, 33, 50), (64, 64, 64)], ids=["40x33x50", "64"])
def table_tracer(request, api, inputs, torch_cuda):
    tr = _tracer(api, inputs, request.param, [0, 1, 2, 3])
    yield tr
    tr.close()


def _targets(api, p):
    d = api.derive(p)
    node = (7, p.ny - 5, 11)
    centre = (node[0] * d.dx + p.xmin, node[1] * d.dy + p.ymin, node[2] * d.dz + p.zmin)   # s == 0 exactly at `node`
    return {"offset": api.Target(OFFSET), "lmax2": api.Target(OFFSET, _random_coeffs(2, 2)),
            "lmax16": api.Target(OFFSET, _random_coeffs(16, 16)), "centre_node": api.Target(centre, _random_coeffs(2, 3)),
            "lmax5": api.Target(OFFSET, _random_coeffs(5, 5)),        # runs the instantiation for 8
            "monopole": api.Target(OFFSET, [0.1])}                    # the instantiation for 0 with 1 + delta != 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["offset", "lmax2", "lmax16", "centre_node", "lmax5", "monopole"])
def test_device_tables_equal_the_host_twin_bitwise(api, inputs, torch_cuda, table_tracer, name):
    _, r, ne, te = inputs
    tr = table_tracer
    p, target = tr.params, _targets(api, tr.params)[name]
    api.tabulate_target(tr.ctx, p, tr.d_te, tr.d_r, tr.d_ne, target, torch_cuda.cuda.current_stream().cuda_stream)
    torch_cuda.cuda.synchronize()
    got = _download(api, tr.ctx, p, tr.gpu)
    want = api.target_tables(p, r, ne, te, target)
    plain = api.target_tables(p, r, ne, te, api.Target())
    for what, g, w, u in zip(("ne3d", "kappa3d"), got, want, plain):
        diff = g != w.view(np.int64)
        print("%s %s: %d of %d words differ" % (name, what, int(diff.sum()), diff.size))
        assert not diff.any(), (what, np.argwhere(diff)[:5].tolist())
        assert (w != u).any()                                         # ... of tables the target really changes


# ---- 7. zero target ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_zero_target_is_the_unperturbed_preparation(api, inputs, torch_cuda):
    tr = _tracer(api, inputs, (40, 33, 50), [0, 1, 2, 3])
    p, d, ctx = tr.params, tr.derived, tr.ctx
    stream = torch_cuda.cuda.current_stream().cuda_stream
    q = p.copy(beam_lo=0, beam_hi=4)

    def trace():
        e = tr.new_grid()
        api.trace_nodes(0, d.nindices, None, None, e, tr.d_bbeam_norm, tr.d_beam_norm, tr.d_pow_r, tr.d_phase_r,
                        d.xconst, d.yconst, d.zconst, q, ctx, stream)
        torch_cuda.cuda.synchronize()

    fused = api.Context(p, tr.gpu)
    api.prepare_plasma(fused, p, tr.d_te, tr.d_r, tr.d_ne, d.xconst, d.yconst, d.zconst, stream)
    builds = ctx.step_records()[1]
    api.tabulate_target(ctx, p, tr.d_te, tr.d_r, tr.d_ne, api.Target((0.0, 0.0, 0.0), np.zeros(25), lmax=4), stream)
    assert ctx.step_records()[1] == builds                 # tabulating builds no records ...
    trace()
    assert ctx.step_records()[1] == builds + 1             # ... the next launch does, once
    trace()
    assert ctx.step_records()[1] == builds + 1
    got = _download(api, ctx, p, tr.gpu, records=True)
    want = _download(api, fused, p, tr.gpu, records=True)
    for what, g, w in zip(("ne3d", "kappa3d", "records"), got, want):
        assert np.array_equal(g, w), what
    api.tabulate_plasma(ctx, p, tr.d_te, tr.d_r, tr.d_ne, stream)
    torch_cuda.cuda.synchronize()
    for what, g, w in zip(("ne3d", "kappa3d"), _download(api, ctx, p, tr.gpu), got):
        assert np.array_equal(g, w), what
    fused.close()
    tr.close()


# ---- 8 - 10, 12: traces on the perturbed tables -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def perturbed(api, oracle, inputs, torch_cuda):
    """48^3, six beams, the target 20 um off in x and -15 um in z with a 2 % (2, 0) and a 1 % (3, 2) distortion: the
    tracer with that target set, the oracle's deposit on the host twin's tables, and the default kernel's launch."""
    from cbet_raytracing_3d_amd import modes
    bn, r, ne, te = inputs
    n = 48
    offset, coeffs = (20 * UM, 0.0, -15 * UM), modes.target_coeffs(3, {(2, 0): 0.02, (3, 2): 0.01})
    tr = _tracer(api, inputs, (n, n, n), BEAMS)
    ne3d, kap = api.target_tables(tr.params, r, ne, te, api.Target(offset, coeffs))
    cfg = oracle.default_config(n, nbeams=len(BEAMS))
    oe, osteps = oracle.trace_tables(cfg, bn[BEAMS].copy(), ne3d, kap, nthreads=NCPU)
    tr.set_target(offset, coeffs)
    e = tr.new_grid()
    tr.counters(reset=True)
    tr.launch(e)
    steps = tr.counters(reset=True).ray_steps
    yield {"tr": tr, "oe": oe, "osteps": osteps, "launch": e.cpu().numpy(), "steps": steps, "offset": offset, "coeffs": coeffs}
    tr.close()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [1, 2, 3])
def test_trace_of_the_target_against_the_table_oracle(api, torch_cuda, perturbed, variant):
    tr = perturbed["tr"]
    e = tr.new_grid()
    tr.counters(reset=True)
    tr.launch(e, kernel_variant=variant)
    c = tr.counters(reset=True)
    err = parity_err(e.cpu().numpy(), perturbed["oe"])
    print("variant %d: %d ray-steps, parity error %.3e" % (variant, c.ray_steps, err))
    assert c.ray_steps == perturbed["osteps"]
    assert err < PARITY_TOL
    tr.set_target(None)
    try:
        plain = tr.new_grid()
        tr.launch(plain, kernel_variant=variant)
        assert parity_err(plain.cpu().numpy(), perturbed["oe"]) > PARITY_TOL      # the unperturbed target is another plasma
    finally:
        tr.set_target(perturbed["offset"], perturbed["coeffs"])


@pytest.mark.gpu
def test_pipeline_pass_runs_on_the_target(api, torch_cuda, perturbed):
    from cbet_raytracing_3d_amd.tracer import SweepPipeline
    tr, n = perturbed["tr"], 48
    assert perturbed["steps"] == perturbed["osteps"]
    pipe = SweepPipeline(tr, 0, 1)
    try:
        for _ in range(2):                                    # both buffer sets
            pipe.run_pass()
            got = pipe.finish().cpu().numpy()[: n + 2]
            assert parity_err(got, perturbed["launch"]) < 1e-11
        tr.set_target(None)
        plain = tr.new_grid()
        tr.launch(plain)
        pipe.run_pass()
        got = pipe.finish().cpu().numpy()[: n + 2]
        assert parity_err(got, plain.cpu().numpy()) < 1e-11
        assert parity_err(got, perturbed["launch"]) > PARITY_TOL
    finally:
        tr.set_target(perturbed["offset"], perturbed["coeffs"])
        pipe.close()


@pytest.mark.gpu
def test_exit_pass_on_the_target(api, torch_cuda, perturbed):
    tr = perturbed["tr"]
    ex = tr.trace_exits(tr.new_exits())
    rec = ex.cpu().numpy().copy().view(api.EXIT_DTYPE)[..., 0]
    assert int(rec["steps"].astype(np.int64).sum()) == perturbed["steps"] == perturbed["osteps"]
    grids = tr.new_grid(per_beam=True)
    tr.launch(grids)
    dep = grids.sum(dim=(1, 2, 3)).cpu().numpy()
    tally = tr.energy_balance(ex).cpu().numpy()
    assert np.all(np.abs(tally[:, 2] - dep) <= 1e-12 * np.abs(dep))
    assert abs(dep.sum() / perturbed["launch"].sum() - 1.0) < 1e-11


@pytest.mark.gpu
def test_cbet_stage_refuses_a_target(api, torch_cuda, perturbed):
    tr = perturbed["tr"]
    gp = api.default_gain_params()
    with pytest.raises(ValueError):
        tr.cbet_solve(tr.new_grid(), gp)
    with pytest.raises(ValueError):
        tr.launch_cbet(tr.new_grid(), gp)


# ---- 11. capture and replay -------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_target_pass_is_hip_graph_capturable(api, inputs, torch_cuda):
    """tabulate_target + zero + trace captured in a HIP graph: the replay deposits what the eager calls deposit, with the
    coefficients of the capture -- the target's host array is overwritten before the replays."""
    n, beams = 32, list(range(0, 60, 12))
    tr = _tracer(api, inputs, (n, n, n), beams)
    d, p = tr.derived, tr.params.copy(beam_lo=0, beam_hi=len(beams))
    target = api.Target((0.0, 30 * UM, -10 * UM), _random_coeffs(3, 11))
    e = tr.new_grid()

    def one_pass():
        stream = torch_cuda.cuda.current_stream().cuda_stream
        api.tabulate_target(tr.ctx, p, tr.d_te, tr.d_r, tr.d_ne, target, stream)
        e.zero_()
        api.trace_nodes(0, d.nindices, None, None, e, tr.d_bbeam_norm, tr.d_beam_norm, tr.d_pow_r, tr.d_phase_r,
                        d.xconst, d.yconst, d.zconst, p, tr.ctx, stream)

    one_pass()
    torch_cuda.cuda.synchronize()
    eager = e.clone()
    side = torch_cuda.cuda.Stream()
    side.wait_stream(torch_cuda.cuda.current_stream())
    with torch_cuda.cuda.stream(side):
        one_pass()
        graph = torch_cuda.cuda.CUDAGraph()
        with torch_cuda.cuda.graph(graph, stream=side):
            one_pass()
    torch_cuda.cuda.current_stream().wait_stream(side)
    torch_cuda.cuda.synchronize()
    target._keep[:] = 0.0                                     # the host array the capture read
    target.offset[1] = 0.0
    for _ in range(3):
        e.fill_(-1.0)
        graph.replay()
    torch_cuda.cuda.synchronize()
    assert parity_err(e.cpu().numpy(), eager.cpu().numpy()) < 1e-11
    one_pass()                                                # eagerly, the overwritten target is another plasma
    torch_cuda.cuda.synchronize()
    assert parity_err(e.cpu().numpy(), eager.cpu().numpy()) > PARITY_TOL
    del graph
    tr.close()
