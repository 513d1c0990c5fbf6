"""Hydro-mesh plasma on the device (include/cbet_mi355x.h cbet_tabulate_mesh / cbet_tabulate_mesh_flow, DESIGN.md section
14): k_tabulate_mesh and k_mesh_flow against their host twins, the traces that run on a mesh's tables -- launch(), the
pipeline, the exit pass, a captured graph -- against the oracle's node-table tracer fed with the device's own tables, and the
CBET stage's plumbing of a mesh's flow."""
import numpy as np
import pytest

from conftest import NCPU, parity_err
from helpers import mesh_cases as M
from helpers.device_tables import context_flow, context_tables

pytestmark = pytest.mark.gpu

PARITY_TOL = 1e-9          # the project's bound on the SURVEY 8(c) metric (tests/test_gpu_parity.py)
BEAMS = [1, 16, 29, 38, 47, 55]
BIG = (104, 101, 103)      # 1,081,912 nodes: more than the launch's 4096 x 256 threads, so the grid-stride loop turns


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


def _tracer(api, inputs, shape, beams):
    from cbet_raytracing_3d_amd.tracer import RayTracer
    bn, r, ne, te = inputs
    return RayTracer(M.params(api, shape, nbeams=len(beams)), r, ne, te, beam_norm=bn[beams])


def _download(api, tr):
    """(ne3d, kappa3d) of the tracer's context and the flow table it has selected ([3, nx, ny, nz]; None without one)."""
    import torch
    torch.cuda.synchronize()
    return context_tables(api, tr.ctx, tr.params, tr.gpu, bits=False) + [context_flow(api, tr.ctx, tr.params, tr.gpu, bits=False)]


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _mesh3d(api):
    """Item 2's mesh with the density raised tenfold, so that the critical surface lies inside it and rays turn."""
    mesh, a = M.mesh3d(api)
    a["ne"] = 10.0 * a["ne"]
    return api.Mesh(a["r"], a["theta"], a["phi"], a["ne"], a["te"], a["u"], a["center"]), a


# ---- 6. device against twin, all fields --------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=M.SHAPES + [BIG], ids=M.SHAPE_IDS + ["104x101x103"])
def table_tracer(request, api, inputs, torch_cuda):
    tr = _tracer(api, inputs, request.param, [0, 1, 2, 3])
    yield tr
    tr.close()


def _tabulate_both(api, torch, tr, mesh):
    stream = torch.cuda.current_stream().cuda_stream
    dmesh = mesh.to(tr.device)
    api.tabulate_mesh(tr.ctx, tr.params, dmesh, stream)
    api.tabulate_mesh_flow(tr.ctx, tr.params, dmesh, stream)
    torch.cuda.synchronize()
    got = _download(api, tr)
    tr.ctx.set_flow(None)
    return got


@pytest.mark.parametrize("name", ["1d_centred", "1d_offset", "5x7_centred", "5x7_offset"])
def test_angle_independent_mesh_equals_the_host_twin_bitwise(api, inputs, torch_cuda, table_tracer, name):
    tr = table_tracer
    angles, centre = name.split("_")
    mesh = M.profile_mesh(api, inputs, (1, 1) if angles == "1d" else (5, 7), M.OFFSET if centre == "offset" else (0.0, 0.0, 0.0))
    got = _tabulate_both(api, torch_cuda, tr, mesh)
    want = list(api.mesh_tables(tr.params, mesh)) + [api.mesh_flow_table(tr.params, mesh)]
    for what, g, w in zip(("ne3d", "kappa3d", "flow"), got, want):
        diff = g.view(np.int64) != w.view(np.int64)
        print("%s %s: %d of %d words differ" % (name, what, int(diff.sum()), diff.size))
        assert not diff.any(), (what, np.argwhere(diff)[:5].tolist())
    assert np.abs(want[2]).max() > 1e6                                          # a flow that is there (cm/s)


def test_3d_mesh_agrees_with_the_host_twin(api, torch_cuda, table_tracer):
    """Device and host atan2 are different functions: within the bound of tests/test_mesh_host.py's item 2 -- 1e-12 of the
    largest of the node's eight corner values, carried through kappa's statements; 1e-12 of max |u| for the flow."""
    tr = table_tracer
    mesh, a = M.mesh3d(api)
    got = _tabulate_both(api, torch_cuda, tr, mesh)
    want = list(api.mesh_tables(tr.params, mesh)) + [api.mesh_flow_table(tr.params, mesh)]
    R = M.Restatement(api, tr.params, a["r"], a["theta"], a["phi"], a["center"])
    _, _, ne_bound, kap_bound = R.tables(a["ne"], a["te"])
    flow_bound = M.TOL * np.abs(want[2]).max()
    for what, g, w, bound in zip(("ne3d", "kappa3d", "flow"), got, want, (ne_bound, kap_bound, flow_bound)):
        worst = float((np.abs(g - w) / bound).max()) * M.TOL
        words = int((g.view(np.int64) != w.view(np.int64)).sum())
        print("3d %s: %d of %d words differ, max |diff| = %.3e of the bound's base (bound %.0e)" % (what, words, g.size, worst, M.TOL))
        assert np.all(np.abs(g - w) <= bound), what


# ---- 7. traces run on it ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def meshed(api, oracle, inputs, torch_cuda):
    """24^3, six beams, item 2's mesh set on the tracer: the launch's deposit, the device's tables and the oracle's deposit
    on those very tables."""
    bn = inputs[0]
    n = 24
    tr = _tracer(api, inputs, (n, n, n), BEAMS)
    mesh, a = _mesh3d(api)
    tr.set_plasma_mesh(a["r"], a["theta"], a["phi"], a["ne"], a["te"], a["u"], a["center"])
    e = tr.new_grid()
    tr.counters(reset=True)
    tr.launch(e)
    steps = tr.counters(reset=True).ray_steps
    ne3d, kap, _ = _download(api, tr)
    cfg = oracle.default_config(n, nbeams=len(BEAMS))
    oe, osteps = oracle.trace_tables(cfg, bn[BEAMS].copy(), ne3d, kap, nthreads=NCPU)
    yield {"tr": tr, "mesh": mesh, "a": a, "oe": oe, "osteps": osteps, "launch": e.cpu().numpy(), "steps": steps,
           "ne3d": ne3d, "kap": kap}
    tr.close()


def test_launch_on_the_mesh_against_the_table_oracle(api, inputs, torch_cuda, meshed):
    tr = meshed["tr"]
    want = api.mesh_tables(tr.params, meshed["mesh"])
    assert np.abs(meshed["ne3d"] - want[0]).max() <= 1e-9 * np.abs(want[0]).max()     # the mesh's tables (item 6 has the bound)
    assert meshed["ne3d"].max() > api.derive(tr.params).ncrit                         # with a critical surface in them
    err = parity_err(meshed["launch"], meshed["oe"])
    print("launch: %d ray-steps (oracle %d), parity error %.3e" % (meshed["steps"], meshed["osteps"], err))
    assert meshed["steps"] == meshed["osteps"]
    assert err < PARITY_TOL
    a = meshed["a"]
    tr.set_plasma_mesh(None)
    try:
        plain = tr.new_grid()
        tr.launch(plain)
        assert parity_err(plain.cpu().numpy(), meshed["oe"]) > PARITY_TOL             # the profiles are another plasma
    finally:
        tr.set_plasma_mesh(a["r"], a["theta"], a["phi"], a["ne"], a["te"], a["u"], a["center"])


def test_pipeline_and_exit_pass_run_on_the_mesh(api, torch_cuda, meshed):
    from cbet_raytracing_3d_amd.tracer import SweepPipeline
    tr, n = meshed["tr"], 24
    pipe = SweepPipeline(tr, 0, 1)
    try:
        for _ in range(2):                                    # both buffer sets
            pipe.run_pass()
            got = pipe.finish().cpu().numpy()[: n + 2]
            assert parity_err(got, meshed["oe"]) < PARITY_TOL
    finally:
        pipe.close()
    ex = tr.trace_exits(tr.new_exits())
    rec = ex.cpu().numpy().copy().view(api.EXIT_DTYPE)[..., 0]
    assert int(rec["steps"].astype(np.int64).sum()) == meshed["osteps"]
    grids = tr.new_grid(per_beam=True)
    tr.launch(grids)
    dep = grids.sum(dim=(1, 2, 3)).cpu().numpy()
    tally = tr.energy_balance(ex).cpu().numpy()
    assert dep.min() > 0 and np.all(np.abs(tally[:, 2] - dep) <= 1e-12 * np.abs(dep))
    assert abs(tally[:, 2].sum() / meshed["launch"].sum() - 1.0) < 1e-12


def test_mesh_pass_is_hip_graph_capturable(api, torch_cuda, meshed):
    """tabulate + launch captured on one stream and replayed twice: the tables are, bit for bit, the eager ones."""
    torch = torch_cuda
    tr = meshed["tr"]
    e = tr.new_grid()

    def one_pass():
        e.zero_()
        tr.launch(e)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        one_pass()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            one_pass()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ne_addr, kap_addr = tr.ctx.tables()
    junk = np.full(24 ** 3, -3.0)
    for _ in range(2):
        api.moveToAndFromGPU(ne_addr, junk, junk.nbytes, tr.gpu)
        api.moveToAndFromGPU(kap_addr, junk, junk.nbytes, tr.gpu)
        e.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
    ne3d, kap, _ = _download(api, tr)
    assert _same_bits(ne3d, meshed["ne3d"]) and _same_bits(kap, meshed["kap"])
    assert parity_err(e.cpu().numpy(), meshed["launch"]) < 1e-11
    del graph


# ---- 8. CBET plumbing ------------------------------------------------------------------------------------------------------
def test_cbet_stage_on_a_mesh(api, torch_cuda, meshed):
    torch = torch_cuda
    tr, a = meshed["tr"], meshed["a"]
    gp = api.default_gain_params(relax=1.0, max_passes=2)
    for call in (lambda: tr.launch_cbet(tr.new_grid(), gp), lambda: tr.cbet_solve(tr.new_grid(), gp)):
        with pytest.raises(ValueError):
            call()                                              # a mesh and no flow: refused, like a target
    try:
        tr.set_flow("mesh")
        assert tr.ctx.flow() is None
        with pytest.raises(ValueError):
            tr.gain_field(tr.new_fields(), tr.new_grid(per_beam=True), gp)     # ... and no table before tabulate()
        tr.tabulate()
        torch.cuda.synchronize()
        flow = _download(api, tr)[2]
        want = api.mesh_flow_table(tr.params, meshed["mesh"])
        assert np.abs(flow - want).max() <= 1e-9 * np.abs(want).max() and np.abs(want).max() > 1e6
        fields = tr.new_fields()
        tr.launch_cbet(fields, gp, fields=True)
        assert float(fields[0].max()) > 0

        def update():
            f, k = fields.clone(), tr.new_grid(per_beam=True)
            tr.gain_field(f, k, gp, pair_once=True)
            return f, k

        f0, k0 = update()
        own = tr.ctx.flow()
        tr.set_flow(torch.from_numpy(flow).to(tr.device))       # the downloaded table, passed back as the caller's
        assert tr.ctx.flow() not in (None, own)
        f1, k1 = update()
        assert torch.equal(k0, k1) and torch.equal(f0, f1)
        assert float(k0.abs().max()) > 0
        tr.set_flow(torch.zeros_like(torch.from_numpy(flow)).to(tr.device))
        _, kz = update()
        assert not torch.equal(kz, k0)                          # the table is what the update reads
        tr.set_flow("mesh")
        rep = tr.cbet_solve(tr.new_grid(), gp)
        assert rep["passes"] >= 1 and np.isfinite(np.asarray(rep["beam_gain"])).all()
    finally:
        tr.set_flow(None)
    # a mesh without velocity has no flow to give
    tr.set_plasma_mesh(a["r"], a["theta"], a["phi"], a["ne"], a["te"], None, a["center"])
    try:
        with pytest.raises(ValueError):
            tr.set_flow("mesh")
    finally:
        tr.set_plasma_mesh(a["r"], a["theta"], a["phi"], a["ne"], a["te"], a["u"], a["center"])


# ---- 5 (the part that needs a tracer): a mesh and a target exclude each other -----------------------------------------------
def test_mesh_and_target_exclude_each_other(api, inputs, torch_cuda):
    tr = _tracer(api, inputs, (24, 24, 24), [0, 1, 2, 3])
    _, a = M.mesh3d(api)
    args = (a["r"], a["theta"], a["phi"], a["ne"], a["te"], a["u"], a["center"])
    try:
        with pytest.raises(ValueError):
            tr.set_flow("mesh")                                 # no mesh
        tr.set_plasma_mesh(*args)
        with pytest.raises(ValueError):
            tr.set_target(M.OFFSET)
        tr.set_target(None)                                     # clearing what is not set is no offence
        tr.set_flow("mesh")
        tr.set_plasma_mesh(None)
        assert tr.mesh is None and tr.flow is None              # the mesh's flow went with it
        tr.set_target(M.OFFSET)
        with pytest.raises(ValueError):
            tr.set_plasma_mesh(*args)
        tr.set_target(None)
        bad = a["te"].copy()
        bad[3, 2, 1] = 0.0
        with pytest.raises(ValueError) as ei:
            tr.set_plasma_mesh(a["r"], a["theta"], a["phi"], a["ne"], bad, a["u"], a["center"])
        assert "te[" in str(ei.value) and tr.mesh is None
        # tensors are taken like arrays, and a cleared mesh leaves the profiles' plasma
        tr.tabulate()
        plain = _download(api, tr)[:2]
        tr.set_plasma_mesh(*[torch_cuda.from_numpy(np.ascontiguousarray(x)) for x in args[:5]], center=a["center"])
        tr.tabulate()
        torch_cuda.cuda.synchronize()
        meshed = _download(api, tr)[:2]
        want = api.mesh_tables(tr.params, api.Mesh(*args[:5], None, a["center"]))
        assert np.abs(meshed[0] - want[0]).max() <= 1e-9 * np.abs(want[0]).max() and not np.array_equal(meshed[0], plain[0])
        tr.set_plasma_mesh(None)
        tr.tabulate()
        torch_cuda.cuda.synchronize()
        again = _download(api, tr)[:2]
        assert _same_bits(again[0], plain[0]) and _same_bits(again[1], plain[1])
    finally:
        tr.close()
