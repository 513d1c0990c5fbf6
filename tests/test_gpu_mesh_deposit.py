"""Deposit on the hydro mesh on the device (include/cbet_mi355x.h "deposit on the hydro mesh"):
k_mesh_deposit's two arms against the host twin -- the counts exactly, the energies within the any-order bound of
helpers/mesh_deposit_cases.py -- the automatic choice, the refusal of an LDS arm that does not fit, the grid-stride loop,
padded rows, overwriting, graph capture, and RayTracer.deposit_on_mesh end to end."""
import numpy as np
import pytest

from helpers import mesh_cases as M
from helpers import mesh_deposit_cases as D

pytestmark = pytest.mark.gpu

STACK = 7                  # the LDS arm takes ceil(7 / 8) = 1 grid per workgroup: seven parts of the stack


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


@pytest.fixture(scope="module")
def gpu(torch_cuda):
    return torch_cuda.cuda.current_device()


class Twin:
    """The host twin's result for grids [G, ...] (dense or padded) and what the bound needs: sum|terms| per cell is the
    twin's result for the |grid| (the grid's own for the non-negative grids here)."""

    def __init__(self, api, kind_or_cells, grids, p, S, center=D.CENTER):
        own = isinstance(kind_or_cells, str)
        c = D.cells(api, kind_or_cells, center=center) if own else kind_or_cells
        self.energy, self.outside, self.counts = api.mesh_deposit_host(c, grids, p, S)
        dense = grids[..., : p.nz + 2]
        self.mag = (self.energy, self.outside) if (dense >= 0).all() else api.mesh_deposit_host(c, np.abs(grids), p, S)[:2]
        self.n_outside = D.total_samples(p, S) - int(self.counts.sum())
        if own:
            c.close()

    def check(self, got, grids=slice(None), what=""):
        want = (self.energy[grids], self.outside[grids], self.counts)
        D.check(got, want, self.counts, self.n_outside, mag=(np.abs(self.mag[0][grids]), np.abs(self.mag[1][grids])), what=what)


def _device(api, torch, cells, grids, p, S, method, out=None):
    """api.mesh_deposit of host grids [G, nx+2, ny+2, row] (row > nz + 2: padded); returns numpy outputs."""
    dev = torch.device("cuda", cells.gpu)
    G, row = grids.shape[0], grids.shape[-1]
    q = p.copy(edep_zpitch=row if row > p.nz + 2 else 0)
    d = torch.from_numpy(np.ascontiguousarray(grids)).to(dev)
    if out is None:
        out = (torch.full((G,) + cells.shape, np.nan, dtype=torch.float64, device=dev),
               torch.full((G,), np.nan, dtype=torch.float64, device=dev),
               torch.full(cells.shape, -7, dtype=torch.int64, device=dev))
    api.mesh_deposit(cells, d, G, int(np.prod(grids.shape[1:])), q, S, method, *out, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


# ---- 1. device against twin: four grids x three kinds of cells x both arms x one grid and a stack -----------------
@pytest.fixture(scope="module", params=list(D.CASES), ids=list(D.CASES))
def case(request, api):
    shape, box, S = D.CASES[request.param]
    p = D.params(api, shape, box)
    g = D.grids(shape, STACK, seed=23)
    return {"p": p, "S": S, "grids": g, "shape": shape, "twin": {k: Twin(api, k, g, p, S) for k in D.KINDS}}


@pytest.mark.parametrize("method", [1, 2], ids=["global", "lds"])
@pytest.mark.parametrize("kind", D.KINDS)
def test_device_matches_twin(api, torch_cuda, gpu, case, kind, method):
    p, S, g, twin = case["p"], case["S"], case["grids"], case["twin"][kind]
    with D.cells(api, kind, gpu=gpu) as c:
        twin.check(_device(api, torch_cuda, c, g, p, S, method), what="stack of %d" % STACK)
        twin.check(_device(api, torch_cuda, c, g[2:3], p, S, method), grids=slice(2, 3), what="one grid")


@pytest.mark.parametrize("kind", D.KINDS)
def test_auto_is_one_of_the_arms(api, torch_cuda, gpu, case, kind):
    p, S, g, twin = case["p"], case["S"], case["grids"], case["twin"][kind]
    with D.cells(api, kind, gpu=gpu) as c:
        twin.check(_device(api, torch_cuda, c, g, p, S, 0), what="method 0")
        # counts alone: edep NULL writes cell_samples and nothing else
        dev = torch_cuda.device("cuda", gpu)
        n = torch_cuda.full(c.shape, -7, dtype=torch_cuda.int64, device=dev)
        for method in (0, 1, 2):
            api.mesh_deposit(c, None, 1, 0, p, S, method, None, None, n, torch_cuda.cuda.current_stream(dev).cuda_stream)
            torch_cuda.cuda.synchronize()
            assert np.array_equal(n.cpu().numpy(), twin.counts)


def test_lds_arm_that_does_not_fit_is_refused(api, torch_cuda, gpu, case):
    """11 x 7 x 9 cells and 64 grids: ceil(64 / 8) = 8 grids per workgroup, 693 * (8 * 8 + 4) bytes of accumulators and
    counts alone exceed the arm's 40960 bytes; the automatic choice takes the global arm."""
    p, S = case["p"], case["S"]
    g = np.concatenate([case["grids"]] * 10)[:64]
    with D.cells(api, "3d", gpu=gpu) as c:
        with pytest.raises(api.CbetError) as e:
            _device(api, torch_cuda, c, g, p, S, 2)
        assert e.value.code == api.EINVAL and "LDS" in str(e.value)
        got = _device(api, torch_cuda, c, g, p, S, 0)
    twin = case["twin"]["3d"]
    idx = np.arange(64) % STACK
    D.check(got, (twin.energy[idx], twin.outside[idx], twin.counts), twin.counts, twin.n_outside, what="64 grids, method 0")


# ---- 2. the grid-stride loop, padded rows -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(api):
    shape, box, S = D.BIG
    p = D.params(api, shape, box)
    g = D.grids(shape, 1, seed=29)
    return p, S, g, {k: Twin(api, k, g, p, S) for k in ("1d", "3d")}


@pytest.mark.parametrize("method", [1, 2], ids=["global", "lds"])
@pytest.mark.parametrize("kind", ["1d", "3d"])
def test_grid_stride_loop(api, torch_cuda, gpu, big, kind, method):
    p, S, g, twins = big
    assert (p.nx + 2) * (p.ny + 2) * (p.nz + 2) > 4096 * 256
    with D.cells(api, kind, gpu=gpu) as c:
        twins[kind].check(_device(api, torch_cuda, c, g, p, S, method), what="104x101x103")


@pytest.mark.parametrize("method", [1, 2], ids=["global", "lds"])
def test_padded_rows(api, torch_cuda, gpu, method):
    """12x7x70 at a row pitch of 77 doubles, NaN in the padding: the counts and, within the bound, the energies of the
    dense grids."""
    shape, box, S = D.CASES["12x7x70-S1"]
    p = D.params(api, shape, box)
    padded = D.grids(shape, 3, seed=31, pitch=77)
    assert np.isnan(padded[..., 72:]).all()
    twin = Twin(api, "3d", np.ascontiguousarray(padded[..., :72]), p, S)
    with D.cells(api, "3d", gpu=gpu) as c:
        for s in (S, 2):
            t = twin if s == S else Twin(api, "3d", np.ascontiguousarray(padded[..., :72]), p, s)
            got = _device(api, torch_cuda, c, padded, p, s, method)
            assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any()
            t.check(got, what="pitch 77, S = %d" % s)


# ---- 3. overwrite, graph capture ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [1, 2], ids=["global", "lds"])
def test_second_call_overwrites(api, torch_cuda, gpu, case, method):
    p, S, g, twin = case["p"], case["S"], case["grids"], case["twin"]["3d"]
    dev = torch_cuda.device("cuda", gpu)
    with D.cells(api, "3d", gpu=gpu) as c:
        out = (torch_cuda.empty((3,) + c.shape, dtype=torch_cuda.float64, device=dev),
               torch_cuda.empty(3, dtype=torch_cuda.float64, device=dev),
               torch_cuda.empty(c.shape, dtype=torch_cuda.int64, device=dev))
        _device(api, torch_cuda, c, g[4:7], p, S, method, out)
        twin.check(_device(api, torch_cuda, c, g[:3], p, S, method, out), grids=slice(0, 3), what="second call")


@pytest.mark.parametrize("method", [1, 2], ids=["global", "lds"])
def test_graph_capture(api, torch_cuda, gpu, method):
    torch = torch_cuda
    shape, box, S = D.CASES["9x14x21-S2"]
    p = D.params(api, shape, box)
    g = D.grids(shape, 3, seed=37)
    twin = Twin(api, "3d", g, p, S)
    dev = torch.device("cuda", gpu)
    with D.cells(api, "3d", gpu=gpu) as c:
        eager = _device(api, torch, c, g, p, S, method)
        twin.check(eager, what="eager")
        d = torch.from_numpy(g).to(dev)
        out = (torch.empty((3,) + c.shape, dtype=torch.float64, device=dev), torch.empty(3, dtype=torch.float64, device=dev),
               torch.empty(c.shape, dtype=torch.int64, device=dev))

        def call():
            api.mesh_deposit(c, d, 3, g[0].size, p, S, method, *out, torch.cuda.current_stream(dev).cuda_stream)

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                call()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        for _ in range(2):
            for t in out:
                t.fill_(5)
            graph.replay()
            torch.cuda.synchronize()
            twin.check(tuple(t.cpu().numpy() for t in out), what="replay")
        del graph


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def traced(api, inputs, torch_cuda):
    """A tracer on the 20x17x25 grid with helpers/mesh_cases.mesh3d at ten times its density (the critical surface lies
    inside the mesh and rays turn, as tests/test_gpu_mesh.py has it), four beams traced into per-beam grids."""
    from cbet_raytracing_3d_amd.tracer import RayTracer
    bn, r, ne, te = inputs
    tr = RayTracer(M.params(api, M.SHAPES[1], nbeams=4), r, ne, te, beam_norm=bn[[0, 1, 2, 3]])
    _, a = M.mesh3d(api)
    stack = tr.new_grid(per_beam=True)
    with pytest.raises(ValueError):
        tr.deposit_on_mesh(stack)                          # no mesh, no cells
    tr.set_plasma_mesh(a["r"], a["theta"], a["phi"], 10.0 * a["ne"], a["te"], a["u"], a["center"])
    tr.launch(stack)
    torch_cuda.cuda.synchronize()
    yield tr, a, stack
    tr.close()


@pytest.mark.parametrize("method", [0, 1], ids=["auto", "global"])     # 37 x 9 x 14 cells do not fit the LDS arm
def test_end_to_end(api, torch_cuda, traced, method):
    torch = torch_cuda
    tr, a, stack = traced
    host = stack.cpu().numpy()
    assert (host.sum(axis=(1, 2, 3)) > 0).all()
    energy, outside, samples = tr.deposit_on_mesh(stack, method=method)
    total_e, total_o, total_n = tr.deposit_on_mesh(stack.sum(dim=0), method=method)
    torch.cuda.synchronize()
    nr, nth, nph = len(a["r"]), len(a["theta"]), len(a["phi"])
    assert energy.shape == (4, nr, nth, nph) and outside.shape == (4,) and samples.shape == (nr, nth, nph)
    assert total_e.shape == (nr, nth, nph) and total_o.shape == () and torch.equal(total_n, samples)
    assert samples.dtype == torch.int64
    p, S = tr.params, 2
    n_all = D.total_samples(p, S)
    e, o, n = energy.cpu().numpy(), outside.cpu().numpy(), samples.cpu().numpy()
    assert 0 < n.sum() <= n_all
    mag = np.abs(host).sum(axis=(1, 2, 3))
    # conservation per beam: the device's cells, their sum here and numpy's grid sum are three orders of one sum
    assert np.all(np.abs(e.sum(axis=(1, 2, 3)) + o - host.sum(axis=(1, 2, 3))) <= 2.0 * n_all * D.EPS * mag)
    # against the twin on the same cells; the tracer hands out column k as node k's cell, the cells' own order may start
    # one column later (MeshCells.from_nodes)
    cells = tr._mesh_cells
    twin = Twin(api, cells, host, p, S)
    nodes = lambda x: np.roll(x, cells.column_shift, axis=-1)      # noqa: E731
    D.check((e, o, n), (nodes(twin.energy), twin.outside, nodes(twin.counts)), nodes(twin.counts), twin.n_outside,
            what="per-beam grids")
    # The stack's cells summed over the beams against the summed grid's cells.  Both are the exact sum over beams and
    # samples up to: n - 1 additions per cell and 3 over the beams on one side; 3 roundings in every node's sum over the
    # beams and n - 1 additions on the other: (n + 2) 2^-53 M each, M = the cell's sum|terms| over all beams.
    M_e, M_o = nodes(np.abs(twin.energy)).sum(axis=0), np.abs(twin.outside).sum()
    be, bo = D.bounds(n + 2, twin.n_outside + 2, M_e, M_o)
    assert np.all(np.abs(e.sum(axis=0) - total_e.cpu().numpy()) <= be) and abs(o.sum() - float(total_o)) <= bo
