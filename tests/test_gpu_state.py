"""The local plasma state of the CBET gain kernels on the device (include/cbet_mi355x.h "local plasma state of the gain
kernels"): k_mesh_state against its host twin, a uniform state table against no table (bitwise, both
gain kernels, with and without a flow table, whole grid, slab and packed slab), a table that changes from node to node
against the unchanged oracle run once per state, and the CBET stage end to end on a hydro mesh with ion fields.

Grids: 13 x 11 x 148 with sixty synthetic crowded beams (haloed rows of 150 cells: three 64-cell state groups, the last of 22
cells, rows that start off a 128-byte line: CROWDED of helpers/gain_worlds.py) and 48 x 21 x 134 with six traced beams.
The bounds are the project's: bit for bit where both sides execute the same IEEE statements, 1e-12 for two formulations of one
quantity and for the pair-once kernel against the ordered one, 1e-9 of max |K| against the oracle.

The two convergence sums (`change`) are compared as tests/test_gpu_gain_shapes.py compares them: every wavefront adds its share
with one fp64 atomicAdd in the order the wavefronts finish, so two launches of the SAME kernel need not agree in the last bits;
the addends are the same bits (the gain is), and n non-negative addends summed in two orders differ by at most (n - 1) 2^-53
relative, n the launch's wavefront count."""
import numpy as np
import pytest

from conftest import NCPU, parity_err
from helpers import gain_calls as D
from helpers import gain_worlds as W
from helpers import mesh_cases as M
from helpers import state_cases as S
from helpers.device_tables import download
from helpers.gain_worlds import BEAMS, LAST_BITS, TOL

pytestmark = pytest.mark.gpu

BIG = (104, 101, 103)      # 1,081,912 nodes: more than the launch's 4096 x 256 threads, so the grid-stride loop turns
SHIFT = W.OFFSET
# this module's own slab and cuts on the crowded grid: (9, 22) and the traced cuts clipped to its fifteen planes
SLABS = {W.TRACED: W.SLABS["traced"], W.CROWDED: (9, 15)}
CUTS = {W.TRACED: W.CUTS["traced"], W.CROWDED: [0, 1, 12, 13, 15]}


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
    return D.tracer(inputs, W.params(api, shape, len(beams)), inputs[0][beams], tabulate=False)


def _state(api, tr, bits=False):
    """The state table the tracer's context has selected, [2, nx, ny, nz]."""
    import torch
    torch.cuda.synchronize()
    addr = tr.ctx.state()
    assert addr
    return download(api, addr, (2, tr.params.nx, tr.params.ny, tr.params.nz), tr.gpu, bits)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---- 1. producer: device against twin -----------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=M.SHAPES + [BIG], ids=M.SHAPE_IDS + ["104x101x103"])
def table_tracer(request, api, inputs, torch_cuda):
    tr = _tracer(api, inputs, request.param, [0, 1, 2, 3])
    yield tr
    tr.close()


def _profile_mesh(api, inputs, angles, center):
    """The s83177 profile with ion fields derived from its te, alone or broadcast over angles."""
    _, r, ne, te = inputs
    nth, nph = angles
    theta = None if nth == 1 else np.linspace(0.1, 3.0, nth)
    phi = None if nph == 1 else np.linspace(-3.0, 2.9, nph)
    full = lambda f: np.broadcast_to(f[:, None, None], (r.size, nth, nph))      # noqa: E731
    return api.Mesh(r, theta, phi, full(ne), full(te), None, center, ti=full(0.5 * te), zbar=full(1.0 + 2.5 * te / te.max()))


@pytest.mark.parametrize("ions", [True, False], ids=["ti_zbar", "ions_null"])
@pytest.mark.parametrize("name", ["1d_centred", "1d_offset", "5x7_centred", "5x7_offset"])
def test_angle_independent_state_equals_the_host_twin_bitwise(api, inputs, torch_cuda, table_tracer, name, ions):
    tr = table_tracer
    angles, centre = name.split("_")
    mesh = _profile_mesh(api, inputs, (1, 1) if angles == "1d" else (5, 7), M.OFFSET if centre == "offset" else (0.0, 0.0, 0.0))
    gp = api.default_gain_params()
    try:
        api.tabulate_mesh_state(tr.ctx, tr.params, gp, mesh.to(tr.device), D.stream(torch_cuda), ions=ions)
        got = _state(api, tr)
    finally:
        tr.ctx.set_state(None)
    want = api.mesh_state_table(tr.params, gp, mesh, ions=ions)
    diff = got.view(np.int64) != want.view(np.int64)
    print("%s: %d of %d words differ" % (name, int(diff.sum()), diff.size))
    assert not diff.any(), np.argwhere(diff)[:5].tolist()
    assert want[0].max() > 1.2 * want[0].min() and want[0].min() > 1e6           # a state that varies (cm/s)


def test_3d_mesh_state_agrees_with_the_host_twin(api, torch_cuda, table_tracer):
    """Device and host atan2 are different functions: within 1e-12 of the largest value the model gives at the node's eight
    corners (tests/test_state_host.py's bound)."""
    tr = table_tracer
    mesh, a = S.mesh3d_ions(api)
    gp = api.default_gain_params()
    try:
        api.tabulate_mesh_state(tr.ctx, tr.params, gp, mesh.to(tr.device), D.stream(torch_cuda))
        got = _state(api, tr)
    finally:
        tr.ctx.set_state(None)
    want = api.mesh_state_table(tr.params, gp, mesh)
    R = M.Restatement(api, tr.params, a["r"], a["theta"], a["phi"], a["center"])
    _, top = S.restated_table(api, tr.params, gp, R, a["te"], a["ti"], a["zbar"])
    for c, what in enumerate(("cs", "gain_const")):
        worst = float((np.abs(got[c] - want[c]) / top[c]).max())
        words = int((got[c].view(np.int64) != want[c].view(np.int64)).sum())
        print("3d %s: %d of %d words differ, max |diff| = %.3e of the largest corner-derived value (bound %.0e)" %
              (what, words, got[c].size, worst, M.TOL))
        assert np.all(np.abs(got[c] - want[c]) <= M.TOL * top[c]), what


def test_second_and_replayed_calls_give_the_same_bits(api, inputs, torch_cuda):
    """The first call on a context allocates the table; later calls only enqueue: a second call and a captured, replayed one
    (one stream, no parallel branches) rewrite the eager bits over a spoiled table."""
    torch = torch_cuda
    n = 24
    tr = _tracer(api, inputs, (n, n, n), [0, 1, 2, 3])
    p, gp = tr.params, api.default_gain_params()
    mesh, _ = S.mesh3d_ions(api)
    dmesh = mesh.to(tr.device)
    junk = np.full(2 * n ** 3, -3.0)
    assert tr.ctx.state() is None
    api.tabulate_mesh_state(tr.ctx, p, gp, dmesh, D.stream(torch))
    addr = tr.ctx.state()
    eager = _state(api, tr, bits=True)
    api.moveToAndFromGPU(addr, junk, junk.nbytes, tr.gpu)
    api.tabulate_mesh_state(tr.ctx, p, gp, dmesh, D.stream(torch))
    assert tr.ctx.state() == addr and np.array_equal(_state(api, tr, bits=True), eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            api.tabulate_mesh_state(tr.ctx, p, gp, dmesh, side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    api.moveToAndFromGPU(addr, junk, junk.nbytes, tr.gpu)
    graph.replay()
    torch.cuda.synchronize()
    assert tr.ctx.state() == addr and np.array_equal(_state(api, tr, bits=True), eager)
    del graph
    tr.close()


# ---- the gain updates: helpers/gain_calls.py on the CPU side of helpers/gain_worlds.py ----------------------------------------
@pytest.fixture(scope="module")
def crowded(api, oracle, inputs, torch_cuda):
    """13 x 11 x 148, sixty beams, the crowded synthetic fields of W.crowded_world, whose builder asserts the preconditions:
    all three run classes beyond the first 64 cells, super-critical nodes, rows that start off a 128-byte line."""
    w = W.crowded_world(api, oracle, inputs, NCPU)
    tr = _tracer(api, inputs, W.CROWDED, list(range(60)))
    tr.tabulate()
    assert tr.grid_shape == (15, 13, 150)
    yield dict(tr=tr, raw=torch_cuda.from_numpy(w["raw"]).cuda(), raw_host=w["raw"], cfg=w["cfg"], ne3d=w["ne3d"], shape=W.CROWDED)
    tr.close()


@pytest.fixture(scope="module")
def traced(api, inputs, torch_cuda):
    """48 x 21 x 134, six beams, the device's own traced fields."""
    tr = _tracer(api, inputs, W.TRACED, BEAMS)
    tr.tabulate()
    raw = tr.new_fields()
    tr.launch_cbet(raw, api.default_gain_params(), fields=True)
    torch_cuda.cuda.synchronize()
    assert tr.grid_shape == (50, 23, 136) and float(raw[0].max()) > 0
    assert int((raw[0][..., 64:] > 0).sum()) >= 10000                           # most of it beyond the first 64-cell group
    yield dict(tr=tr, raw=raw, shape=W.TRACED)
    tr.close()


# ---- 2. a uniform table changes no bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair_once", [False, True], ids=["ordered", "pair_once"])
@pytest.mark.parametrize("flow", [False, True], ids=["ramp", "flow_table"])
@pytest.mark.parametrize("grid", ["crowded", "traced"])
def test_uniform_table_changes_no_bit(request, api, torch_cuda, grid, flow, pair_once):
    """A caller's table filled with cbet_gain_constants' two values against no table: gains and normalised fields
    torch.equal -- first call and frozen, whole grid, slab and packed slab -- and the convergence sums equal to the rounding
    of their accumulation order (the module's docstring)."""
    torch = torch_cuda
    world = request.getfixturevalue(grid)
    tr, raw, shape = world["tr"], world["raw"], world["shape"]
    gp = api.default_gain_params(relax=1.0)
    slab = SLABS[shape]
    _, cs, gc = api.gain_constants(tr.params, gp)
    table = torch.empty((2,) + shape, dtype=torch.float64, device="cuda")
    table[0], table[1] = cs, gc

    def calls():
        return [t for _, t in D.all_calls(torch, api, tr, raw, gp, pair_once, slab)]

    names = ["fields", "gain", "change", "frozen fields", "frozen gain", "frozen change", "slab fields", "slab gain",
             "slab change", "packed fields", "packed gain", "packed change"]
    waves = [D.waves(tr, pair_once, 0, tr.grid_shape[0])] * 6 + [D.waves(tr, pair_once, *slab)] * 6
    try:
        if flow:
            api.tabulate_flow(tr.ctx, tr.params, gp, api.Target(SHIFT), D.stream(torch))
        assert tr.ctx.state() is None and (tr.ctx.flow() is not None) == flow
        plain = calls()
        tr.set_gain_state(table)
        assert tr.ctx.state() == table.data_ptr()
        with_table = calls()
    finally:
        tr.set_gain_state(None)
        tr.ctx.set_flow(None)
    assert float(plain[1].abs().max()) > 1.0 and float(plain[7].abs().max()) > 1.0 and float(plain[10].abs().max()) > 1.0
    for what, n, a, b in zip(names, waves, plain, with_table):
        if what.endswith("change"):
            a, b = a.cpu().numpy(), b.cpu().numpy()
            print("%s %s: %s against %s (%d wavefronts)" % (grid, what, a.tolist(), b.tolist(), n))
            assert np.all(a > 0) and np.all(np.abs(a - b) <= (n - 1) * 2.0 ** -53 * np.abs(a)), what
        else:
            assert torch.equal(a, b), what


# ---- 3. a varying table against the unchanged oracle ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def per_state(api, oracle, crowded):
    """What does not depend on the node pattern: per state the gain constants, the host twin's flow table of the ramp with
    that state's sound speed, and the oracle's gain of the crowded fields -- each computed once."""
    tr = crowded["tr"]
    out = []
    for st in W.STATES:
        gp = api.default_gain_params(relax=1.0, **st)
        _, cs, gc = api.gain_constants(tr.params, gp)
        want, _ = oracle.gain_field(crowded["cfg"], oracle.gain_default(**st), crowded["raw_host"], crowded["ne3d"], relax=1.0,
                                    nthreads=NCPU)
        out.append(dict(cs=cs, gc=gc, flow=api.flow_table(tr.params, gp), want=want))
    assert max(s["te_ev"] for s in W.STATES) >= 4 * min(s["te_ev"] for s in W.STATES)
    return out


@pytest.fixture(scope="module", params=[3, 1], ids=["i+2j+3k", "i+2j+k"])
def varying(request, api, torch_cuda, crowded, per_state):
    """The caller's state and flow tables composed node by node, and the reference composed cell by cell, for one node
    pattern (helpers/gain_worlds.node_pattern: 3 as the request words it, 1 the cell-to-cell change along z it describes)."""
    torch = torch_cuda
    kz = request.param
    nodes, cells = W.node_pattern(W.CROWDED, kz), W.cell_pattern(W.CROWDED, kz)
    if kz == 1:                                  # the state changes from cell to cell along z: in every run, in every group
        assert np.all(cells[:, :, 1:-2] != cells[:, :, 2:-1])
    assert all((cells[..., z] == s).any() for z in W.Z_GROUPS for s in range(3))
    state = np.stack([np.choose(nodes, [s["cs"] for s in per_state]), np.choose(nodes, [s["gc"] for s in per_state])])
    flow = np.choose(nodes[None], [s["flow"] for s in per_state])
    want = np.choose(cells[None], [s["want"] for s in per_state])
    scale = float(np.abs(want).max())
    assert scale > 1.0 and all(np.abs(want[..., z]).max() > 1e-3 * scale for z in W.Z_GROUPS)
    # a kernel that ignores the table, or reads it at another node, cannot pass: the states' gains differ far beyond the bounds
    assert min(np.abs(a["want"] - b["want"]).max() for a in per_state for b in per_state if a is not b) > 1e-2 * scale
    tr = crowded["tr"]
    tr.set_flow(torch.from_numpy(np.ascontiguousarray(flow)).cuda())
    tr.set_gain_state(torch.from_numpy(np.ascontiguousarray(state)).cuda())
    yield dict(want=want, scale=scale, gp=api.default_gain_params(relax=1.0))
    tr.set_gain_state(None)
    tr.set_flow(None)


def test_varying_table_matches_the_oracle_per_state(torch_cuda, crowded, varying):
    """Ordered kernel bit for bit, pair-once within 1e-9 of max |K| of the reference and within 1e-12 of the ordered kernel,
    whole grid and per 64-cell z group, first call and frozen."""
    torch = torch_cuda
    tr, raw, want, scale, gp = crowded["tr"], crowded["raw"], varying["want"], varying["scale"], varying["gp"]
    f_o, k_o, ch_o, f2_o, k2_o, _ = [t.cpu().numpy() for t in D.first_and_frozen(torch, tr, raw, gp, False, change2=True)]
    f_p, k_p, ch_p, f2_p, k2_p, _ = [t.cpu().numpy() for t in D.first_and_frozen(torch, tr, raw, gp, True, change2=True)]
    err_o, err_p = float(np.abs(k_o - want).max() / scale), float(np.abs(k_p - want).max() / scale)
    by_group, by_group_oracle = D.group_errors(k_p, k_o, scale), D.group_errors(k_p, want, scale)
    print("13x11x148 varying state (max |K| %.3e): ordered vs oracle %.3e, pair-once vs oracle %.3e (by z group %s), pair-once "
          "vs ordered by z group %s, frozen vs first %.3e / %.3e" % (scale, err_o, err_p, by_group_oracle, by_group,
                                                                     np.abs(k2_o - k_o).max() / scale, np.abs(k2_p - k_o).max() / scale))
    assert np.array_equal(k_o, want)                                    # the oracle's operations in the oracle's order
    assert err_p < TOL
    assert np.abs(k_p - k_o).max() < LAST_BITS * scale
    for z, e, eo in zip(W.Z_GROUPS, by_group, by_group_oracle):
        assert e < LAST_BITS, (z, e)
        assert eo < TOL, (z, eo)
        assert np.array_equal(k_o[..., z], want[..., z]), z
    assert _same_bits(f_p, f_o) and _same_bits(f2_p, f2_o)
    assert np.abs(k2_o - k_o).max() < LAST_BITS * scale and np.abs(k2_p - k_o).max() < LAST_BITS * scale      # frozen
    assert np.abs(k2_p - want).max() < TOL * scale
    assert abs(ch_p[1] / ch_o[1] - 1.0) < 1e-12 and abs(ch_p[0] / ch_o[0] - 1.0) < 1e-12
    inten = np.where(f_p[0] > 0, f_p[0], 0.0)
    for k in (k_o, k_p):                                                # the exchange cancels per cell, whatever the cell's state
        assert np.abs((inten * k).sum(axis=0)).max() <= 1e-11 * np.abs(inten * k).sum(axis=0).max()


def test_varying_table_by_slabs_and_packed(api, torch_cuda, crowded, varying):
    """Slab-wise updates with cuts through the two-plane bricks equal the whole-grid update bit for bit in the ordered
    kernel; the packed slab, whose runs are cut elsewhere, is within 1e-12 of max |K| in the pair-once kernel (bit for bit
    in the ordered one)."""
    torch = torch_cuda
    tr, raw, gp, scale = crowded["tr"], crowded["raw"], varying["gp"], varying["scale"]
    ref = tr.new_grid(per_beam=True).fill_(-7.0)
    tr.gain_field(raw.clone(), ref, gp, None, pair_once=False)
    parts = tr.new_grid(per_beam=True).fill_(-7.0)
    fields = raw.clone()
    cuts = CUTS[W.CROWDED]
    for x0, x1 in zip(cuts[:-1], cuts[1:]):
        before = parts.clone()
        tr.gain_field(fields, parts, gp, None, pair_once=False, x_lo=x0, x_hi=x1)
        assert torch.equal(parts[:, :x0], before[:, :x0]) and torch.equal(parts[:, x1:], before[:, x1:])
    assert torch.equal(parts, ref)
    x0, x1 = SLABS[W.CROWDED]
    for pair_once in (False, True):
        f_ref, k_ref, _ = D.update(torch, tr, raw, gp, pair_once, x=(x0, x1))
        f_pk, k_pk, _ = D.packed(torch, api, tr, raw, gp, pair_once, (x0, x1))
        err = float((k_pk - k_ref[:, x0:x1]).abs().max()) / scale
        print("13x11x148 varying state, packed slab [%d, %d), %s: max |K packed - K whole| / max |K| = %.3e" %
              (x0, x1, "pair-once" if pair_once else "ordered", err))
        assert float(k_ref[:, x0:x1].abs().max()) > 1e-3 * scale
        assert torch.equal(f_pk, f_ref[:, :, x0:x1])
        if pair_once:
            assert err < LAST_BITS
        else:
            assert torch.equal(k_pk, k_ref[:, x0:x1])


# ---- 4. end to end on the mesh ----------------------------------------------------------------------------------------------
def test_cbet_stage_on_the_mesh_state(api, inputs, torch_cuda):
    """24^3, six beams, tests/test_gpu_mesh.py's 3-D mesh (density x 10: a critical surface) with ti and zbar,
    set_flow("mesh") and set_gain_state("mesh")."""
    torch = torch_cuda
    n = 24
    tr = _tracer(api, inputs, (n, n, n), BEAMS)
    gp = api.default_gain_params(relax=1.0)
    mesh, a = S.mesh3d_ions(api, dense=10.0)
    args = (a["r"], a["theta"], a["phi"], a["ne"], a["te"], a["u"], a["center"])

    def update(fields, pair_once=True):
        return D.update(torch, tr, fields, gp, pair_once, change=False)[:2]

    try:
        # the scalar path on the profiles, for the end
        tr.tabulate()
        plain_fields = tr.new_fields()
        tr.launch_cbet(plain_fields, gp, fields=True)
        f_plain, k_plain = update(plain_fields)
        assert float(k_plain.abs().max()) > 0
        with pytest.raises(ValueError):
            tr.set_gain_state("mesh")                                   # no mesh
        tr.set_plasma_mesh(*args, ti=a["ti"], zbar=a["zbar"])
        tr.set_flow("mesh")
        tr.set_gain_state("mesh")
        assert tr.ctx.state() is None
        with pytest.raises(ValueError):
            tr.gain_field(tr.new_fields(), tr.new_grid(per_beam=True), gp)      # no table before tabulate()
        # every reader of the gain model refuses alike: first the missing state table, then -- the state set aside -- the
        # missing table of the "mesh" flow
        blank = tr.new_fields()
        readers = (lambda: tr.gain_field(blank, tr.new_grid(per_beam=True), gp), lambda: tr.pair_amplitude(blank, gp),
                   lambda: tr.exchange_matrix(blank, gp), lambda: tr.backscatter_gain(blank, gp, domega=[0.0]))
        for reader in readers:
            with pytest.raises(ValueError, match="set_gain_state"):
                reader()
        tr.set_gain_state(None)
        assert tr.ctx.flow() is None
        for reader in readers:
            with pytest.raises(ValueError, match="set_flow"):
                reader()
        tr.set_gain_state("mesh")
        tr.tabulate()
        assert tr.ctx.state() is not None
        state = _state(api, tr)
        want = api.mesh_state_table(tr.params, gp, mesh)
        R = M.Restatement(api, tr.params, a["r"], a["theta"], a["phi"], a["center"])
        _, top = S.restated_table(api, tr.params, gp, R, a["te"], a["ti"], a["zbar"])
        assert np.all(np.abs(state - want) <= M.TOL * top)
        fields = tr.new_fields()
        tr.launch_cbet(fields, gp, fields=True)
        assert float(fields[0].max()) > 0
        f0, k0 = update(fields)
        own = tr.ctx.state()
        tr.set_gain_state(torch.from_numpy(state).to(tr.device))       # the downloaded table, passed back as the caller's
        assert tr.ctx.state() not in (None, own)
        f1, k1 = update(fields)
        assert torch.equal(k0, k1) and torch.equal(f0, f1) and float(k0.abs().max()) > 0
        tr.set_gain_state(None)
        assert tr.ctx.state() is None
        _, ks = update(fields)
        assert not torch.equal(ks, k0)                                  # the table is what the update reads
        print("24^3 mesh: max |K local - K uniform| / max |K local| = %.3e" % float((ks - k0).abs().max() / k0.abs().max()))
        # the exchange cancels per cell with the local state (both kernels)
        tr.set_gain_state("mesh")
        tr.tabulate()
        for pair_once in (False, True):
            f, k = update(fields, pair_once)
            inten = torch.where(f[0] > 0, f[0], torch.zeros_like(f[0]))
            terms = inten * k
            assert float(terms.sum(dim=0).abs().max()) <= 1e-11 * float(terms.abs().sum(dim=0).max())
        # the solve loops: what test_solve_on_a_displaced_distorted_target asks of the reports
        sgp = api.default_gain_params(tolerance=1e-6, max_passes=12, relax=1.0)
        e1, e2 = tr.new_grid(), tr.new_grid()
        r1 = tr.cbet_solve(e1, sgp)
        print("24^3 mesh solve: %d passes, converged %s, imbalance %.3e, max |beam gain| %.3e" %
              (r1["passes"], r1["converged"], r1["imbalance"], np.abs(r1["beam_gain"]).max()))
        assert r1["converged"] and 2 <= r1["passes"] <= sgp.max_passes
        assert r1["imbalance"] < 1e-4
        assert np.abs(r1["beam_gain"]).max() > 1e12                     # energy really moves between beams
        r2 = tr.cbet_solve(e2, sgp, slabs=True)
        assert r2["converged"] and r2["passes"] == r1["passes"]
        kmax = float(r1["gain"].abs().max())
        assert kmax > 1.0 and float((r2["gain"] - r1["gain"]).abs().max()) < 1e-9 * kmax
        assert parity_err(e2.cpu().numpy(), e1.cpu().numpy()) < 1e-9
        assert np.abs(r1["beam_gain"] - r2["beam_gain"]).max() < 1e-9 * np.abs(r1["beam_gain"]).max()
        # the native loop refuses a selected state table
        assert tr.ctx.state() is not None
        tr.ctx.set_flow(None)                                           # (so that the state is what it objects to)
        with pytest.raises(api.CbetError) as ei:
            api.cbet_solve(tr.d_te, tr.d_r, tr.d_ne, tr.new_grid(), tr.d_bbeam_norm, tr.d_beam_norm, tr.d_pow_r, tr.d_phase_r,
                           tr.params, api.default_gain_params(max_passes=1), ctx=tr.ctx, stream=D.stream(torch))
        assert ei.value.code == api.EINVAL and "state" in str(ei.value)
        # the mesh gone, the scalar path's bits are back
        tr.set_plasma_mesh(None)
        assert tr.mesh is None and tr.gain_state is None and tr.flow is None and tr.ctx.state() is None and tr.ctx.flow() is None
        tr.tabulate()
        f_again, k_again = update(plain_fields)
        assert torch.equal(k_again, k_plain) and torch.equal(f_again, f_plain)
        api.cbet_solve(tr.d_te, tr.d_r, tr.d_ne, tr.new_grid(), tr.d_bbeam_norm, tr.d_beam_norm, tr.d_pow_r, tr.d_phase_r,
                       tr.params, api.default_gain_params(max_passes=1), ctx=tr.ctx, stream=D.stream(torch))    # and the native loop runs
        torch.cuda.synchronize()
    finally:
        tr.close()


def test_set_plasma_mesh_checks_the_ion_fields(api, inputs, torch_cuda):
    tr = _tracer(api, inputs, (24, 24, 24), [0, 1, 2, 3])
    _, a = S.mesh3d_ions(api)
    args = (a["r"], a["theta"], a["phi"], a["ne"], a["te"], a["u"], a["center"])
    try:
        bad = a["zbar"].copy()
        bad[3, 2, 1] = 0.0
        with pytest.raises(ValueError) as ei:
            tr.set_plasma_mesh(*args, ti=a["ti"], zbar=bad)
        assert "zbar[" in str(ei.value) and tr.mesh is None
        with pytest.raises(ValueError):
            tr.set_gain_state("target")
        with pytest.raises(ValueError):
            tr.set_gain_state(torch_cuda.zeros((3, 24, 24, 24), dtype=torch_cuda.float64, device="cuda"))
        tr.set_plasma_mesh(*args)                                       # a mesh without ion fields: the gain parameters' Ti and Z
        tr.set_gain_state("mesh", api.default_gain_params(ti_ev=300.0, z_ion=2.0))
        tr.tabulate()
        want = api.mesh_state_table(tr.params, api.default_gain_params(ti_ev=300.0, z_ion=2.0), api.Mesh(*args[:5], None, a["center"]))
        got = _state(api, tr)
        assert np.abs(got - want).max(axis=(1, 2, 3)).max() <= 1e-9 * np.abs(want).max() and np.all(np.abs(got / want - 1.0) < 1e-9)
    finally:
        tr.close()
