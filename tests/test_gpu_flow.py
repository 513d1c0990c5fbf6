"""The flow table of the CBET gain kernels on the device (include/cbet_mi355x.h cbet_tabulate_flow):
k_tabulate_flow against its host twin (bitwise), the sphere's table against no table (bitwise, both gain kernels), an
offset and a monopole target against the unchanged oracle with a shifted box / scaled ramp radii, a caller's table, and
the CBET stage end to end on a displaced, distorted target."""
import math

import numpy as np
import pytest

from conftest import NCPU, parity_err
from helpers import gain_calls as D
from helpers import gain_worlds as W
from helpers.device_tables import context_flow
from helpers.gain_worlds import BEAMS, TOL

pytestmark = pytest.mark.gpu

UM = 1e-4                  # cm
OFFSET = (20 * UM, -35 * UM, 10 * UM)
SHIFT = W.OFFSET                         # the offset of the oracle comparisons and of the end-to-end target
N = 32


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
    return D.tracer(inputs, W.params(api, shape, len(beams)), inputs[0][beams], tabulate=False)


def _flow_bits(api, tr):
    """The flow table the tracer's context has selected, [3, nx, ny, nz] int64 bit patterns."""
    flow = context_flow(api, tr.ctx, tr.params, tr.gpu)
    assert flow is not None
    return flow


# ---- 1. device = host twin, bitwise -----------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(40, 33, 50), (32, 32, 32)], ids=["40x33x50", "32"])
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
            "monopole": api.Target(OFFSET, [0.1])}, node              # the instantiation for 0 with 1 + delta != 1


@pytest.mark.parametrize("name", ["offset", "lmax2", "lmax5", "lmax16", "centre_node", "monopole"])
def test_device_table_equals_the_host_twin_bitwise(api, torch_cuda, table_tracer, name):
    tr = table_tracer
    p, gp = tr.params, api.default_gain_params()
    targets, node = _targets(api, p)
    target = targets[name]
    api.tabulate_flow(tr.ctx, p, gp, target, D.stream(torch_cuda))
    torch_cuda.cuda.synchronize()
    got = _flow_bits(api, tr)
    want = api.flow_table(p, gp, target)
    diff = got != want.view(np.int64)
    print("%s: %d of %d words differ" % (name, int(diff.sum()), diff.size))
    assert not diff.any(), np.argwhere(diff)[:5].tolist()
    assert (want != api.flow_table(p, gp)).any()                      # ... of a table the target really changes
    if name == "centre_node":
        assert not want[(slice(None),) + node].any()


def test_second_and_replayed_calls_give_the_same_bits(api, inputs, torch_cuda):
    """The first call on a context allocates the table; later calls only enqueue: a second call and a captured, replayed
    one -- with the coefficients of the capture, the target's host array overwritten before the replay -- rewrite the
    same bits over whatever the table holds."""
    tr = _tracer(api, inputs, (N, N, N), [0, 1, 2, 3])
    p, gp = tr.params, api.default_gain_params()
    target = api.Target(OFFSET, _random_coeffs(5, 55))
    want = api.flow_table(p, gp, target).view(np.int64)
    junk = np.full(3 * N ** 3, -3.0)
    assert tr.ctx.flow() is None
    api.tabulate_flow(tr.ctx, p, gp, target, D.stream(torch_cuda))
    torch_cuda.cuda.synchronize()
    addr = tr.ctx.flow()
    assert np.array_equal(_flow_bits(api, tr), want)
    api.moveToAndFromGPU(addr, junk, junk.nbytes, tr.gpu)
    api.tabulate_flow(tr.ctx, p, gp, target, D.stream(torch_cuda))
    torch_cuda.cuda.synchronize()
    assert tr.ctx.flow() == addr and np.array_equal(_flow_bits(api, tr), want)
    side = torch_cuda.cuda.Stream()
    side.wait_stream(torch_cuda.cuda.current_stream())
    with torch_cuda.cuda.stream(side):
        graph = torch_cuda.cuda.CUDAGraph()
        with torch_cuda.cuda.graph(graph, stream=side):
            api.tabulate_flow(tr.ctx, p, gp, target, side.cuda_stream)
    torch_cuda.cuda.current_stream().wait_stream(side)
    torch_cuda.cuda.synchronize()
    target._keep[:] = 0.0                                     # the host array the capture read
    target.offset[0] = 0.0
    api.moveToAndFromGPU(addr, junk, junk.nbytes, tr.gpu)
    graph.replay()
    torch_cuda.cuda.synchronize()
    assert tr.ctx.flow() == addr and np.array_equal(_flow_bits(api, tr), want)
    del graph
    tr.close()


# ---- shared: the offset target's oracle fields and gains --------------------------------------------------------------
def _shifted(oracle, offset, **kw):
    """The oracle's config with the box moved by -offset: its flow, centred on its origin, sits where the target does."""
    cfg = oracle.default_config(N, nbeams=len(BEAMS), **kw)
    cfg.xmin -= offset[0]; cfg.xmax -= offset[0]
    cfg.ymin -= offset[1]; cfg.ymax -= offset[1]
    cfg.zmin -= offset[2]; cfg.zmax -= offset[2]
    return cfg


@pytest.fixture(scope="module")
def world(api, oracle, inputs, torch_cuda):
    """32^3, six beams, the target SHIFT off centre: the oracle's field pass on the host twin's tables of that target
    (unshifted box), its gain with the flow centred on the target (box shifted for the gain step only) and centred on the
    origin; a tracer of the sphere and one with the target and set_flow("target")."""
    bn, r, ne, te = inputs
    bn = bn[BEAMS].copy()
    sphere, tr = _tracer(api, inputs, (N, N, N), BEAMS), _tracer(api, inputs, (N, N, N), BEAMS)
    sphere.tabulate()
    gp = api.default_gain_params(relax=1.0)
    tr.set_target(SHIFT)
    tr.set_flow("target", gp)
    tr.tabulate()
    cfg, og = oracle.default_config(N, nbeams=len(BEAMS)), oracle.gain_default()
    ne3d, kap = api.target_tables(tr.params, r, ne, te, api.Target(SHIFT))
    traced = [oracle.trace_cbet(cfg, og, bn, ne3d, kap, quantity=q, per_beam=True, nthreads=NCPU) for q in (1, 2, 3, 4)]
    ofields = np.stack([t[0] for t in traced])
    k_shift, _ = oracle.gain_field(_shifted(oracle, SHIFT), og, ofields, ne3d, relax=1.0, nthreads=NCPU)
    k_centre, _ = oracle.gain_field(cfg, og, ofields, ne3d, relax=1.0, nthreads=NCPU)
    yield dict(sphere=sphere, tr=tr, gp=gp, cfg=cfg, og=og, bn=bn, ne3d=ne3d, kap=kap, ofields=ofields,
               raw=torch_cuda.from_numpy(ofields).cuda(), osteps=traced[0][1], k_shift=k_shift, k_centre=k_centre)
    sphere.close()
    tr.close()


# ---- 2. the sphere's table is a no-op ---------------------------------------------------------------------------------
@pytest.mark.parametrize("pair_once", [False, True], ids=["ordered", "pair_once"])
def test_the_spheres_table_changes_no_bit(api, torch_cuda, world, pair_once):
    """tabulate_flow(target=None) selected against no flow selected: gain and normalised fields bit for bit, the convergence
    sums `change` to the rounding of their atomic accumulation order (below) -- first call and frozen, the whole grid, a
    slab [9, 22) and the packed storage of that slab."""
    torch = torch_cuda
    tr, gp = world["sphere"], world["gp"]
    x0, x1 = 9, 22

    def calls():
        out = []
        f, k, ch = D.update(torch, tr, world["raw"], gp, pair_once)
        out += [f, k, ch]
        f2 = f.clone()
        f2[0] = torch.from_numpy(world["ofields"][0].copy()).cuda()        # fresh energy on the k entries of that call
        k2, ch2 = tr.new_grid(per_beam=True), torch.zeros(2, dtype=torch.float64, device="cuda")
        tr.gain_field(f2, k2, gp, ch2, pair_once=pair_once, frozen=True)
        out += [f2, k2, ch2]
        out += list(D.update(torch, tr, world["raw"], gp, pair_once, x=(x0, x1)))
        f_pk = torch.from_numpy(world["ofields"][:, :, x0:x1].copy()).cuda()
        g_pk = torch.zeros_like(f_pk[0])
        ch_pk = torch.zeros(2, dtype=torch.float64, device="cuda")
        api.gain_field_packed(f_pk, None, g_pk, g_pk if pair_once else None, ch_pk, x0, x1, tr.params, gp, tr.ctx, D.stream(torch))
        out += [f_pk, g_pk, ch_pk]
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in out]

    assert tr.ctx.flow() is None
    plain = calls()
    api.tabulate_flow(tr.ctx, tr.params, gp, None, D.stream(torch))
    try:
        assert tr.ctx.flow() is not None
        table = calls()
    finally:
        tr.ctx.set_flow(None)
    names = [a + b for a in ("", "frozen ", "slab ", "packed ") for b in ("fields", "gain", "change")]
    assert np.abs(plain[1]).max() > 1.0                                     # a non-trivial gain (1/cm)
    for name, a, b in zip(names, plain, table):
        same = np.array_equal(a.view(np.int64), b.view(np.int64))
        print("%-14s %s" % (name, "same bits" if same else "max |diff| %.3e of max %.3e" % (np.abs(a - b).max(), np.abs(a).max())))
    for name, a, b in zip(names, plain, table):
        if name.endswith("change"):
            # the two sums are accumulated with one fp64 atomicAdd per wavefront, in the order the wavefronts happen to finish:
            # two runs of the SAME kernel need not agree in the last bits, so bit equality cannot be asked of them.  Every
            # wavefront's addend is the same bits in both calls (the gain is); sums of n non-negative addends taken in two
            # orders differ by at most (n - 1) * 2^-53 relative, and no launch here has more than 34 * 34 = 1156 wavefronts.
            assert np.all(np.abs(a - b) <= 1156 * 2.0 ** -53 * np.abs(a)), name
        else:
            assert np.array_equal(a.view(np.int64), b.view(np.int64)), name


# ---- 3. an offset target against the unchanged oracle -----------------------------------------------------------------
def test_offset_target_matches_the_oracle_with_a_shifted_box(api, torch_cuda, world):
    want, centred = world["k_shift"], world["k_centre"]
    scale = np.abs(want).max()
    assert scale > 1.0
    moved = np.abs(want - centred).max()
    print("offset: the oracle's shifted and centred gains differ by %.3e of max |K|" % (moved / scale))
    assert moved >= 100 * TOL * scale                                       # a kernel that ignores the table cannot pass
    for pair_once in (False, True):
        _, k, _ = D.update(torch_cuda, world["tr"], world["raw"], world["gp"], pair_once)
        err = np.abs(k.cpu().numpy() - want).max() / scale
        print("offset, %s kernel: max |K - oracle| / max |K| = %.3e" % ("pair-once" if pair_once else "ordered", err))
        assert err < TOL, (pair_once, err)


# ---- 4. a monopole target against the oracle with scaled ramp radii ---------------------------------------------------
def test_monopole_target_matches_the_oracle_with_scaled_radii(api, oracle, inputs, torch_cuda, world):
    """(The fields are the offset target's: to the gain kernels they are an input like any other.)"""
    _, r, ne, te = inputs
    a = 0.06
    c00 = [a * math.sqrt(4.0 * math.pi)]                                    # 1 + c00 Y00 = 1 + a
    tr, gp, og = _tracer(api, inputs, (N, N, N), BEAMS), world["gp"], world["og"]
    tr.set_target((0.0, 0.0, 0.0), c00)
    tr.set_flow("target", gp)
    tr.tabulate()
    ne3d, _ = api.target_tables(tr.params, r, ne, te, api.Target((0.0, 0.0, 0.0), c00))
    scaled = oracle.gain_default(mach_r0=og.mach_r0 * (1.0 + a), mach_r1=og.mach_r1 * (1.0 + a))
    want, _ = oracle.gain_field(world["cfg"], scaled, world["ofields"], ne3d, relax=1.0, nthreads=NCPU)
    plain, _ = oracle.gain_field(world["cfg"], og, world["ofields"], ne3d, relax=1.0, nthreads=NCPU)
    scale = np.abs(want).max()
    assert np.abs(want - plain).max() >= 100 * TOL * scale
    for pair_once in (False, True):
        _, k, _ = D.update(torch_cuda, tr, world["raw"], gp, pair_once)
        err = np.abs(k.cpu().numpy() - want).max() / scale
        print("monopole, %s kernel: max |K - oracle| / max |K| = %.3e" % ("pair-once" if pair_once else "ordered", err))
        assert err < TOL, (pair_once, err)
    tr.close()


# ---- 5. a caller's table ----------------------------------------------------------------------------------------------
def test_callers_table(api, torch_cuda, world):
    torch = torch_cuda
    tr, gp = world["tr"], world["gp"]
    p = tr.params
    host = api.flow_table(p, gp, api.Target(SHIFT))
    try:
        # a "target" flow is tabulated from one ramp: gain parameters that carry another are refused by the callers that
        # hand theirs to the model
        tr.set_flow("target", gp)
        tr.tabulate()
        other = type(gp).from_buffer_copy(gp)
        other.mach_0 = gp.mach_0 + 0.25
        for reader in (lambda: tr.gain_field(tr.new_fields(), tr.new_grid(per_beam=True), other),
                       lambda: tr.backscatter_gain(tr.new_fields(), other, domega=[0.0])):
            with pytest.raises(ValueError, match="Mach ramp"):
                reader()
        for pair_once in (False, True):
            tr.set_flow("target", gp)
            tr.tabulate()
            f0, k0, ch0 = D.update(torch, tr, world["raw"], gp, pair_once, change=False)
            own = tr.ctx.flow()
            tr.set_flow(torch.from_numpy(host).cuda())
            assert tr.ctx.flow() not in (None, own)
            f1, k1, _ = D.update(torch, tr, world["raw"], gp, pair_once, change=False)
            assert torch.equal(k1, k0) and torch.equal(f1, f0)              # the host twin's array: tabulate_flow's bits
            assert float(k0.abs().max()) > 1.0
            tr.set_flow(torch.zeros((3, p.nx, p.ny, p.nz), dtype=torch.float64, device="cuda"))
            _, kz, _ = D.update(torch, tr, world["raw"], gp, pair_once, change=False)
            assert not bool(kz.any())                                       # no flow: eta = 0, P = 0, K = 0 exactly
        for bad in (torch.zeros((3, p.nx, p.ny, p.nz + 1), dtype=torch.float64, device="cuda"),
                    torch.zeros((p.nx, p.ny, p.nz, 3), dtype=torch.float64, device="cuda"),
                    torch.zeros((3, p.nx, p.ny, p.nz), dtype=torch.float32, device="cuda"),
                    torch.zeros((3, p.nx, p.ny, 2 * p.nz), dtype=torch.float64, device="cuda")[..., ::2]):
            with pytest.raises(ValueError):
                tr.set_flow(bad)
        with pytest.raises(ValueError):
            tr.set_flow("sphere")
    finally:
        tr.set_flow("target", gp)
        tr.tabulate()


# ---- 6. end to end on a target ----------------------------------------------------------------------------------------
def test_one_iteration_by_hand_matches_the_oracle(api, oracle, torch_cuda, world):
    """Field pass -> gain update -> energy-field pass on the offset target, against the same sequence of oracle calls (the
    shifted box for the gain step only), with equal ray-step counts."""
    tr, gp, n = world["tr"], world["gp"], len(BEAMS)
    tr.tabulate()
    f = tr.new_fields()
    tr.counters(reset=True)
    tr.launch_cbet(f, gp, fields=True)
    steps = [tr.counters(reset=True).ray_steps]
    got = f.cpu().numpy()
    err_f = max(parity_err(got[q, b], world["ofields"][q, b]) for q in range(4) for b in range(n))
    gain = tr.new_grid(per_beam=True)
    tr.gain_field(f, gain, gp, None, pair_once=True)
    scale = np.abs(world["k_shift"]).max()
    err_k = np.abs(gain.cpu().numpy() - world["k_shift"]).max() / scale
    fe = tr.new_fields()
    tr.launch_cbet(fe[0], gp, fields="energy", gain=gain)
    steps.append(tr.counters(reset=True).ray_steps)
    oe, osteps, _ = oracle.trace_cbet(world["cfg"], world["og"], world["bn"], world["ne3d"], world["kap"],
                                      gain=world["k_shift"], quantity=1, per_beam=True, nthreads=NCPU)
    fe = fe.cpu().numpy()
    err_e = max(parity_err(fe[0, b], oe[b]) for b in range(n))
    print("by hand: fields %.3e  K %.3e  energy field %.3e  steps %s (oracle %d, %d)" % (err_f, err_k, err_e, steps,
                                                                                        world["osteps"], osteps))
    assert steps == [world["osteps"], osteps]
    assert max(err_f, err_k, err_e) < TOL
    assert parity_err(fe[0].reshape(-1), world["ofields"][0].reshape(-1)) > 1e-3      # the gain really moved energy


def test_solve_on_a_displaced_distorted_target(api, inputs, torch_cuda):
    """20 um / -15 um off centre with a 2 % (2, 0) distortion, set_flow("target"): the iteration converges, what the beams
    gain and lose cancels as for the centred solve, the slab-owned loop on one rank gives the plain loop's gain, and the
    exit pass with that gain balances."""
    from cbet_raytracing_3d_amd import modes
    tr = _tracer(api, inputs, (N, N, N), BEAMS)
    tr.set_target(SHIFT, modes.target_coeffs(2, {(2, 0): 0.02}))
    gp = api.default_gain_params(tolerance=1e-6, max_passes=12, relax=1.0)
    with pytest.raises(ValueError):
        tr.cbet_solve(tr.new_grid(), gp)                                    # no flow set: refused, as before
    tr.set_flow("target")
    e1, e2 = tr.new_grid(), tr.new_grid()
    r1 = tr.cbet_solve(e1, gp)
    assert r1["converged"] and 2 <= r1["passes"] <= gp.max_passes
    assert r1["imbalance"] < 1e-4
    assert np.abs(r1["beam_gain"]).max() > 1e12                             # energy really moves between beams
    r2 = tr.cbet_solve(e2, gp, slabs=True)
    assert r2["converged"] and r2["passes"] == r1["passes"]
    kmax = float(r1["gain"].abs().max())
    assert kmax > 1.0 and float((r2["gain"] - r1["gain"]).abs().max()) < 1e-9 * kmax
    assert parity_err(e2.cpu().numpy(), e1.cpu().numpy()) < 1e-9
    assert np.abs(r1["beam_gain"] - r2["beam_gain"]).max() < 1e-9 * np.abs(r1["beam_gain"]).max()
    # the sphere's solve is another answer
    tr.set_target(None)
    e0 = tr.new_grid()
    tr.cbet_solve(e0, gp)
    assert parity_err(e0.cpu().numpy(), e1.cpu().numpy()) > 1e-3
    tr.set_target(SHIFT, modes.target_coeffs(2, {(2, 0): 0.02}))
    tally = tr.energy_balance(tr.trace_exits(tr.new_exits(), gain=r1["gain"], gain_params=gp)).cpu().numpy()
    launched, gained, absorbed, escaped, stranded, unfinished = tally[:, :6].T
    assert np.abs(gained).max() > 0
    assert np.all(np.abs((launched + gained) - (absorbed + escaped + stranded + unfinished)) <= 1e-13 * launched)
    assert abs(float(e1.sum()) / absorbed.sum() - 1.0) < 1e-9                # the exit pass absorbs what the solve deposited
    tr.close()


# ---- 7. refusal and response ------------------------------------------------------------------------------------------
def test_native_loop_refuses_a_selected_flow(api, torch_cuda, world):
    tr, gp = world["sphere"], world["gp"]
    args = (tr.d_te, tr.d_r, tr.d_ne, tr.new_grid(), tr.d_bbeam_norm, tr.d_beam_norm, tr.d_pow_r, tr.d_phase_r, tr.params,
            api.default_gain_params(max_passes=1))
    api.tabulate_flow(tr.ctx, tr.params, gp, None, D.stream(torch_cuda))
    try:
        with pytest.raises(api.CbetError) as ei:
            api.cbet_solve(*args, ctx=tr.ctx, stream=D.stream(torch_cuda))
        assert ei.value.code == api.EINVAL and "flow" in str(ei.value)
    finally:
        tr.ctx.set_flow(None)
    api.cbet_solve(*args, ctx=tr.ctx, stream=D.stream(torch_cuda))          # and runs again without one
    torch_cuda.cuda.synchronize()


def test_offset_response_with_cbet(api, inputs, torch_cuda):
    from cbet_raytracing_3d_amd import modes
    tr = _tracer(api, inputs, (N, N, N), BEAMS)
    deltas = [0.0, 20 * UM]
    gp = api.default_gain_params(max_passes=3, relax=1.0)
    plain, plain_rms = modes.offset_response(tr, deltas, lmax=4)
    cbet, cbet_rms = modes.offset_response(tr, deltas, lmax=4, cbet=gp)
    assert cbet.shape == plain.shape == (2, 5) and np.isfinite(cbet).all()
    assert tr.target is None and tr.flow is None and tr.ctx.flow() is None  # restored
    for i in range(2):
        assert np.abs(cbet[i] - plain[i]).max() > 1e-6 * np.abs(plain[i]).max()
    assert np.abs(cbet[1] - cbet[0]).max() > 1e-6 * np.abs(cbet[0]).max()   # and the CBET rows answer the offset
    tr.close()
