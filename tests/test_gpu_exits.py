"""Exit pass on the GPU (include/cbet_mi355x.h cbet_trace_exits): per-ray records against the
CPU oracle's ray paths, step counts and energy against the shipped deposit kernel, layout and determinism, the
vacuum case worked out analytically, the far field against numpy, and the CBET gain hook."""
import numpy as np
import pytest

from conftest import NCPU
from helpers import config_matrix as M

pytestmark = pytest.mark.gpu

SURVEY_256_TOTAL = 1.0076068555e19    # SURVEY: sum of the 256^3 / 60-beam deposit


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


def _records(api, exits):
    """[nbeams, L, 10] float64 tensor -> numpy structured array [nbeams, L] of api.EXIT_DTYPE."""
    return exits.cpu().numpy().copy().view(api.EXIT_DTYPE)[..., 0]


def _tracer(api, inputs, n, ne=None, **kw):
    from cbet_raytracing_3d_amd.tracer import RayTracer
    bn, r, ne0, te = inputs
    return RayTracer(api.default_params(n, **kw), r, ne0 if ne is None else ne, te, beam_norm=bn)


@pytest.fixture(scope="module")
def t64(api, inputs, torch_cuda):
    tr = _tracer(api, inputs, 64)
    ex = tr.trace_exits(tr.new_exits())
    yield tr, ex
    tr.close()


@pytest.fixture(scope="module")
def t100(api, inputs, torch_cuda):
    tr = _tracer(api, inputs, 100)
    ex = tr.trace_exits(tr.new_exits())
    yield tr, ex
    tr.close()


def _check_against_oracle(api, oracle, inputs, tr, rec, pairs, cfg=None, beam_table=None):
    """pairs: (beam, slot) -> every record field against the oracle's ray path; returns the worst relative error.
    cfg, beam_table: the oracle's configuration and beam rows when they are not the default box and the OMEGA table."""
    bn, r, ne, te = inputs
    if beam_table is not None:
        bn = beam_table
    if cfg is None:
        cfg = oracle.default_config(tr.params.nx)
    d = tr.derived
    p = tr.params
    ids = tr.ray_ids()
    lo = (p.xmin - (d.dx / 2.0), p.ymin - (d.dy / 2.0), p.zmin - (d.dz / 2.0))
    hi = (p.xmax + (d.dx / 2.0), p.ymax + (d.dy / 2.0), p.zmax + (d.dz / 2.0))
    worst = 0.0
    for b, li in pairs:
        e = rec[b, li]
        path = oracle.ray_path(cfg, bn, r, ne, te, int(b), int(ids[li]))
        live, lp = oracle.launch_point(cfg, bn, int(b), int(ids[li]))
        assert live and len(path) > 0
        n = len(path)
        x, y, z, uray = path[-1, 0], path[-1, 1], path[-1, 2], path[-1, 7]
        cut = uray <= 0.05 * lp[3]
        out = x < lo[0] or x > hi[0] or y < lo[1] or y > hi[1] or z < lo[2] or z > hi[2]
        status = api.RAY_LAUNCHED | (api.RAY_CUTOFF if cut else 0) | (api.RAY_ESCAPED if out else 0)
        if not (cut or out):
            assert n == d.nt
            status = api.RAY_LAUNCHED | api.RAY_TIMEOUT
        assert (int(e["steps"]), int(e["status"])) == (n, status), (b, li, int(e["steps"]), n, int(e["status"]), status)
        for got, want in ((e["x"], x), (e["y"], y), (e["z"], z), (e["uray"], uray), (e["uray0"], lp[3])):
            err = abs(got - want) / max(abs(want), 1e-300)
            worst = max(worst, err)
            assert err <= 1e-12, (b, li, got, want)
        prev = path[-2, :3] if n > 1 else lp[:3]
        for k, comp in enumerate(("vx", "vy", "vz")):
            v = (path[-1, k] - prev[k]) / d.dt
            speed = np.sqrt(e["vx"] ** 2 + e["vy"] ** 2 + e["vz"] ** 2)
            assert abs(e[comp] - v) <= 1e-9 * speed, (b, li, comp, e[comp], v)
        assert e["gained"] == 0.0
    return worst


def test_per_ray_against_oracle_64(api, oracle, inputs, t64):
    tr, ex = t64
    rec = _records(api, ex)
    ids = tr.ray_ids()
    beams = [0, 19, 38, 59]
    pairs = [(b, li) for b in beams for li in np.nonzero(ids >= 0)[0]]
    worst = _check_against_oracle(api, oracle, inputs, tr, rec, pairs)
    # idle lanes: zero records
    assert not np.ascontiguousarray(rec[:, ids < 0]).view(np.uint8).any()
    assert np.all(rec[:, ids >= 0]["status"] & api.RAY_LAUNCHED)
    print("64^3, %d rays of beams %s: worst relative difference to the oracle %.2e" % (len(pairs), beams, worst))


@pytest.mark.parametrize("name", M.EXIT_ENTRIES)
def test_per_ray_against_oracle_across_the_knobs(api, oracle, inputs, torch_cuda, name):
    """Entries of the configuration matrix (tests/helpers/config_matrix.py) whose rays are lost after a far jump, start
    outside the box, run along grid lines or come from a strided launch rule: EVERY live ray of every beam against the
    oracle's ray path, the per-beam step counts, and the energy balance against the beam-resolved deposit."""
    from cbet_raytracing_3d_amd.tracer import RayTracer
    entry = M.BY_NAME[name]
    bn, r, ne, te = inputs
    cfg, bt = entry.config(oracle), entry.beam_table(bn)
    tr = RayTracer(entry.params(api), r, ne, te, beam_norm=bt)
    ex = tr.trace_exits(tr.new_exits())
    rec = _records(api, ex)
    ids = tr.ray_ids()
    pairs = [(b, li) for b in range(cfg.nbeams) for li in np.nonzero(ids >= 0)[0]]
    worst = _check_against_oracle(api, oracle, inputs, tr, rec, pairs, cfg=cfg, beam_table=bt)
    assert not np.ascontiguousarray(rec[:, ids < 0]).view(np.uint8).any()
    _, steps, per_beam = oracle.trace(cfg, bt, r, ne, te, nthreads=NCPU, want_per_beam=True)
    got = rec["steps"].astype(np.int64).sum(axis=1)
    assert np.array_equal(got, per_beam[:cfg.nbeams]) and int(got.sum()) == steps
    grids = tr.new_grid(per_beam=True)
    tr.launch(grids)
    dep = grids.sum(dim=(1, 2, 3)).cpu().numpy()
    tally = tr.energy_balance(ex).cpu().numpy()
    launched, gained, absorbed, escaped, stranded, unfinished = tally[:, :6].T
    status = rec[:, ids >= 0]["status"]
    print("%s: %d rays, worst relative difference to the oracle %.2e; absorbed vs deposit grids %.2e; balance %.2e; "
          "cut off %d, escaped %d, timed out %d" %
          (name, len(pairs), worst, float(np.abs(absorbed / dep - 1).max()),
           float((np.abs((launched + gained) - (absorbed + escaped + stranded + unfinished)) / launched).max()),
           int(((status & api.RAY_CUTOFF) != 0).sum()), int(((status & api.RAY_ESCAPED) != 0).sum()),
           int(((status & api.RAY_TIMEOUT) != 0).sum())))
    assert np.all(np.abs(absorbed - dep) <= 1e-12 * np.abs(dep))
    assert np.all(gained == 0.0)
    assert np.all(np.abs((launched + gained) - (absorbed + escaped + stranded + unfinished)) <= 1e-13 * launched)
    tr.close()


def test_per_ray_sample_against_oracle_100(api, oracle, inputs, t100):
    tr, ex = t100
    rec = _records(api, ex)
    slots = np.nonzero(tr.ray_ids() >= 0)[0]
    rng = np.random.default_rng(20261016)
    pairs = [(int(b), int(rng.choice(slots))) for b in rng.integers(0, 60, size=2400)]
    assert len({b for b, _ in pairs}) == 60
    worst = _check_against_oracle(api, oracle, inputs, tr, rec, pairs)
    print("100^3, %d sampled rays: worst relative difference to the oracle %.2e" % (len(pairs), worst))


def test_steps_per_beam_equal_oracle_100(api, oracle, inputs, t100):
    tr, ex = t100
    bn, r, ne, te = inputs
    rec = _records(api, ex)
    _, steps, per_beam = oracle.trace(oracle.default_config(100), bn, r, ne, te, nthreads=NCPU, want_per_beam=True)
    got = rec["steps"].astype(np.int64).sum(axis=1)
    assert np.array_equal(got, per_beam)
    assert int(got.sum()) == steps


def test_absorbed_equals_per_beam_grids_100(api, t100, torch_cuda):
    tr, ex = t100
    grids = tr.new_grid(per_beam=True)
    tr.launch(grids)
    dep = grids.sum(dim=(1, 2, 3)).cpu().numpy()
    del grids
    tally = tr.energy_balance(ex).cpu().numpy()
    assert np.all(np.abs(tally[:, 2] - dep) <= 1e-12 * np.abs(dep))
    launched, gained, absorbed, escaped, stranded, unfinished = tally[:, :6].T
    assert np.all(gained == 0.0)
    assert np.all(np.abs((launched + gained) - (absorbed + escaped + stranded + unfinished)) <= 1e-13 * launched)
    rec = _records(api, ex)
    launched_n = (rec["status"] & api.RAY_LAUNCHED) != 0
    assert np.array_equal(tally[:, 6], launched_n.sum(axis=1))
    assert np.array_equal(tally[:, 7], ((rec["status"] & api.RAY_ESCAPED) != 0).sum(axis=1))


def test_layout_and_determinism_64(api, inputs, t64, torch_cuda):
    tr, ex = t64
    tally = tr.energy_balance(ex)
    again = tr.trace_exits(tr.new_exits())
    assert torch_cuda.equal(again, ex)
    assert torch_cuda.equal(tr.energy_balance(again), tally)
    # three shards fill one buffer between them
    sh = tr.new_exits()
    for s in range(3):
        tr.trace_exits(sh, shard_index=s, shard_count=3)
    assert torch_cuda.equal(sh, ex)
    # a beam range writes its own beams' slots only
    part = tr.new_exits()
    tr.trace_exits(part, beam_lo=10, beam_hi=20)
    assert torch_cuda.equal(part[10:20], ex[10:20]) and not part[:10].any() and not part[20:].any()
    # counters: the exit pass counts like a trace
    tr.counters(reset=True)
    tr.trace_exits(tr.new_exits())
    c_exit = tr.counters(reset=True)
    tr.launch(tr.new_grid())
    c_launch = tr.counters(reset=True)
    assert (c_exit.ray_steps, c_exit.rays_traced) == (c_launch.ray_steps, c_launch.rays_traced)
    # a regrouped launch list (rays sorted by length, as scripts/regroup_by_length.py groups them): the same record per
    # (beam, ray id)
    rec = _records(api, ex)
    ids = tr.ray_ids()
    live = np.nonzero(ids >= 0)[0]
    order = live[np.argsort(-rec[0, live]["steps"], kind="stable")]
    regrouped = np.full(-(-len(order) // 64) * 64, -1, dtype=np.int32)
    regrouped[:len(order)] = ids[order]
    tr2 = _tracer(api, inputs, 64)
    tr2.set_launch_list(regrouped)
    assert tr2.ctx.list_length() == len(regrouped) and np.array_equal(tr2.ray_ids(), regrouped)
    ex2 = _records(api, tr2.trace_exits(tr2.new_exits()))
    tr2.close()
    ids2 = regrouped
    for b in range(60):
        a = {int(i): rec[b, k] for k, i in enumerate(ids) if i >= 0}
        for k, i in enumerate(ids2):
            if i >= 0:
                assert ex2[b, k].tobytes() == a[int(i)].tobytes(), (b, i)
            else:
                assert not ex2[b, k].tobytes().strip(b"\0")


def _bin(c, n):
    return int(min(np.floor(c), n - 1)) if c > 0.0 else 0


def test_vacuum_is_analytic(api, inputs, torch_cuda):
    bn = inputs[0]
    tr = _tracer(api, inputs, 64, ne=np.zeros_like(inputs[2]))
    ex = tr.trace_exits(tr.new_exits())
    rec = _records(api, ex)
    ids = tr.ray_ids()
    L = rec[:, ids >= 0]
    assert np.all(L["status"] == api.RAY_LAUNCHED | api.RAY_ESCAPED)
    assert np.array_equal(L["uray"], L["uray0"]) and np.all(L["uray0"] > 0)
    v = np.stack([L["vx"], L["vy"], L["vz"]], axis=-1)
    dirn = v / np.linalg.norm(v, axis=-1, keepdims=True)
    want = -bn / np.linalg.norm(bn, axis=1, keepdims=True)
    assert np.abs(dirn - want[:, None, :]).max() <= 1e-12
    # bins with no beam direction within 1e-6 of an edge
    ct, cp = api.farfield_bins(-bn[:, 0], -bn[:, 1], -bn[:, 2], 1, 1)
    found = None
    for ntheta in range(7, 60):
        for nphi in range(11, 80):
            a, b = ct * ntheta, cp * nphi
            if min(np.abs(a - np.round(a)).min(), np.abs(b - np.round(b)).min()) > 1e-6:
                found = (ntheta, nphi)
                break
        if found:
            break
    assert found is not None
    ntheta, nphi = found
    a, b = ct * ntheta, cp * nphi
    assert min(np.abs(a - np.round(a)).min(), np.abs(b - np.round(b)).min()) > 1e-6
    tally = tr.energy_balance(ex).cpu().numpy()
    assert np.array_equal(tally[:, 3], tally[:, 0]) and not tally[:, [1, 2, 4, 5]].any()
    for beam in range(60):
        h = tr.farfield(ex, ntheta, nphi, beams=[beam]).cpu().numpy()
        it, ip = _bin(a[beam], ntheta), _bin(b[beam], nphi)
        assert abs(h[it, ip] - tally[beam, 0]) <= 1e-12 * tally[beam, 0], beam
        h[it, ip] = 0.0
        assert not h.any(), beam
    tr.close()


def test_farfield_against_numpy_100(api, t100, torch_cuda):
    tr, ex = t100
    ntheta, nphi = 36, 72
    hist = tr.farfield(ex, ntheta, nphi).cpu().numpy()
    rec = _records(api, ex).reshape(-1)
    want = api.farfield_numpy(rec, ntheta, nphi)
    esc = rec[(rec["status"] & (api.RAY_LAUNCHED | api.RAY_ESCAPED)) == (api.RAY_LAUNCHED | api.RAY_ESCAPED)]
    ct, cp = api.farfield_bins(esc["vx"], esc["vy"], esc["vz"], ntheta, nphi)
    amb = (np.abs(ct - np.round(ct)) < 1e-9) | (np.abs(cp - np.round(cp)) < 1e-9)
    allowed = np.zeros_like(want)
    for k in np.nonzero(amb)[0]:       # a ray on an edge may land in either neighbour
        it, ip = _bin(ct[k], ntheta), _bin(cp[k], nphi)
        allowed[max(0, it - 1):it + 2, :] += esc["uray"][k] if abs(ct[k] - round(ct[k])) < 1e-9 else 0.0
        allowed[it, [(ip - 1) % nphi, ip, (ip + 1) % nphi]] += esc["uray"][k]
    assert np.all(np.abs(hist - want) <= 1e-12 * want.max() + 2 * allowed)
    tally = tr.energy_balance(ex).cpu().numpy()
    assert abs(hist.sum() - tally[:, 3].sum()) <= 1e-12 * tally[:, 3].sum()
    assert hist.sum() > 0 and (hist > 0).sum() > 10
    print("100^3 far field: %d escaped rays, %d on a bin edge" % (len(esc), int(amb.sum())))


def test_cbet_gain_hook_64(api, oracle, inputs, t64, torch_cuda):
    tr, _ = t64
    bn, r, ne, te = inputs
    gp = api.default_gain_params()
    e = tr.new_grid()
    rep = tr.cbet_solve(e, gp)
    gain = rep["gain"]
    ex = tr.trace_exits(tr.new_exits(), gain=gain, gain_params=gp)
    tally = tr.energy_balance(ex).cpu().numpy()
    gained = tally[:, 1]
    scale = 1e-9 * tally[:, 2].mean()
    assert np.abs(gained).max() > 1000 * scale            # the gain does something
    # the shipped CBET kernel's beam gain with the same gain
    bg = torch_cuda.zeros(60, dtype=torch_cuda.float64, device="cuda")
    tr.tabulate()
    out = tr.launch_cbet(tr.new_grid(), gp, gain=gain, beam_gain=bg)
    assert np.abs(gained - bg.cpu().numpy()).max() <= scale
    # the deposit of that pass is the exit pass's absorbed energy
    assert abs(float(out.sum()) - tally[:, 2].sum()) <= 1e-9 * tally[:, 2].sum()
    # ... and the CPU checker's
    cfg = oracle.default_config(64)
    ne3d, kap = oracle.node_tables(cfg, r, ne, te)
    _, _, obg = oracle.trace_cbet(cfg, oracle.gain_default(), bn, ne3d, kap, gain=gain.cpu().numpy(), quantity=0,
                                  nthreads=NCPU)
    assert np.abs(gained - obg).max() <= scale
    launched, _, absorbed, escaped, stranded, unfinished = tally[:, :6].T
    assert np.all(np.abs((launched + gained) - (absorbed + escaped + stranded + unfinished)) <= 1e-13 * launched)


@pytest.fixture(scope="module")
def t256(api, inputs, torch_cuda):
    tr = _tracer(api, inputs, 256)
    yield tr
    tr.close()


def test_steps_and_energy_tie_to_the_shipped_pass_256(api, t256, torch_cuda):
    tr = t256
    e = tr.new_grid()
    tr.counters(reset=True)
    tr.launch(e)
    c = tr.counters(reset=True)
    ex = tr.trace_exits(tr.new_exits())
    c_exit = tr.counters(reset=True)
    rec = _records(api, ex)
    total_steps = int(rec["steps"].astype(np.int64).sum())
    assert total_steps == c.ray_steps == c_exit.ray_steps == 2123497670
    tally = tr.energy_balance(ex).cpu().numpy()
    absorbed, edep = tally[:, 2].sum(), float(e.sum())
    assert abs(absorbed - edep) <= 1e-11 * edep
    assert abs(absorbed / SURVEY_256_TOTAL - 1.0) < 5e-11
    launched, gained, _, escaped, stranded, unfinished = tally[:, :6].T
    assert np.all(np.abs((launched + gained) - (tally[:, 2] + escaped + stranded + unfinished)) <= 1e-13 * launched)
    print("256^3 plain: absorbed %.6f, escaped %.6f, stranded %.6f, unfinished %.6f of the launched energy" %
          tuple(x / launched.sum() for x in (absorbed, escaped.sum(), stranded.sum(), unfinished.sum())))


def test_cbet_solve_exit_pass_256(api, t256, torch_cuda):
    tr = t256
    gp = api.default_gain_params()
    plain = tr.energy_balance(tr.trace_exits(tr.new_exits())).cpu().numpy()
    ws = torch_cuda.empty(api.cbet_workspace_bytes(tr.params) // 8, dtype=torch_cuda.float64, device="cuda")
    e = tr.new_grid()
    rep = api.cbet_solve(tr.d_te, tr.d_r, tr.d_ne, e, tr.d_bbeam_norm, tr.d_beam_norm, tr.d_pow_r, tr.d_phase_r,
                         tr.params, gp, workspace=ws, ctx=tr.ctx, stream=torch_cuda.cuda.current_stream().cuda_stream)
    torch_cuda.cuda.synchronize()
    assert rep.converged == 1
    nb, hs = tr.params.nbeams, int(np.prod(tr.grid_shape))
    gain = ws[4 * nb * hs:5 * nb * hs].view((nb,) + tr.grid_shape)
    assert gain.data_ptr() == api.cbet_workspace_gain(tr.params, ws)
    ex = tr.trace_exits(tr.new_exits(), gain=gain, gain_params=gp)
    t = tr.energy_balance(ex).cpu().numpy()
    del ws, gain
    launched = t[:, 0].sum()
    assert np.array_equal(t[:, 0], plain[:, 0])
    assert abs(t[:, 2].sum() - float(e.sum())) <= 1e-9 * float(e.sum())
    assert t[:, 3].sum() > plain[:, 3].sum()
    rest = lambda x: x[:, 3:6].sum()
    drop = plain[:, 2].sum() - t[:, 2].sum()
    assert abs((rest(t) - rest(plain)) - (drop + t[:, 1].sum())) <= 1e-9 * launched
    gained = t[:, 1]
    assert gained.sum() != 0.0
    imbalance = abs(gained.sum()) / np.abs(gained).sum()
    assert abs(imbalance - rep.imbalance) <= 1e-6 * rep.imbalance + 1e-12
    assert np.abs(gained - np.array(rep.beam_gain[:nb])).max() <= 1e-9 * t[:, 2].mean()
    print("256^3 absorption fraction: plain %.4f, after the CBET solve %.4f; escaped %.4f -> %.4f; imbalance %.2e" %
          (plain[:, 2].sum() / launched, t[:, 2].sum() / launched, plain[:, 3].sum() / launched, t[:, 3].sum() / launched,
           imbalance))
