"""The arms of the exit pass (csrc/cbet_trace_exit.hip) that a trace of the shipped plasma does
not reach: the gain hook record by record (short series, long series, clamp; ragged grid, far jumps, strided launch
rule), the wide-index instantiations, rays that run out of steps, and the two reductions on synthetic records against
long-double references written from include/cbet_mi355x.h.  Cases and references: helpers/exit_cases.py; their regimes
are asserted on the CPU oracle in test_exit_oracle.py."""
import numpy as np
import pytest

from helpers import exit_cases as X
from test_gpu_exits import _check_against_oracle, _records

pytestmark = pytest.mark.gpu


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


def _entry_tracer(api, inputs, entry, ne=None, **extra):
    from cbet_raytracing_3d_amd.tracer import RayTracer
    bn, r, ne0, te = inputs
    return RayTracer(entry.params(api, **extra), r, ne0 if ne is None else ne, te, beam_norm=entry.beam_table(bn))


@pytest.fixture(scope="module")
def ragged(api, inputs, torch_cuda):
    tr = _entry_tracer(api, inputs, X.RAGGED)
    yield tr
    tr.close()


@pytest.fixture(scope="module")
def ragged_wide(api, inputs, torch_cuda):
    tr = _entry_tracer(api, inputs, X.RAGGED, force_wide_index=1)
    yield tr
    tr.close()


def _gain_args(api, torch, name, entry=X.RAGGED):
    return (torch.from_numpy(X.gain_field(name, entry)).cuda(),
            api.default_gain_params(max_exponent=X.GAIN_MAX_EXPONENT[name]))


# ---- 1. per-ray records under a gain ---------------------------------------------------------------------------------
def _compare_with_ray_exit(api, oracle, tr, rec, ids_o, orec, label):
    """Every live record of every beam against cbet_oracle_ray_exit: steps and status equal; x, y, z, uray0 (and the
    velocity, whose kicks are the position's arithmetic) within 1e-12 relative; gained and uray within 1e-9 uray0, the
    project's bound for CBET quantities against the oracle (the kernel's gain sum is fused, the oracle's is not)."""
    ids = tr.ray_ids()
    slots = np.nonzero(ids >= 0)[0]
    assert sorted(int(i) for i in ids[slots]) == sorted(int(i) for i in ids_o)
    col = {int(i): j for j, i in enumerate(ids_o)}
    order = np.array([col[int(i)] for i in ids[slots]])
    g, o = rec[:, slots], orec[:, order]
    f = lambda k: o[..., oracle.EXIT_FIELDS.index(k)]
    assert not np.ascontiguousarray(rec[:, ids < 0]).view(np.uint8).any()
    bad = np.argwhere((g["steps"] != f("steps")) | (g["status"] != f("status")))
    assert len(bad) == 0, (label, [(int(b), int(ids[slots[j]]), int(g["steps"][b, j]), int(f("steps")[b, j]),
                                    int(g["status"][b, j]), int(f("status")[b, j])) for b, j in bad[:5]])
    worst = {}
    for k in ("x", "y", "z", "uray0"):
        worst[k] = float((np.abs(g[k] - f(k)) / np.maximum(np.abs(f(k)), 1e-300)).max())
    speed = np.sqrt(f("vx") ** 2 + f("vy") ** 2 + f("vz") ** 2)
    worst["v"] = float(max((np.abs(g[k] - f(k)) / speed).max() for k in ("vx", "vy", "vz")))
    for k in ("gained", "uray"):
        worst[k] = float((np.abs(g[k] - f(k)) / f("uray0")).max())
    reach = float((np.abs(g["gained"]) / g["uray0"]).max())
    print("%s: %d rays; worst x %.2e y %.2e z %.2e uray0 %.2e v %.2e (relative); gained %.2e uray %.2e (of uray0); "
          "max |gained| / uray0 %.3g" % (label, g.size, worst["x"], worst["y"], worst["z"], worst["uray0"], worst["v"],
                                         worst["gained"], worst["uray"], reach))
    for k in ("x", "y", "z", "uray0", "v"):
        assert worst[k] <= 1e-12, (label, k, worst[k])
    for k in ("gained", "uray"):
        assert worst[k] <= 1e-9, (label, k, worst[k])
    return reach


@pytest.mark.parametrize("name", X.GAIN_FIELDS)
def test_gain_records_against_oracle_ragged(api, oracle, inputs, ragged, torch_cuda, name):
    gain, gp = _gain_args(api, torch_cuda, name)
    rec = _records(api, ragged.trace_exits(ragged.new_exits(), gain=gain, gain_params=gp))
    ids_o, orec = X.oracle_exits(oracle, X.RAGGED, inputs, gain=X.gain_field(name),
                                 gain_cfg=X.oracle_gain_config(oracle, name))
    reach = _compare_with_ray_exit(api, oracle, ragged, rec, ids_o, orec, "20x17x25 %s" % name)
    assert reach > (1e-3 if name != "small" else 0.0)


@pytest.mark.parametrize("entry", X.MIXED_ENTRIES[1:], ids=lambda e: e.name)
def test_gain_records_against_oracle_across_the_knobs(api, oracle, inputs, torch_cuda, entry):
    """The "mixed" field where the gain hook meets rays that start outside the box and jump far (box_small) and a launch
    rule of five strided passes (strided_5)."""
    tr = _entry_tracer(api, inputs, entry)
    gain, gp = _gain_args(api, torch_cuda, "mixed", entry)
    rec = _records(api, tr.trace_exits(tr.new_exits(), gain=gain, gain_params=gp))
    ids_o, orec = X.oracle_exits(oracle, entry, inputs, gain=X.gain_field("mixed", entry),
                                 gain_cfg=X.oracle_gain_config(oracle, "mixed"))
    reach = _compare_with_ray_exit(api, oracle, tr, rec, ids_o, orec, "%s mixed" % entry.name)
    tr.close()
    assert reach > 1e-3


def test_gain_hook_rounds_as_the_deposit_kernel_lane_by_lane(api, inputs, torch_cuda):
    """The hook takes an axis's two deposit factors in the lane-dependent order of k_trace_window<16, ., 1> so that it
    "rounds exactly as the shipped kernel".  A flip on the wrong lane bit changes roundings only -- the own node's
    factor becomes 1 - (1 - |o|) for |o| -- and only where 1 - |o| is inexact: |o| < 1/2 with bits below 2^-53, which
    takes a position within half a cell of a LOW face of the grid (f < 1/2).  No comparison at 1e-9 sees that, so the
    claim is tested as stated, bit for bit, on every ray (each enters and leaves through some face).  The launch list
    is regrouped into one bundle per ray, ray j alone in lane j % 64; with shard_count = the number of (beam, bundle)
    items a shard is one ray, so the deposit kernel's beam_gain[b] of that launch is the ray's `gained` (one fp64 atomic
    onto zero), and the wave-wide choice of the series sees the same single lane in both kernels."""
    tr = _entry_tracer(api, inputs, X.RAGGED)
    nb = tr.params.nbeams
    gain, gp = _gain_args(api, torch_cuda, "mixed")
    ids = tr.ray_ids()
    live = ids[ids >= 0]
    lanes = np.arange(len(live)) % 64
    regrouped = np.full(64 * len(live), -1, dtype=np.int32)
    regrouped[64 * np.arange(len(live)) + lanes] = live
    tr.set_launch_list(regrouped)
    ex = tr.trace_exits(tr.new_exits(), gain=gain, gain_params=gp)
    items = nb * len(live)                                   # item g: beam g // len(live), bundle g % len(live)
    bg = torch_cuda.zeros((items, nb), dtype=torch_cuda.float64, device="cuda")
    dep = tr.new_grid(per_beam=True)
    for g in range(items):
        tr.launch_cbet(dep, gp, gain=gain, beam_gain=bg[g], shard_index=g, shard_count=items)
    rec = _records(api, ex)[:, 64 * np.arange(len(live)) + lanes]          # [nb][ray]
    assert np.all(rec["status"] & api.RAY_LAUNCHED) and (np.abs(rec["gained"]) > 0).mean() > 0.99
    bg = bg.cpu().numpy().reshape(nb, len(live), nb)
    for b in range(nb):
        assert not np.delete(bg[b], b, axis=1).any()        # a shard of beam b adds to beam_gain[b] alone
        got, want = rec[b]["gained"], np.ascontiguousarray(bg[b, :, b])
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (b, len(bad), [(int(live[j]), int(lanes[j]), got[j], want[j]) for j in bad[:5]])
    # every item was traced once: the deposit kernel's per-beam deposit is the records' absorbed energy
    tally = tr.energy_balance(ex).cpu().numpy()
    assert np.all(np.abs(dep.sum(dim=(1, 2, 3)).cpu().numpy() - tally[:, 2]) <= 1e-12 * tally[:, 2])
    tr.close()


# ---- 2. wide-index instantiations ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", (None, "mixed", "clamped"))
def test_wide_index_records_equal_narrow(api, ragged, ragged_wide, torch_cuda, name):
    gain, gp = (None, None) if name is None else _gain_args(api, torch_cuda, name)
    a = ragged.trace_exits(ragged.new_exits(), gain=gain, gain_params=gp)
    b = ragged_wide.trace_exits(ragged_wide.new_exits(), gain=gain, gain_params=gp)
    assert ragged_wide.params.force_wide_index == 1 and ragged.params.force_wide_index == 0
    assert torch_cuda.equal(a, b)
    assert (_records(api, b)["status"] & api.RAY_LAUNCHED).sum() > 1000
    assert torch_cuda.equal(ragged.energy_balance(a), ragged_wide.energy_balance(b))
    if name is not None:
        assert np.abs(_records(api, b)["gained"]).max() > 0.0


def test_wide_index_records_against_oracle(api, oracle, inputs, ragged_wide):
    tr = ragged_wide
    rec = _records(api, tr.trace_exits(tr.new_exits()))
    ids = tr.ray_ids()
    cfg, bt = X.RAGGED.config(oracle), X.RAGGED.beam_table(inputs[0])
    pairs = [(b, li) for b in range(cfg.nbeams) for li in np.nonzero(ids >= 0)[0]]
    worst = _check_against_oracle(api, oracle, inputs, tr, rec, pairs, cfg=cfg, beam_table=bt)
    assert not np.ascontiguousarray(rec[:, ids < 0]).view(np.uint8).any()
    print("20x17x25 wide index, %d rays: worst relative difference to the oracle %.2e" % (len(pairs), worst))


# ---- 3. rays that run out of steps -----------------------------------------------------------------------------------
def test_timed_out_rays_long_box(api, oracle, inputs, torch_cuda):
    bn, r, ne, te = inputs
    vac = np.zeros_like(ne)
    entry = X.LONG_BOX
    cfg, bt = entry.config(oracle), entry.beam_table(bn)
    tr = _entry_tracer(api, inputs, entry, ne=vac)
    nt, dt = tr.derived.nt, tr.derived.dt
    assert nt == X.LONG_BOX_NT
    ex = tr.trace_exits(tr.new_exits())
    rec = _records(api, ex)
    ids = tr.ray_ids()
    slots = np.nonzero(ids >= 0)[0]
    assert len(slots) == X.LONG_BOX_LIVE
    ids_o, orec = X.oracle_exits(oracle, entry, inputs, ne=vac, beams=X.LONG_BOX_Y_BEAMS)
    col = {int(i): j for j, i in enumerate(ids_o)}
    for k, b in enumerate(X.LONG_BOX_Y_BEAMS):
        g = rec[b, slots]
        assert np.all(g["status"] == (api.RAY_LAUNCHED | api.RAY_TIMEOUT)) and np.all(g["steps"] == nt)
        assert np.array_equal(g["uray"], g["uray0"]) and np.all(g["uray0"] > 0) and not g["gained"].any()
        # the launch velocity (the kicks are +-0): the oracle's, bit for bit, along -beam_norm at the speed of light
        o = orec[k, [col[int(i)] for i in ids[slots]]]
        v = np.stack([g["vx"], g["vy"], g["vz"]], axis=-1)
        assert v.tobytes() == np.ascontiguousarray(o[:, 3:6]).tobytes()
        assert np.all(v == v[0]) and np.all(v[0][[0, 2]] == 0.0)
        assert v[0][1] * bt[b][1] < 0 and abs(abs(v[0][1]) / X.C_LIGHT - 1.0) < 1e-14
        for j, li in enumerate(slots):
            live, lp = oracle.launch_point(cfg, bt, b, int(ids[li]))
            assert live
            pos = np.array([g["x"][j], g["y"][j], g["z"][j]])
            want = lp[:3] + v[j] * (nt * dt)
            assert np.abs(pos - want).max() <= 1e-12 * np.linalg.norm(pos), (b, li, pos, want)
    pairs = [(b, li) for b in range(cfg.nbeams) for li in slots]
    _check_against_oracle(api, oracle, (bn, r, vac, te), tr, rec, pairs, cfg=cfg, beam_table=bt)
    tally = tr.energy_balance(ex).cpu().numpy()
    yb, ob = list(X.LONG_BOX_Y_BEAMS), list(X.LONG_BOX_OTHER_BEAMS)
    assert np.all(tally[yb, 6] == X.LONG_BOX_LIVE) and np.all(tally[yb, 0] > 0)
    assert np.all(np.abs(tally[yb, 5] - tally[yb, 0]) <= X.LONG_BOX_LIVE * X.EPS * tally[yb, 0])
    assert not tally[yb][:, [1, 2, 3, 4, 7]].any()
    assert not tally[ob, 5].any() and np.all(tally[ob, 7] == X.LONG_BOX_LIVE) and np.all(tally[ob, 3] > 0)
    assert not tr.farfield(ex, 9, 13, beams=yb).cpu().numpy().any()
    assert tr.farfield(ex, 9, 13, beams=ob).cpu().numpy().sum() > 0
    tr.close()


# ---- 4. k_exit_tally on synthetic records ----------------------------------------------------------------------------
def _upload(torch, rec):
    return torch.from_numpy(np.ascontiguousarray(rec).view(np.float64).reshape(rec.shape + (10,))).cuda()


@pytest.mark.parametrize("nbeams", (1, 3))
@pytest.mark.parametrize("L", (1, 63, 255, 256, 257, 1000))
def test_exit_tally_synthetic(api, torch_cuda, L, nbeams):
    rec = X.tally_records(nbeams, L)
    want, bound = X.tally_reference(rec)
    if L == 1000:      # no vacuous pass: every status word occurs, and no two of the three exits' columns are alike
        for b in range(nbeams):
            assert set(rec[b]["status"].tolist()) == set(range(16))
            for c, d in ((3, 4), (3, 5), (4, 5)):
                assert abs(want[b, c] - want[b, d]) > 100 * max(bound[b, c], bound[b, d])
    exits = _upload(torch_cuda, rec)
    tally = torch_cuda.full((nbeams, 8), -1.0, dtype=torch_cuda.float64, device="cuda")
    api.exit_tally(exits, L, nbeams, tally)
    torch_cuda.cuda.synchronize()
    got = tally.cpu().numpy()
    err = np.abs(got.astype(np.longdouble) - want)
    frac = float(np.max(np.where(bound[:, :6] > 0, err[:, :6] / np.where(bound[:, :6] > 0, bound[:, :6], 1), 0)))
    print("tally L = %d, %d beams: worst error %.3f of the bound" % (L, nbeams, frac))
    assert np.all(err[:, :6] <= bound[:, :6]), (got, want, bound)
    assert np.array_equal(got[:, 6:], want[:, 6:].astype(np.float64))
    again = torch_cuda.full((nbeams, 8), -1.0, dtype=torch_cuda.float64, device="cuda")
    api.exit_tally(exits, L, nbeams, again)
    assert torch_cuda.equal(again, tally)


# ---- 5. k_farfield on synthetic records ------------------------------------------------------------------------------
@pytest.mark.parametrize("ntheta,nphi", ((1, 1), (7, 11), (36, 72)))
def test_farfield_exact_cases(api, torch_cuda, ntheta, nphi):
    rec, where = X.farfield_exact_records()
    want = np.zeros((ntheta, nphi))
    for k, it_of, ip_of in where:
        if it_of is not None:
            want[it_of(ntheta), ip_of(nphi)] += rec[k]["uray"]       # powers of two: exact in any order
    assert sum(1 for _, it_of, _ in where if it_of is None) >= 6
    hist = torch_cuda.zeros((ntheta, nphi), dtype=torch_cuda.float64, device="cuda")
    api.farfield(_upload(torch_cuda, rec), len(rec), ntheta, nphi, hist)
    torch_cuda.cuda.synchronize()
    got = hist.cpu().numpy()
    assert np.array_equal(got, want), (np.argwhere(got != want), got[got != want], want[got != want])
    ref, _, _ = X.farfield_reference(rec, ntheta, nphi)             # ... and the helper's reference follows the same rule
    assert np.array_equal(ref.astype(np.float64), want)


BULK_N = 4096 * 256 + 777        # one record set more than the launch cap of 4096 blocks of 256: the grid-stride loop turns
BULK_BINS = (36, 72)


@pytest.fixture(scope="module")
def bulk(api, torch_cuda):
    rec = X.farfield_bulk_records(BULK_N, *BULK_BINS)
    want, bound, count = X.farfield_reference(rec, *BULK_BINS)
    return rec, _upload(torch_cuda, rec), want, bound, count


def test_farfield_bulk(api, torch_cuda, bulk):
    rec, exits, want, bound, _ = bulk
    assert rec["uray"].max() / rec["uray"].min() > 0.9e6 and (want > 0).all()
    tail = rec[4096 * 256:]
    assert ((tail["status"] & 5) == 5).sum() > 100                # the records only a second turn of the loop reaches
    hist = torch_cuda.zeros(BULK_BINS, dtype=torch_cuda.float64, device="cuda")
    api.farfield(exits, BULK_N, *BULK_BINS, hist)
    torch_cuda.cuda.synchronize()
    err = np.abs(hist.cpu().numpy().astype(np.longdouble) - want)
    print("far field, %d records: worst error %.3f of the bound" % (BULK_N, float((err / bound).max())))
    assert np.all(err <= bound)
    # without the tail the histogram is another one in every bin the tail reaches: the comparison above sees the second turn
    head_want, _, _ = X.farfield_reference(rec[:4096 * 256], *BULK_BINS)
    touched = head_want != want
    assert touched.sum() > 100 and np.all(np.abs(head_want - want)[touched] > 100 * bound[touched])


def test_farfield_adds_into_the_histogram(api, torch_cuda, bulk):
    rec, exits, want, bound, m = bulk
    ld = np.longdouble
    pattern = 10.0 ** np.random.default_rng(20261018).uniform(3.0, 11.0, size=BULK_BINS)
    hist = torch_cuda.from_numpy(pattern.copy()).cuda()
    for calls in (1, 2):
        api.farfield(exits, BULK_N, *BULK_BINS, hist)
        torch_cuda.cuda.synchronize()
        # a bin now sums calls * m + 1 terms, the pattern among them: the same bound with those terms
        expect = pattern.astype(ld) + calls * want
        limit = (calls * m) * ld(X.EPS) * (np.abs(pattern).astype(ld) + calls * want)
        err = np.abs(hist.cpu().numpy().astype(ld) - expect)
        print("far field added %d time(s): worst error %.3f of the bound" % (calls, float((err / limit).max())))
        assert np.all(err <= limit)
        assert np.all(np.abs(hist.cpu().numpy() - pattern) > 0.5 * calls * want.astype(np.float64))
