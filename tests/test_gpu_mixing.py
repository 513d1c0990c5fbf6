"""Anderson mixing of the gain iterate on the GPU: the kernels of cbet_mix.hip against their host twins,
RayTracer.cbet_solve(mixing=) on test_gpu_cbet.py's 32^3 six-beam case against the oracle engine's mixed solve, and the
argument errors.

Bounds: bit for bit where both sides run the same IEEE statements (f, the combination, and the Gram row, whose sum order the
twin walks as the kernels do); 1e-12 of sum |a b| for a dot product summed in two orders; the solve against the oracle: the
bounds of test_gpu_cbet.py::test_solve_converges_conserves_and_matches_oracle."""
import numpy as np
import pytest

from conftest import NCPU, parity_err
from helpers import mixing_cases as MC

pytestmark = pytest.mark.gpu

N = 32
BEAMS = [0, 16, 29, 38, 47, 55]


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


def _device(torch, a, offset):
    """`a` on the device: offset 0 -- at the start of an allocation (16-byte aligned); 1 -- a view one double into one."""
    buf = torch.empty(a.size + offset, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:]
    view.copy_(torch.from_numpy(a))
    return view


def _residual(api, torch, y, x, held, offset):
    n = y.size
    dy, dx, dheld = _device(torch, y, offset), _device(torch, x, offset), [_device(torch, h, offset) for h in held]
    f = _device(torch, np.full(n, np.nan), offset)
    row = torch.full((len(held) + 1,), float("nan"), dtype=torch.float64, device="cuda")
    work = torch.empty(max(1, api.mix_work_bytes(n) // 8), dtype=torch.float64, device="cuda")
    api.mix_residual(dy, dx, f, dheld, row, work)
    return f.cpu().numpy(), row.cpu().numpy()


def _check_size(api, torch, n, depths):
    for h in depths:
        y, x, *held = MC.arrays(n, h, seed=100 * n + h)
        want_f = np.empty(n)
        want_row = api.mix_residual_host(y, x, want_f, held)
        _, fsum_row, scale = MC.residual_numpy(y, x, held)
        f0, row0 = _residual(api, torch, y, x, held, 0)
        f1, row1 = _residual(api, torch, y, x, held, 1)
        f2, row2 = _residual(api, torch, y, x, held, 0)
        print("n %d h %d: |row - twin| / sum|ab| %s, |row - fsum| / sum|ab| %s" % (
            n, h, (np.abs(row0 - want_row) / scale).tolist(), (np.abs(row0 - fsum_row) / scale).tolist()))
        assert MC.same_bytes(f0, want_f) and MC.same_bytes(f1, want_f), (n, h)
        assert (np.abs(row0 - want_row) <= 1e-12 * scale).all() and (np.abs(row0 - fsum_row) <= 1e-12 * scale).all(), (n, h)
        assert MC.same_bytes(row0, row2), (n, h)                 # two calls: the same bytes
        assert MC.same_bytes(row0, row1), (n, h)                 # a view one double into an allocation: the aligned copy's bytes
        assert MC.same_bytes(row0, want_row), (n, h)             # the twin walks the kernels' order
        # the combination of h + 1 entries, oldest first
        entries = held + [y]
        alpha = np.random.default_rng(n + h).standard_normal(h + 1)
        alpha[-1] = 1.0 - alpha[:-1].sum()
        want = np.empty(n)
        api.mix_apply_host(entries, alpha, want)
        for offset in (0, 1):
            dev = [_device(torch, e, offset) for e in entries]
            out, keep = _device(torch, np.full(n, np.nan), offset), _device(torch, np.full(n, np.nan), offset)
            api.mix_apply(dev, alpha, out, keep)
            assert MC.same_bytes(out.cpu().numpy(), want) and MC.same_bytes(keep.cpu().numpy(), want), (n, h, offset)
            api.mix_apply(dev, alpha, dev[0])                    # x_out is the oldest slot, no x_keep
            assert MC.same_bytes(dev[0].cpu().numpy(), want), (n, h, offset)
            assert all(MC.same_bytes(d.cpu().numpy(), e) for d, e in zip(dev[1:], entries[1:]))
    dy, out = _device(torch, y, 1), _device(torch, np.full(n, np.nan), 0)
    api.mix_apply([dy], [1.0], out)
    assert MC.same_bytes(out.cpu().numpy(), y)                   # alpha = {1.0}: y's bytes


# the CPU list, then three workgroup partials with a ragged tail
@pytest.mark.parametrize("n", MC.SIZES + [2 * 2048 + 3])
def test_kernels_match_the_twins(api, torch_cuda, n):
    assert api.MIX_SPAN == 2048
    _check_size(api, torch_cuda, n, range(api.MIX_MAX_DEPTH + 1))


def test_kernels_beyond_the_workgroup_cap(api, torch_cuda):
    """More spans than workgroups: the first three workgroups take a second span, the last of them a ragged one."""
    n = api.MIX_SPAN * (api.MIX_MAX_GROUPS + 2) + 5
    assert api.mix_work_bytes(n) == 8 * (api.MIX_MAX_DEPTH + 1) * api.MIX_MAX_GROUPS
    _check_size(api, torch_cuda, n, (1,))


# ---- cbet_solve ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def setup(api, oracle, inputs, torch_cuda):
    from cbet_raytracing_3d_amd.tracer import RayTracer
    bn, r, ne, te = inputs
    tr = RayTracer(api.default_params(N, nbeams=len(BEAMS)), r, ne, te, beam_norm=bn[BEAMS])
    tr.tabulate()
    cfg = oracle.default_config(N, nbeams=len(BEAMS))
    ne3d, kap = oracle.node_tables(cfg, r, ne, te)
    yield dict(tr=tr, cfg=cfg, bn=bn[BEAMS].copy(), ne3d=ne3d, kap=kap)
    tr.close()


def test_mixing_zero_is_the_plain_solve(api, setup, torch_cuda, monkeypatch):
    """mixing=0 against a call without the keyword, bit for bit.  A trace pass deposits with floating-point atomics, whose
    order differs from run to run (two solves without the keyword differ by 3e-12 relative in `change`: measured), so the
    second solve REPLAYS the fields the first one's passes deposited; every gain update, the pass count and the gain are then
    the same bytes.  The update's convergence scalars are summed with atomics too and get the bound of a sum taken in two
    orders; the deposition pass behind the loop is a trace pass again: its energy balance is compared as the existing tests
    compare two solves (1e-9)."""
    from cbet_raytracing_3d_amd import cbet_loop
    tr = setup["tr"]
    gp = api.default_gain_params(tolerance=1e-6, max_passes=12, relax=1.0)
    real, tape = cbet_loop._DeviceCbetEngine.field_passes, []

    def record(self, use_gain, si, sc, full=True):
        fields = real(self, use_gain, si, sc, full)
        tape.append((fields if full else fields[0]).clone())
        return fields

    def replay(self, use_gain, si, sc, full=True):
        (self.fields if full else self.fields[0]).copy_(tape.pop(0))
        return self.fields

    monkeypatch.setattr(cbet_loop._DeviceCbetEngine, "field_passes", record)
    rep0 = tr.cbet_solve(tr.new_grid(), gp)
    gain0 = rep0["gain"].clone()
    assert len(tape) == rep0["passes"]
    monkeypatch.setattr(cbet_loop._DeviceCbetEngine, "field_passes", replay)
    rep1 = tr.cbet_solve(tr.new_grid(), gp, mixing=0)
    assert not tape and "mixing" not in rep1 and sorted(rep0) == sorted(rep1)
    assert (rep0["passes"], rep0["converged"]) == (rep1["passes"], rep1["converged"])
    assert torch_cuda.equal(gain0, rep1["gain"])
    # `change` is the ratio of two sums of non-negative terms that the update adds up with two atomics per wavefront: each
    # within 1e-12 of itself between two orders, the ratio within 2e-12 (measured: 6e-16)
    assert abs(rep0["change"] - rep1["change"]) <= 2e-12 * rep0["change"]
    assert np.abs(rep0["beam_gain"] - rep1["beam_gain"]).max() < 1e-9 * np.abs(rep0["beam_gain"]).max()


def test_solve_with_mixing_converges_conserves_and_matches_oracle(api, oracle, setup, torch_cuda):
    from cbet_raytracing_3d_amd.cbet_loop import cbet_fixed_point
    tr = setup["tr"]
    gp = api.default_gain_params(tolerance=1e-6, max_passes=12, relax=1.0)       # the existing solve test's
    e, mine = tr.new_grid(), tr.new_grid(per_beam=True)
    rep = tr.cbet_solve(e, gp, gain=mine, mixing=3)
    mix = rep["mixing"]
    print("device: passes %d change %.3g imbalance %.3g held %s restarts %d dropped %d residual_l2 %s alpha %s" % (
        rep["passes"], rep["change"], rep["imbalance"], mix["held"], mix["restarts"], mix["dropped"], mix["residual_l2"], mix["alpha"]))
    assert rep["converged"] and rep["passes"] <= gp.max_passes
    assert rep["gain"] is mine and float(mine.abs().max()) > 1.0        # the caller's tensor holds the returned gain
    assert mix["depth"] == 3 and max(mix["held"]) <= 4 and min(mix["held"]) >= 1
    assert len(mix["residual_l2"]) == len(mix["held"]) == rep["passes"] - gp.direction_passes
    assert len(mix["alpha"]) <= max(mix["held"]) and len(mix["alpha_history"]) == len(mix["held"]) - 1
    assert mix["bytes"] == 8 * mine.numel() * 9
    # the existing solve's conservation checks
    assert rep["imbalance"] < 1e-4
    ref = tr.new_grid()
    tr.launch(ref)
    ratio = float(e.sum() / ref.sum())
    assert 0.9 < ratio < 1.1 and abs(ratio - 1.0) > 1e-4
    # the oracle engine's mixed solve of the same case
    eng = MC.mixed_oracle_engine(oracle, api, setup["cfg"], oracle.gain_default(), setup["bn"], setup["ne3d"], setup["kap"],
                                 len(BEAMS), nthreads=NCPU)
    orep = cbet_fixed_point(eng, gp, mixing=3)
    omix = orep["mixing"]
    err_e = parity_err(e.cpu().numpy(), eng.edep)
    obg = orep["beam_gain"]
    err_bg = float(np.abs(rep["beam_gain"] - obg).max() / np.abs(obg).max())
    err_gain = float(np.abs(mine.cpu().numpy() - eng.gain).max() / np.abs(eng.gain).max())
    print("oracle: passes %d held %s restarts %d alpha %s sum|alpha| %.3g" % (
        orep["passes"], omix["held"], omix["restarts"], omix["alpha"], float(np.abs(omix["alpha"]).sum())))
    print("device vs oracle-engine mixed solve: deposit %.3g, beam gain %.3g, gain %.3g" % (err_e, err_bg, err_gain))
    assert orep["converged"]
    assert err_e < 1e-7 and err_bg < 1e-7                        # the existing solve test's bounds against the oracle
    assert abs(obg.sum()) / np.abs(obg).sum() < 1e-4


def test_mixing_argument_errors(api, setup, torch_cuda):
    tr = setup["tr"]
    gp = api.default_gain_params(relax=1.0)
    for bad in (5, -1, 1.5, True):
        with pytest.raises(ValueError):
            tr.cbet_solve(tr.new_grid(), gp, mixing=bad)
    with pytest.raises(ValueError):
        tr.cbet_solve(tr.new_grid(), gp, slabs=True, mixing=2)
    a = torch_cuda.zeros(8, dtype=torch_cuda.float64, device="cuda")
    row = torch_cuda.zeros(5, dtype=torch_cuda.float64, device="cuda")
    for call in (lambda: api.mix_residual(a, a, a.clone(), [], row, a, n=-1),
                 lambda: api.mix_residual(a, a, a.clone(), [a] * 5, row, a),
                 lambda: api.mix_residual(a, a, a.clone(), [], row, None),
                 lambda: api.mix_apply([], [], a),
                 lambda: api.mix_apply([a], [1.0], a.clone(), n=-1)):
        with pytest.raises(api.CbetError) as ei:
            call()
        assert ei.value.code == api.EINVAL
