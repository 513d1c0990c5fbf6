"""Ray path recorder on the GPU (include/cbet_mi355x.h cbet_trace_paths, csrc/cbet_trace_path.hip):
every sample against the CPU oracle's ray paths, the end state against the exit pass bit for bit, stride and truncation,
the closest approach against a numpy restatement on the oracle's paths, idle and invalid items, the CBET gain hook and
the wide-index instantiations.  Shapes: helpers/exit_cases.py and helpers/config_matrix.py; their regimes are asserted on
the CPU oracle in test_paths_host.py."""
import math

import numpy as np
import pytest

from helpers import config_matrix as M
from helpers import exit_cases as X
from test_paths_host import FAR_CENTRE_BEAM, closest_approach

pytestmark = pytest.mark.gpu

TOL = 1e-12            # relative, the bound test_gpu_exits.py holds the exit records to against the same oracle
GAIN_TOL = 1e-9        # of uray0, the bound of test_gpu_exit_arms.py for the gain hook against the same oracle
NAN_PATTERN = 0x7FF8DEADBEEF0001      # a quiet NaN with a payload: the guard rows behind the arrays


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


def _host(api, samples, turns):
    """(samples [capacity, nitems] of api.PATH_DTYPE or None, turns [nitems] of api.TURN_DTYPE) as numpy."""
    s = None if samples is None else samples.cpu().numpy().copy().view(api.PATH_DTYPE)[..., 0]
    return s, turns.cpu().numpy().copy().view(api.TURN_DTYPE)[..., 0]


def _raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return a.shape == b.shape and _raw(a).tobytes() == _raw(b).tobytes()


class Case:
    """A tracer, an item list, the stride-1 run of it about the origin, and the oracle's launch point and path per item."""

    def __init__(self, api, oracle, inputs, entry, tr, beams, raynums, ne=None):
        bn, r, ne0, te = inputs
        self.entry, self.tr, self.beams, self.raynums = entry, tr, beams, raynums
        self.cfg, self.bt = entry.config(oracle), entry.beam_table(bn)
        self.S, self.T = _host(api, *tr.trace_paths(beams, raynums))
        self.lp, self.path = [], []
        for b, i in zip(beams, raynums):
            live, lp = oracle.launch_point(self.cfg, self.bt, int(b), int(i))
            assert live
            self.lp.append(lp)
            self.path.append(oracle.ray_path(self.cfg, self.bt, r, ne0 if ne is None else ne, te, int(b), int(i)))


@pytest.fixture(scope="module")
def ragged(api, oracle, inputs, torch_cuda):
    tr = _entry_tracer(api, inputs, X.RAGGED)
    beams, raynums = tr.ray_items()
    assert len(beams) == 4 * 426
    yield Case(api, oracle, inputs, X.RAGGED, tr, beams, raynums)
    tr.close()


@pytest.fixture(scope="module")
def box_small(api, oracle, inputs, torch_cuda):
    entry = M.BY_NAME["box_small"]
    tr = _entry_tracer(api, inputs, entry)
    beams, raynums = tr.ray_items()
    pick = np.random.default_rng(20261020).choice(len(beams), size=M.SAMPLE, replace=False)
    yield Case(api, oracle, inputs, entry, tr, beams[pick], raynums[pick])
    tr.close()


@pytest.fixture(scope="module")
def ragged_wide(api, inputs, torch_cuda):
    tr = _entry_tracer(api, inputs, X.RAGGED, force_wide_index=1)
    yield tr
    tr.close()


def _first_node(p, lo, d, n):
    """launch_ray_XZ.cu:162-180: the first node within 0.5001 cells of p, 0 when there is none."""
    ok = np.abs(np.arange(n) * d + lo - p) <= 0.5001 * d
    return int(np.argmax(ok)) if ok.any() else 0


def _launch_node(case, k):
    p, d, lp = case.tr.params, case.tr.derived, case.lp[k]
    return (_first_node(lp[0], p.xmin, d.dx, p.nx), _first_node(lp[1], p.ymin, d.dy, p.ny), _first_node(lp[2], p.zmin, d.dz, p.nz))


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(got - want) / np.maximum(np.abs(want), 1e-300)).max()) if got.size else 0.0


def _oracle_status(api, case, k):
    """steps and status of item k as test_gpu_exits._check_against_oracle derives them from the oracle's path."""
    p, d = case.tr.params, case.tr.derived
    path, lp = case.path[k], case.lp[k]
    lo = (p.xmin - (d.dx / 2.0), p.ymin - (d.dy / 2.0), p.zmin - (d.dz / 2.0))
    hi = (p.xmax + (d.dx / 2.0), p.ymax + (d.dy / 2.0), p.zmax + (d.dz / 2.0))
    n = len(path)
    assert n > 0
    x, y, z, uray = path[-1, 0], path[-1, 1], path[-1, 2], path[-1, 7]
    cut = uray <= 0.05 * lp[3]
    out = x < lo[0] or x > hi[0] or y < lo[1] or y > hi[1] or z < lo[2] or z > hi[2]
    status = api.RAY_LAUNCHED | (api.RAY_CUTOFF if cut else 0) | (api.RAY_ESCAPED if out else 0)
    if not (cut or out):
        assert n == d.nt
        status = api.RAY_LAUNCHED | api.RAY_TIMEOUT
    return n, status


# ---- 1. per step against the oracle -----------------------------------------------------------------------------------
def _check_per_step(api, case, label):
    S, T = case.S, case.T
    assert S.shape == (1 + case.tr.derived.nt, len(case.beams)) and T.shape == (len(case.beams),)
    worst = 0.0
    for k in range(len(case.beams)):
        path, lp = case.path[k], case.lp[k]
        n, status = _oracle_status(api, case, k)
        got = (int(T["steps"][k]), int(T["status"][k]), int(T["nsamples"][k]))
        assert got == (n, status, 1 + n), (label, k, got, (n, status, 1 + n))
        s0 = S[0, k]
        assert (int(s0["step"]), s0["absorbed"], s0["gained"]) == (0, 0.0, 0.0), (label, k)
        assert (int(s0["ci"]), int(s0["cj"]), int(s0["ck"])) == _launch_node(case, k), (label, k)
        err = _rel([s0["x"], s0["y"], s0["z"], s0["uray"]], lp)
        s = S[1:n + 1, k]
        assert np.array_equal(s["step"], np.arange(1, n + 1)), (label, k)
        node = np.stack([s["ci"], s["cj"], s["ck"]], axis=1)
        assert np.array_equal(node, path[:, 3:6].astype(np.int64)), (label, k)
        assert not s["gained"].any()
        for name, col in (("x", 0), ("y", 1), ("z", 2), ("uray", 7), ("absorbed", 6)):
            e = _rel(s[name], path[:, col])
            assert e <= TOL, (label, k, name, e)
            err = max(err, e)
        assert err <= TOL, (label, k, err)
        worst = max(worst, err)
        assert not _raw(S[n + 1:, k]).any(), (label, k)         # samples the ray does not have stay as they were
    return worst


def test_per_step_against_oracle_ragged(api, ragged):
    worst = _check_per_step(api, ragged, "20x17x25")
    steps = ragged.T["steps"]
    assert (int(steps.min()), int(steps.max())) == (11, 59)
    print("20x17x25: %d rays, %d samples: worst relative difference to the oracle %.2e" %
          (len(steps), int(ragged.T["nsamples"].sum()), worst))


def test_per_step_against_oracle_box_small(api, box_small):
    case = box_small
    worst = _check_per_step(api, case, "box_small")
    p, d = case.tr.params, case.tr.derived
    lo = np.array([p.xmin - d.dx / 2.0, p.ymin - d.dy / 2.0, p.zmin - d.dz / 2.0])
    hi = np.array([p.xmax + d.dx / 2.0, p.ymax + d.dy / 2.0, p.zmax + d.dz / 2.0])
    lp = np.array(case.lp)[:, :3]
    outside = int(((lp < lo) | (lp > hi)).any(axis=1).sum())
    dd = np.array([d.dx, d.dy, d.dz])
    far = sum(bool((np.abs((path[:, :3] - np.array([p.xmin, p.ymin, p.zmin])) / dd - path[:, 3:6]).max(axis=1) >= M.FAR).any())
              for path in case.path)
    steps = case.T["steps"]
    # the regimes the entry exists for are in the sample: rays launched outside the box, far jumps, the shortest rays
    assert outside > 0.25 * len(steps) and far > 0.25 * len(steps) and int(steps.min()) <= 2 and int(steps.max()) > 60
    print("box_small: %d rays (%d launched outside, %d with far jumps, %d .. %d steps): worst relative difference to the "
          "oracle %.2e" % (len(steps), outside, far, int(steps.min()), int(steps.max()), worst))


# ---- 2. against the exit pass, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("which, gain_name, wide", (
    pytest.param("ragged", None, False, id="ragged"), pytest.param("box_small", None, False, id="box_small"),
    pytest.param("ragged", None, True, id="ragged-wide"), pytest.param("ragged", "mixed", False, id="ragged-mixed"),
    pytest.param("ragged", "mixed", True, id="ragged-mixed-wide")))
def test_end_state_is_the_exit_pass_bit_for_bit(api, request, torch_cuda, which, gain_name, wide):
    """Both kernels call one step function (ray_step): every arm of it -- plain and gain, narrow and wide index -- gives
    the recorder the exit pass's end state.  The gain hook picks phi's form by a vote of the wave's live lanes (gain_phi),
    and the two forms differ in the last bit or two, so under a gain the identity holds between equal wavefronts: those
    cases take the same rays with the launch list's idle entries kept (ray_items(bundles=True): a wavefront of the recorder
    is then a wavefront of the exit pass).  The compacted list regroups the rays, and with the `mixed` grid some rays'
    energies then differ from the exit pass's in those last bits; test_gain_hook_against_oracle holds both to the oracle."""
    case = request.getfixturevalue(which)
    tr = request.getfixturevalue("ragged_wide") if wide else case.tr
    assert tr.params.force_wide_index == int(wide)
    gain, gp = (None, None) if gain_name is None else _gain_args(api, torch_cuda, gain_name)
    beams, raynums, S, T = case.beams, case.raynums, case.S, case.T
    if gain is not None:
        beams, raynums = tr.ray_items(bundles=True)
        live = raynums >= 0
        assert np.array_equal(beams[live], case.beams) and np.array_equal(raynums[live], case.raynums)     # the same rays
    if wide or gain is not None:
        S, T = _host(api, *tr.trace_paths(beams, raynums, gain=gain, gain_params=gp))
    if gain is not None:
        assert not _raw(T[~live]).any() and not _raw(S[:, ~live]).any()         # idle items
        S, T = S[:, live], T[live]
    rec = tr.trace_exits(tr.new_exits(), gain=gain, gain_params=gp).cpu().numpy().copy().view(api.EXIT_DTYPE)[..., 0]
    slot = {int(i): li for li, i in enumerate(tr.ray_ids()) if i >= 0}
    e = rec[case.beams, [slot[int(i)] for i in case.raynums]]
    every = np.arange(len(case.beams))
    last = S[T["nsamples"] - 1, every]
    assert np.all(e["status"] & api.RAY_LAUNCHED)
    for name in ("x", "y", "z", "uray"):
        assert _same(last[name], e[name]), name
    assert np.array_equal(last["step"], e["steps"])
    assert np.array_equal(T["steps"], e["steps"]) and np.array_equal(T["status"], e["status"])
    assert _same(S[0, :]["uray"], e["uray0"])
    if gain is not None:
        # the record's `gained` is the stride-1 samples' summed in step order from sample 0's 0.0 (cumsum: sequential)
        assert np.array_equal(T["nsamples"], 1 + T["steps"]) and not _raw(S["gained"][0]).any()
        assert _same(np.cumsum(S["gained"], axis=0)[T["nsamples"] - 1, every], e["gained"])
        assert np.abs(e["gained"]).max() > 0


# ---- 3. stride and truncation ------------------------------------------------------------------------------------------
def _guarded(torch, nrows, nitems, capacity):
    """Zeroed samples [nrows, nitems, 8] and turns [nitems, 8], each with one more trailing row that holds NAN_PATTERN;
    returns (samples_full, turns_full, out) with out the views trace_paths takes: capacity rows, nitems records."""
    samples = torch.zeros((nrows + 1, nitems, 8), dtype=torch.float64, device="cuda")
    turns = torch.zeros((nitems + 1, 8), dtype=torch.float64, device="cuda")
    samples[nrows].view(torch.int64).fill_(NAN_PATTERN)
    turns[nitems].view(torch.int64).fill_(NAN_PATTERN)
    return samples, turns, (samples[:capacity], turns[:nitems])


def _strided_equals_unit(S1, T1, S, T, stride, capacity):
    """The run (S, T) at `stride` against the stride-1 run (S1, T1) of the same items: written samples are the stride-1
    samples at steps min(stride m, steps), absorbed / gained the sequential sums of the stride-1 values in between."""
    steps = T1["steps"]
    assert np.array_equal(T["steps"], steps) and np.array_equal(T["status"], T1["status"])
    assert np.array_equal(T["nsamples"], 1 + -(-steps // stride))
    for name in ("r2", "x", "y", "z", "uray", "ne", "step"):
        assert _same(T[name], T1[name]), name
    for k in range(len(steps)):
        n = int(steps[k])
        for m in range(min(capacity, int(T["nsamples"][k]))):
            t = min(stride * m, n)
            a, b = S[m, k], S1[t, k]
            for name in ("x", "y", "z", "uray", "ci", "cj", "ck", "step"):
                assert a[name].tobytes() == b[name].tobytes(), (k, m, name)
            lo = stride * (m - 1) + 1
            for name in ("absorbed", "gained"):
                want = np.cumsum(S1[name][lo:t + 1, k])[-1] if m > 0 else 0.0        # cumsum: in step order
                assert a[name] == want, (k, m, name, a[name], want)
        assert not _raw(S[min(capacity, int(T["nsamples"][k])):, k]).any(), k


def test_stride_and_truncation_long_box(api, inputs, torch_cuda):
    torch = torch_cuda
    vac = np.zeros_like(inputs[2])
    tr = _entry_tracer(api, inputs, X.LONG_BOX, ne=vac)
    assert tr.derived.nt == X.LONG_BOX_NT
    beams, raynums = tr.ray_items()
    n = len(beams)
    assert n == 6 * X.LONG_BOX_LIVE
    S1, T1 = _host(api, *tr.trace_paths(beams, raynums))
    assert S1.shape == (97, n)
    yb = np.isin(beams, X.LONG_BOX_Y_BEAMS)
    assert np.all(T1["steps"][yb] == 96) and np.all(T1["steps"][~yb] == 41)
    assert np.all(T1["status"][yb] == (api.RAY_LAUNCHED | api.RAY_TIMEOUT))

    stride, capacity, rows = 8, 10, 14
    full_s, full_t, out = _guarded(torch, rows, n, capacity)
    samples, turns = tr.trace_paths(beams, raynums, stride=stride, capacity=capacity, out=out)
    assert samples.data_ptr() == full_s.data_ptr() and turns.data_ptr() == full_t.data_ptr()
    S, T = _host(api, full_s[:rows], full_t[:n])
    # both truncated and whole rays occur
    assert np.all(T["nsamples"][yb] == 13) and np.all(T["nsamples"][~yb] == 7) and yb.any() and (~yb).any()
    _strided_equals_unit(S1, T1, S, T, stride, capacity)
    assert S[:capacity, yb]["step"].max() == 72 and S[6, ~yb]["step"].min() == 41       # the last sample is the end state
    assert not _raw(S[capacity:, :]).any()                    # rows m >= capacity: still zero, the +-y items' among them
    assert not _raw(S[7:, ~yb]).any()
    # nothing outside the arrays was touched
    assert bool((full_s[rows].view(torch.int64) == NAN_PATTERN).all()) and bool((full_t[n].view(torch.int64) == NAN_PATTERN).all())

    # capacity 0: no sample array at all, the same turn records
    full_s0, full_t0, out0 = _guarded(torch, 1, n, 0)
    none, turns0 = tr.trace_paths(beams, raynums, stride=stride, capacity=0, out=(None, out0[1]))
    assert none is None
    assert torch.equal(turns0, full_t[:n])
    assert bool((full_t0[n].view(torch.int64) == NAN_PATTERN).all())
    # out= of other shapes than new_paths(n, capacity) gives is refused before the launch
    good_s, good_t = tr.new_paths(n, capacity)
    for bad in ((good_s[:-1], good_t), (good_s, good_t[:-1]), (good_s, good_t.float())):
        with pytest.raises(ValueError):
            tr.trace_paths(beams, raynums, stride=stride, capacity=capacity, out=bad)
    tr.close()


def test_stride_sums_in_step_order_ragged(api, ragged):
    """The same relation where something is absorbed: stride 3, and stride 64 (more than any ray's steps: two samples)."""
    for stride in (3, 64):
        S, T = _host(api, *ragged.tr.trace_paths(ragged.beams, ragged.raynums, stride=stride))
        assert S.shape[0] == 1 + -(-ragged.tr.derived.nt // stride)
        _strided_equals_unit(ragged.S, ragged.T, S, T, stride, S.shape[0])
        assert (S["absorbed"][1:] > 0).sum() >= len(ragged.beams)      # every ray absorbs: at stride 64, in its one interval


# ---- 4. closest approach ------------------------------------------------------------------------------------------------
def _check_turns(case, T, center, ne3d, label):
    worst = 0.0
    steps_seen = set()
    for k in range(len(case.beams)):
        path, lp = case.path[k], case.lp[k]
        r2, j = closest_approach(lp, path, center)
        t = T[k]
        assert int(t["step"]) == j, (label, k, int(t["step"]), j)
        pos = lp[:3] if j == 0 else path[j - 1, :3]
        uray = lp[3] if j == 0 else path[j - 1, 7]
        err = max(_rel(t["r2"], r2[j]), _rel([t["x"], t["y"], t["z"]], pos), _rel(t["uray"], uray))
        assert err <= TOL, (label, k, err)
        worst = max(worst, err)
        node = _launch_node(case, k) if j == 0 else tuple(int(c) for c in path[j - 1, 3:6])
        assert t["ne"].tobytes() == ne3d[node].tobytes(), (label, k, node)
        steps_seen.add("launch" if j == 0 else "last" if j == len(path) else "interior")
    return worst, steps_seen


def test_closest_approach_ragged(api, ragged):
    tr = ragged.tr
    ne3d = tr.node_tables()[0]
    assert ne3d.max() > 0
    worst, seen = _check_turns(ragged, ragged.T, (0.0, 0.0, 0.0), ne3d, "origin")
    assert {"interior", "last"} <= seen
    print("closest approach to the origin, %d rays: worst relative difference to the numpy restatement %.2e" %
          (len(ragged.beams), worst))
    offset = (0.013, -0.021, 0.008)
    _, T = _host(api, *tr.trace_paths(ragged.beams, ragged.raynums, capacity=0, center=offset))
    worst, seen = _check_turns(ragged, T, offset, ne3d, "offset")
    assert {"interior", "last"} <= seen
    assert not _same(T["r2"], ragged.T["r2"])
    print("closest approach to %s: worst %.2e" % (offset, worst))
    far = 5.0 * ragged.bt[FAR_CENTRE_BEAM]
    _, T = _host(api, *tr.trace_paths(ragged.beams, ragged.raynums, capacity=0, center=far))
    worst, _ = _check_turns(ragged, T, far, ne3d, "far")
    own = ragged.beams == FAR_CENTRE_BEAM
    assert own.sum() == 426 and not T["step"][own].any()                       # every record of that beam: the launch point
    for name in ("x", "y", "z", "uray"):
        assert _same(T[name][own], ragged.S[0, own][name]), name
    print("closest approach to 5 beam_norm[%d]: worst %.2e" % (FAR_CENTRE_BEAM, worst))


# ---- 5. idle and invalid items --------------------------------------------------------------------------------------------
def test_idle_and_invalid_items(api, oracle, ragged):
    tr = ragged.tr
    nrays, nb = tr.derived.nrays, tr.params.nbeams
    culled = next(i for i in range(nrays) if not oracle.launch_point(ragged.cfg, ragged.bt, 0, i)[0])
    keep = np.arange(0, len(ragged.beams), 14)[:120]           # 120 live rays of all four beams
    assert len(keep) == 120 and len(set(ragged.beams[keep].tolist())) == 4
    a_live = int(ragged.raynums[0])
    invalid = [(0, culled), (1, -1), (2, nrays), (-1, a_live), (nb, a_live), (0, -2 ** 31), (2 ** 31 - 1, a_live),
               (3, 2 ** 31 - 1), (-2 ** 31, -2 ** 31), (nb, nrays)]
    where = [0, 5, 62, 63, 64, 65, 100, 127, 128, 129]          # ends of the list, both sides of a wave's edge
    n = len(keep) + len(invalid)
    assert n == 130 and n % 64 != 0
    beams, raynums = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    is_bad = np.zeros(n, dtype=bool)
    is_bad[where] = True
    beams[is_bad], raynums[is_bad] = np.array(invalid, dtype=np.int64).T.astype(np.int32)
    beams[~is_bad], raynums[~is_bad] = ragged.beams[keep], ragged.raynums[keep]

    S, T = _host(api, *tr.trace_paths(beams, raynums))
    assert not _raw(T[is_bad]).any() and not _raw(S[:, is_bad]).any()       # all-zero turn records, no sample written
    assert np.all(T["status"][~is_bad] & api.RAY_LAUNCHED)
    # the live items: their values from a list without the invalid ones, and from the whole fan's run
    Sl, Tl = _host(api, *tr.trace_paths(ragged.beams[keep], ragged.raynums[keep]))
    assert _same(T[~is_bad], Tl) and _same(S[:, ~is_bad], Sl)
    assert _same(Tl, ragged.T[keep]) and _same(Sl, ragged.S[:, keep])
    again = _host(api, *tr.trace_paths(beams, raynums))
    assert _same(again[0], S) and _same(again[1], T)
    # an empty list is legal
    s0, t0 = tr.trace_paths([], [])
    assert s0.shape[1] == 0 and t0.shape[0] == 0


# ---- 6. gain hook ---------------------------------------------------------------------------------------------------------
def _gain_args(api, torch, name):
    return torch.from_numpy(X.gain_field(name)).cuda(), api.default_gain_params(max_exponent=X.GAIN_MAX_EXPONENT[name])


@pytest.mark.parametrize("name", X.GAIN_FIELDS)
def test_gain_hook_against_oracle(api, oracle, inputs, ragged, torch_cuda, name):
    tr = ragged.tr
    gain, gp = _gain_args(api, torch_cuda, name)
    S, T = _host(api, *tr.trace_paths(ragged.beams, ragged.raynums, gain=gain, gain_params=gp))
    ids_o, orec = X.oracle_exits(oracle, X.RAGGED, inputs, gain=X.gain_field(name), gain_cfg=X.oracle_gain_config(oracle, name))
    col = {int(i): j for j, i in enumerate(ids_o)}
    f = oracle.EXIT_FIELDS.index
    worst_u = worst_g = worst_b = 0.0
    for k in range(len(ragged.beams)):
        o = orec[int(ragged.beams[k]), col[int(ragged.raynums[k])]]
        n = int(T["steps"][k])
        assert (n, int(T["status"][k])) == (int(o[f("steps")]), int(o[f("status")])), (name, k)
        assert int(T["nsamples"][k]) == n + 1
        s = S[:n + 1, k]
        uray0, last = float(s["uray"][0]), float(s["uray"][n])
        assert _rel(uray0, o[f("uray0")]) <= TOL
        gained, absorbed = [float(v) for v in s["gained"]], [float(v) for v in s["absorbed"]]
        eu, eg = abs(last - o[f("uray")]) / uray0, abs(math.fsum(gained) - o[f("gained")]) / uray0
        assert eu <= GAIN_TOL and eg <= GAIN_TOL, (name, k, eu, eg)
        # the ray's own balance: four roundings per step -- the gain add, the absorption product, its subtraction, the
        # interval sum
        residual = abs(math.fsum([uray0] + gained + [-v for v in absorbed] + [-last]))
        bound = 4 * (n + 1) * X.EPS * math.fsum([uray0] + [abs(v) for v in gained] + absorbed)
        assert residual <= bound, (name, k, residual, bound)
        worst_u, worst_g, worst_b = max(worst_u, eu), max(worst_g, eg), max(worst_b, residual / bound)
    assert np.abs(S["gained"]).max() > 0
    print("20x17x25 %s: %d rays; worst uray %.2e, sum of gained %.2e (of uray0); balance residual %.3f of its bound" %
          (name, len(ragged.beams), worst_u, worst_g, worst_b))
    # gain never steers a ray: positions and nodes equal the no-gain run's at every common step
    common = np.minimum(T["steps"], ragged.T["steps"])
    mask = np.arange(S.shape[0])[:, None] <= common[None, :]
    for fld in ("x", "y", "z", "ci", "cj", "ck", "step"):
        assert _same(S[fld][mask], ragged.S[fld][mask]), (name, fld)
    if name != "small":
        assert (T["steps"] != ragged.T["steps"]).any()        # ... while the energy, and with it a ray's end, does change


def test_gain_of_zeros_is_the_plain_run(api, ragged, torch_cuda):
    tr = ragged.tr
    zeros = torch_cuda.zeros((tr.params.nbeams,) + tr.grid_shape, dtype=torch_cuda.float64, device="cuda")
    S, T = _host(api, *tr.trace_paths(ragged.beams, ragged.raynums, gain=zeros, gain_params=api.default_gain_params()))
    assert not S["gained"].any()
    assert _same(S, ragged.S) and _same(T, ragged.T)           # x = 0 makes the hook the identity


def test_gain_sums_in_step_order(api, ragged, torch_cuda):
    gain, gp = _gain_args(api, torch_cuda, "mixed")
    tr = ragged.tr
    S1, T1 = _host(api, *tr.trace_paths(ragged.beams, ragged.raynums, gain=gain, gain_params=gp))
    S, T = _host(api, *tr.trace_paths(ragged.beams, ragged.raynums, stride=4, gain=gain, gain_params=gp))
    _strided_equals_unit(S1, T1, S, T, 4, S.shape[0])
    assert (S["gained"][1:] != 0).sum() > len(ragged.beams)


# ---- 7. wide index ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", (None, "mixed"))
def test_wide_index_equals_narrow(api, ragged, ragged_wide, torch_cuda, name):
    gain, gp = (None, None) if name is None else _gain_args(api, torch_cuda, name)
    assert ragged_wide.params.force_wide_index == 1 and ragged.tr.params.force_wide_index == 0
    a = ragged.tr.trace_paths(ragged.beams, ragged.raynums, gain=gain, gain_params=gp)
    b = ragged_wide.trace_paths(ragged.beams, ragged.raynums, gain=gain, gain_params=gp)
    assert torch_cuda.equal(a[0], b[0]) and torch_cuda.equal(a[1], b[1])
    S, T = _host(api, *b)
    assert (T["status"] & api.RAY_LAUNCHED).all() and len(T) == 4 * 426
    if name is None:
        assert _same(S, ragged.S) and _same(T, ragged.T)
    else:
        assert np.abs(S["gained"]).max() > 0.0
