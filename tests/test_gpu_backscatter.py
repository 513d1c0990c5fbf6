"""Backscatter SBS gain spectra along rays on the GPU (include/cbet_mi355x.h cbet_trace_backscatter, csrc/cbet_backscatter.hip,
DESIGN.md section 24): the device spectra and records against the host twin bit for bit -- the twin fed the device path
recorder's own stride-1 samples of the same items -- for every NS arm and every flow / state combination; the end state
against the exit pass; idle and invalid items and guard rows; list order; the per-beam tally; and one case through a
bounds-audited build.  Shapes and scans: helpers/backscatter_cases.py; the twin itself is held to a numpy restatement and to
the model's exact properties in test_backscatter_host.py."""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import ROOT
from helpers import backscatter_cases as B
from helpers import exit_cases as X
from helpers.lpi_cases import any_order_bound

pytestmark = pytest.mark.gpu

NAN_PATTERN = 0x7FF8DEADBEEF0001      # a quiet NaN with a payload: the guard rows around the arrays


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


def _raw(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def _records(api, rays):
    return rays.cpu().numpy().copy().view(api.SBS_DTYPE)[..., 0]


class World:
    """A tracer with filled tables, its whole item list, the device recorder's stride-1 samples of it (the twin's input),
    the host node table and the synthetic fields on both sides."""

    def __init__(self, api, torch, inputs, entry, **extra):
        from cbet_raytracing_3d_amd.tracer import RayTracer
        bn, r, ne, te = inputs
        self.entry = entry
        self.tr = RayTracer(entry.params(api, **extra), r, ne, te, beam_norm=entry.beam_table(bn))
        self.tr.tabulate()
        self.p = self.tr.params
        self.beams, self.raynums = self.tr.ray_items()
        samples, turns = self.tr.trace_paths(self.beams, self.raynums, tabulate=False)
        self.S = samples.cpu().numpy().copy().view(api.PATH_DTYPE)[..., 0]
        self.T = turns.cpu().numpy().copy().view(api.TURN_DTYPE)[..., 0]
        self.ne3d = self.tr.node_tables()[0]
        self.fields = B.synthetic_fields(entry)
        self.d_fields = torch.from_numpy(self.fields).cuda()
        self.tables = {}

    def select(self, api, torch, flow, state, pol):
        """The context's flow table, state table and polarization mode; returns the host tables for the twin."""
        gp = api.default_gain_params()
        if "flow" not in self.tables:
            f, s = B.flow_table(self.p), B.state_table(api, self.p, gp)
            self.tables = dict(flow=f, state=s, d_flow=torch.from_numpy(f).cuda(), d_state=torch.from_numpy(s).cuda())
        self.tr.set_flow(self.tables["d_flow"] if flow == "table" else None)
        self.tr.set_gain_state(self.tables["d_state"] if state == "table" else None)
        self.tr.set_polarization(pol)
        return (self.tables["flow"] if flow == "table" else None), (self.tables["state"] if state == "table" else None)

    def reset(self):
        self.tr.set_flow(None)
        self.tr.set_gain_state(None)
        self.tr.set_polarization("aligned")


@pytest.fixture(scope="module")
def ragged(api, torch_cuda, inputs):
    w = World(api, torch_cuda, inputs, X.RAGGED)
    assert len(w.beams) == 4 * 426 and len(w.beams) % 64 != 0
    yield w
    w.tr.close()


@pytest.fixture(scope="module")
def long_box(api, torch_cuda, inputs):
    w = World(api, torch_cuda, inputs, X.LONG_BOX)
    assert len(w.beams) == 6 * X.LONG_BOX_LIVE
    yield w
    w.tr.close()


@pytest.fixture(scope="module")
def ragged_wide(api, torch_cuda, inputs):
    w = World(api, torch_cuda, inputs, X.RAGGED, force_wide_index=1)
    yield w
    w.tr.close()


# ---- 1. device against twin, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("which, nshift, flow, state, pol", (
    ("ragged", 1, "closed", "scalar", "aligned"), ("ragged", 5, "table", "table", "smoothed"),
    ("ragged", 8, "table", "scalar", "aligned"), ("ragged", 16, "closed", "table", "smoothed"),
    ("ragged", 16, "closed", "scalar", "aligned"), ("ragged", 4, "table", "table", "aligned"),
    ("long_box", 5, "table", "table", "smoothed"), ("long_box", 16, "closed", "scalar", "aligned")))
def test_device_equals_twin_bit_for_bit(api, request, torch_cuda, which, nshift, flow, state, pol):
    """nshift 1 and 4 run the NS = 4 instantiation (one slot and all of them), 5 and 8 the NS = 8 one (partially and wholly
    filled), 16 the NS = 16 one; the four flow / state combinations are the four arms of cell_state's run-time selection."""
    w = request.getfixturevalue(which)
    gp = api.default_gain_params()
    shifts = B.SCANS[nshift] if nshift in B.SCANS else B.SCANS[5][:nshift]
    assert len(shifts) == nshift
    try:
        ft, st = w.select(api, torch_cuda, flow, state, pol)
        res = w.tr.backscatter_gain(w.d_fields, gp, domega=shifts, beams=w.beams, raynums=w.raynums)
        gamma, rays = res["gamma"].cpu().numpy(), _records(api, res["rays"])
    finally:
        w.reset()
    want_gamma, want_rays = api.backscatter_host(w.S, w.T, w.beams, w.fields, w.ne3d, shifts, w.p, gp, flow=ft, state=st, polarization=pol)
    assert gamma.shape == (nshift, len(w.beams)) and np.isfinite(gamma).all() and np.abs(gamma).max() > 0
    assert _raw(gamma) == _raw(want_gamma), float(np.abs(gamma - want_gamma).max())
    assert _raw(rays) == _raw(want_rays)
    assert np.array_equal(res["shifts"], np.asarray(shifts))
    print("%s nshift %d, flow %s, state %s, %s: %d rays, max |Gamma| %.3e: device == twin" %
          (which, nshift, flow, state, pol, len(w.beams), float(np.abs(gamma).max())))


def test_wavelength_scan_is_the_detuning_conversion(api, ragged):
    gp, dl = api.default_gain_params(), [-2.0, 0.0, 3.0, 6.0]
    a = ragged.tr.backscatter_gain(ragged.d_fields, gp, dlambda_angstrom=dl, beams=ragged.beams[:200], raynums=ragged.raynums[:200])
    domega = api.wavelength_shift_to_domega(ragged.p, np.asarray(dl))
    b = ragged.tr.backscatter_gain(ragged.d_fields, gp, domega=domega, beams=ragged.beams[:200], raynums=ragged.raynums[:200])
    assert np.array_equal(a["shifts"], domega) and _raw(a["gamma"].cpu().numpy()) == _raw(b["gamma"].cpu().numpy())
    with pytest.raises(ValueError):
        ragged.tr.backscatter_gain(ragged.d_fields, gp)
    with pytest.raises(ValueError):
        ragged.tr.backscatter_gain(ragged.d_fields, gp, domega=[0.0] * 17)
    # out=: tensors of the result's own shapes are written into; any other shape is refused before the launch
    gamma, rays = a["gamma"].clone().zero_(), a["rays"].clone().zero_()
    c = ragged.tr.backscatter_gain(ragged.d_fields, gp, domega=domega, beams=ragged.beams[:200], raynums=ragged.raynums[:200],
                                   out=(gamma, rays))
    assert c["gamma"] is gamma and c["rays"] is rays and _raw(gamma.cpu().numpy()) == _raw(b["gamma"].cpu().numpy())
    for bad in ((gamma[:, :199].contiguous(), rays), (gamma, rays[:199]), (gamma.float(), rays)):
        with pytest.raises(ValueError):
            ragged.tr.backscatter_gain(ragged.d_fields, gp, domega=domega, beams=ragged.beams[:200], raynums=ragged.raynums[:200],
                                       out=bad)
    table = ragged.tr.backscatter_tally(a)
    with pytest.raises(ValueError):
        ragged.tr.backscatter_tally(a, out=table[:, :3].contiguous())


# ---- 2. the end state is the exit pass's -----------------------------------------------------------------------------------
@pytest.mark.parametrize("gain_name, wide", ((None, False), ("mixed", False), (None, True), ("mixed", True)))
def test_end_state_is_the_exit_pass(api, request, torch_cuda, ragged, gain_name, wide):
    """steps, status and the energies equal the exit pass's, without and with a gain grid (the GAIN arms), narrow and forced
    wide index.  Under a gain the hook picks phi's form by a vote of the wave's live lanes, so those cases take the launch
    list's idle entries along (ray_items(bundles=True)): a wavefront here is then a wavefront of the exit pass.  Forced wide
    index gives the narrow bytes."""
    w = request.getfixturevalue("ragged_wide") if wide else ragged
    tr, gp, shifts = w.tr, api.default_gain_params(), B.SCANS[5]
    assert tr.params.force_wide_index == int(wide)
    gain = None
    if gain_name is not None:
        gain = torch_cuda.from_numpy(X.gain_field(gain_name)).cuda()
        gp = api.default_gain_params(max_exponent=X.GAIN_MAX_EXPONENT[gain_name])
    beams, raynums = tr.ray_items(bundles=gain is not None)
    res = tr.backscatter_gain(w.d_fields, gp, domega=shifts, beams=beams, raynums=raynums, gain=gain)
    gamma, rays = res["gamma"].cpu().numpy(), _records(api, res["rays"])
    live = raynums >= 0
    assert not np.frombuffer(_raw(rays[~live]), dtype=np.uint8).any() and not gamma[:, ~live].any()
    rec = tr.trace_exits(tr.new_exits(), gain=gain, gain_params=gp, tabulate=False).cpu().numpy().copy().view(api.EXIT_DTYPE)[..., 0]
    slot = {int(i): li for li, i in enumerate(tr.ray_ids()) if i >= 0}
    e = rec[beams[live], [slot[int(i)] for i in raynums[live]]]
    r = rays[live]
    assert np.all(e["status"] & api.RAY_LAUNCHED)
    assert np.array_equal(r["steps"], e["steps"]) and np.array_equal(r["status"], e["status"])
    assert _raw(r["uray0"]) == _raw(e["uray0"]) and _raw(r["uray_end"]) == _raw(e["uray"])
    if gain is not None:
        assert np.abs(e["gained"]).max() > 0 and (r["steps"] != ragged.T["steps"]).any()     # the gain changed some rays' ends
    if wide:
        narrow = ragged.tr.backscatter_gain(ragged.d_fields, gp, domega=shifts, beams=beams, raynums=raynums, gain=gain)
        assert torch_cuda.equal(narrow["gamma"], res["gamma"]) and torch_cuda.equal(narrow["rays"], res["rays"])


# ---- 3. idle and invalid items, guard rows ---------------------------------------------------------------------------------
def test_idle_and_invalid_items_and_guards(api, oracle, inputs, torch_cuda, ragged):
    torch, tr, gp, shifts = torch_cuda, ragged.tr, api.default_gain_params(), B.SCANS[5]
    nrays, nb = tr.derived.nrays, tr.params.nbeams
    cfg, bt = X.RAGGED.config(oracle), X.RAGGED.beam_table(inputs[0])
    culled = next(i for i in range(nrays) if not oracle.launch_point(cfg, bt, 0, i)[0])
    keep = np.arange(0, len(ragged.beams), 14)[:120]           # 120 live rays of all four beams
    a_live = int(ragged.raynums[0])
    invalid = [(0, culled), (1, -1), (2, nrays), (-1, a_live), (nb, a_live), (0, -2 ** 31), (2 ** 31 - 1, a_live),
               (3, 2 ** 31 - 1), (-2 ** 31, -2 ** 31), (nb, nrays)]
    where = [0, 5, 62, 63, 64, 65, 100, 127, 128, 129]          # ends of the list, both sides of a wave's edge
    n = len(keep) + len(invalid)
    assert n == 130 and n % 64 != 0 and len(set(ragged.beams[keep].tolist())) == 4
    beams, raynums = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    is_bad = np.zeros(n, dtype=bool)
    is_bad[where] = True
    beams[is_bad], raynums[is_bad] = np.array(invalid, dtype=np.int64).T.astype(np.int32)
    beams[~is_bad], raynums[~is_bad] = ragged.beams[keep], ragged.raynums[keep]
    # one guard row in front of and behind each array, and the arrays themselves pre-filled with the pattern: every entry
    # must be written (zeros for idle items), nothing outside
    nshift = len(shifts)
    g_full = torch.zeros((nshift + 2, n), dtype=torch.float64, device="cuda")
    r_full = torch.zeros((n + 2, 4), dtype=torch.float64, device="cuda")
    g_full.view(torch.int64).fill_(NAN_PATTERN)
    r_full.view(torch.int64).fill_(NAN_PATTERN)
    res = tr.backscatter_gain(ragged.d_fields, gp, domega=shifts, beams=beams, raynums=raynums, out=(g_full[1:nshift + 1], r_full[1:n + 1]))
    assert res["gamma"].data_ptr() == g_full[1].data_ptr() and res["rays"].data_ptr() == r_full[1].data_ptr()
    for guard in (g_full[0], g_full[nshift + 1], r_full[0], r_full[n + 1]):
        assert bool((guard.view(torch.int64) == NAN_PATTERN).all())
    gamma, rays = res["gamma"].cpu().numpy(), _records(api, res["rays"])
    assert not (np.ascontiguousarray(gamma).view(np.int64) == np.int64(NAN_PATTERN)).any()
    assert not gamma[:, is_bad].any() and not np.frombuffer(_raw(rays[is_bad]), dtype=np.uint8).any()      # zero columns, zero records
    assert np.all(rays["status"][~is_bad] & api.RAY_LAUNCHED) and np.abs(gamma[:, ~is_bad]).max() > 0
    # the live items: their values from a list without the invalid ones, and from the whole list's run
    alone = tr.backscatter_gain(ragged.d_fields, gp, domega=shifts, beams=ragged.beams[keep], raynums=ragged.raynums[keep])
    assert _raw(gamma[:, ~is_bad]) == _raw(alone["gamma"].cpu().numpy()) and _raw(rays[~is_bad]) == _raw(_records(api, alone["rays"]))
    whole = tr.backscatter_gain(ragged.d_fields, gp, domega=shifts, beams=ragged.beams, raynums=ragged.raynums)
    assert _raw(gamma[:, ~is_bad]) == _raw(whole["gamma"].cpu().numpy()[:, keep])
    # an empty list is legal
    empty = tr.backscatter_gain(ragged.d_fields, gp, domega=shifts, beams=[], raynums=[])
    assert tuple(empty["gamma"].shape) == (nshift, 0) and tuple(empty["rays"].shape) == (0, 4)
    # the default list is ray_items()
    default = tr.backscatter_gain(ragged.d_fields, gp, domega=shifts)
    assert torch.equal(default["gamma"], whole["gamma"]) and torch.equal(default["rays"], whole["rays"])


# ---- 4. list order -----------------------------------------------------------------------------------------------------------
def test_whole_list_equals_its_halves(api, torch_cuda, ragged):
    tr, gp, shifts = ragged.tr, api.default_gain_params(), B.SCANS[8]
    n = len(ragged.beams)
    h = n // 2 + 7                                             # neither half is a multiple of 64
    assert h % 64 != 0 and (n - h) % 64 != 0
    whole = tr.backscatter_gain(ragged.d_fields, gp, domega=shifts, beams=ragged.beams, raynums=ragged.raynums)
    a = tr.backscatter_gain(ragged.d_fields, gp, domega=shifts, beams=ragged.beams[:h], raynums=ragged.raynums[:h])
    b = tr.backscatter_gain(ragged.d_fields, gp, domega=shifts, beams=ragged.beams[h:], raynums=ragged.raynums[h:])
    assert torch_cuda.equal(whole["gamma"], torch_cuda.cat([a["gamma"], b["gamma"]], dim=1))
    assert torch_cuda.equal(whole["rays"], torch_cuda.cat([a["rays"], b["rays"]], dim=0))


# ---- 5. the tally --------------------------------------------------------------------------------------------------------------
def test_tally(api, torch_cuda, ragged):
    """Two calls give identical bytes; counts and maxima are exact; the sums are within the order-of-summation bound of a
    long-double sum, and the tally of the two halves merged is within the bound of the whole list's: two sums of the same n
    terms in any two orders are each within (n - 1) 2^-53 sum |terms| of the exact sum, so at most twice that apart
    (helpers/lpi_cases.any_order_bound; the products uray0 * Gamma are rounded once, the same on both sides)."""
    torch, tr, gp, shifts = torch_cuda, ragged.tr, api.default_gain_params(), B.SCANS[8]
    nb, nshift, n = tr.params.nbeams, len(shifts), len(ragged.beams)
    whole = tr.backscatter_gain(ragged.d_fields, gp, domega=shifts, beams=ragged.beams, raynums=ragged.raynums)
    t1, t2 = tr.backscatter_tally(whole), tr.backscatter_tally(whole, ragged.beams)
    assert tuple(t1.shape) == (nb, nshift, 4) and torch.equal(t1, t2)
    gamma, rays, tally = whole["gamma"].cpu().numpy(), _records(api, whole["rays"]), t1.cpu().numpy()
    h = n // 2 + 7
    parts = [tr.backscatter_gain(ragged.d_fields, gp, domega=shifts, beams=ragged.beams[s], raynums=ragged.raynums[s])
             for s in (slice(0, h), slice(h, n))]
    merged = tr.backscatter_tally(parts[1], out=tr.backscatter_tally(parts[0])).cpu().numpy()
    worst = 0.0
    for b in range(nb):
        own = (ragged.beams == b) & ((rays["status"] & api.RAY_LAUNCHED) != 0)
        assert own.sum() == 426
        u = rays["uray0"][own]
        for m in range(nshift):
            terms = u * gamma[m, own]
            for got in (tally[b, m], merged[b, m]):
                assert got[3] == own.sum() and got[2] == gamma[m, own].max()              # exact
                assert abs(np.longdouble(got[0]) - u.astype(np.longdouble).sum()) <= any_order_bound(u) / 2
                assert abs(np.longdouble(got[1]) - terms.astype(np.longdouble).sum()) <= any_order_bound(terms) / 2
            assert abs(tally[b, m, 0] - merged[b, m, 0]) <= any_order_bound(u)
            bound = any_order_bound(terms)
            diff = abs(tally[b, m, 1] - merged[b, m, 1])
            assert diff <= bound
            worst = max(worst, diff / bound if bound > 0 else 0.0)
    print("tally: whole list against merged halves, %d x %d entries: worst difference %.3f of the bound n eps sum |terms|" % (nb, nshift, worst))
    # sum uray0 is the exit tally's `launched` of the same rays, up to the order of the sum
    balance = tr.energy_balance(tr.trace_exits(tr.new_exits(), tabulate=False)).cpu().numpy()
    for b in range(nb):
        u = rays["uray0"][ragged.beams == b]
        assert balance[b, 6] == tally[b, 0, 3] == len(u)
        assert abs(balance[b, 0] - tally[b, 0, 0]) <= any_order_bound(u)
    # items that count nowhere: a beam outside the table, an idle record
    odd = np.concatenate([ragged.beams[:100], [7, -1]]).astype(np.int32)
    res = tr.backscatter_gain(ragged.d_fields, gp, domega=shifts, beams=odd, raynums=np.concatenate([ragged.raynums[:100], [0, 0]]))
    t = tr.backscatter_tally(res).cpu().numpy()
    assert t[:, :, 3].sum() == 100 * nshift
    from cbet_raytracing_3d_amd import lpi
    spec = lpi.backscatter_spectrum(t1)
    assert spec["mean"].shape == (nb, nshift) and spec["rays"].tolist() == [426] * nb
    assert (spec["max"] >= spec["mean"]).all()
    refl = lpi.linear_reflectivity(whole["gamma"], whole["rays"], 1e-9)
    assert 0.0 < refl <= 1.0


# ---- 6. the bounds-audited build -------------------------------------------------------------------------------------------------
WORKER = r'''
import json, os, sys
import numpy as np, torch
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
from conftest import load_inputs
from cbet_raytracing_3d_amd import api
from cbet_raytracing_3d_amd.tracer import RayTracer
from helpers import backscatter_cases as B
from helpers import exit_cases as X
bn, r, ne, te = load_inputs()
entry = X.RAGGED
tr = RayTracer(entry.params(api), r, ne, te, beam_norm=entry.beam_table(bn))
tr.tabulate()
api.debug_bounds_violations(reset=True)
beams, raynums = tr.ray_items()
n = len(beams)
beams = np.concatenate([beams, [0, 9, -1, 2]]).astype(np.int32)          # ... and idle items behind the last whole wave
raynums = np.concatenate([raynums, [-1, 5, 5, tr.derived.nrays]]).astype(np.int32)
fields = torch.from_numpy(B.synthetic_fields(entry)).cuda()
gp = api.default_gain_params()
p = tr.params
tr.set_flow(torch.from_numpy(B.flow_table(p)).cuda())
tr.set_gain_state(torch.from_numpy(B.state_table(api, p, gp)).cuda())
out = []
for nshift in (5, 16):
    for gain in (None, torch.from_numpy(X.gain_field("mixed")).cuda()):
        res = tr.backscatter_gain(fields, gp, domega=B.SCANS[nshift], beams=beams, raynums=raynums, gain=gain)
        tally = tr.backscatter_tally(res)
        torch.cuda.synchronize()
        rays = res["rays"].cpu().numpy().view(api.SBS_DTYPE)[..., 0]
        out.append(dict(nshift=nshift, gain=gain is not None, violations=api.debug_bounds_violations(reset=True),
                        launched=int((rays["status"] != 0).sum()), counted=float(tally[:, 0, 3].sum().item()), items=len(beams),
                        finite=bool(torch.isfinite(res["gamma"]).all().item()), peak=float(res["gamma"].abs().max().item())))
tr.close()
print("RESULT " + json.dumps(out))
'''


def test_bounds_audited_build_reports_no_violation(tmp_path):
    """One case through a -DCBET_DEBUG_BOUNDS build of the library (compiled here, the files in parallel; the library path is
    fixed at import, so the case runs in a child process): every store of the spectra and of the records, the step-record
    and gain-grid gathers of the step; all four tables' arms, both NS = 8 and NS = 16, without and with a gain grid, idle
    items behind the last whole wave.  The build is what takes the time here, as in test_gpu_bounds_audit.py."""
    csrc = os.path.join(ROOT, "cbet_raytracing_3d_amd", "csrc")
    lib = str(tmp_path / "libcbet_audit.so")
    srcs = sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".cpp")))
    flags = ["hipcc", "-O1", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fPIC", "-DCBET_DEBUG_BOUNDS",
             "-I", os.path.join(ROOT, "include"), "-I", csrc]

    def compile_one(f):
        obj = str(tmp_path / (f + ".o"))
        subprocess.check_call(flags + ["-x", "hip", "-c", os.path.join(csrc, f), "-o", obj])
        return obj

    with ThreadPoolExecutor(8) as pool:
        objs = list(pool.map(compile_one, srcs))
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs + ["-lrccl"])
    env = dict(os.environ, CBET_LIB_PATH=lib)
    run = subprocess.run([sys.executable, "-c", WORKER % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    results = json.loads([l for l in run.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    assert len(results) == 4
    for res in results:
        print(res)
        assert res["violations"] == 0, res
        assert res["launched"] == 4 * 426 == res["counted"] and res["items"] == 4 * 426 + 4, res
        assert res["finite"] and res["peak"] > 0, res
