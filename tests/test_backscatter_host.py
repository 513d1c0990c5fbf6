"""Backscatter SBS gain spectra along rays, host side (no GPU; include/cbet_mi355x.h cbet_trace_backscatter, DESIGN.md section
24): the entry points exported, the record's layout in the header, the ctypes mirror and the numpy dtype; every bad argument
refused before the context is looked at; the host twin (cbet_backscatter_host) on the CPU oracle's ray paths against a numpy
restatement of the model (helpers/backscatter_cases.py) and against the model's exact properties; and the gfx950 listing of
cbet_backscatter.hip, cross-compiled here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from helpers import backscatter_cases as B
from helpers import exit_cases as X

CSRC = os.path.join(ROOT, "cbet_raytracing_3d_amd", "csrc")
TWIN_TOL = 1e-12           # of max |Gamma|: the bound section 23 holds its twin to against its numpy restatement


@pytest.fixture(scope="module")
def api():
    from cbet_raytracing_3d_amd import api as a
    a.lib()
    return a


@pytest.fixture(scope="module", params=["ragged", "long_box"])
def world(request, api, oracle, inputs):
    return B.oracle_world(api, oracle, inputs, X.RAGGED if request.param == "ragged" else X.LONG_BOX)


@pytest.fixture(scope="module")
def ragged(api, oracle, inputs):
    return B.oracle_world(api, oracle, inputs, X.RAGGED)


def _raw(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


# ---- exports and layout ----------------------------------------------------------------------------------------------
def test_entry_points_exported(api):
    for name in ("backscatter_gain", "backscatter_tally"):
        from cbet_raytracing_3d_amd.tracer import RayTracer
        assert callable(getattr(RayTracer, name))
    from cbet_raytracing_3d_amd import lpi
    assert callable(lpi.backscatter_spectrum) and callable(lpi.linear_reflectivity)


def test_struct_layout_matches_header(api, tmp_path):
    names = [f for f, _ in api.RaySbs._fields_]
    assert names == ["gmax", "uray0", "uray_end", "steps", "imax", "status"]
    lines = ['#include <stdio.h>', '#include "cbet_mi355x.h"', 'int main(void){', 'printf("max %d\\n", CBET_SBS_MAX_SHIFTS);',
             'printf("columns %d\\n", CBET_SBS_TALLY_COLUMNS);', 'return 0;}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "probe")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = {k: int(v) for k, v in (l.split() for l in subprocess.check_output([exe], text=True).splitlines())}
    assert C.sizeof(api.RaySbs) == api.SBS_DTYPE.itemsize == 32
    assert got["max"] == api.SBS_MAX_SHIFTS == 16 and got["columns"] == len(api.SBS_TALLY_COLUMNS) == 4
    # a [.., 4] float64 row viewed as the dtype: the integers sit in column 3
    row = np.zeros(4)
    row.view(np.int32)[6] = 77
    row.view(np.int16)[14:16] = (5, 3)
    rec = row.view(api.SBS_DTYPE)[0]
    assert (int(rec["steps"]), int(rec["imax"]), int(rec["status"])) == (77, 5, 3)


# ---- argument checks -------------------------------------------------------------------------------------------------
def _trace(api, p, g, ctx=None, **kw):
    """cbet_trace_backscatter with never-dereferenced pointers (the checks fail first) and the keyword overrides."""
    fake = C.c_void_p(4096)
    shifts = (C.c_double * 16)(*([0.0] * 16))
    a = dict(gain=None, beams=fake, raynums=fake, nitems=130, fields=fake, shifts=shifts, nshift=5, gamma=fake, rays=fake)
    a.update(kw)
    rc = api.lib().cbet_trace_backscatter(None, None, a["gain"], a["beams"], a["raynums"], a["nitems"], a["fields"], a["shifts"],
                                          a["nshift"], a["gamma"], a["rays"], None, fake, fake, fake, 1.0, 1.0, 1.0,
                                          C.byref(p) if p is not None else None, C.byref(g) if g is not None else None, ctx, None)
    return rc, api.lib().cbet_last_error().decode()


def test_argument_checks_without_a_gpu(api):
    """Every refusal below happens with a NULL context and before any HIP call (no device on this host); each message names
    its offence."""
    p, g = api.default_params(32, nbeams=4), api.default_gain_params()
    bad = lambda v: (C.c_double * 16)(*([0.0, v] + [0.0] * 14))                          # noqa: E731
    cases = [
        (dict(nshift=0), "nshift"), (dict(nshift=-1), "nshift"), (dict(nshift=17), "nshift"),
        (dict(shifts=None), "shifts"), (dict(shifts=bad(float("nan"))), "finite"), (dict(shifts=bad(float("inf"))), "finite"),
        (dict(fields=None), "fields"),
        (dict(nitems=-1), "nitems"), (dict(nitems=2 ** 62), "overflow"), (dict(nitems=2 ** 40), "one launch"),
        (dict(rays=None), "ray-record"), (dict(gamma=None), "gamma"),
        (dict(beams=None), "beams"), (dict(raynums=None), "raynums"),
    ]
    for kw, word in cases:
        rc, msg = _trace(api, p, g, **kw)
        assert rc == api.EINVAL and word in msg, (kw, rc, msg)
    # the FIRST offence is named: a bad nshift before a NULL fields, a non-finite shift before NULL fields
    rc, msg = _trace(api, p, g, nshift=17, fields=None)
    assert rc == api.EINVAL and "nshift" in msg
    rc, msg = _trace(api, p, g, shifts=bad(float("nan")), fields=None)
    assert rc == api.EINVAL and "finite" in msg
    # a non-finite entry behind nshift is not read
    rc, msg = _trace(api, p, g, shifts=bad(float("nan")), nshift=1)
    assert rc == api.EINVAL and "context" in msg, msg
    rc, msg = _trace(api, p, None)
    assert rc == api.EINVAL and "gain params" in msg, msg
    rc, msg = _trace(api, p.copy(absorption=0), g)
    assert rc == api.EINVAL and "absorbing" in msg, msg
    rc, msg = _trace(api, p, api.default_gain_params(max_exponent=2.0), gain=C.c_void_p(4096))
    assert rc == api.EINVAL, msg
    rc, msg = _trace(api, None, g)
    assert rc == api.EINVAL
    # what is legal reaches the context check
    for kw in (dict(), dict(nshift=1), dict(nshift=16), dict(beams=None, raynums=None, nitems=0), dict(gain=C.c_void_p(4096))):
        rc, msg = _trace(api, p, g, **kw)
        assert rc == api.EINVAL and "context" in msg, (kw, msg)


def test_tally_and_twin_argument_checks(api):
    L, fake = api.lib(), C.c_void_p(4096)
    assert api.backscatter_work_bytes(1000, 5, 4) == 1 * 5 * 4 * 32            # one chunk of the list
    assert api.backscatter_work_bytes(4097, 16, 60) == 2 * 16 * 60 * 32
    assert api.backscatter_work_bytes(0, 1, 1) == 0
    for bad in ((-1, 5, 4), (10, 0, 4), (10, 17, 4), (10, 5, 0), (10, 5, 65)):
        assert api.backscatter_work_bytes(*bad) == 0, bad
    for args, word in (((fake, fake, fake, 10, 0, 4, fake, fake, None), "nshift"), ((fake, fake, fake, 10, 17, 4, fake, fake, None), "nshift"),
                       ((fake, fake, fake, 10, 5, 0, fake, fake, None), "nbeams"), ((fake, fake, fake, 10, 5, 65, fake, fake, None), "nbeams"),
                       ((fake, fake, fake, -1, 5, 4, fake, fake, None), "nitems"), ((fake, fake, fake, 10, 5, 4, None, fake, None), "tally"),
                       ((None, fake, fake, 10, 5, 4, fake, fake, None), "gamma"), ((fake, fake, fake, 10, 5, 4, fake, None, None), "work")):
        rc = L.cbet_backscatter_tally(*args)
        assert rc == api.EINVAL and word in L.cbet_last_error().decode(), (args, L.cbet_last_error())
    assert L.cbet_backscatter_tally(fake, fake, fake, 0, 5, 4, fake, None, None) == api.OK      # an empty list adds nothing
    # the twin: the shared refusals, and its own
    p, g = api.default_params(8, nbeams=2), api.default_gain_params()
    grid = (p.nx + 2, p.ny + 2, p.nz + 2)
    S, T = np.zeros((2, 1), dtype=api.PATH_DTYPE), np.zeros(1, dtype=api.TURN_DTYPE)
    S["x"][1, 0] = 1e-3
    T["status"], T["steps"], T["nsamples"] = 1, 1, 2
    fields, ne3d = np.ones((4, 2) + grid), np.zeros((8, 8, 8))
    good = dict(samples=S, turns=T, beams=[0], fields=fields, ne3d=ne3d, shifts=[0.0], params=p, gain_params=g)
    gamma, rays = api.backscatter_host(**good)
    assert gamma.shape == (1, 1) and int(rays["status"][0]) == 1 and int(rays["steps"][0]) == 1
    for kw, word in ((dict(shifts=[0.0] * 17), "nshift"), (dict(shifts=[float("nan")]), "finite"), (dict(gain_params=None), "gain params"),
                     (dict(beams=[2]), "beam"), (dict(beams=[-1]), "beam"), (dict(polarization=7), "polarization")):
        with pytest.raises(api.CbetError, match=word):
            api.backscatter_host(**dict(good, **kw))
    T2 = T.copy()
    T2["nsamples"] = 3                                        # more samples than the array holds
    with pytest.raises(api.CbetError, match="nsamples"):
        api.backscatter_host(**dict(good, turns=T2))
    S2 = S.copy()
    S2["ci"][1, 0] = 8                                        # a node outside the grid is refused, not gathered
    with pytest.raises(api.CbetError, match="outside the grid"):
        api.backscatter_host(**dict(good, samples=S2))
    with pytest.raises(ValueError):
        api.sbs_shifts([])
    with pytest.raises(ValueError):
        api.sbs_shifts([0.0, float("inf")])


# ---- the twin against numpy ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flow, state, pol", (("closed", "scalar", "aligned"), ("table", "table", "smoothed"),
                                              ("table", "scalar", "aligned"), ("closed", "table", "smoothed")))
def test_twin_against_numpy(api, world, flow, state, pol):
    w, p = world, world["p"]
    gp = api.default_gain_params()
    ft = B.flow_table(p) if flow == "table" else None
    st = B.state_table(api, p, gp) if state == "table" else None
    shifts = B.SCANS[16]
    gamma, rays = api.backscatter_host(w["S"], w["T"], w["beams"], w["fields"], w["ne3d"], shifts, p, gp, flow=ft, state=st,
                                       polarization=pol)
    want = B.sbs_reference(api, p, gp, w["S"], w["T"], w["beams"], w["fields"], w["ne3d"], shifts, flow=ft, state=st,
                           smoothed=pol == "smoothed")
    scale = float(np.abs(want).max())
    assert scale > 0 and np.isfinite(want).all() and int((np.abs(want) > 1e-3 * scale).sum()) > 0.2 * want.size
    err = float(np.abs(gamma - want).max() / scale)
    print("%s, flow %s, state %s, %s: %d rays x %d shifts, max |Gamma| %.3e, twin against numpy %.2e of it" %
          (w["entry"].name, flow, state, pol, gamma.shape[1], gamma.shape[0], scale, err))
    assert err <= TWIN_TOL
    # the records: the first maximum, and the paths' own end state
    assert np.array_equal(rays["imax"], np.argmax(gamma, axis=0)) and _raw(rays["gmax"]) == _raw(gamma.max(axis=0))
    assert np.array_equal(rays["steps"], w["T"]["steps"]) and np.array_equal(rays["status"], w["T"]["status"])
    every = np.arange(len(w["beams"]))
    assert _raw(rays["uray0"]) == _raw(w["S"]["uray"][0]) and _raw(rays["uray_end"]) == _raw(w["S"]["uray"][w["T"]["steps"], every])


# ---- exact properties of the twin ------------------------------------------------------------------------------------
def _twin(api, w, gp, shifts, **kw):
    kw.setdefault("fields", w["fields"])
    kw.setdefault("ne3d", w["ne3d"])
    return api.backscatter_host(w["S"], w["T"], w["beams"], kw.pop("fields"), kw.pop("ne3d"), shifts, w["p"], gp, **kw)[0]


def test_still_plasma_is_odd_in_the_shift_and_zero_at_zero(api, world):
    still = api.default_gain_params(mach_0=0.0, mach_1=0.0)
    scan = [s for s in B.SCANS[8] if s != 0.0][:7]
    gamma = _twin(api, world, still, [0.0] + scan)
    assert not gamma[0].any()                                 # delta = 0: exactly zero for every ray
    assert np.abs(gamma[1:]).max() > 0
    mirrored = _twin(api, world, still, [0.0] + [-s for s in scan])
    assert np.array_equal(mirrored, -gamma)                   # equal values: the same bits wherever Gamma != 0
    nz = gamma != 0
    assert nz.sum() > 0.5 * gamma[1:].size and _raw(mirrored[nz]) == _raw(-gamma[nz])
    # ... and with the flow on the spectrum is not odd: the Doppler term shifts the resonance
    moving = api.default_gain_params()
    assert (moving.mach_0, moving.mach_1) != (0.0, 0.0)
    assert not np.array_equal(_twin(api, world, moving, [-s for s in scan]), -_twin(api, world, moving, scan))


def test_fields_doubled_and_smoothing_halved_bit_for_bit(api, world):
    gp, shifts = api.default_gain_params(), B.SCANS[5]
    gamma = _twin(api, world, gp, shifts)
    assert _raw(_twin(api, world, gp, shifts, fields=2.0 * world["fields"])) == _raw(2.0 * gamma)
    assert _raw(_twin(api, world, gp, shifts, polarization="smoothed")) == _raw(0.5 * gamma)
    assert np.abs(gamma[gamma != 0]).min() > 1e-280          # far from underflow: doubling and halving are exact


def _single_steps(api, w, k):
    """Item k's steps as items of their own: two-sample records (p_(t-1), p_t) for t = 1 .. steps."""
    n = int(w["T"]["steps"][k])
    S = np.zeros((2, n), dtype=api.PATH_DTYPE)
    S[0], S[1] = w["S"][:n, k], w["S"][1:n + 1, k]
    T = np.zeros(n, dtype=api.TURN_DTYPE)
    T["status"], T["steps"], T["nsamples"] = 1, 1, 2
    return S, T, np.full(n, w["beams"][k], dtype=np.int32)


def test_gamma_is_the_sum_of_its_steps_in_step_order(api, ragged):
    w, gp, shifts = ragged, api.default_gain_params(), B.SCANS[8]
    whole = _twin(api, w, gp, shifts)
    for k in (0, 431, 1000, len(w["beams"]) - 1):             # rays of different beams and lengths
        S, T, b = _single_steps(api, w, k)
        steps = api.backscatter_host(S, T, b, w["fields"], w["ne3d"], shifts, w["p"], gp)[0]
        for m in range(len(shifts)):
            acc = 0.0
            for t in range(steps.shape[1]):
                acc = acc + steps[m, t]
            assert acc == whole[m, k] and np.float64(acc).tobytes() == whole[m, k].tobytes(), (k, m)
        assert (steps != 0).any()


def test_cells_at_and_above_critical_contribute_exactly_nothing(api, ragged):
    w, gp, shifts = ragged, api.default_gain_params(), B.SCANS[8]
    for k in range(431, len(w["beams"])):                      # the first ray from there on with nine steps that add something
        S, T, b = _single_steps(api, w, k)
        before = api.backscatter_host(S, T, b, w["fields"], w["ne3d"], shifts, w["p"], gp)[0]
        live = np.flatnonzero((before != 0).any(axis=0))
        if len(live) >= 9:
            break
    assert len(live) >= 9
    n = int(w["T"]["steps"][k])
    node = tuple(w["S"][c][1:n + 1, k] for c in ("ci", "cj", "ck"))
    ne3d = w["ne3d"].copy()
    at, above = live[1:len(live):3], live[2:len(live):3]      # some of the ray's steps: exactly critical, and 1.5 critical
    ne3d[node[0][at], node[1][at], node[2][at]] = w["d"].ncrit
    ne3d[node[0][above], node[1][above], node[2][above]] = 1.5 * w["d"].ncrit
    hit = np.array([(ne3d[node[0][t], node[1][t], node[2][t]] >= w["d"].ncrit) for t in range(n)])
    assert hit[at].all() and hit[above].all() and not hit.all()
    after = api.backscatter_host(S, T, b, w["fields"], ne3d, shifts, w["p"], gp)[0]
    assert not after[:, hit].any()                            # exactly nothing, at every shift
    assert _raw(after[:, ~hit]) == _raw(before[:, ~hit])      # the other steps keep their bits
    whole = api.backscatter_host(w["S"][:, k:k + 1], w["T"][k:k + 1], w["beams"][k:k + 1], w["fields"], ne3d, shifts, w["p"], gp)[0]
    for m in range(len(shifts)):
        acc = 0.0
        for t in np.flatnonzero(~hit):
            acc = acc + after[m, t]
        assert np.float64(acc).tobytes() == whole[m, 0].tobytes(), m


def test_idle_items_and_zero_length_steps(api, ragged):
    w, gp, shifts = ragged, api.default_gain_params(), B.SCANS[5]
    keep = np.arange(0, 40)
    S, T, b = w["S"][:, keep].copy(), w["T"][keep].copy(), w["beams"][keep].copy()
    T[[3, 17]] = np.zeros((), dtype=api.TURN_DTYPE)           # idle items: all-zero turn records
    b[3] = -5                                                 # ... whose beam may be anything
    S["x"][5:, 8], S["y"][5:, 8], S["z"][5:, 8] = S["x"][4, 8], S["y"][4, 8], S["z"][4, 8]      # a ray that stops moving
    gamma, rays = api.backscatter_host(S, T, b, w["fields"], w["ne3d"], shifts, w["p"], gp)
    assert not gamma[:, [3, 17]].any() and not np.frombuffer(_raw(rays[[3, 17]]), dtype=np.uint8).any()
    first4 = api.backscatter_host(S[:5, 8:9], np.array([(0, 0, 0, 0, 0, 0, 0, 4, 1, 5)], dtype=api.TURN_DTYPE), b[8:9], w["fields"],
                                  w["ne3d"], shifts, w["p"], gp)[0]
    assert _raw(gamma[:, 8]) == _raw(first4[:, 0]) and np.isfinite(gamma).all()      # ds == 0.0 steps add nothing


# ---- Python layer (no device) ----------------------------------------------------------------------------------------
def test_spectrum_and_reflectivity_helpers(api):
    from cbet_raytracing_3d_amd import lpi
    tally = np.zeros((2, 3, 4))
    tally[0, :, 0], tally[0, :, 1], tally[0, :, 2], tally[0, :, 3] = 10.0, (5.0, 20.0, -10.0), (1.0, 4.0, 0.5), 7
    spec = lpi.backscatter_spectrum(tally)
    assert np.array_equal(spec["mean"][0], [0.5, 2.0, -1.0]) and np.array_equal(spec["max"][0], [1.0, 4.0, 0.5])
    assert not spec["mean"][1].any() and spec["rays"].tolist() == [7, 0]                  # a beam without rays: zeros, no 0 / 0
    assert spec["peak"].tolist() == [1, 0]
    gamma = np.array([[0.0, 2.0, 50.0], [1.0, 1.0, 0.0]])
    rays = np.zeros(3, dtype=api.SBS_DTYPE)
    rays["uray0"], rays["status"] = (1.0, 2.0, 4.0), (1, 1, 0)                            # the third item is idle
    seed = 1e-3
    want = (1.0 * min(1.0, seed * np.exp(1.0)) + 2.0 * min(1.0, seed * np.exp(2.0))) / 3.0
    assert lpi.linear_reflectivity(gamma, rays, seed) == pytest.approx(want, rel=1e-15)
    rays["status"][2] = 1
    want = (1.0 * seed * np.exp(1.0) + 2.0 * seed * np.exp(2.0) + 4.0 * 1.0) / 7.0        # exp(50) seed > 1: capped
    assert lpi.linear_reflectivity(gamma, rays, seed) == pytest.approx(want, rel=1e-15)


# ---- the gfx950 listing ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from cbet_raytracing_3d_amd import build
    out = tmp_path_factory.mktemp("isa_backscatter") / "backscatter.s"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [build.hipcc()] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                                     "-o", str(out), os.path.join(CSRC, "cbet_backscatter.hip")]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if run.returncode != 0 and "structurizecfg-skip-uniform-regions" in run.stderr:      # build.build()'s own fallback
        k = cmd.index("-structurizecfg-skip-uniform-regions=true")
        run = subprocess.run(cmd[:k - 1] + cmd[k + 1:], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-2000:]
    text = out.read_text()
    kernels = {}
    for m in re.finditer(r"^(_ZN4cbet\S*k_\w+?E\S*):[^\n]*\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M):
        kernels[m.group(1)] = m.group(2)
    return kernels


def _loop_lines(body):
    """Instruction lines of the basic blocks the compiler marks as inside a loop (test_paths_host.py's rule)."""
    out, inside = [], False
    for line in body.splitlines():
        if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", line):
            inside = "Loop" in line
        elif inside and line.startswith("\t") and not line.strip().startswith(";"):
            out.append(line.strip())
    return out


def test_kernel_instantiations_no_scratch_no_lds(listing):
    trace = [n for n in listing if "k_trace_backscatter" in n]
    assert len(trace) == 12 and len(listing) == 14            # GAIN x IDX64 x NS, the tally and its second stage
    for gain in "01":
        for wide in "01":
            for ns in (4, 8, 16):
                inst = "ILb%sELb%sELi%dEE" % (gain, wide, ns)
                assert sum(inst in n for n in trace) == 1, inst
    assert sum("k_backscatter_tally" in n for n in listing) == 1 and sum("k_backscatter_reduce" in n for n in listing) == 1
    for name, body in listing.items():
        meta = dict(re.findall(r"\.amdhsa_(\w+)\s+(\S+)", body))
        assert int(meta["private_segment_fixed_size"]) == 0, name
        assert int(meta["group_segment_fixed_size"]) == 0, name
        assert not re.search(r"^\s*(scratch_|ds_(read|write|load|store))", body, re.M), name
        print("%s: %s VGPRs" % (name[:70], meta["next_free_vgpr"]))


def test_plain_step_loop_has_no_contracted_multiply_add(listing):
    """GAIN = false: the step loop is one IEEE operation per written operator.  The fp64 quotients and square roots the model
    writes are correctly rounded, and the compiler expands each into a fixed sequence that holds fused multiply-adds of its
    own -- five per quotient (two Newton steps on the reciprocal, the quotient's residual: the sequence that ends in
    v_div_fixup_f64), seven per square root (the sequence that starts at v_rsq_f64) -- so the loop holds exactly those and
    no other: no product and sum of the model was contracted."""
    plain = {n: b for n, b in listing.items() if "k_trace_backscatterILb0E" in n}
    assert len(plain) == 6
    for name, body in plain.items():
        loop = _loop_lines(body)
        ops = [re.sub(r"_e(32|64)$", "", l.split()[0]) for l in loop]           # (the encoding suffix is not part of the operation)
        ndiv, nsqrt = ops.count("v_div_fixup_f64"), ops.count("v_rsq_f64")
        nfma = ops.count("v_fma_f64") + ops.count("v_fmac_f64")
        ns = int(re.search(r"ELi(\d+)EE", name).group(1))
        print("%s: %d loop instructions, %d quotients, %d square roots, %d fused multiply-adds" % (name[:60], len(loop), ndiv, nsqrt, nfma))
        assert len(loop) > 200 and ndiv >= 2 * ns and nsqrt >= 2, name             # the step loop and its model were found
        assert nfma == 5 * ndiv + 7 * nsqrt, name
        assert ops.count("v_mul_f64") >= 6 * ns and ops.count("v_add_f64") >= 3 * ns, name
