"""Ray path recorder, host side (no GPU; include/cbet_mi355x.h cbet_trace_paths): the two records'
layout in the header, the ctypes mirrors and the numpy dtypes; the entry point exported and refusing every bad argument
before it looks at the context or touches a device; the Python wrapper's checks of the item arrays; the gfx950 listing
of cbet_trace_path.hip (cross-compiled here); and, on the CPU oracle, the regimes the GPU tests (test_gpu_paths.py) rely
on, so a helper that drifts fails here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from helpers import exit_cases as X

CSRC = os.path.join(ROOT, "cbet_raytracing_3d_amd", "csrc")
FAR_CENTRE_BEAM = 3        # the beam of RAGGED whose rays are all closest to 5 beam_norm[b] at their launch point


@pytest.fixture(scope="module")
def api():
    from cbet_raytracing_3d_amd import api as a
    a.lib()
    return a


def test_struct_layouts_match_header(api):
    sample = [f for f, _ in api.PathSample._fields_]
    turn = [f for f, _ in api.RayTurn._fields_]
    assert sample == ["x", "y", "z", "uray", "absorbed", "gained", "ci", "cj", "ck", "step"]
    assert turn == ["r2", "x", "y", "z", "uray", "ne", "step", "steps", "status", "nsamples"]
    assert C.sizeof(api.PathSample) == api.PATH_DTYPE.itemsize == 64 and C.sizeof(api.RayTurn) == api.TURN_DTYPE.itemsize == 64
    # a [.., 8] float64 row viewed as the dtypes: the integers sit in columns 6 and 7
    row = np.zeros(8)
    row.view(np.int32)[12:16] = (3, 4, 5, 77)
    rec = row.view(api.PATH_DTYPE)[0]
    assert (rec["ci"], rec["cj"], rec["ck"], rec["step"]) == (3, 4, 5, 77)
    rec = row.view(api.TURN_DTYPE)[0]
    assert (rec["step"], rec["steps"], rec["status"], rec["nsamples"]) == (3, 4, 5, 77)


def _call(api, p, g=None, ctx=None, **kw):
    """cbet_trace_paths with never-dereferenced pointers (the checks fail first) and the keyword overrides; returns
    (code, message)."""
    fake = C.c_void_p(4096)
    a = dict(ne3d=None, kappa3d=None, gain=None, beams=fake, raynums=fake, nitems=130, stride=1, capacity=4,
             center=(C.c_double * 3)(0.0, 0.0, 0.0), samples=fake, turns=fake)
    a.update(kw)
    rc = api.lib().cbet_trace_paths(a["ne3d"], a["kappa3d"], a["gain"], a["beams"], a["raynums"], a["nitems"], a["stride"],
                                    a["capacity"], a["center"], a["samples"], a["turns"], None, fake, fake, fake, 1.0, 1.0,
                                    1.0, C.byref(p) if p is not None else None, C.byref(g) if g is not None else None, ctx,
                                    None)
    return rc, api.lib().cbet_last_error().decode()


def test_argument_checks_without_a_gpu(api):
    """Every refusal below happens with a NULL context and before any HIP call (no device on this host); each message
    names its offence."""
    p = api.default_params(32, nbeams=4)
    fake = C.c_void_p(4096)
    cases = [
        (dict(stride=0), "stride"), (dict(stride=-3), "stride"),
        (dict(capacity=-1), "capacity"),
        (dict(nitems=-1), "nitems"),
        (dict(nitems=2 ** 62, capacity=1), "overflow"), (dict(nitems=2 ** 62, capacity=0), "overflow"),
        (dict(nitems=2 ** 40, capacity=2 ** 20), "overflow"),
        (dict(nitems=2 ** 40, capacity=0), "one launch"),
        (dict(turns=None), "turn"),
        (dict(beams=None), "beams"), (dict(raynums=None), "raynums"),
        (dict(samples=None), "sample"),
        (dict(center=(C.c_double * 3)(0.0, float("nan"), 0.0)), "center"),
        (dict(center=(C.c_double * 3)(float("inf"), 0.0, 0.0)), "center"),
        (dict(center=(C.c_double * 3)(0.0, 0.0, float("-inf"))), "center"),
        (dict(center=None), "center"),
        (dict(gain=fake), "gain params"),
    ]
    for kw, word in cases:
        rc, msg = _call(api, p, **kw)
        assert rc == api.EINVAL and word in msg, (kw, rc, msg)
    rc, msg = _call(api, p.copy(absorption=0))
    assert rc == api.EINVAL and "absorbing" in msg, msg
    rc, msg = _call(api, p, g=api.default_gain_params(max_exponent=2.0), gain=fake)
    assert rc == api.EINVAL, msg
    rc, msg = _call(api, None)
    assert rc == api.EINVAL
    # what is legal reaches the context check: NULL samples with capacity 0, NULL items with nitems 0, a gain with params
    for kw in (dict(samples=None, capacity=0), dict(beams=None, raynums=None, nitems=0), dict(capacity=0, nitems=0)):
        rc, msg = _call(api, p, **kw)
        assert rc == api.EINVAL and "context" in msg, (kw, msg)
    rc, msg = _call(api, p, g=api.default_gain_params(), gain=fake)
    assert rc == api.EINVAL and "context" in msg, msg


def test_wrapper_refuses_bad_item_arrays(api, monkeypatch):
    """api.path_items, which RayTracer.trace_paths runs the caller's arrays through before the upload: unequal lengths,
    a dtype or values an int32 does not hold, more than one dimension -- refused without a library call."""
    def no_library(*a, **k):
        raise AssertionError("the item checks made a library call")
    monkeypatch.setattr(api, "lib", no_library)
    b, r = api.path_items([0, 1, 2], np.array([5, 6, 7], dtype=np.int64))
    assert b.dtype == r.dtype == np.int32 and b.flags.c_contiguous and r.tolist() == [5, 6, 7]
    b, r = api.path_items(np.array([-1, 3], dtype=np.int16), np.array([2 ** 31 - 1, -2 ** 31], dtype=np.int64))
    assert r.tolist() == [2 ** 31 - 1, -2 ** 31]          # ids that name no ray are the kernel's to judge
    b, r = api.path_items(np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))
    assert b.size == r.size == 0
    for beams, raynums, word in (
            ([0, 1, 2], [5, 6], "length"),
            ([0], [], "length"),
            ([0.0, 1.0], [5, 6], "integers"),
            ([0, 1], np.array([5.5, 6.0]), "integers"),
            ([True, False], [5, 6], "integers"),
            ([0, 1], np.array([5, 2 ** 31], dtype=np.int64), "int32"),
            (np.array([0, -2 ** 31 - 1], dtype=np.int64), [5, 6], "int32"),
            (np.array([0, 2 ** 32 + 1], dtype=np.uint64), [5, 6], "int32"),
            (np.zeros((2, 2), dtype=np.int32), np.zeros((2, 2), dtype=np.int32), "one-dimensional"),
    ):
        with pytest.raises(ValueError, match=word):
            api.path_items(beams, raynums)


# ---- the gfx950 listing ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from cbet_raytracing_3d_amd import build
    out = tmp_path_factory.mktemp("isa_path") / "path.s"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [build.hipcc()] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                                     "-o", str(out), os.path.join(CSRC, "cbet_trace_path.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    text = out.read_text()
    kernels = {}
    for m in re.finditer(r"^(_ZN4cbet\S*k_\w+?E\S*):[^\n]*\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M):
        kernels[m.group(1)] = m.group(2)
    return kernels


def _loop_lines(body):
    """Instruction lines of the basic blocks the compiler marks as inside a loop."""
    out, inside = [], False
    for line in body.splitlines():
        if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", line):
            inside = "Loop" in line
        elif inside and line.startswith("\t") and not line.strip().startswith(";"):
            out.append(line.strip())
    return out


def test_path_kernel_instantiations_no_scratch_no_lds(listing):
    assert len(listing) == 4
    for inst in ("ILb0ELb0EE", "ILb0ELb1EE", "ILb1ELb0EE", "ILb1ELb1EE"):      # GAIN x IDX64
        assert sum("k_trace_path" in n and inst in n for n in listing) == 1, inst
    for name, body in listing.items():
        meta = dict(re.findall(r"\.amdhsa_(\w+)\s+(\S+)", body))
        assert int(meta["private_segment_fixed_size"]) == 0, name
        assert int(meta["group_segment_fixed_size"]) == 0, name


def test_plain_path_loop_has_no_fused_multiply_add(listing):
    """GAIN = false: the step loop -- the reference's arithmetic and the r2 of the closest approach, whose
    parenthesisation the header fixes -- is one IEEE operation per statement."""
    plain = {n: b for n, b in listing.items() if "k_trace_pathILb0E" in n}
    assert len(plain) == 2
    for name, body in plain.items():
        loop = _loop_lines(body)
        assert len(loop) > 50, name          # the step loop was found
        assert not [l for l in loop if l.split()[0] in ("v_fma_f64", "v_fmac_f64")], name
        # r2: three squares and two sums on top of the step's own multiplies and adds
        assert sum(l.split()[0] == "v_mul_f64" for l in loop) >= 3 and sum(l.split()[0] == "v_add_f64" for l in loop) >= 5, name


# ---- the regimes the GPU tests rely on, on the oracle ----------------------------------------------------------------
def closest_approach(lp, path, center):
    """The header's closest approach restated in numpy on an oracle path: (r2, step) of the FIRST minimum over the launch
    point and the position after every step, r2 = ((x-cx)*(x-cx) + (y-cy)*(y-cy)) + (z-cz)*(z-cz)."""
    pos = np.vstack([lp[:3], path[:, :3]])
    e = pos - np.asarray(center, dtype=np.float64)
    r2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    return r2, int(np.argmin(r2))            # argmin: the first occurrence of the minimum


def test_regime_ragged_closest_approaches(oracle, inputs):
    """RAGGED: 426 live rays per beam, 11 .. 59 steps; for 88 .. 132 rays per beam the closest approach to the origin is
    the last step, for the rest it is interior, and no ray has a tie."""
    from helpers import config_matrix as M
    bn, r, ne, te = inputs
    cfg, bt = X.RAGGED.config(oracle), X.RAGGED.beam_table(bn)
    ids = M.live_ids(oracle, cfg, bt)
    assert len(ids) == 426 and cfg.nbeams == 4
    nmin, nmax = 10 ** 9, 0
    for b in range(cfg.nbeams):
        last = interior = 0
        for i in ids:
            live, lp = oracle.launch_point(cfg, bt, b, int(i))
            path = oracle.ray_path(cfg, bt, r, ne, te, b, int(i))
            assert live
            r2, k = closest_approach(lp, path, (0.0, 0.0, 0.0))
            assert (r2 == r2[k]).sum() == 1, (b, i)                   # no ties
            nmin, nmax = min(nmin, len(path)), max(nmax, len(path))
            last += k == len(path)
            interior += 0 < k < len(path)
        assert 88 <= last <= 132 and last + interior == len(ids), (b, last, interior)
    assert (nmin, nmax) == (11, 59)


def test_regime_long_box_steps(oracle, inputs):
    """LONG_BOX in vacuum: 124 live rays per beam, 41 steps for the x and z beams, 96 = nt for the +-y beams -- at stride
    8 that is 7 and 13 samples, on either side of a capacity of 10."""
    from helpers import config_matrix as M
    bn, r, ne, te = inputs
    vac = np.zeros_like(ne)
    cfg, bt = X.LONG_BOX.config(oracle), X.LONG_BOX.beam_table(bn)
    ids = M.live_ids(oracle, cfg, bt)
    assert len(ids) == X.LONG_BOX_LIVE and oracle.derive(cfg).nt == X.LONG_BOX_NT == 96
    for b in range(cfg.nbeams):
        n = {len(oracle.ray_path(cfg, bt, r, vac, te, b, int(i))) for i in ids}
        assert n == ({96} if b in X.LONG_BOX_Y_BEAMS else {41}), (b, n)
    assert 1 + -(-41 // 8) == 7 and 1 + -(-96 // 8) == 13


def test_regime_far_centre_is_closest_at_launch(oracle, inputs):
    """With the centre at 5 beam_norm[b] -- beyond the launch plane, on the beam's own side -- every ray of beam b =
    FAR_CENTRE_BEAM of RAGGED is closest at step 0, the launch point.  (Not of every beam: a ray that the plasma turns
    straight back leaves the box beyond its launch plane -- 25, 17 and 4 of the 426 rays of RAGGED's beams 0, 1, 2.)"""
    from helpers import config_matrix as M
    bn, r, ne, te = inputs
    cfg, bt = X.RAGGED.config(oracle), X.RAGGED.beam_table(bn)
    ids = M.live_ids(oracle, cfg, bt)
    b = FAR_CENTRE_BEAM
    for i in ids:
        _, lp = oracle.launch_point(cfg, bt, b, int(i))
        path = oracle.ray_path(cfg, bt, r, ne, te, b, int(i))
        r2, k = closest_approach(lp, path, 5.0 * bt[b])
        assert k == 0 and (r2[1:] > r2[0]).all(), (b, i)
    # ... and the other beams' rays, against that same centre, are not all closest at launch: the general rule is at work
    other = sum(closest_approach(oracle.launch_point(cfg, bt, 0, int(i))[1], oracle.ray_path(cfg, bt, r, ne, te, 0, int(i)),
                                 5.0 * bt[b])[1] != 0 for i in ids)
    assert other > 0
