"""Exit pass, host side (no GPU): the record's layout in the header, the ctypes mirror and the numpy dtype; the new
entry points exported and refusing bad arguments before touching a device; the gfx950 listing of
cbet_trace_exit.hip (cross-compiled here); the far-field bin formula against hand-computed directions."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "cbet_raytracing_3d_amd", "csrc")


@pytest.fixture(scope="module")
def api():
    from cbet_raytracing_3d_amd import api as a
    a.lib()
    return a


def test_record_layout_header_ctypes_numpy(api, tmp_path):
    fields = [f for f, _ in api.RayExit._fields_]
    assert fields == ["x", "y", "z", "vx", "vy", "vz", "uray", "uray0", "gained", "steps", "status"]
    lines = ['#include <stdio.h>', '#include "cbet_mi355x.h"', 'int main(void){',
             'printf("bits %d %d %d %d\\n", CBET_RAY_LAUNCHED, CBET_RAY_CUTOFF, CBET_RAY_ESCAPED, CBET_RAY_TIMEOUT);',
             'printf("cols %d\\n", CBET_TALLY_COLUMNS);', 'return 0;}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "probe")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(l.split(None, 1) for l in subprocess.check_output([exe], text=True).splitlines())
    assert C.sizeof(api.RayExit) == api.EXIT_DTYPE.itemsize == 80
    assert [int(v) for v in got["bits"].split()] == [api.RAY_LAUNCHED, api.RAY_CUTOFF, api.RAY_ESCAPED, api.RAY_TIMEOUT]
    assert int(got["cols"]) == len(api.TALLY_COLUMNS) == 8
    # a [.., 10] float64 row viewed as the dtype: column 9 holds steps and status
    row = np.zeros(10)
    row.view(np.int32)[18:20] = (123, api.RAY_LAUNCHED | api.RAY_ESCAPED)
    rec = row.view(api.EXIT_DTYPE)[0]
    assert (rec["steps"], rec["status"]) == (123, 5)


def test_argument_checks_without_a_gpu(api):
    """Every refusal below happens before any HIP call (no device on this host)."""
    L = api.lib()
    p = api.default_params(32, nbeams=4)
    g = api.default_gain_params()
    fake = C.c_void_p(4096)   # never dereferenced: the checks fail first
    n = C.c_long()
    assert L.cbet_context_list_length(None, C.byref(n)) == api.EINVAL
    assert L.cbet_context_list_length(fake, None) == api.EINVAL
    # exit pass: NULL context, NULL records, bookkeeping mode, a gain grid without gain params, bad gain params
    args = (None, None, None, fake, None, fake, fake, fake, 1.0, 1.0, 1.0)
    assert L.cbet_trace_exits(*args, C.byref(p), None, None, None) == api.EINVAL
    assert L.cbet_trace_exits(None, None, None, None, None, fake, fake, fake, 1.0, 1.0, 1.0, C.byref(p), None, fake,
                              None) == api.EINVAL
    assert L.cbet_trace_exits(*args, C.byref(p.copy(absorption=0)), None, fake, None) == api.EINVAL
    assert "absorbing" in api.lib().cbet_last_error().decode()
    gargs = (None, None, fake, fake, None, fake, fake, fake, 1.0, 1.0, 1.0)
    assert L.cbet_trace_exits(*gargs, C.byref(p), None, fake, None) == api.EINVAL
    bad_g = api.default_gain_params(max_exponent=2.0)
    assert L.cbet_trace_exits(*gargs, C.byref(p), C.byref(bad_g), fake, None) == api.EINVAL
    assert L.cbet_trace_exits(*args, None, C.byref(g), fake, None) == api.EINVAL
    # tally and far field
    assert L.cbet_exit_tally(None, 64, 4, fake, None) == api.EINVAL
    assert L.cbet_exit_tally(fake, 64, 4, None, None) == api.EINVAL
    assert L.cbet_exit_tally(fake, -1, 4, fake, None) == api.EINVAL
    assert L.cbet_farfield(None, 10, 4, 4, fake, None) == api.EINVAL
    assert L.cbet_farfield(fake, 10, 4, 4, None, None) == api.EINVAL
    for nt, nph in ((0, 4), (4, 0), (-1, 4)):
        assert L.cbet_farfield(fake, 10, nt, nph, fake, None) == api.EINVAL
    # the gain accessor: NULL on bad arguments, else the fixed offset behind the four field components
    assert not L.cbet_cbet_workspace_gain(None, fake)
    assert not L.cbet_cbet_workspace_gain(C.byref(p), None)
    hsize = 34 ** 3
    assert L.cbet_cbet_workspace_gain(C.byref(p), fake) == 4096 + 8 * 4 * 4 * hsize


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from cbet_raytracing_3d_amd import build
    out = tmp_path_factory.mktemp("isa_exit") / "exit.s"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [build.hipcc()] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                                     "-o", str(out), os.path.join(CSRC, "cbet_trace_exit.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    text = out.read_text()
    kernels = {}
    for m in re.finditer(r"^(_ZN4cbet\S*k_\w+?E\S*):[^\n]*\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M):
        kernels[m.group(1)] = m.group(2)
    return kernels


def _named(listing, part):
    return {n: b for n, b in listing.items() if part in n}


def _loop_lines(body):
    """Instruction lines of the basic blocks the compiler marks as inside a loop."""
    out, inside = [], False
    for line in body.splitlines():
        if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", line):
            inside = "Loop" in line
        elif inside and line.startswith("\t") and not line.strip().startswith(";"):
            out.append(line.strip())
    return out


def test_exit_kernel_instantiations_and_no_scratch(listing):
    trace = _named(listing, "k_trace_exit")
    # GAIN x IDX64
    for inst in ("ILb0ELb0EE", "ILb0ELb1EE", "ILb1ELb0EE", "ILb1ELb1EE"):
        assert sum(inst in n for n in trace) == 1, inst
    assert len(trace) == 4
    assert _named(listing, "k_exit_tally") and _named(listing, "k_farfield")
    for name, body in listing.items():
        meta = dict(re.findall(r"\.amdhsa_(\w+)\s+(\S+)", body))
        assert int(meta["private_segment_fixed_size"]) == 0, name


def test_plain_exit_loop_has_no_fused_multiply_add(listing):
    """GAIN = false: the step loop is the reference's arithmetic, one IEEE operation per statement.  (The launch's
    divisions and square roots, before the loop, are the compiler's correctly rounded expansions.)"""
    for name, body in _named(listing, "k_trace_exitILb0E").items():
        loop = _loop_lines(body)
        assert len(loop) > 50, name          # the step loop was found
        assert not [l for l in loop if l.split()[0] in ("v_fma_f64", "v_fmac_f64")], name
    # (the gain instantiations do use them: the CBET hook's arithmetic is the model's, as in the shipped kernel)
    for name, body in _named(listing, "k_trace_exitILb1E").items():
        assert any(l.split()[0] == "v_fma_f64" for l in _loop_lines(body)), name


def test_tally_kernel_uses_no_atomics(listing):
    (name, body), = _named(listing, "k_exit_tally").items()
    ops = [l.split()[0] for l in body.splitlines() if l.startswith("\t") and not l.strip().startswith(";")]
    assert ops and not [o for o in ops if "atomic" in o], name
    # every memory write of the tally is a plain vector or LDS store
    assert any(o.startswith("global_store") for o in ops)


def test_farfield_bin_formula_hand_table(api):
    """(1 - cos theta) / 2 * ntheta and (phi + pi) / (2 pi) * nphi for directions worked out by hand."""
    ntheta, nphi = 4, 8
    s2 = math.sqrt(0.5)
    table = [
        # (vx, vy, vz): (theta bin coordinate, phi bin coordinate) -> bins (it, ip)
        ((0.0, 0.0, 1.0), (0.0, 4.0), (0, 4)),          # +z: theta 0; atan2(0, 0) = 0 -> phi bin nphi / 2
        ((0.0, 0.0, -1.0), (4.0, 4.0), (3, 4)),         # -z: the last polar bin (min(ntheta - 1, .))
        ((1.0, 0.0, 0.0), (2.0, 4.0), (2, 4)),          # +x: equator, phi = 0
        ((-1.0, 1e-300, 0.0), (2.0, 8.0), (2, 7)),      # -x (phi -> +pi): the last azimuthal bin
        ((0.0, 1.0, 0.0), (2.0, 6.0), (2, 6)),          # +y: phi = pi / 2
        ((0.0, -1.0, 0.0), (2.0, 2.0), (2, 2)),         # -y: phi = -pi / 2
        ((0.5, math.sqrt(0.75), 0.0), (2.0, 16.0 / 3.0), (2, 5)),   # phi = pi / 3: (4/3) / 2 * 8
        ((0.5, 0.0, 0.5), (2.0 * (1.0 - s2), 4.0), (0, 4)),         # 45 degrees from +z: (1 - 1/sqrt 2) / 2 * 4 = 0.586
        ((-3.0, -3.0, -3.0 * math.sqrt(2.0)), (2.0 + s2 * 2.0, 1.0), (3, 1)),   # cos theta = -1/sqrt 2, phi = -3 pi / 4
    ]
    for (vx, vy, vz), (ct_want, cp_want), (it_want, ip_want) in table:
        ct, cp = api.farfield_bins(vx, vy, vz, ntheta, nphi)
        assert abs(float(ct) - ct_want) < 1e-12 and abs(float(cp) - cp_want) < 1e-12, ((vx, vy, vz), ct, cp)
        rec = np.zeros(1, dtype=api.EXIT_DTYPE)
        rec["vx"], rec["vy"], rec["vz"], rec["uray"] = vx, vy, vz, 2.5
        rec["status"] = api.RAY_LAUNCHED | api.RAY_ESCAPED
        h = api.farfield_numpy(rec, ntheta, nphi)
        assert h[it_want, ip_want] == 2.5 and h.sum() == 2.5, ((vx, vy, vz), np.argwhere(h))
    # records that did not escape (or were never launched) are not binned
    rec = np.zeros(3, dtype=api.EXIT_DTYPE)
    rec["vz"], rec["uray"] = 1.0, 1.0
    rec["status"] = [api.RAY_LAUNCHED | api.RAY_CUTOFF, api.RAY_ESCAPED, api.RAY_LAUNCHED | api.RAY_TIMEOUT]
    assert api.farfield_numpy(rec, ntheta, nphi).sum() == 0.0
