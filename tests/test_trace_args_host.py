"""TraceArgs::exit_planes, host side (no GPU): host_exit_planes (csrc/cbet_host_internal.h) is the ONE function that fills
both the array cbet_context_create uploads for the other kernels and the by-value copy in the shipped trace kernel's
argument block.  Checked here: the function's six values are, bit for bit, the reference's expressions xmin - (dx / 2.0),
xmax + (dx / 2.0), ... on the derived cell sizes of a ragged extent (three different cell sizes, no face at a round
number), and both of its callers really go through it (their source names no other expression for the planes).  That the
device sees the same values on both routes is what the GPU tests of the faces check."""
import os
import struct
import subprocess

import numpy as np

from cbet_raytracing_3d_amd import build
from conftest import ROOT

CSRC = os.path.join(ROOT, "cbet_raytracing_3d_amd", "csrc")

DRIVER = r'''
#include <cstddef>
#include <cstdio>
#include <cstring>
#include "cbet_host_internal.h"

int main()
{
    cbet_params p;
    if (cbet_params_default(&p, 20) != CBET_OK) return 1;
    p.ny = 17; p.nz = 25;
    p.xmin = -0.0131; p.xmax = 0.0477; p.ymin = -0.0293; p.ymax = 0.0119; p.zmin = -0.0071; p.zmax = 0.0302;
    cbet_derived d;
    if (cbet_derive(&p, &d) != CBET_OK) { std::printf("derive: %s\n", cbet_last_error()); return 1; }
    cbet::TraceArgs a{};                     // as trace_impl fills the argument block's copy
    cbet::host_exit_planes(&p, d, a.exit_planes);
    static_assert(sizeof a.exit_planes == 6 * sizeof(double), "six doubles");
    static_assert(offsetof(cbet::TraceArgs, exit_planes) % 8 == 0, "scalar loads of whole doubles");
    std::printf("cells %a %a %a\n", d.dx, d.dy, d.dz);
    for (int k = 0; k < 6; ++k) {
        unsigned long long bits;
        std::memcpy(&bits, &a.exit_planes[k], 8);
        std::printf("plane %d %016llx\n", k, bits);
    }
    return 0;
}
'''


def test_both_callers_fill_the_planes_through_the_one_function():
    ctx = open(os.path.join(CSRC, "cbet_context.cpp")).read()
    abi = open(os.path.join(CSRC, "cbet_trace_abi.cpp")).read()
    assert "host_exit_planes(p, d, hb)" in ctx and "hipMemcpy(ctx->bounds, hb" in ctx
    assert "host_exit_planes(&ctx->p, ctx->d, a.exit_planes)" in abi
    for text in (ctx, abi):                       # no second statement of the planes beside the shared one
        assert "/ 2.0)" not in text


def test_exit_planes_are_the_reference_expressions_bit_for_bit(tmp_path):
    src = tmp_path / "planes.cpp"
    src.write_text(DRIVER)
    exe = str(tmp_path / "planes")
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc()))), "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", rocm_include,
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC, str(src), os.path.join(CSRC, "cbet_params.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split("\n")
    dx, dy, dz = (float.fromhex(w) for w in [l for l in lines if l.startswith("cells")][0].split()[1:])
    assert len({dx, dy, dz}) == 3
    got = [int(l.split()[2], 16) for l in lines if l.startswith("plane")]
    lo, hi = (-0.0131, -0.0293, -0.0071), (0.0477, 0.0119, 0.0302)
    want = []
    for axis, cell in enumerate((dx, dy, dz)):       # launch_ray_XZ.cu:352-354
        want += [np.float64(lo[axis]) - (np.float64(cell) / np.float64(2.0)), np.float64(hi[axis]) + (np.float64(cell) / np.float64(2.0))]
    assert got == [struct.unpack("<Q", struct.pack("<d", float(w)))[0] for w in want]
