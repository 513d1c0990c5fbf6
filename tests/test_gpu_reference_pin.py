"""The three kernel formulations against grids that the REFERENCE's own kernel source wrote, with no oracle in between.

tests/golden/reference_grid_<case>.npy are the whole grids of single-threaded runs of launch_ray_XZ.cu compiled as host
C++ (oracle/ref_build.py, tests/golden/make_reference_golden.py; tests/test_reference_pin.py holds them to the live
binaries bit for bit).  Four small cases, each moving an axis on which the kernels used to be checked against the
oracle's generalisation of the reference's compile-time constants only:

    ragged_60            20 x 17 x 25, all 60 OMEGA beams: nt from nx alone, dt from min(dx, dz) without dy
    tall_y               20 x 80 x 20: far jumps along y, rays that lose their cell
    rpz6_24              24^3 with 6 rays per zone
    descending_20x17x25  the s83177 profile reversed: the descending branch of interp_cuda, bisecting as written there.
                         The first TRACE of a descending profile on the device (test_gpu_node_tables.py fills tables on one).

Per case and kernel variant, with dense and padded rows and the narrow and the forced wide index: the counters'
ray_steps equal the reference's count, the project's parity metric is below PARITY_TOL = 1e-9 (each run prints what it
observed) and the zero pattern is the reference's -- on every cell, except for the far-jump case, where deposit weights
of both signs cancel and the pattern is compared as test_gpu_config_space.py compares it: on the cells whose zero-ness
and sign two summation orders of the CPU oracle agree on.
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, parity_err
from helpers import reference_cases as RC

pytestmark = pytest.mark.gpu

PARITY_TOL = 1e-9
VARIANTS = [1, 2, 3]     # GLOBAL_ATOMICS, LDS_COMBINE, LDS_WINDOW (default)
PAD = 5                  # extra doubles per z row of the padded grid
NTHREADS = 8


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


@pytest.fixture(scope="module")
def want(oracle, inputs):
    """case name -> (the reference's grid, its ray-step count, cells whose zero-ness is compared, cells whose sign is)."""
    kat = json.load(open(os.path.join(GOLDEN, "reference_kat.json")))["cases"]
    cache = {}

    def get(case):
        if case.name not in cache:
            grid = np.load(os.path.join(GOLDEN, "reference_grid_%s.npy" % case.name))
            assert list(grid.shape) == kat[case.name]["shape"] and np.count_nonzero(grid) == kat[case.name]["nonzero"]
            zero_ok = np.ones(grid.shape, dtype=bool)
            sign_ok = np.abs(grid) > 1e-9 * np.abs(grid).max()      # a sign means something above the metric's floor only
            if case.far_jump:       # test_gpu_config_space.py's rule: the oracle forwards and with the beams reversed
                cfg, bt, prof = case.config(oracle), case.beam_table(inputs[0]), case.profile(oracle, inputs)
                oe, _ = oracle.trace(cfg, bt, *prof, nthreads=NTHREADS)
                oe2, _ = oracle.trace(cfg, bt[::-1].copy(), *prof, nthreads=NTHREADS)
                zero_ok = (oe == 0) == (oe2 == 0)
                sign_ok &= zero_ok & ((oe < 0) == (oe2 < 0))
            cache[case.name] = (grid, kat[case.name]["ray_steps"], zero_ok, sign_ok)
        return cache[case.name]
    return get


def _run(tr, e, **kw):
    tr.counters(reset=True)
    tr.launch(e, **kw)
    return e.cpu().numpy(), tr.counters(reset=True)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", RC.FULL_GRID)
def test_kernels_match_the_reference_grid(api, oracle, inputs, want, torch_cuda, name, variant):
    from cbet_raytracing_3d_amd.tracer import RayTracer
    case = RC.BY_NAME[name]
    grid, steps, zero_ok, sign_ok = want(case)
    r, ne, te = case.profile(oracle, inputs)
    if name.startswith("descending"):
        assert r[0] > r[-1]
    tr = RayTracer(case.params(api, kernel_variant=variant), r, ne, te, beam_norm=case.beam_table(inputs[0]))
    nz = tr.params.nz
    for rows in ("dense", "padded"):
        for wide in (0, 1):
            e = tr.new_grid() if rows == "dense" else tr.new_grid(zpitch=nz + 2 + PAD)
            got, c = _run(tr, e, force_wide_index=wide)
            if rows == "padded":
                assert got.shape[2] == nz + 2 + PAD and not got[..., nz + 2:].any()      # the padding is never touched
                got = np.ascontiguousarray(got[..., :nz + 2])
            err = parity_err(got, grid)
            print("%-20s variant %d %-6s rows %s index: steps %d (reference %d)  parity err vs reference %.2e  "
                  "zero pattern differs in %d cells (%d of them compared)"
                  % (name, variant, rows, "wide" if wide else "narrow", c.ray_steps, steps, err,
                     int(((got == 0) != (grid == 0)).sum()), int((((got == 0) != (grid == 0)) & zero_ok).sum())))
            what = (name, variant, rows, wide)
            assert c.ray_steps == steps, what
            assert c.rays_traced == tr.params.nbeams * tr.derived.nlive_rays, what
            assert np.isfinite(got).all(), what
            assert err < PARITY_TOL, what + (err,)
            assert np.array_equal((got == 0)[zero_ok], (grid == 0)[zero_ok]), what
            assert np.array_equal((got < 0)[sign_ok], (grid < 0)[sign_ok]), what
    tr.close()
