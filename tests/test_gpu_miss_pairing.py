"""The plain trace kernel's paired window misses (cbet_trace_window.hip, hbm_add8: a lane outside both deposit boxes sends
each of its four (x, y) columns as ONE atomic instruction shared with its quad neighbour, which carries the column's other
z node) on the smallest worlds in which that path runs.

Cases (chosen with the CPU oracle for their size and step counts, and on the device for `wave_steps_miss > 0`; every test
asserts that first, from a `window_stats = 1` launch, so a case that stops reaching the path fails instead of passing idly):

  * n40     40^3, beams 0 / 17 / 42 of the OMEGA-60 table, the s83177 profile (tests/test_gpu_layout_arms.py's N40): bundles
            fan out behind the turning point, 297 wave-steps with a lane outside both boxes;
  * ragged  20 x 17 x 25, the same beams: rows of nz + 2 = 27 doubles, so dense rows start and end mid-line and a column's
            pair straddles a 64-byte line wherever the lower node ends one; 168 such wave-steps;
  * n24     24^3, the same beams: the three formulations cell by cell; 107 such wave-steps.

Bounds: the full grid against the oracle at the suite's 1e-9 (conftest.parity_err; the pairing only reorders
fp64 sums: observed 2e-15 .. 2e-14), ray-step and ray counts exact; rim-merged against unmerged bundles at 1e-12 (sums of
non-negative terms in another order: a few thousand terms' worth of 1.1e-16).  The window counters are lane-atomics and
ray-steps, which the pairing must not change: they equal the values the parent commit 9ec5164 (window misses as eight
single-lane atomics) counted on the same cases."""
import numpy as np
import pytest

from conftest import NCPU, parity_err
from helpers import config_matrix as M

pytestmark = pytest.mark.gpu

PARITY_TOL = 1e-9
MERGE_TOL = 1e-12
BEAMS = (0, 17, 42)
CASES = {
    "n40": M.Entry("n40_three_beams", n=40, beams=BEAMS),
    "ragged": M.Entry("ragged_20x17x25", n=20, ny=17, nz=25, beams=BEAMS),
    "n24": M.Entry("n24_three_beams", n=24, beams=BEAMS),
}
# window_stats counters of the parent commit 9ec5164 on these cases (the same in the compiled-in and the generic
# instantiation, with dense and with padded rows)
PARENT_COUNTERS = {
    "n40": dict(wave_steps_miss=297, lds_evictions=1181, global_atomics=101949),
    "ragged": dict(wave_steps_miss=168, lds_evictions=1043, global_atomics=18533),
    "n24": dict(wave_steps_miss=107, lds_evictions=409, global_atomics=25123),
}


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
def references(oracle, inputs):
    """case -> (grid, ray-steps) of the oracle, computed once and left unchanged."""
    out = {}
    for name, entry in CASES.items():
        grid, steps = M.oracle_trace(oracle, entry, inputs, nthreads=NCPU)
        grid.setflags(write=False)
        out[name] = (grid, steps)
    return out


def _tracer(api, inputs, entry, **extra):
    from cbet_raytracing_3d_amd.tracer import RayTracer
    bn, r, ne, te = inputs
    return RayTracer(entry.params(api, **extra), r, ne, te, beam_norm=entry.beam_table(bn))


def _run(tr, padded=False, **kw):
    """One launch into a fresh grid -> (the reference-shaped grid, counters)."""
    e = tr.new_grid(zpitch=True) if padded else tr.new_grid()
    tr.counters(reset=True)
    tr.launch(e, **kw)
    c = tr.counters(reset=True)
    return e.cpu().numpy()[..., : tr.params.nz + 2], c


def _misses(tr, **kw):
    """The path runs: wave-steps with a lane outside both boxes, from the counting instantiation."""
    _, c = _run(tr, stats=True, **kw)
    assert c.wave_steps_miss > 0 and c.lds_evictions > 0, (c.wave_steps_miss, c.lds_evictions)
    return c


@pytest.mark.parametrize("padded", [False, True], ids=["dense_rows", "padded_rows"])
@pytest.mark.parametrize("case", ["n40", "ragged"])
def test_parity_with_the_oracle(api, inputs, references, torch_cuda, case, padded):
    """The full grid at 1e-9, ray-steps and rays exact -- with the reference's dense rows and with rows padded to whole
    64-byte lines (cbet_params.edep_zpitch); on the ragged shape dense rows are 27 doubles, so pairs straddle lines and
    rows end mid-line."""
    want, steps = references[case]
    tr = _tracer(api, inputs, CASES[case])
    _misses(tr, padded=padded)
    got, c = _run(tr, padded=padded)
    err = parity_err(got, want)
    print(case, "padded" if padded else "dense", "parity %.2e" % err, "ray-steps", c.ray_steps)
    assert c.ray_steps == steps and c.rays_traced == len(BEAMS) * tr.derived.nlive_rays
    assert err < PARITY_TOL, err
    tr.close()


def test_the_three_formulations_agree(api, inputs, references, torch_cuda):
    """kernel_variant 0 (the window kernel), 1 (one global atomic per node and step) and 2 (the tagged LDS scheme): the
    same grid cell by cell, the same ray-steps."""
    want, steps = references["n24"]
    tr = _tracer(api, inputs, CASES["n24"])
    _misses(tr)
    grids = {}
    for variant in (0, 1, 2):
        grids[variant], c = _run(tr, kernel_variant=variant)
        assert c.ray_steps == steps, variant
        assert parity_err(grids[variant], want) < PARITY_TOL, variant
    for variant in (1, 2):
        err = parity_err(grids[0], grids[variant])
        print("variant 0 against", variant, "%.2e" % err)
        assert err < PARITY_TOL, (variant, err)
        assert np.array_equal(grids[0] != 0.0, grids[variant] != 0.0), variant      # the same cells touched
    tr.close()


def test_rim_merged_bundles_carry_for_holes(api, inputs, references, torch_cuda):
    """A rim-merged launch list (cbet_params.rim_merge = 4) packs rim patches into bundles with holes, so a miss lane's quad
    neighbour may be a lane without a ray: it lends its slot like any other.  The same rays unmerged (rim_merge = 0)
    deposit the same grid to 1e-12."""
    want, steps = references["n40"]
    grids = {}
    for merge in (4, 0):
        tr = _tracer(api, inputs, CASES["n40"], rim_merge=merge)
        live = api.live_ray_list(tr.params).reshape(-1, 64)
        pairs = live.reshape(-1, 32, 2)
        hole_beside_ray = int(((pairs < 0).any(axis=2) & (pairs >= 0).any(axis=2)).sum())
        if merge:
            assert hole_beside_ray > 0                  # live lanes whose quad neighbour is a hole
        _misses(tr)
        grids[merge], c = _run(tr)
        print("rim_merge", merge, "bundles", len(live), "pairs of a ray and a hole", hole_beside_ray)
        assert c.ray_steps == steps, merge
        assert parity_err(grids[merge], want) < PARITY_TOL, merge
        tr.close()
    err = parity_err(grids[4], grids[0])
    print("merged against unmerged %.2e" % err)
    assert err < MERGE_TOL, err


def test_generic_instantiation(api, inputs, references, torch_cuda):
    """k_trace_window<16, true, 0, *>: 64-bit addresses behind the same picks (force_wide_index, the hook the parity tests
    use), on the ragged shape."""
    want, steps = references["ragged"]
    tr = _tracer(api, inputs, CASES["ragged"])
    _misses(tr, force_wide_index=1)
    got, c = _run(tr, force_wide_index=1)
    assert c.ray_steps == steps
    assert parity_err(got, want) < PARITY_TOL
    tr.close()


@pytest.mark.parametrize("case", list(CASES))
def test_window_counters_are_the_parents(api, inputs, torch_cuda, case):
    """global_atomics counts lane-atomics -- eight per flush of a miss lane, credited to that lane -- and lds_evictions the
    ray-steps bound for HBM: what the parent commit counted, in both counting instantiations."""
    tr = _tracer(api, inputs, CASES[case])
    for wide in (0, 1):
        c = _misses(tr, force_wide_index=wide)
        got = {k: int(getattr(c, k)) for k in PARENT_COUNTERS[case]}
        assert got == PARENT_COUNTERS[case], (case, wide, got)
    tr.close()
