"""Parity of the three kernel formulations across the run-time knobs of cbet_params (tests/helpers/config_matrix.py):
Courant multipliers past the point where the nearest-node update can follow a ray, boxes that are off centre, smaller
than the focal length or thin along one axis, strided and truncating launch rules, beams along grid axes and diagonals,
and nt at the window kernel's 16-bit edge -- every entry against the CPU oracle: equal ray-step counts, the project's
parity metric below PARITY_TOL = 1e-9, and the same zero / sign pattern.

Margin: reordering alone (oracle serial vs 8-thread atomics vs beams reversed) moves the metric by <= 5e-14 on the
tracked entries and by up to 1.1e-11 on the far-jump ones, where deposit weights of both signs cancel; each test prints
what it observed.
"""
import numpy as np
import pytest

from conftest import parity_err
from helpers import config_matrix as M

pytestmark = pytest.mark.gpu

PARITY_TOL = 1e-9
VARIANTS = [1, 2, 3]     # GLOBAL_ATOMICS, LDS_COMBINE, LDS_WINDOW (default)
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
    """Oracle results per entry, computed once: (grid, steps, cells whose zero-ness / sign both of the oracle's own
    orderings agree on)."""
    cache = {}

    def get(entry):
        if entry.name not in cache:
            bn, r, ne, te = inputs
            cfg, bt = entry.config(oracle), entry.beam_table(bn)
            oe, osteps = oracle.trace(cfg, bt, r, ne, te, nthreads=NTHREADS)
            oe2, osteps2 = oracle.trace(cfg, bt[::-1].copy(), r, ne, te, nthreads=NTHREADS)   # the beams reversed
            assert osteps == osteps2 and np.isfinite(oe).all() and np.abs(oe).max() > 0
            zero_ok = (oe == 0) == (oe2 == 0)
            sign_ok = zero_ok & ((oe < 0) == (oe2 < 0))
            if entry.far_jump:      # weights of both signs cancel: a sign means something above the metric's floor only
                sign_ok &= np.abs(oe) > 1e-9 * np.abs(oe).max()
            cache[entry.name] = (oe, osteps, zero_ok, sign_ok, parity_err(oe2, oe))
        return cache[entry.name]
    return get


def _tracer(api, inputs, entry, **extra):
    from cbet_raytracing_3d_amd.tracer import RayTracer
    bn, r, ne, te = inputs
    return RayTracer(entry.params(api, **extra), r, ne, te, beam_norm=entry.beam_table(bn))


def _run(tr, e=None, shards=1, **kw):
    e = tr.new_grid() if e is None else e
    tr.counters(reset=True)
    for s in range(shards):
        tr.launch(e, shard_index=s, shard_count=shards, **kw)
    return e.cpu().numpy(), tr.counters(reset=True)


def _check(entry, got, c, tr, w, what):
    oe, osteps, zero_ok, sign_ok, own = w
    err = parity_err(got, oe)
    print("%-16s %-22s steps %9d (oracle %9d)  parity err %.2e  (oracle vs its own reordering %.2e)"
          % (entry.name, what, c.ray_steps, osteps, err, own))
    assert c.ray_steps == osteps, (entry.name, what)
    assert c.rays_traced == tr.params.nbeams * tr.derived.nlive_rays, (entry.name, what)
    assert np.isfinite(got).all()
    assert err < PARITY_TOL, (entry.name, what, err)
    assert np.array_equal((got == 0)[zero_ok], (oe == 0)[zero_ok]), (entry.name, what)
    assert np.array_equal((got < 0)[sign_ok], (oe < 0)[sign_ok]), (entry.name, what)
    if entry.name in M.PINNED_STEPS:
        assert osteps == M.PINNED_STEPS[entry.name]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("entry", M.ENTRIES, ids=str)
def test_matrix_entry_matches_the_oracle(api, inputs, want, torch_cuda, entry, variant):
    tr = _tracer(api, inputs, entry, kernel_variant=variant)
    got, c = _run(tr)
    _check(entry, got, c, tr, want(entry), "variant %d" % variant)
    if variant == 3:      # the counting instantiation of the window kernel
        got, c = _run(tr, stats=True)
        _check(entry, got, c, tr, want(entry), "variant 3 stats")
        assert c.wave_steps > 0
    tr.close()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", M.EXTRAS)
def test_matrix_entry_wide_index_per_beam_padded_and_sharded(api, oracle, inputs, want, torch_cuda, name, variant):
    entry = M.BY_NAME[name]
    bn, r, ne, te = inputs
    w = want(entry)
    tr = _tracer(api, inputs, entry, kernel_variant=variant)
    got, c = _run(tr, force_wide_index=1)
    _check(entry, got, c, tr, w, "v%d wide index" % variant)
    got, c = _run(tr, shards=3)
    _check(entry, got, c, tr, w, "v%d three shards" % variant)
    nz = tr.params.nz
    got, c = _run(tr, e=tr.new_grid(zpitch=nz + 2 + 5))
    assert not got[..., nz + 2:].any()                      # the padding is never touched
    _check(entry, np.ascontiguousarray(got[..., :nz + 2]), c, tr, w, "v%d padded rows" % variant)
    got, c = _run(tr, e=tr.new_grid(per_beam=True))
    cfg, bt = entry.config(oracle), entry.beam_table(bn)
    osteps = 0
    for b in range(cfg.nbeams):
        ob, st = oracle.trace(cfg, bt, r, ne, te, beam_lo=b, beam_hi=b + 1, nthreads=NTHREADS)
        osteps += st
        err = parity_err(got[b], ob)
        print("%-16s v%d beam %d of per-beam grids: parity err %.2e" % (name, variant, b, err))
        assert err < PARITY_TOL, (name, variant, b, err)
    assert c.ray_steps == osteps == w[1]
    tr.close()


def test_nt_one_past_the_edge_is_refused_by_the_window_kernel_only(api, oracle, inputs, torch_cuda):
    """nt == 65535 is the last value the window kernel's 16-bit counters hold (the long_nt entry runs on it above);
    nt == 65536 is refused by it with EINVAL and runs -- and matches the oracle -- on the two cross-check kernels."""
    base = M.BY_NAME["long_nt"]
    entry = M.Entry("nt_65536", n=base.n, beams=base._beams, overrides=dict(courant_mult=M.courant_for_nt(base.n, 65536)))
    bn, r, ne, te = inputs
    tr = _tracer(api, inputs, entry)
    assert tr.derived.nt == 65536 and api.derive(base.params(api)).nt == M.NT_EDGE
    for variant in (3, 0):
        with pytest.raises(api.CbetError) as ei:
            tr.launch(tr.new_grid(), kernel_variant=variant)
        assert ei.value.code == api.EINVAL and "16 bits" in str(ei.value)
    oe, osteps = oracle.trace(entry.config(oracle), entry.beam_table(bn), r, ne, te, nthreads=NTHREADS)
    for variant in (1, 2):
        got, c = _run(tr, kernel_variant=variant)
        err = parity_err(got, oe)
        print("nt_65536 variant %d steps %d (oracle %d) parity err %.2e" % (variant, c.ray_steps, osteps, err))
        assert c.ray_steps == osteps and err < PARITY_TOL
    tr.close()


def test_axis_beams_device_trig_is_close(api, inputs, torch_cuda):
    """acos(+-1) and atan2(0, 0) evaluated on the device (bbeam_norm == NULL), held to what
    test_device_trig_fallback_is_close asserts for the OMEGA rows."""
    tr = _tracer(api, inputs, M.BY_NAME["axis_beams"])
    a, ca = _run(tr)
    b, cb = _run(tr, use_host_trig=False)
    print("axis_beams device trig: steps %d vs %d, sum ratio - 1 = %.2e" % (cb.ray_steps, ca.ray_steps, b.sum() / a.sum() - 1))
    assert np.isfinite(b).all()
    assert abs(int(ca.ray_steps) - int(cb.ray_steps)) <= 1e-4 * ca.ray_steps
    assert abs(b.sum() / a.sum() - 1) < 1e-6
    tr.close()
