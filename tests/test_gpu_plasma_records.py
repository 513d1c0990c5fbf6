"""k_plasma_records (cbet_prepare_plasma) against the two kernels it fuses: node tables and step records must be the
bits k_tabulate + k_step_table write -- face nodes included, where the record's pairs are one-sided -- and the context
must remember the records exactly as after the two calls (reused while nothing changed, rebuilt for other constants)."""
import numpy as np
import pytest

from helpers.device_tables import context_tables

pytestmark = pytest.mark.gpu


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


def _download(api, ctx, p, gpu):
    """(ne3d, kappa3d, records[nx, ny, nz, 4]) of a context as int64 bit patterns."""
    return context_tables(api, ctx, p, gpu, records=True)


def _params(api, shape, padded):
    nx, ny, nz = shape
    p = api.default_params(nx, nbeams=4)
    p.ny, p.nz = ny, nz
    if padded:
        p.edep_zpitch = -(-(nz + 2) // 8) * 8 + 8          # rows of whole 64-byte lines, one line of padding
    return p


@pytest.mark.parametrize("padded", [False, True], ids=["dense", "padded"])
@pytest.mark.parametrize("shape", [(64, 64, 64), (100, 100, 100), (256, 256, 256), (40, 33, 50)],
                         ids=["64", "100", "256", "40x33x50"])
def test_fused_tables_and_records_are_bitwise_the_two_kernels(api, inputs, torch_cuda, shape, padded):
    from cbet_raytracing_3d_amd.tracer import RayTracer
    bn, r, ne, te = inputs
    p = _params(api, shape, padded)
    tr = RayTracer(p.copy(edep_zpitch=0), r, ne, te, beam_norm=bn[:4])
    d = tr.derived
    two, one = tr.ctx, api.Context(p, tr.gpu)
    stream = torch_cuda.cuda.current_stream().cuda_stream
    api.tabulate_plasma(two, p, tr.d_te, tr.d_r, tr.d_ne, stream)
    api.prepare_step_records(two, p, None, None, d.xconst, d.yconst, d.zconst, stream)
    api.prepare_plasma(one, p, tr.d_te, tr.d_r, tr.d_ne, d.xconst, d.yconst, d.zconst, stream)
    torch_cuda.cuda.synchronize()
    want = _download(api, two, p, tr.gpu)
    got = _download(api, one, p, tr.gpu)
    for name, w, g in zip(("ne3d", "kappa3d", "records"), want, got):
        diff = w != g
        print("%s %s: %d of %d words differ" % (shape, name, int(diff.sum()), diff.size))
        assert not diff.any(), (name, np.argwhere(diff)[:5].tolist())
    # the faces on their own (the one-sided pairs): every node with an index 0 or n-1, all four record words
    rec_w, rec_g = want[2], got[2]
    for ax in range(3):
        for side in (0, -1):
            sl = [slice(None)] * 3
            sl[ax] = side
            assert np.array_equal(rec_w[tuple(sl)], rec_g[tuple(sl)]), (ax, side)
    # and the records are not trivially equal: kicks are non-zero somewhere on every axis
    assert all((rec_g[..., c] != 0).any() for c in range(4))
    one.close()
    tr.close()


def test_records_are_reused_until_a_constant_changes(api, inputs, torch_cuda):
    from cbet_raytracing_3d_amd.tracer import RayTracer
    bn, r, ne, te = inputs
    p = _params(api, (48, 48, 48), False)
    tr = RayTracer(p, r, ne, te, beam_norm=bn[:4])
    d = tr.derived
    stream = torch_cuda.cuda.current_stream().cuda_stream
    q = tr.params.copy(beam_lo=0, beam_hi=4)

    def trace(ctx, xconst):
        e = tr.new_grid()
        api.trace_nodes(0, d.nindices, None, None, e, tr.d_bbeam_norm, tr.d_beam_norm, tr.d_pow_r, tr.d_phase_r,
                        xconst, d.yconst, d.zconst, q, ctx, stream)
        torch_cuda.cuda.synchronize()
        return e

    ctx = tr.ctx
    assert ctx.step_records()[1] == 0
    api.prepare_plasma(ctx, p, tr.d_te, tr.d_r, tr.d_ne, d.xconst, d.yconst, d.zconst, stream)
    assert ctx.step_records()[1] == 1
    first = trace(ctx, d.xconst)
    assert ctx.step_records()[1] == 1                      # unchanged inputs: the fused kernel's records are reused
    trace(ctx, d.xconst)
    assert ctx.step_records()[1] == 1
    trace(ctx, 2.0 * d.xconst)
    assert ctx.step_records()[1] == 2                      # another constant: rebuilt (k_step_table, from the fused tables)
    other = api.Context(p, tr.gpu)
    api.tabulate_plasma(other, p, tr.d_te, tr.d_r, tr.d_ne, stream)
    api.prepare_step_records(other, p, None, None, 2.0 * d.xconst, d.yconst, d.zconst, stream)
    torch_cuda.cuda.synchronize()
    assert np.array_equal(_download(api, ctx, p, tr.gpu)[2], _download(api, other, p, tr.gpu)[2])
    # (_download asked for the writable table pointers: that marks the tables as edited, the next launch rebuilds)
    api.prepare_plasma(ctx, p, tr.d_te, tr.d_r, tr.d_ne, d.xconst, d.yconst, d.zconst, stream)
    n = ctx.step_records()[1]
    again = trace(ctx, d.xconst)
    assert ctx.step_records()[1] == n
    # the same records give the same rays: equal ray-for-ray, sums differ only by the atomics' order
    assert float((again - first).abs().max()) <= 1e-11 * float(first.abs().max())
    # one half alone is what it was: tabulating marks the records stale, the next launch rebuilds them
    api.tabulate_plasma(ctx, p, tr.d_te, tr.d_r, tr.d_ne, stream)
    trace(ctx, d.xconst)
    assert ctx.step_records()[1] == n + 1
    other.close()
    tr.close()
