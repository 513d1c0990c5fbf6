"""The three device paths that fill a context's plain node tables -- k_tabulate (cbet_tabulate_plasma), k_plasma_records
(cbet_prepare_plasma) and k_tabulate_target with a zero target (cbet_tabulate_target) -- on a DESCENDING profile: the
reversed s83177 arrays take the other branch of the shared bracket's clamp tests and go-low rule (csrc/cbet_node_model.h).
Each path's tables equal the host twin's bit for bit, and the fused kernel's records equal k_step_table's.  No trace."""
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


# 9 x 7 x 13: smaller than one k_plasma_records tile (8 x 64 in y-z, 16 planes) and ragged on every side;
# 40 x 33 x 50: the shape of tests/test_gpu_target.py, several workgroups of every kernel
@pytest.mark.parametrize("shape", [(9, 7, 13), (40, 33, 50)], ids=["9x7x13", "40x33x50"])
def test_descending_profile_fills_equal_the_host_twin_bitwise(api, inputs, torch_cuda, shape):
    _, r, ne, te = (np.ascontiguousarray(v[::-1]) for v in inputs)
    assert r[0] > r[-1]
    p = api.default_params(shape[0], nbeams=4)
    p.ny, p.nz = shape[1], shape[2]
    d = api.derive(p)
    want = [w.view(np.int64) for w in api.target_tables(p, r, ne, te, api.Target())]
    ascending = api.target_tables(p, *(np.ascontiguousarray(v[::-1]) for v in (r, ne, te)), api.Target())
    assert any((w != a.view(np.int64)).any() for w, a in zip(want, ascending))      # the order changes the bits

    ctx = api.Context(p, 0)
    d_r, d_ne, d_te = (torch_cuda.from_numpy(v).cuda() for v in (r, ne, te))
    stream = torch_cuda.cuda.current_stream().cuda_stream
    n = p.nx * p.ny * p.nz

    def poison():
        """NaN into both tables and the records, so that a fill that wrote nothing cannot pass on the last one's values."""
        junk = np.full(4 * n, np.nan)
        for addr, count in zip(ctx.tables() + (ctx.step_records()[0],), (n, n, 4 * n)):
            api.moveToAndFromGPU(addr, junk, 8 * count, 0)

    def check(path, got):
        for what, g, w in zip(("ne3d", "kappa3d"), got, want):
            diff = g != w
            print("%s %s %s: %d of %d words differ" % (shape, path, what, int(diff.sum()), diff.size))
            assert not diff.any(), (path, what, np.argwhere(diff)[:5].tolist())

    poison()
    api.tabulate_plasma(ctx, p, d_te, d_r, d_ne, stream)
    api.prepare_step_records(ctx, p, None, None, d.xconst, d.yconst, d.zconst, stream)
    torch_cuda.cuda.synchronize()
    two = context_tables(api, ctx, p, 0, records=True)
    check("tabulate_plasma", two)
    assert all((two[2][..., c] != 0).any() for c in range(4)) and not np.isnan(two[2].view(np.float64)).any()

    poison()
    api.prepare_plasma(ctx, p, d_te, d_r, d_ne, d.xconst, d.yconst, d.zconst, stream)
    torch_cuda.cuda.synchronize()
    fused = context_tables(api, ctx, p, 0, records=True)
    check("prepare_plasma", fused)
    diff = fused[2] != two[2]
    print("%s records: %d of %d words differ" % (shape, int(diff.sum()), diff.size))
    assert not diff.any(), np.argwhere(diff)[:5].tolist()

    poison()
    api.tabulate_target(ctx, p, d_te, d_r, d_ne, api.Target((0.0, 0.0, 0.0), np.zeros(25), lmax=4), stream)
    torch_cuda.cuda.synchronize()
    check("tabulate_target", context_tables(api, ctx, p, 0))
    ctx.close()
