"""The three device paths that fill a context's plain node tables -- k_tabulate (cbet_tabulate_plasma), k_plasma_records
(cbet_prepare_plasma) and k_tabulate_target with a zero target (cbet_tabulate_target) -- on a DESCENDING profile: the
reversed s83177 arrays take the other branch of the shared bracket's clamp tests and go-low rule (csrc/cbet_node_model.h).
Each path's tables equal the host twin's bit for bit, and the fused kernel's records equal k_step_table's.  And on any
profile the records of both paths equal the reference's stencil with its edge rule, restated here in numpy.  No trace."""
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


def _reference_stencil(ne, consts):
    """launch_ray_XZ.cu:212-238, 268-270 restated in numpy: per axis const * (ne[plus] - ne[minus]) with (minus, plus) =
    (c - 1, c + 1), one-sided on the faces: (0, 2) at 0 and (n - 3, n - 1) at n - 1.  One IEEE subtraction and one
    multiplication per word, as on the device (built without fused multiply-adds): [nx, ny, nz, 3]."""
    kicks = []
    for axis, const in enumerate(consts):
        n = ne.shape[axis]
        c = np.arange(n)
        minus = np.where(c == 0, 0, np.where(c == n - 1, n - 3, c - 1))
        plus = np.where(c == 0, 2, np.where(c == n - 1, n - 1, c + 1))
        kicks.append(np.float64(const) * (np.take(ne, plus, axis) - np.take(ne, minus, axis)))
    return np.stack(kicks, axis=-1)


# Every axis is 3 nodes long once -- there (0, 2) and (n - 3, n - 1) are the same pair and a wrong branch of the rule picks
# a node outside it -- and 70 long once: more than one k_plasma_records tile or chunk (64 in z, 8 in y, 16 in x).
@pytest.mark.parametrize("shape", [(3, 9, 70), (70, 3, 9), (9, 70, 3)], ids=["3x9x70", "70x3x9", "9x70x3"])
def test_step_records_equal_the_reference_stencil(api, inputs, torch_cuda, shape):
    _, r, ne, te = inputs
    p = api.default_params(shape[0], nbeams=4)
    p.ny, p.nz = shape[1], shape[2]
    d = api.derive(p)
    d_r, d_ne, d_te = (torch_cuda.from_numpy(np.ascontiguousarray(v)).cuda() for v in (r, ne, te))
    stream = torch_cuda.cuda.current_stream().cuda_stream
    n = p.nx * p.ny * p.nz

    def two(ctx):
        api.tabulate_plasma(ctx, p, d_te, d_r, d_ne, stream)
        api.prepare_step_records(ctx, p, None, None, d.xconst, d.yconst, d.zconst, stream)

    def fused(ctx):
        api.prepare_plasma(ctx, p, d_te, d_r, d_ne, d.xconst, d.yconst, d.zconst, stream)

    face = np.zeros(shape, dtype=bool)
    for axis in range(3):
        for side in (0, -1):
            sl = [slice(None)] * 3
            sl[axis] = side
            face[tuple(sl)] = True
    for path, fill in (("tabulate_plasma + prepare_step_records", two), ("prepare_plasma", fused)):
        ctx = api.Context(p, 0)
        api.moveToAndFromGPU(ctx.step_records()[0], np.full(4 * n, np.nan), 8 * 4 * n, 0)   # a fill that wrote nothing fails
        fill(ctx)
        torch_cuda.cuda.synchronize()
        ne3d, kap3d, rec = context_tables(api, ctx, p, 0, records=True, bits=False)
        ctx.close()
        want = np.concatenate([_reference_stencil(ne3d, (d.xconst, d.yconst, d.zconst)), kap3d[..., None]], axis=-1)
        diff = rec.view(np.int64) != want.view(np.int64)
        print("%s %s: %d of %d record words differ; non-zero kicks on the faces: %s" % (
            shape, path, int(diff.sum()), diff.size, [int((rec[face][:, c] != 0).sum()) for c in range(3)]))
        assert not diff.any(), (path, np.argwhere(diff)[:5].tolist())
        assert (rec[face][:, :3] != 0).any(), path
