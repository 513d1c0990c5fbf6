"""Downloads of a context's device tables for the GPU tests: node tables, step records and the flow table in use."""
import numpy as np


def download(api, addr, shape, gpu, bits=True):
    """The doubles at device address `addr` as an array of `shape`: int64 bit patterns, or the values with bits=False."""
    h = np.empty(int(np.prod(shape)))
    api.moveToAndFromGPU(h, addr, 8 * h.size, gpu)
    return (h.view(np.int64) if bits else h).reshape(shape)


def context_tables(api, ctx, p, gpu, records=False, bits=True):
    """[ne3d, kappa3d] of a context, each [nx, ny, nz], and with records=True its step records [nx, ny, nz, 4].
    (Asks for the writable table pointers: that marks the tables as edited, the next launch rebuilds the records.)"""
    shape = (p.nx, p.ny, p.nz)
    parts = [(addr, shape) for addr in ctx.tables()]
    if records:
        parts.append((ctx.step_records()[0], shape + (4,)))
    return [download(api, addr, shp, gpu, bits) for addr, shp in parts]


def context_flow(api, ctx, p, gpu, bits=True):
    """The flow table the context has selected, [3, nx, ny, nz]; None without one."""
    addr = ctx.flow()
    return download(api, addr, (3, p.nx, p.ny, p.nz), gpu, bits) if addr else None
