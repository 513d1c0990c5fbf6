"""The device-side calls of the gain stage's GPU tests: a tracer, one gain update from a zero gain and the sequences built on
it (first call and frozen call, slab, packed slab), the table set-ups, and the two small host statements the comparisons need
(a launch's wavefront count, errors per 64-cell z group).  torch is the caller's: the functions take it as an argument, so that
the host tests can import the helper package on a machine without a device."""
import numpy as np

from helpers import gain_worlds as W


def tracer(inputs, p, beam_norm, tabulate=True):
    from cbet_raytracing_3d_amd.tracer import RayTracer
    _, r, ne, te = inputs
    tr = RayTracer(p, r, ne, te, beam_norm=beam_norm)
    if tabulate:
        tr.tabulate()
    return tr


def stream(torch):
    return torch.cuda.current_stream().cuda_stream


def device_worlds(api, oracle, inputs, torch, nthreads):
    """Per grid: the CPU world, a tracer that gets limits or shifts (`tr`), one that never has any (`base`), the device
    fields and tables (`dev`).  close_worlds closes the tracers."""
    out = {}
    for name, world in (("traced", W.traced_world(api, oracle, inputs, nthreads)),
                        ("crowded", W.crowded_world(api, oracle, inputs, nthreads))):
        tr, base = tracer(inputs, world["p"], world["bn"]), tracer(inputs, world["p"], world["bn"])
        dev = {k: torch.from_numpy(np.ascontiguousarray(world[k])).cuda() for k in ("raw", "flow", "shifted", "state")}
        out[name] = dict(world, name=name, tr=tr, base=base, dev=dev)
    return out


def close_worlds(worlds):
    for w in worlds.values():
        w["tr"].close()
        w["base"].close()


def tables(api, torch, w, which):
    """The table set-ups of the tests as (flow, state) device tensors or None: "none"; "flow" the sphere's own table handed in
    as a caller's; "uniform" flow plus a state table holding the scalars everywhere; "three" flow plus the three-state
    pattern with kz = 1; "tabled" the reference's: the offset target's flow plus the three-state pattern."""
    dev = w["dev"]
    if which == "none":
        return None, None
    if which == "flow":
        return dev["flow"], None
    if which == "uniform":
        _, cs, gc = api.gain_constants(w["p"], w["gp"])
        uni = torch.empty_like(dev["state"])
        uni[0], uni[1] = cs, gc
        return dev["flow"], uni
    assert which in ("three", "tabled"), which
    return (dev["shifted"] if which == "tabled" else dev["flow"]), dev["state"]


def select(tr, flow=None, state=None):
    tr.set_flow(flow)
    tr.set_gain_state(state)


def update(torch, tr, raw, gp, pair_once, x=(0, None), change=True):
    """One gain update from a zero gain on a copy of the device fields `raw`: (fields, gain, change)."""
    f = raw.clone()
    k = tr.new_grid(per_beam=True)
    ch = torch.zeros(2, dtype=torch.float64, device="cuda") if change else None
    tr.gain_field(f, k, gp, ch, pair_once=pair_once, x_lo=x[0], x_hi=x[1])
    return f, k, ch


def first_and_frozen(torch, tr, raw, gp, pair_once, change=True, change2=False):
    """A first call, then a frozen call on fresh energy over the k entries of the first: f, k, change, f2, k2, change2 (the
    frozen call's sums, None unless asked for)."""
    f, k, ch = update(torch, tr, raw, gp, pair_once, change=change)
    f2 = f.clone()
    f2[0] = raw[0]
    k2 = torch.zeros_like(k)
    ch2 = torch.zeros(2, dtype=torch.float64, device="cuda") if change2 else None
    tr.gain_field(f2, k2, gp, ch2, pair_once=pair_once, frozen=True)
    return f, k, ch, f2, k2, ch2


def packed(torch, api, tr, raw, gp, pair_once, slab, frozen=False, change=True):
    """cbet_gain_field_packed on the planes `slab` alone, from a zero gain: (fields, gain, change)."""
    x0, x1 = slab
    f = raw[:, :, x0:x1].contiguous()
    k = torch.zeros((raw.shape[1], x1 - x0) + tuple(raw.shape[3:]), dtype=torch.float64, device="cuda")
    ch = torch.zeros(2, dtype=torch.float64, device="cuda") if change else None
    if frozen:
        from cbet_raytracing_3d_amd.tracer import _frozen
        gp = _frozen(gp, True)
    api.gain_field_packed(f, None, k, torch.empty_like(k) if pair_once else None, ch, x0, x1, tr.params, gp, tr.ctx, stream(torch))
    return f, k, ch


def all_calls(torch, api, tr, raw, gp, pair_once, slab, change=True, packed_frozen=False):
    """First call, frozen call on fresh energy, slab, packed slab, and if asked a frozen call on the packed slab:
    [(what, tensor)], the change sums ("... change") among them unless change=False."""
    f, k, ch, f2, k2, ch2 = first_and_frozen(torch, tr, raw, gp, pair_once, change=change, change2=change)
    fs, ks, chs = update(torch, tr, raw, gp, pair_once, x=slab, change=change)
    fp, kp, chp = packed(torch, api, tr, raw, gp, pair_once, slab, change=change)
    out = [("first fields", f), ("first gain", k), ("first change", ch), ("frozen fields", f2), ("frozen gain", k2),
           ("frozen change", ch2), ("slab fields", fs), ("slab gain", ks), ("slab change", chs), ("packed fields", fp),
           ("packed gain", kp), ("packed change", chp)]
    if packed_frozen:
        f3 = f.clone()
        f3[0] = raw[0]
        fq, kq, chq = packed(torch, api, tr, f3, gp, pair_once, slab, frozen=True, change=change)
        out += [("packed frozen fields", fq), ("packed frozen gain", kq), ("packed frozen change", chq)]
    torch.cuda.synchronize()
    return [(what, t) for what, t in out if change or not what.endswith("change")]


def waves(tr, pair_once, x_lo, x_hi):
    """Wavefronts of one gain launch over the planes [x_lo, x_hi): the tests' one host statement of the launch geometry of
    launch_gain_field / brick_grid (cbet_grid_kernels.hip).  Each wavefront adds its share of the two convergence sums with one
    atomicAdd."""
    hy, hz = tr.grid_shape[1], tr.grid_shape[2]
    if pair_once:
        return (x_hi - x_lo) * hy                                       # one single-wavefront workgroup per z-row
    bricks = (((x_hi + 1) >> 1) - (x_lo >> 1)) * ((hy + 3) // 4) * ((hz + 7) // 8)
    return 4 * min((bricks + 3) // 4, 256 * 64)                         # four wavefronts per workgroup


def group_errors(a, b, scale):
    """max |a - b| / scale in each of the 64-cell z groups."""
    return [float(np.abs(a[..., z] - b[..., z]).max() / scale) for z in W.Z_GROUPS]
