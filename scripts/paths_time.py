"""Times the path recorder (cbet_trace_paths) at 256^3 / 60 beams, in one process, with HIP events:

  * bookkeeping: every live ray of every beam (RayTracer.ray_items()) with capacity = 0 -- turn records only -- against
    the exit pass (cbet_trace_exits) over the same rays, launches interleaved, medians of `reps` each;
  * samples: 4,096 rays of one beam at stride 1 and stride 16: time, bytes written, achieved write rate;
  * the energy-weighted quartiles of ne / ncrit at the closest approach to the origin, plain and with the converged gain
    of a native CBET solve (--no-gain skips the solve).

The item arrays are uploaded once; the timed call is api.trace_paths on torch's current stream.  One JSON line.
usage: python scripts/paths_time.py [--no-gain] [--reps N]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_inputs  # noqa: E402
from cbet_raytracing_3d_amd import api  # noqa: E402
from cbet_raytracing_3d_amd.tracer import RayTracer  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def interleaved(fns, reps):
    """{name: [ms] * reps}: one warm-up of each, then the functions in turn, reps times."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            out[k].append(event_ms(fn))
    return out


def weighted_quartiles(x, w):
    order = np.argsort(x)
    x, c = x[order], np.cumsum(w[order])
    return [float(x[np.searchsorted(c, q * c[-1])]) for q in (0.25, 0.5, 0.75)]


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 7
    bn, r, ne, te = load_inputs()
    tr = RayTracer(api.default_params(256), r, ne, te, beam_norm=bn)
    d, p = tr.derived, tr.params
    stream = torch.cuda.current_stream().cuda_stream
    tr.tabulate()
    api.prepare_step_records(tr.ctx, p, None, None, d.xconst, d.yconst, d.zconst, stream)
    tail = tr._tail()
    out = {"n": 256, "nbeams": 60, "nt": d.nt, "reps": reps}

    def paths(beams, raynums, stride, capacity, samples, turns, gain=None, gp=None):
        api.trace_paths(None, None, gain, beams, raynums, beams.numel(), stride, capacity, (0.0, 0.0, 0.0), samples, turns,
                        *tail, p, gp, tr.ctx, stream)

    # ---- bookkeeping: turn records of every live ray against the exit pass ----
    hb, hr = tr.ray_items()
    beams, raynums = torch.from_numpy(hb).cuda(), torch.from_numpy(hr).cuda()
    nitems = beams.numel()
    ex = tr.new_exits()
    _, turns = tr.new_paths(nitems, 0)
    # ... and the same rays with the launch list's idle entries kept (ray_items(bundles=True)): a wave is then one ray
    # bundle of the exit pass, where the compacted list lets a wave straddle two
    hbb, hrb = tr.ray_items(bundles=True)
    beams_b, raynums_b = torch.from_numpy(hbb).cuda(), torch.from_numpy(hrb).cuda()
    _, turns_b = tr.new_paths(beams_b.numel(), 0)
    t = interleaved({"exit": lambda: tr.trace_exits(ex, tabulate=False),
                     "paths_turns_only": lambda: paths(beams, raynums, 1, 0, None, turns),
                     "paths_turns_only_bundles": lambda: paths(beams_b, raynums_b, 1, 0, None, turns_b)}, reps)
    out["items"], out["items_bundles"] = nitems, beams_b.numel()
    for k in t:
        out[k + "_ms"], out[k + "_ms_median"] = t[k], float(np.median(t[k]))
    out["paths_over_exit"] = out["paths_turns_only_ms_median"] / out["exit_ms_median"]
    out["paths_bundles_over_exit"] = out["paths_turns_only_bundles_ms_median"] / out["exit_ms_median"]
    Tb = turns_b.cpu().numpy().view(api.TURN_DTYPE)[..., 0]
    assert Tb[hrb >= 0].tobytes() == turns.cpu().numpy().view(api.TURN_DTYPE)[..., 0].tobytes()     # the same records
    del turns_b, beams_b, raynums_b
    T = turns.cpu().numpy().view(api.TURN_DTYPE)[..., 0]
    rec = ex.cpu().numpy().view(api.EXIT_DTYPE)[..., 0]
    out["ray_steps"] = int(T["steps"].astype(np.int64).sum())
    assert out["ray_steps"] == int(rec["steps"].astype(np.int64).sum())

    # ---- the distribution of ne / ncrit at the closest approach, weighted with the launch energy ----
    s0, turns1 = tr.new_paths(nitems, 1)
    paths(beams, raynums, 1, 1, s0, turns1)
    uray0 = s0.cpu().numpy().view(api.PATH_DTYPE)[0, :, 0]["uray"]
    out["plain"] = {"ne_over_ncrit_quartiles": weighted_quartiles(T["ne"] / d.ncrit, uray0),
                    "closest_r_cm_quartiles": weighted_quartiles(np.sqrt(T["r2"]), uray0)}
    if "--no-gain" not in sys.argv:
        gp = api.default_gain_params()
        ws = torch.empty(api.cbet_workspace_bytes(p) // 8, dtype=torch.float64, device="cuda")
        e = tr.new_grid()
        rep = api.cbet_solve(tr.d_te, tr.d_r, tr.d_ne, e, tr.d_bbeam_norm, tr.d_beam_norm, tr.d_pow_r, tr.d_phase_r, p, gp,
                             workspace=ws, ctx=tr.ctx, stream=stream)
        nb, hs = 60, int(np.prod(tr.grid_shape))
        gain = ws[4 * nb * hs:5 * nb * hs].view((nb,) + tr.grid_shape)
        assert gain.data_ptr() == api.cbet_workspace_gain(p, ws)
        t = interleaved({"exit_gain": lambda: tr.trace_exits(ex, gain=gain, gain_params=gp, tabulate=False),
                         "paths_gain_turns_only": lambda: paths(beams, raynums, 1, 0, None, turns, gain, gp)}, reps)
        out["exit_gain_ms"], out["paths_gain_turns_only_ms"] = t["exit_gain"], t["paths_gain_turns_only"]
        out["exit_gain_ms_median"], out["paths_gain_turns_only_ms_median"] = (
            float(np.median(t[k])) for k in ("exit_gain", "paths_gain_turns_only"))
        out["paths_over_exit_gain"] = out["paths_gain_turns_only_ms_median"] / out["exit_gain_ms_median"]
        Tg = turns.cpu().numpy().view(api.TURN_DTYPE)[..., 0]
        # the energy a ray carries at its closest approach, against the plain pass's: where the exchange put the light
        out["cbet"] = {"passes": rep.passes,
                       "ne_over_ncrit_quartiles_by_launch_energy": weighted_quartiles(Tg["ne"] / d.ncrit, uray0),
                       "ne_over_ncrit_quartiles_by_energy_there": weighted_quartiles(Tg["ne"] / d.ncrit, Tg["uray"]),
                       "plain_ne_over_ncrit_quartiles_by_energy_there": weighted_quartiles(T["ne"] / d.ncrit, T["uray"]),
                       "energy_there_over_plain": float(Tg["uray"].sum() / T["uray"].sum())}
        del ws, gain
    del s0, turns1, ex

    # ---- samples: 4,096 rays of one beam ----
    ids = tr.ray_ids()
    live = ids[ids >= 0][:4096].astype(np.int32)
    b1, r1 = torch.zeros(len(live), dtype=torch.int32, device="cuda"), torch.from_numpy(live).cuda()
    out["sampled"] = {}
    for stride in (1, 16):
        capacity = 1 + -(-d.nt // stride)
        samples, tn = tr.new_paths(len(live), capacity)
        ms = interleaved({"s": lambda: paths(b1, r1, stride, capacity, samples, tn)}, reps)["s"]
        nsamples = tn.cpu().numpy().view(api.TURN_DTYPE)[..., 0]["nsamples"].astype(np.int64)
        written = int(64 * (nsamples.sum() + len(live)))          # the samples and the turn records
        med = float(np.median(ms))
        out["sampled"]["stride_%d" % stride] = {"rays": len(live), "capacity": capacity, "ms": ms, "ms_median": med,
                                                 "bytes_written": written, "write_GB_per_s": written / med / 1e6}
        del samples, tn
    turns_only = interleaved({"s": lambda: paths(b1, r1, 1, 0, None, turns[:len(live)])}, reps)["s"]
    out["sampled"]["turns_only_ms_median"] = float(np.median(turns_only))
    print(json.dumps(out))
    tr.close()


if __name__ == "__main__":
    main()
