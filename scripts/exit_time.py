"""Times the exit pass (cbet_trace_exits) at 256^3 / 60 beams against the plain deposit pass, in one process, with HIP
events: 3 timed launches after a warm-up each.  The plain exit pass; the exit pass with a gain grid (the converged gain
of a native CBET solve, read through cbet_cbet_workspace_gain); the plain deposit pass as bench.py times it (tabulate +
step records + trace) and its trace alone.  One JSON line.
usage: python scripts/exit_time.py [--no-gain]"""
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


def timed(fn, reps=3):
    fn()                                       # warm-up
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def main():
    bn, r, ne, te = load_inputs()
    tr = RayTracer(api.default_params(256), r, ne, te, beam_norm=bn)
    out = {"n": 256, "nbeams": 60}
    edep = tr.new_grid()

    def deposit():
        edep.zero_()
        tr.launch(edep)
    out["deposit_ms"] = timed(deposit)
    tr.tabulate()
    d = tr.derived
    stream = torch.cuda.current_stream().cuda_stream
    api.prepare_step_records(tr.ctx, tr.params, None, None, d.xconst, d.yconst, d.zconst, stream)

    def trace_only():
        edep.zero_()
        api.trace_nodes(0, d.nindices, None, None, edep, tr.d_bbeam_norm, tr.d_beam_norm, tr.d_pow_r, tr.d_phase_r,
                        d.xconst, d.yconst, d.zconst, tr.params.copy(beam_lo=0, beam_hi=60), tr.ctx, stream)
    out["deposit_trace_only_ms"] = timed(trace_only)
    ex = tr.new_exits()
    out["exit_ms"] = timed(lambda: tr.trace_exits(ex, tabulate=False))
    tally = tr.energy_balance(ex).cpu().numpy()
    launched = tally[:, 0].sum()
    out["plain"] = {"absorbed_fraction": tally[:, 2].sum() / launched, "escaped_fraction": tally[:, 3].sum() / launched,
                    "stranded_fraction": tally[:, 4].sum() / launched, "unfinished_fraction": tally[:, 5].sum() / launched}
    out["tally_ms"] = timed(lambda: tr.energy_balance(ex))
    hist = torch.zeros((36, 72), dtype=torch.float64, device="cuda")
    out["farfield_ms"] = timed(lambda: api.farfield(ex, ex.shape[0] * ex.shape[1], 36, 72, hist, stream))
    if "--no-gain" not in sys.argv:
        gp = api.default_gain_params()
        ws = torch.empty(api.cbet_workspace_bytes(tr.params) // 8, dtype=torch.float64, device="cuda")
        e = tr.new_grid()
        rep = api.cbet_solve(tr.d_te, tr.d_r, tr.d_ne, e, tr.d_bbeam_norm, tr.d_beam_norm, tr.d_pow_r, tr.d_phase_r,
                             tr.params, gp, workspace=ws, ctx=tr.ctx, stream=stream)
        nb, hs = 60, int(np.prod(tr.grid_shape))
        gain = ws[4 * nb * hs:5 * nb * hs].view((nb,) + tr.grid_shape)
        assert gain.data_ptr() == api.cbet_workspace_gain(tr.params, ws)
        out["exit_gain_ms"] = timed(lambda: tr.trace_exits(ex, gain=gain, gain_params=gp, tabulate=False))
        t = tr.energy_balance(ex).cpu().numpy()
        out["cbet"] = {"passes": rep.passes, "absorbed_fraction": t[:, 2].sum() / launched,
                       "escaped_fraction": t[:, 3].sum() / launched, "stranded_fraction": t[:, 4].sum() / launched,
                       "unfinished_fraction": t[:, 5].sum() / launched, "gained_sum": t[:, 1].sum(),
                       "absorbed_vs_solve_edep": t[:, 2].sum() / float(e.sum()) - 1.0}
        del ws, gain
    for k in [k for k in out if k.endswith("_ms")]:
        out[k + "_min"] = min(out[k])
    out["exit_over_deposit"] = out["exit_ms_min"] / out["deposit_ms_min"]
    print(json.dumps(out))
    tr.close()


if __name__ == "__main__":
    main()
