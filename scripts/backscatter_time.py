#!/usr/bin/env python3
"""Times the backscatter SBS gain spectra at 256^3, 60 beams, on the normalised fields and the gain
grid of one gain update of a real field pass, with HIP events, nothing running beside the kernels; three interleaved
repetitions of 8 calls each, reported as the mean of the repetitions' medians and their spread:
  * k_trace_backscatter for every live ray of every beam at nshift = 1, 8 and 16 (the NS = 4, 8 and 16 instantiations), with
    the gain grid -- the GAIN arm, like the exit pass beside it -- and at nshift = 16 without it;
  * k_backscatter_tally + k_backscatter_reduce at nshift = 16;
  * the exit pass with the gain grid, on this build and on a build of the PARENT commit (--parent-lib FILE, loaded through
    CBET_LIB_PATH), in the same run on the same machine.
A repetition is one child process per build, this build's and the parent's in turn.  Every GPU step is a child process under
its own `timeout`; the first failure ends the run and nothing more is started.
Writes profiles/backscatter/backscatter_time.json (or --out FILE).
usage: python scripts/backscatter_time.py [--parent-lib FILE] [--n N] [--out FILE]"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from saturation_time import spread, summary, timed  # noqa: E402

N, CALLS, REPS = 256, 8, 3
LIMITS = {"new": 420, "parent": 300}                         # seconds a step may take (set-up of 45 GB included)
NEW = ("cbet_trace_backscatter", "cbet_backscatter_work_bytes", "cbet_backscatter_tally", "cbet_backscatter_host")
STEP = 2.0 ** 38                                             # rad/s: the scan is 2 STEP (m - 13), m = 0 .. nshift - 1


def step(name, n):
    """One GPU step, in this process: a dict of results."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import load_inputs
    from cbet_raytracing_3d_amd import api
    from cbet_raytracing_3d_amd.tracer import RayTracer
    if name == "parent":
        api.lib(tolerate=NEW)                   # the parent's build lacks this commit's entries; only its exit pass is run
    bn, r, ne, te = load_inputs()
    gp = api.default_gain_params()
    tr = RayTracer(api.default_params(n), r, ne, te, beam_norm=bn)
    tr.tabulate()
    fields = tr.new_fields()
    tr.launch_cbet(fields, gp, fields=True)
    gain = tr.new_grid(per_beam=True)
    tr.gain_field(fields, gain, gp, None, pair_once=True)           # normalised fields and the gain grid of one update
    exits = tr.new_exits()
    torch.cuda.synchronize()
    out = {"library": os.path.relpath(os.path.abspath(api.LIB_PATH), ROOT)}
    out["exit_gain"] = summary(timed(torch, lambda: tr.trace_exits(exits, gain=gain, gain_params=gp, tabulate=False), CALLS))
    if name == "parent":
        tr.close()
        return out
    beams, raynums = tr.ray_items()
    nitems = int(beams.size)
    d_beams, d_raynums = torch.from_numpy(beams).cuda(), torch.from_numpy(raynums).cuda()
    gamma = torch.zeros((16, nitems), dtype=torch.float64, device="cuda")
    rays = torch.zeros((nitems, 4), dtype=torch.float64, device="cuda")
    out["items"] = nitems

    def trace(nshift, grid):
        shifts = np.array([2.0 * STEP * (m - 13.0) for m in range(nshift)])
        api.trace_backscatter(None, None, grid, d_beams, d_raynums, nitems, fields, shifts, gamma, rays, *tr._tail(), tr.params, gp,
                              tr.ctx, tr._stream())

    for nshift in (1, 8, 16):
        out["sbs_gain_%d" % nshift] = summary(timed(torch, lambda: trace(nshift, gain), CALLS))
    out["sbs_plain_16"] = summary(timed(torch, lambda: trace(16, None), CALLS))
    nb = tr.params.nbeams
    work = torch.empty(max(api.backscatter_work_bytes(nitems, 16, nb) // 8, 1), dtype=torch.float64, device="cuda")
    tally = torch.zeros((nb, 16, 4), dtype=torch.float64, device="cuda")
    out["tally_16"] = summary(timed(torch, lambda: api.backscatter_tally(gamma, rays, d_beams, nitems, 16, nb, tally, work, tr._stream()),
                                    CALLS, before=tally.zero_))
    rec = rays.cpu().numpy().view(api.SBS_DTYPE)[..., 0]
    out["ray_steps"] = int(rec["steps"].sum())
    out["max_gamma"] = float(gamma.max().item())
    tr.close()
    return out


def run_step(name, n, env=None):
    """Start a step as a child under its own time limit; returns its results, or None after a failure."""
    with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--step", name, tmp.name, "--n", str(n)]
        rc = subprocess.call(cmd, env=env)
        if rc != 0:
            print("backscatter_time: step %s ended with status %d -- nothing more is started" % (name, rc), flush=True)
            return None
        with open(tmp.name) as f:
            return json.load(f)


def main():
    arg = lambda flag, default=None: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else default    # noqa: E731
    n = int(arg("--n", N))
    if "--step" in sys.argv:
        i = sys.argv.index("--step")
        res = step(sys.argv[i + 1], n)
        with open(sys.argv[i + 2], "w") as f:
            json.dump(res, f)
        return 0
    parent = arg("--parent-lib")
    out = {"n": n, "nbeams": 60, "calls_per_repetition": CALLS, "repetitions": REPS}
    reps, failed = {}, False
    for _ in range(REPS):                      # interleaved: this build, the parent's, three times
        for name in ("new", "parent") if parent else ("new",):
            env = dict(os.environ, CBET_LIB_PATH=os.path.abspath(parent)) if name == "parent" else None
            res = None if failed else run_step(name, n, env)
            if res is None:
                failed = True
                break
            for case, v in res.items():
                if isinstance(v, dict) and "median" in v:
                    reps.setdefault(("parent_" if name == "parent" else "") + case, []).append(v)
                else:
                    out.setdefault(name, {})[case] = v
        if failed:
            break
    out["ms"] = {k: spread(rr) for k, rr in reps.items()}
    base = out["ms"].get("parent_exit_gain") or out["ms"].get("exit_gain")
    if base:
        out["ratio_to_exit_pass"] = {k: v["mean_of_medians_ms"] / base["mean_of_medians_ms"] for k, v in out["ms"].items()}
        out["ratio_base"] = "parent_exit_gain" if "parent_exit_gain" in out["ms"] else "exit_gain"
    out["complete"] = not failed
    line = json.dumps(out)
    print(line)
    path = arg("--out", os.path.join(ROOT, "profiles", "backscatter", "backscatter_time.json"))
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
