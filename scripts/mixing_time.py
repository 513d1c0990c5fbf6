#!/usr/bin/env python3
"""Times the Anderson-mixing kernels on one gain stack of the 256^3 / 60-beam solve and records what
mixing does to three solves.

  * kernels: n = 60 * 258^3 doubles per array (8.24 GB), random contents, HIP events, nothing running beside the kernels,
    medians of 10 calls: a device-to-device copy of one array (the yardstick of the SAME run), k_mix_residual + k_mix_reduce
    with 0 .. 4 held residuals, k_mix_apply over 1 .. 5 entries (x_out and x_keep both written).  Every kernel's time is set
    against its compulsory bytes at the measured copy rate; the goal is a ratio of 1.25 or less, MISSED is reported as such.
  * headline: the 256^3 / 60-beam solve with default gain parameters at depth 0 .. 4: passes, convergence, wall time.
  * state: section 16's solve at 128^3 (--solve-n N) -- the s83177 profile as a 1-D mesh, local Te, Ti = Te / 2, Z = 3.1, no
    saturation, relax 0.5, 40 passes at the most -- at depth 0 and 3.
  * colours: section 19's three-colour scheme (-3, 0, +3 Angstrom by beam mod 3) without a line spectrum at 128^3, depth 0 and 3.
The solves are recorded, not judged.  Every GPU step is a child process under its own `timeout`; the first failure ends the
run and nothing more is started.  Writes profiles/mixing/mixing_time.json (or --out FILE).
usage: python scripts/mixing_time.py [--steps kernels,headline,state,colours] [--solve-n N] [--out FILE]"""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from saturation_time import summary, timed  # noqa: E402

N, CALLS = 256, 10
STEPS = ("kernels", "headline", "state", "colours")
LIMITS = {"kernels": 300, "headline": 420, "state": 300, "colours": 300}
GOAL = 1.25


def kernels(torch, api):
    n = 60 * (N + 2) ** 3
    arrays = [torch.randn(n, dtype=torch.float64, device="cuda") for _ in range(8)]
    row = torch.zeros(api.MIX_MAX_DEPTH + 1, dtype=torch.float64, device="cuda")
    work = torch.empty(api.mix_work_bytes(n) // 8, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    out = {"n": n, "array_bytes": 8 * n}
    out["copy"] = summary(timed(torch, lambda: arrays[1].copy_(arrays[0]), CALLS))
    rate = 2 * 8 * n / (out["copy"]["median"] * 1e-3)               # bytes / s, read + write
    out["copy"]["TB_s"] = rate / 1e12

    def judged(ts, stacks):
        s = summary(ts)
        s["compulsory_bytes"] = 8 * n * stacks
        s["ms_at_copy_rate"] = 8 * n * stacks / rate * 1e3
        s["ratio"] = s["median"] / s["ms_at_copy_rate"]
        s["goal_%.2f" % GOAL] = "met" if s["ratio"] <= GOAL else "MISSED"
        return s

    y, x, f, held = arrays[0], arrays[1], arrays[2], arrays[3:7]
    out["residual"] = {str(h): judged(timed(torch, lambda: api.mix_residual(y, x, f, held[:h], row, work), CALLS), 3 + h)
                       for h in range(api.MIX_MAX_DEPTH + 1)}
    ys, x_out, x_keep = arrays[:5], arrays[5], arrays[6]
    alpha = [0.1, -0.2, 0.3, 0.35, 0.45]
    out["apply"] = {str(c): judged(timed(torch, lambda: api.mix_apply(ys[:c], alpha[:c], x_out, x_keep), CALLS), c + 2)
                    for c in range(1, api.MIX_MAX_DEPTH + 2)}
    # one mixed pass at depth 3 when the history is full: residual against 3 held, apply over 4 entries
    out["pass_depth3"] = {"stacks": (3 + 3) + (4 + 2), "ms": out["residual"]["3"]["median"] + out["apply"]["4"]["median"]}
    return out


def solve_record(torch, tr, gp, depth, **kw):
    edep = tr.new_grid()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rep = tr.cbet_solve(edep, gp, mixing=depth, **kw)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    rec = {"depth": depth, "passes": int(rep["passes"]), "converged": bool(rep["converged"]), "change": float(rep["change"]),
           "imbalance": float(rep["imbalance"]), "wall_s": wall}
    if "mixing" in rep:
        m = rep["mixing"]
        rec.update(restarts=m["restarts"], dropped=m["dropped"], held=m["held"], residual_l2=m["residual_l2"], alpha=m["alpha"],
                   bytes_held=m["bytes"])
    del rep, edep
    return rec


def step(name, solve_n):
    """One GPU step, in this process: a dict of results."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import load_inputs
    from cbet_raytracing_3d_amd import api
    from cbet_raytracing_3d_amd.tracer import RayTracer
    if name == "kernels":
        return kernels(torch, api)
    bn, r, ne, te = load_inputs()
    out = {"runs": []}

    def run(tr, gp, depth, **kw):
        out["runs"].append(solve_record(torch, tr, gp, depth, **kw))
        print("mixing_time: %s: %s" % (name, json.dumps(out["runs"][-1])), flush=True)

    if name == "headline":
        gp = api.default_gain_params()
        tr = RayTracer(api.default_params(N), r, ne, te, beam_norm=bn)
        out.update(n=N, nbeams=60, relax=gp.relax, tolerance=gp.tolerance, max_passes=gp.max_passes)
        fields = tr.new_fields()
        solve_record(torch, tr, gp, 0, fields=fields)              # warm-up: allocations, the step records, the first launches
        for depth in range(api.MIX_MAX_DEPTH + 1):
            run(tr, gp, depth, fields=fields)
        tr.close()
        return out
    gp = api.default_gain_params(relax=0.5, max_passes=40)
    tr = RayTracer(api.default_params(solve_n), r, ne, te, beam_norm=bn)
    out.update(n=solve_n, nbeams=60, relax=gp.relax, tolerance=gp.tolerance, max_passes=gp.max_passes)
    if name == "state":                                            # scripts/saturation_time.py's local state, no limit
        cs = api.gain_constants(tr.params, gp)[1]
        t = np.clip((r - gp.mach_r0) / (gp.mach_r1 - gp.mach_r0), 0.0, 1.0)
        ramp = (gp.mach_0 + (gp.mach_1 - gp.mach_0) * t) * cs
        tr.set_plasma_mesh(r, None, None, ne, te, (ramp, None, None), (0.0, 0.0, 0.0), ti=0.5 * te)
        tr.set_flow("mesh")
        tr.set_gain_state("mesh")
    else:                                                          # scripts/detuning_time.py's three colours, no lines
        tr.set_detuning(dlambda_angstrom=[3.0 * ((b % 3) - 1.0) for b in range(tr.params.nbeams)])
    for depth in (0, 3):
        run(tr, gp, depth)
    tr.close()
    return out


def run_step(name, solve_n):
    """Start a step as a child under its own time limit; returns its results, or None after a failure."""
    with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--step", name, tmp.name,
               "--solve-n", str(solve_n)]
        rc = subprocess.call(cmd)
        if rc != 0:
            print("mixing_time: step %s ended with status %d -- nothing more is started" % (name, rc), flush=True)
            return None
        with open(tmp.name) as f:
            return json.load(f)


def main():
    arg = lambda flag, default=None: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else default    # noqa: E731
    solve_n = int(arg("--solve-n", 128))
    if "--step" in sys.argv:
        i = sys.argv.index("--step")
        res = step(sys.argv[i + 1], solve_n)
        with open(sys.argv[i + 2], "w") as f:
            json.dump(res, f)
        return 0
    out, failed = {"n": N, "nbeams": 60, "calls": CALLS}, False
    for name in arg("--steps", ",".join(STEPS)).split(","):
        res = run_step(name, solve_n)
        if res is None:
            failed = True
            break
        out[name] = res
    out["complete"] = not failed
    line = json.dumps(out)
    print(line)
    path = arg("--out", os.path.join(ROOT, "profiles", "mixing", "mixing_time.json"))
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
