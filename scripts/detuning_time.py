#!/usr/bin/env python3
"""Times wavelength detuning in the CBET gain stage at 256^3, 60 beams, frozen fields, with HIP events,
nothing running beside the kernels; three interleaved repetitions of 20 calls each, reported as the mean of the repetitions'
medians and their spread (largest minus smallest median):
  * k_gain_field_sym with frozen directions -- the call the CBET iteration repeats -- on the fields of a real field pass:
    without shifts, with three colours (-3, 0, +3 Angstrom by beam index mod 3) and with sixty distinct shifts
    (4.6e12 ((37 b mod 60) - 29.5) / 30 rad/s);
  * k_exchange_matrix (+ k_exchange_reduce) over the whole grid in the same three configurations;
  * both calls without shifts on a build of the PARENT commit (--parent-lib FILE, loaded through CBET_LIB_PATH).
A repetition is one child process per build, this build's and the parent's in turn.
  * --solve: tracer.cbet_solve at 128^3 (--solve-n N), 60 beams, relax 0.5, 40 passes at the most, without shifts and with the
    three-colour scheme: passes, convergence, imbalance and the absorbed fraction.  Recorded, not judged.
Every GPU step is a child process under its own `timeout`; the first failure ends the run and nothing more is started.
Writes profiles/detuning/detuning_time.json (or --out FILE).
usage: python scripts/detuning_time.py [--parent-lib FILE] [--solve] [--solve-n N] [--out FILE]"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from saturation_time import spread, summary, timed  # noqa: E402

N, CALLS, REPS = 256, 20, 3
LIMITS = {"gain": 300, "parent": 300, "solve": 600}         # seconds a step may take (set-up of 50 GB included)
NEW = ("cbet_context_set_detuning", "cbet_context_detuning", "cbet_exchange_matrix_host_shifted")
SCALE = 4.6e12


def colours(np, api, params):
    b = np.arange(params.nbeams)
    return {"no_shifts": None, "three_colours": api.wavelength_shift_to_domega(params, 3.0 * ((b % 3) - 1.0)),
            "sixty_shifts": SCALE * (((37 * b) % 60) - 29.5) / 30.0}


def step(name, solve_n):
    """One GPU step, in this process: a dict of results."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import load_inputs
    from cbet_raytracing_3d_amd import api
    from cbet_raytracing_3d_amd.tracer import RayTracer
    if name == "parent":
        api.lib(tolerate=NEW)                   # the parent's build lacks this commit's entries; it is only run without shifts
    bn, r, ne, te = load_inputs()
    if name == "solve":
        return solve(np, api, RayTracer, bn, r, ne, te, solve_n)
    gp = api.default_gain_params()
    tr = RayTracer(api.default_params(N), r, ne, te, beam_norm=bn)
    tr.tabulate()
    fields = tr.new_fields()
    tr.launch_cbet(fields, gp, fields=True)
    gain = tr.new_grid(per_beam=True)
    tr.gain_field(fields, gain, gp, None, pair_once=True)           # builds k; the timed calls are the frozen ones
    energy = tr.new_grid(per_beam=True)
    tr.launch_cbet(energy, gp, fields="energy", gain=gain)
    torch.cuda.synchronize()

    def fresh():                               # what a pass of the iteration hands the update: a fresh energy field
        fields[0].copy_(energy)

    def update():
        tr.gain_field(fields, gain, gp, None, pair_once=True, frozen=True)

    def matrix():
        tr.exchange_matrix(fields, gp, gross=True)

    out = {"library": os.path.relpath(os.path.abspath(api.LIB_PATH), ROOT)}
    for case, shift in colours(np, api, tr.params).items():
        if name == "parent" and shift is not None:
            continue
        if name != "parent":
            tr.set_detuning(domega=shift)
        out["gain_" + case] = summary(timed(torch, update, CALLS, before=fresh))
        fresh()
        update()                               # normalised fields for the matrix
        out["matrix_" + case] = summary(timed(torch, matrix, CALLS))
        if shift is not None:                  # how far the shifts move one update from a zero gain
            steps = []
            for w in (shift, None):
                tr.set_detuning(domega=w)
                steps.append(torch.zeros_like(gain))
                fresh()
                tr.gain_field(fields, steps[-1], gp, None, pair_once=True, frozen=True)
            out["gain_" + case]["max_change_of_max_gain"] = float((steps[0] - steps[1]).abs().max() / steps[1].abs().max())
            del steps
    tr.close()
    return out


def solve(np, api, RayTracer, bn, r, ne, te, n):
    gp = api.default_gain_params(relax=0.5, max_passes=40)
    tr = RayTracer(api.default_params(n), r, ne, te, beam_norm=bn)
    out = {"n": n, "nbeams": 60, "relax": gp.relax, "max_passes": gp.max_passes, "runs": {}}
    for label, shift in colours(np, api, tr.params).items():
        if label == "sixty_shifts":
            continue
        tr.set_detuning(domega=shift)
        edep = tr.new_grid()
        rep = tr.cbet_solve(edep, gp)
        tally = tr.energy_balance(tr.trace_exits(tr.new_exits(), gain=rep["gain"], gain_params=gp)).cpu().numpy()
        launched, gained, absorbed = tally[:, 0], tally[:, 1], tally[:, 2]
        rel = gained / launched
        out["runs"][label] = {"passes": int(rep["passes"]), "converged": bool(rep["converged"]), "imbalance": float(rep["imbalance"]),
                              "absorbed_fraction": float(absorbed.sum() / launched.sum()),
                              "beam_gain_over_launched": {"min": float(rel.min()), "max": float(rel.max()), "std": float(rel.std())}}
        print("detuning_time: solve %s: %s" % (label, json.dumps(out["runs"][label])), flush=True)
    tr.close()
    return out


def run_step(name, solve_n, env=None):
    """Start a step as a child under its own time limit; returns its results, or None after a failure."""
    with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--step", name, tmp.name,
               "--solve-n", str(solve_n)]
        rc = subprocess.call(cmd, env=env)
        if rc != 0:
            print("detuning_time: step %s ended with status %d -- nothing more is started" % (name, rc), flush=True)
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
    parent = arg("--parent-lib")
    out = {"n": N, "nbeams": 60, "calls_per_repetition": CALLS, "repetitions": REPS}
    reps, failed = {}, False
    for _ in range(REPS):                      # interleaved: this build, the parent's, three times
        for name in ("gain", "parent") if parent else ("gain",):
            env = dict(os.environ, CBET_LIB_PATH=os.path.abspath(parent)) if name == "parent" else None
            res = None if failed else run_step(name, solve_n, env)
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
    out["k_gain_field_sym_frozen_ms"] = {k.replace("gain_", ""): spread(rr) for k, rr in reps.items() if "gain_" in k}
    out["k_exchange_matrix_ms"] = {k.replace("matrix_", ""): spread(rr) for k, rr in reps.items() if "matrix_" in k}
    if "--solve" in sys.argv and not failed:
        res = run_step("solve", solve_n)
        failed = res is None
        if res is not None:
            out["solve"] = res
    out["complete"] = not failed
    line = json.dumps(out)
    print(line)
    path = arg("--out", os.path.join(ROOT, "profiles", "detuning", "detuning_time.json"))
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
