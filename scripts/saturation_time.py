"""Times the saturation clamp of the CBET gain kernels and the amplitude map at 256^3, 60 beams, with
HIP events, nothing running beside the kernels; three interleaved repetitions of 20 calls each, reported as the mean of the
repetitions' medians and their spread (largest minus smallest median):
  * k_gain_field_sym with frozen directions -- the call the CBET iteration repeats -- on the fields of a real field pass with
    the ramp's closed-form flow: without a limit, with dn_max at the median of that field's own amplitude map (half of the
    cells with a pair hold a clamped pair) and at half its smallest non-zero value (every such cell does);
  * the same call without a limit on a build of the PARENT commit (--parent-lib FILE, loaded through CBET_LIB_PATH);
  * k_pair_amplitude over the whole grid.
A repetition is one child process per build, this build's and the parent's in turn.
  * --solve: section 16's experiment again -- 60 beams, 128^3 (--solve-n N), the s83177 profile as a 1-D mesh with Ti = Te / 2
    and Z = 3.1, relax 0.5, 40 passes at the most: the local state without a limit and with dn_max at the 50th, 90th and 99th
    percentile of the amplitude map of the UNIFORM-state solve.  Recorded, not judged.
Every GPU step is a child process under its own `timeout`; the first failure ends the run and nothing more is started.
Writes profiles/saturation/saturation_time.json (or --out FILE).
usage: python scripts/saturation_time.py [--parent-lib FILE] [--solve] [--solve-n N] [--out FILE]"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, CALLS, REPS = 256, 20, 3
LIMITS = {"gain": 300, "parent": 300, "solve": 900}         # seconds a step may take (set-up of 50 GB included)
NEW = ("cbet_context_set_saturation", "cbet_context_saturation", "cbet_pair_amplitude")


def summary(ts):
    import numpy as np
    return {"min": float(np.min(ts)), "median": float(np.median(ts)), "max": float(np.max(ts))}


def timed(torch, fn, reps, before=None):
    ts = []
    for i in range(reps + 1):                  # the first call is the warm-up
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i > 0:
            ts.append(a.elapsed_time(b))
    return ts


def spread(rr):
    med = [x["median"] for x in rr]
    return {"mean_of_medians_ms": sum(med) / len(med), "spread_ms": max(med) - min(med), "repetitions": rr}


def load_older_library(api):
    """The parent's build lacks this commit's three entries: api.lib() gets no-ops in their place while it loads (a limit of
    zero is what the parent computes anyway), everything else is the library's own."""
    import ctypes

    class Absent:
        argtypes = restype = None

        def __call__(self, *args):
            return 0

    class Older:
        def __init__(self, *args, **kwargs):
            self.__dict__["_lib"] = real(*args, **kwargs)

        def __getattr__(self, name):
            try:
                return getattr(self._lib, name)
            except AttributeError:
                if name not in NEW:
                    raise
                self.__dict__[name] = Absent()
                return self.__dict__[name]

    real = ctypes.CDLL
    ctypes.CDLL = Older
    try:
        api.lib()
    finally:
        ctypes.CDLL = real


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
        load_older_library(api)
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

    out = {"library": os.path.relpath(os.path.abspath(api.LIB_PATH), ROOT)}
    if name == "parent":
        out["no_limit"] = summary(timed(torch, update, CALLS, before=fresh))
        tr.close()
        return out
    fresh()
    update()                                   # normalised fields of the energy the timed calls see
    amp = tr.pair_amplitude(fields, gp)
    nz = amp[amp > 0]
    limits = {"half": float(nz.median()), "all": 0.5 * float(nz.min())}
    out["amplitude_map"] = {"cells": int(amp.numel()), "non_zero_cells": int(nz.numel()), "min": float(nz.min()),
                            "p50": limits["half"], "p90": float(torch.quantile(nz[:: max(1, nz.numel() // 4000000)], 0.9)),
                            "max": float(nz.max())}
    out["dn_max"] = limits
    for case, dn in (("no_limit", 0.0), ("half", limits["half"]), ("all", limits["all"])):
        tr.set_saturation(dn)
        out[case] = summary(timed(torch, update, CALLS, before=fresh))
        if dn > 0:                             # how far the limit moves one update from a zero gain
            steps = []
            for lim in (dn, 0.0):
                tr.set_saturation(lim)
                steps.append(torch.zeros_like(gain))
                fresh()
                tr.gain_field(fields, steps[-1], gp, None, pair_once=True, frozen=True)
            out[case]["max_change_of_max_gain"] = float((steps[0] - steps[1]).abs().max() / steps[1].abs().max())
            del steps
    tr.set_saturation(0.0)
    fresh()
    update()
    out["pair_amplitude"] = summary(timed(torch, lambda: tr.pair_amplitude(fields, gp, out=amp), CALLS))
    tr.close()
    return out


def solve(np, api, RayTracer, bn, r, ne, te, n):
    gp = api.default_gain_params(relax=0.5, max_passes=40)
    tr = RayTracer(api.default_params(n), r, ne, te, beam_norm=bn)
    cs = api.gain_constants(tr.params, gp)[1]
    t = np.clip((r - gp.mach_r0) / (gp.mach_r1 - gp.mach_r0), 0.0, 1.0)
    ramp = (gp.mach_0 + (gp.mach_1 - gp.mach_0) * t) * cs
    tr.set_plasma_mesh(r, None, None, ne, te, (ramp, None, None), (0.0, 0.0, 0.0), ti=0.5 * te)
    tr.set_flow("mesh")
    out = {"n": n, "nbeams": 60, "ti": "Te / 2", "z": gp.z_ion, "relax": gp.relax, "max_passes": gp.max_passes, "runs": {}}

    def run(label, fields=None):
        edep = tr.new_grid()
        rep = tr.cbet_solve(edep, gp, fields=fields)
        tally = tr.energy_balance(tr.trace_exits(tr.new_exits(), gain=rep["gain"], gain_params=gp)).cpu().numpy()
        launched, gained, absorbed = tally[:, 0], tally[:, 1], tally[:, 2]
        rel = gained / launched
        out["runs"][label] = {"dn_max": tr.saturation, "passes": int(rep["passes"]), "converged": bool(rep["converged"]),
                              "imbalance": float(rep["imbalance"]), "absorbed_fraction": float(absorbed.sum() / launched.sum()),
                              "beam_gain_over_launched": {"min": float(rel.min()), "max": float(rel.max()), "std": float(rel.std())}}
        print("saturation_time: solve %s: %s" % (label, json.dumps(out["runs"][label])), flush=True)

    fields = tr.new_fields()
    run("uniform_state", fields)
    amp = tr.pair_amplitude(fields, gp)
    del fields
    nz = np.sort(amp[amp > 0].cpu().numpy())
    out["uniform_state_amplitude_map"] = {"non_zero_cells": int(nz.size), "p50": float(np.percentile(nz, 50)),
                                          "p90": float(np.percentile(nz, 90)), "p99": float(np.percentile(nz, 99)), "max": float(nz[-1])}
    tr.set_gain_state("mesh")
    run("local_state_no_limit")
    for q in (99, 90, 50):
        tr.set_saturation(float(np.percentile(nz, q)))
        run("local_state_p%d" % q)
    tr.close()
    return out


def run_step(name, solve_n, env=None):
    """Start a step as a child under its own time limit; returns its results, or None after a failure."""
    with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--step", name, tmp.name,
               "--solve-n", str(solve_n)]
        rc = subprocess.call(cmd, env=env)
        if rc != 0:
            print("saturation_time: step %s ended with status %d -- nothing more is started" % (name, rc), flush=True)
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
    out["k_gain_field_sym_frozen_ms"] = {k: spread(rr) for k, rr in reps.items() if k != "pair_amplitude"}
    if "pair_amplitude" in reps:
        out["k_pair_amplitude_ms"] = spread(reps["pair_amplitude"])
    if "--solve" in sys.argv and not failed:
        res = run_step("solve", solve_n)
        failed = res is None
        if res is not None:
            out["solve"] = res
    out["complete"] = not failed
    line = json.dumps(out)
    print(line)
    path = arg("--out", os.path.join(ROOT, "profiles", "saturation", "saturation_time.json"))
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
