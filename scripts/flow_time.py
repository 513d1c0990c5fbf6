"""Times the flow table of the CBET gain kernels (cbet_tabulate_flow) at 256^3 with 60 beams, with
HIP events, nothing running beside it:
  * k_tabulate_flow for lmax 0, 2, 8 and 16 (20 calls each);
  * k_gain_field_sym<true, .> -- the pair-once kernel with frozen directions, the call the CBET iteration repeats -- on the
    fields of a real field pass, without a table (the closed-form ramp) and with the sphere's table selected (same bits),
    as three interleaved repetitions of 10 calls each, so that their difference can be read against their spread;
  * with --baseline LIB (another build of the library, e.g. the parent commit's gain kernels): the closed-form call in this
    library and in that one, three interleaved repetitions, each in a process of its own.
Every GPU step is a child process under its own `timeout`; the first failure ends the run and nothing more is started.
Writes profiles/flow/flow_time.json (or --out FILE).
usage: python scripts/flow_time.py [--baseline LIB] [--out FILE]"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UM = 1e-4
N, CALLS = 256, 10
LIMITS = {"tabulate": 240, "gain": 420, "closed": 420}      # seconds a step may take (set-up of 50 GB included)


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


def step(name):
    """One GPU step, in this process: a dict of results."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import load_inputs
    from cbet_raytracing_3d_amd import api
    from cbet_raytracing_3d_amd.tracer import RayTracer
    bn, r, ne, te = load_inputs()
    tr = RayTracer(api.default_params(N), r, ne, te, beam_norm=bn)
    stream = torch.cuda.current_stream().cuda_stream
    gp = api.default_gain_params()
    out = {}
    if name == "tabulate":
        rng = np.random.default_rng(1)
        for lmax in (0, 2, 8, 16):
            c = rng.standard_normal((lmax + 1) ** 2)
            c[: lmax * lmax] = 0.0             # only degree lmax: the instantiation asked for, whatever covers less
            t = api.Target((0.0, 0.0, 10 * UM), c * (0.02 / np.abs(c).sum()))
            out["k_tabulate_flow_lmax%d_ms" % lmax] = summary(timed(
                torch, lambda: api.tabulate_flow(tr.ctx, tr.params, gp, t, stream), 20))
        out["bytes_stored"] = 24 * N ** 3
        tr.close()
        return out
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

    def with_table(on):
        if on:
            api.tabulate_flow(tr.ctx, tr.params, gp, None, stream)
        else:
            tr.ctx.set_flow(None)

    modes = ["closed_form"] if name == "closed" else ["closed_form", "table"]
    reps = {m: [] for m in modes}
    for _ in range(3):                         # interleaved: A B A B A B
        for m in modes:
            with_table(m == "table")
            reps[m].append(summary(timed(torch, update, CALLS, before=fresh)))
    with_table(False)
    out["k_gain_field_sym_frozen_ms"] = reps
    out["library"] = os.environ.get("CBET_LIB_PATH") or "this build"
    tr.close()
    return out


def run_step(name, env=None):
    """Start a step as a child under its own time limit; returns its results, or None after a failure."""
    with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--step", name, tmp.name]
        rc = subprocess.call(cmd, env=env)
        if rc != 0:
            print("flow_time: step %s ended with status %d -- nothing more is started" % (name, rc), flush=True)
            return None
        with open(tmp.name) as f:
            return json.load(f)


def spread(rr):
    med = [x["median"] for x in rr]
    return {"mean_of_medians_ms": sum(med) / len(med), "spread_ms": max(med) - min(med), "repetitions": rr}


def main():
    if "--step" in sys.argv:
        i = sys.argv.index("--step")
        res = step(sys.argv[i + 1])
        with open(sys.argv[i + 2], "w") as f:
            json.dump(res, f)
        return 0
    out = {"n": N, "nbeams": 60, "calls_per_repetition": CALLS}
    baseline = sys.argv[sys.argv.index("--baseline") + 1] if "--baseline" in sys.argv else None
    plan = [("tabulate", None), ("gain", None)]
    if baseline:
        base_env = dict(os.environ, CBET_LIB_PATH=os.path.abspath(baseline))
        plan += [("closed", None), ("closed", base_env)] * 3
    failed = False
    pairs = {"this": [], "baseline": []}
    for name, env in plan:
        res = run_step(name, env)
        if res is None:
            failed = True
            break
        if name == "tabulate":
            out["tabulate"] = res
        elif name == "gain":
            out["gain_update"] = {m: spread(rr) for m, rr in res["k_gain_field_sym_frozen_ms"].items()}
        else:
            pairs["baseline" if env else "this"].append(res["k_gain_field_sym_frozen_ms"]["closed_form"][-1])
    if baseline and not failed:
        out["closed_form_against_baseline"] = {"baseline": os.path.basename(baseline),
                                               "note": "last of three repetitions of every process",
                                               **{k: spread(v) for k, v in pairs.items()}}
    out["complete"] = not failed
    line = json.dumps(out)
    print(line)
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "flow", "flow_time.json")
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
