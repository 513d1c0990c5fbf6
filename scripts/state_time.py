"""Times the local plasma state of the CBET gain kernels (cbet_tabulate_mesh_state) at 256^3 with HIP
events, nothing running beside the kernels, three interleaved repetitions of 20 calls each:
  * producer: k_mesh_state for the 443 x 1 x 1 mesh (the s83177 profile) and for a 443 x 32 x 64 mesh, beside
    k_tabulate_mesh and k_mesh_flow on the same meshes in the same process;
  * gain: k_gain_field_sym with frozen directions -- the call the CBET iteration repeats -- at 60 beams on the fields of a
    real field pass, with the mesh's flow table selected, without and with the mesh's state table, in the same process;
  * solve: a 60-beam solve (128^3 by default, --solve-n N) with the s83177 profile fed as a 1-D mesh, once with the uniform
    state of the gain parameters and once with the local state (Ti = Te / 2, Z = 3.1): passes, absorbed fraction and the
    spread of what the beams gain.  Recorded, not judged.
Every GPU step is a child process under its own `timeout`; the first failure ends the run and nothing more is started.
Writes profiles/state/state_time.json (or --out FILE).
usage: python scripts/state_time.py [--solve-n N] [--out FILE]"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UM = 1e-4
N, CALLS, REPS = 256, 20, 3
LIMITS = {"producer": 240, "gain": 420, "solve": 420}       # seconds a step may take (set-up of 50 GB included)


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


def meshes(api, np, r, ne, te, gp, p):
    """The s83177 profile as a 1-D mesh and spread over 32 x 64 angles with a smooth modulation, each with the ramp's velocity,
    Ti = Te / 2 and a mean charge that follows Te."""
    cs = api.gain_constants(p, gp)[1]
    t = np.clip((r - gp.mach_r0) / (gp.mach_r1 - gp.mach_r0), 0.0, 1.0)
    ur = (gp.mach_0 + (gp.mach_1 - gp.mach_0) * t) * cs
    zbar = 1.0 + 2.5 * te / te.max()
    centre = (0.0, 0.0, 10 * UM)
    nth, nph = 32, 64
    edges = np.linspace(0.0, np.pi, nth + 1)
    theta = 0.5 * (edges[1:] + edges[:-1])
    phi = -np.pi + 2.0 * np.pi * np.arange(nph) / nph
    _, T, P = np.meshgrid(r, theta, phi, indexing="ij")
    wobble = 1.0 + 0.05 * np.cos(2 * T) + 0.03 * np.sin(T) * np.cos(3 * P)
    full = lambda f: f[:, None, None] * wobble                                  # noqa: E731
    return {"mesh_1d": api.Mesh(r, None, None, ne, te, (ur, None, None), centre, ti=0.5 * te, zbar=zbar),
            "mesh_3d": api.Mesh(r, theta, phi, full(ne), full(te), (full(ur), 0.05 * full(ur) * np.sin(2 * T), 0.05 * full(ur) * np.sin(P)),
                                centre, ti=0.5 * full(te), zbar=full(zbar))}


def step(name, solve_n):
    """One GPU step, in this process: a dict of results."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import load_inputs
    from cbet_raytracing_3d_amd import api
    from cbet_raytracing_3d_amd.tracer import RayTracer
    bn, r, ne, te = load_inputs()
    gp = api.default_gain_params()
    if name == "solve":
        tr = RayTracer(api.default_params(solve_n), r, ne, te, beam_norm=bn)
        mesh = meshes(api, np, r, ne, te, gp, tr.params)["mesh_1d"]
        ramp = mesh._keep[5]
        tr.set_plasma_mesh(r, None, None, ne, te, (ramp, None, None), (0.0, 0.0, 0.0), ti=0.5 * te)
        tr.set_flow("mesh")
        out = {"n": solve_n, "nbeams": 60, "ti": "Te / 2", "z": gp.z_ion,
               "uniform_state_ev": {"te_ev": gp.te_ev, "ti_ev": gp.ti_ev, "z_ion": gp.z_ion}}
        for mode in (None, "mesh"):
            tr.set_gain_state(mode)
            edep = tr.new_grid()
            rep = tr.cbet_solve(edep, gp)
            tally = tr.energy_balance(tr.trace_exits(tr.new_exits(), gain=rep["gain"], gain_params=gp)).cpu().numpy()
            launched, gained, absorbed = tally[:, 0], tally[:, 1], tally[:, 2]
            rel = gained / launched
            out["local_state" if mode else "uniform_state"] = {
                "passes": int(rep["passes"]), "converged": bool(rep["converged"]), "imbalance": float(rep["imbalance"]),
                "absorbed_fraction": float(absorbed.sum() / launched.sum()),
                "beam_gain_over_launched": {"min": float(rel.min()), "max": float(rel.max()), "std": float(rel.std())}}
            del rep, edep
        tr.close()
        return out
    tr = RayTracer(api.default_params(N), r, ne, te, beam_norm=bn)
    p = tr.params
    stream = torch.cuda.current_stream().cuda_stream
    host = meshes(api, np, r, ne, te, gp, p)
    for m in host.values():
        api.mesh_check(m)
    dev = {k: m.to(tr.device) for k, m in host.items()}
    out = {"meshes": {k: list(m.shape) for k, m in host.items()}}
    if name == "producer":
        runs = {}
        for k, m in dev.items():
            runs[k + "_tables"] = lambda m=m: api.tabulate_mesh(tr.ctx, p, m, stream)
            runs[k + "_flow"] = lambda m=m: api.tabulate_mesh_flow(tr.ctx, p, m, stream)
            runs[k + "_state"] = lambda m=m: api.tabulate_mesh_state(tr.ctx, p, gp, m, stream)
        reps = {k: [] for k in runs}
        for _ in range(REPS):                  # interleaved: A B C D E F, three times
            for k, fn in runs.items():
                reps[k].append(summary(timed(torch, fn, CALLS)))
        out["interleaved_ms"] = {k: spread(rr) for k, rr in reps.items()}
        out["bytes_stored_per_node"] = {"tables": 16, "flow": 24, "state": 16}
        tr.close()
        return out
    # gain: the 1-D mesh's tables and flow, fields of a real field pass, then frozen updates without / with the state table
    keep, ions = host["mesh_1d"]._keep, host["mesh_1d"]._ions
    tr.set_plasma_mesh(keep[0], None, None, keep[3], keep[4], keep[5:], tuple(host["mesh_1d"].center), ti=ions[0], zbar=ions[1])
    mesh = tr.mesh
    tr.set_flow("mesh")
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
            api.tabulate_mesh_state(tr.ctx, p, gp, mesh, stream)
        else:
            tr.ctx.set_state(None)

    reps = {"no_state_table": [], "state_table": []}
    for _ in range(REPS):                      # interleaved: A B A B A B
        for m in reps:
            with_table(m == "state_table")
            reps[m].append(summary(timed(torch, update, CALLS, before=fresh)))
    with_table(False)
    out["k_gain_field_sym_frozen_mesh_flow_ms"] = {m: spread(rr) for m, rr in reps.items()}
    tr.close()
    return out


def run_step(name, solve_n):
    """Start a step as a child under its own time limit; returns its results, or None after a failure."""
    with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--step", name, tmp.name,
               "--solve-n", str(solve_n)]
        rc = subprocess.call(cmd)
        if rc != 0:
            print("state_time: step %s ended with status %d -- nothing more is started" % (name, rc), flush=True)
            return None
        with open(tmp.name) as f:
            return json.load(f)


def main():
    solve_n = int(sys.argv[sys.argv.index("--solve-n") + 1]) if "--solve-n" in sys.argv else 128
    if "--step" in sys.argv:
        i = sys.argv.index("--step")
        res = step(sys.argv[i + 1], solve_n)
        with open(sys.argv[i + 2], "w") as f:
            json.dump(res, f)
        return 0
    out = {"n": N, "nbeams": 60, "calls_per_repetition": CALLS, "repetitions": REPS}
    failed = False
    for name in ("producer", "gain", "solve"):
        res = run_step(name, solve_n)
        if res is None:
            failed = True
            break
        out[name] = res
    out["complete"] = not failed
    line = json.dumps(out)
    print(line)
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "state", "state_time.json")
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
