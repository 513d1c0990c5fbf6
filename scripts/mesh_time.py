"""Times the hydro-mesh kernels (cbet_tabulate_mesh, cbet_tabulate_mesh_flow) at 256^3 with HIP
events, nothing running beside them: for a 443 x 32 x 64 mesh and for a 1-D mesh (the s83177 profile), against the two
yardsticks k_tabulate (cbet_tabulate_plasma) and the lmax-0 k_tabulate_target in the same process -- all six as three
interleaved repetitions of 20 calls each, so that their differences can be read against their spread.  It also states the
bytes each kernel has to move (16 B per node written by the table kernel, 24 B by the flow kernel, plus the mesh read
once).  One JSON line.
usage: python scripts/mesh_time.py [--calls C] [--repetitions R] [--out FILE]      (defaults 20 and 3; fewer for a counter run)"""
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

UM = 1e-4
N = 256


def option(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn, reps):
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


def summary(ts):
    return {"min": float(np.min(ts)), "median": float(np.median(ts)), "max": float(np.max(ts))}


def mesh_3d(r, ne, te, gp, p):
    """The s83177 profile spread over 32 x 64 angles with a smooth angular modulation, and a velocity with all three
    components."""
    nth, nph = 32, 64
    edges = np.linspace(0.0, np.pi, nth + 1)
    theta = 0.5 * (edges[1:] + edges[:-1])
    phi = -np.pi + 2.0 * np.pi * np.arange(nph) / nph
    _, T, P = np.meshgrid(r, theta, phi, indexing="ij")
    wobble = 1.0 + 0.05 * np.cos(2 * T) + 0.03 * np.sin(T) * np.cos(3 * P)
    cs = api.gain_constants(p, gp)[1]
    t = np.clip((r - gp.mach_r0) / (gp.mach_r1 - gp.mach_r0), 0.0, 1.0)
    ur = ((gp.mach_0 + (gp.mach_1 - gp.mach_0) * t) * cs)[:, None, None] * wobble
    return api.Mesh(r, theta, phi, ne[:, None, None] * wobble, te[:, None, None] * wobble,
                    (ur, 0.05 * ur * np.sin(2 * T), 0.05 * ur * np.sin(P)), (0.0, 0.0, 10 * UM))


def main():
    bn, r, ne, te = load_inputs()
    tr = RayTracer(api.default_params(N), r, ne, te, beam_norm=bn)
    p, gp = tr.params, api.default_gain_params()
    stream = torch.cuda.current_stream().cuda_stream
    cs = api.gain_constants(p, gp)[1]
    t = np.clip((r - gp.mach_r0) / (gp.mach_r1 - gp.mach_r0), 0.0, 1.0)
    host = {"mesh_3d": mesh_3d(r, ne, te, gp, p),
            "mesh_1d": api.Mesh(r, None, None, ne, te, ((gp.mach_0 + (gp.mach_1 - gp.mach_0) * t) * cs, None, None),
                                (0.0, 0.0, 10 * UM))}
    for m in host.values():
        api.mesh_check(m)
    dev = {name: m.to(tr.device) for name, m in host.items()}
    target = api.Target((0.0, 0.0, 10 * UM))
    runs = {"k_tabulate": lambda: api.tabulate_plasma(tr.ctx, p, tr.d_te, tr.d_r, tr.d_ne, stream),
            "target_lmax0": lambda: api.tabulate_target(tr.ctx, p, tr.d_te, tr.d_r, tr.d_ne, target, stream)}
    for name, m in dev.items():
        runs[name + "_tables"] = lambda m=m: api.tabulate_mesh(tr.ctx, p, m, stream)
        runs[name + "_flow"] = lambda m=m: api.tabulate_mesh_flow(tr.ctx, p, m, stream)
    nodes = N ** 3
    calls = option("--calls", 20)
    out = {"n": N, "nodes": nodes, "calls_per_repetition": calls, "meshes": {k: list(m.shape) for k, m in host.items()}}
    reps = {name: [] for name in runs}
    for _ in range(option("--repetitions", 3)):    # interleaved: A B C D E F, three times
        for name, fn in runs.items():
            reps[name].append(summary(timed(fn, calls)))
    out["interleaved_ms"] = reps
    for name, rr in reps.items():
        med = [x["median"] for x in rr]
        out[name + "_ms"] = float(np.mean(med))
        out[name + "_spread_ms"] = float(max(med) - min(med))
    for name, m in host.items():
        cells = int(np.prod(m.shape))
        coords = 8 * sum(m.shape)
        velocity = sum(a is not None for a in m._keep[5:])
        for kind, written, fields in (("tables", 16, 2), ("flow", 24, velocity)):
            compulsory = written * nodes + 8 * fields * cells + coords
            ms = out["%s_%s_ms" % (name, kind)]
            out["%s_%s_compulsory_bytes" % (name, kind)] = compulsory
            out["%s_%s_compulsory_GBps" % (name, kind)] = compulsory / (ms * 1e-3) / 1e9
    out["compulsory_bytes"] = "bytes written (16 B per node: tables; 24 B: flow) + the mesh's fields and coordinates read once"
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")
    tr.close()


if __name__ == "__main__":
    main()
