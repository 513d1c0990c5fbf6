"""Times the deposit on the hydro mesh (cbet_mesh_deposit_device) at 256^3 with HIP events, nothing
running beside it.  The grids are the 60 per-beam grids of one plain pass over the s83177 plasma (and their sum, the one
grid); the cells are the dual cells of the s83177 profile's 443 radii alone (443 x 1 x 1) and with 32 x 64 angles.
Configurations: S = 1, 2, 4; one grid and the stack of 60; the global-atomics arm and the LDS arm (where it fits), plus
what the automatic choice takes.  In the same process, the two yardsticks: cbet_sph_modes_device at lmax 0 on the one
grid with 32 shells (the existing per-node binning of that grid) and cbet_tabulate_mesh on the same two meshes.  All of
them as interleaved repetitions of `calls` calls each, so that differences can be read against the spread; a
configuration whose warm-up call takes longer than 200 ms is timed with 5 calls.  Also recorded, not judged: the radial
heating profile of the pass on the 443 x 1 x 1 cells and its conservation residual.  One JSON line.
usage: python scripts/mesh_deposit_time.py [--calls C] [--repetitions R] [--n N] [--only TEXT] [--out FILE]
(defaults 20, 3, 256; --only: the configurations whose name contains one of the comma-separated TEXTs, for a counter run)"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_inputs  # noqa: E402
from cbet_raytracing_3d_amd import api, modes  # noqa: E402
from cbet_raytracing_3d_amd.tracer import RayTracer  # noqa: E402

UM = 1e-4
CENTER = (0.0, 0.0, 10 * UM)
NTH, NPH = 32, 64


def option(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()                                       # warm-up, and the call that decides how many are timed
    b.record()
    torch.cuda.synchronize()
    if a.elapsed_time(b) > 200.0:
        calls = min(calls, 5)
    ts = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return {"min": float(np.min(ts)), "median": float(np.median(ts)), "max": float(np.max(ts)), "calls": calls}


def angles():
    edges = np.linspace(0.0, np.pi, NTH + 1)
    return 0.5 * (edges[1:] + edges[:-1]), -np.pi + 2.0 * np.pi * (np.arange(NPH) + 0.5) / NPH


def main():
    n = option("--n", 256)
    bn, r, ne, te = load_inputs()
    tr = RayTracer(api.default_params(n), r, ne, te, beam_norm=bn)
    p, dev, gpu = tr.params, tr.device, tr.gpu
    stream = torch.cuda.current_stream().cuda_stream
    stack = tr.new_grid(per_beam=True)
    tr.launch(stack)
    one = stack.sum(dim=0)
    torch.cuda.synchronize()
    G, hsize = stack.shape[0], int(np.prod(tr.grid_shape))
    theta, phi = angles()
    cells = {"443x1x1": api.MeshCells.from_nodes(r, None, None, CENTER, gpu=gpu),
             "443x%dx%d" % (NTH, NPH): api.MeshCells.from_nodes(r, theta, phi, CENTER, gpu=gpu)}
    wobble = 1.0 + 0.05 * np.cos(2 * theta)[None, :, None] + 0.03 * (np.sin(theta)[None, :, None] * np.cos(3 * phi)[None, None, :])
    meshes = {"443x1x1": api.Mesh(r, None, None, ne, te, None, CENTER).to(dev),
              "443x%dx%d" % (NTH, NPH): api.Mesh(r, theta, phi, ne[:, None, None] * wobble, te[:, None, None] * wobble, None,
                                                  CENTER).to(dev)}
    f64 = dict(dtype=torch.float64, device=dev)
    shells = np.ascontiguousarray(modes.default_shells(p, 32), dtype=np.float64)
    sph_out = (torch.empty((1, 32, 1), **f64), torch.empty((1, 32), **f64), torch.empty(32, dtype=torch.int64, device=dev))
    runs = {"sph_modes_lmax0_32shells": lambda: api.sph_modes(one, 1, 0, p, CENTER, shells, 0, *sph_out, stream)}
    for name, m in meshes.items():
        runs["tabulate_mesh_" + name] = lambda m=m: api.tabulate_mesh(tr.ctx, p, m, stream)
    fits, auto = {}, {}
    for cname, c in cells.items():
        for grids, edep, ng, stride in (("1grid", one, 1, 0), ("%dgrids" % G, stack, G, hsize)):
            out = (torch.empty((ng,) + c.shape, **f64), torch.empty(ng, **f64), torch.empty(c.shape, dtype=torch.int64, device=dev))
            key = "%s_%s" % (cname, grids)
            try:                                   # the entry point refuses an LDS arm that does not fit before any device work
                api.mesh_deposit(c, edep, ng, stride, p, 1, api.MESH_DEPOSIT_LDS, *out, stream)
                fits[key] = True
            except api.CbetError:
                fits[key] = False
            auto[key] = "lds" if fits[key] else "global"      # the rule of cbet_mesh_deposit_device: the LDS arm where it fits
            for S in (1, 2, 4):
                for arm, method in (("global", api.MESH_DEPOSIT_GLOBAL), ("lds", api.MESH_DEPOSIT_LDS)):
                    if arm == "lds" and not fits[key]:
                        continue
                    runs["deposit_%s_S%d_%s" % (key, S, arm)] = (
                        lambda c=c, edep=edep, ng=ng, stride=stride, S=S, method=method, out=out:
                        api.mesh_deposit(c, edep, ng, stride, p, S, method, *out, stream))
    torch.cuda.synchronize()
    if "--only" in sys.argv:
        wanted = sys.argv[sys.argv.index("--only") + 1].split(",")
        runs = {name: fn for name, fn in runs.items() if any(w in name for w in wanted)}
    calls = option("--calls", 20)
    res = {"n": n, "nodes_haloed": hsize, "grids": G, "calls_per_repetition": calls, "lds_arm_fits": fits, "auto_takes": auto}
    reps = {name: [] for name in runs}
    for _ in range(option("--repetitions", 3)):
        for name, fn in runs.items():
            reps[name].append(timed(fn, calls))
    res["interleaved_ms"] = reps
    for name, rr in reps.items():
        med = [x["median"] for x in rr]
        res[name + "_ms"] = float(np.mean(med))
        res[name + "_spread_ms"] = float(max(med) - min(med))
    # the radial heating profile of the pass and its conservation residual (S = 2, the automatic arm)
    c = cells["443x1x1"]
    e, o, s = tr.deposit_on_mesh(one, c, subsamples=2)
    eb, ob, _ = tr.deposit_on_mesh(stack, c, subsamples=2)
    torch.cuda.synchronize()
    d = api.derive(p)
    volume = s.double() * (d.dx * d.dy * d.dz / 8.0)
    total = float(one.sum())
    res["radial_profile"] = {
        "r_edges_cm": c.r_edges.tolist(),
        "cell_energy": e.reshape(-1).tolist(),
        "cell_samples": s.reshape(-1).tolist(),
        "energy_per_cm3": torch.where(volume > 0, e / volume.clamp_min(1e-300), torch.zeros_like(e)).reshape(-1).tolist(),
        "outside": float(o), "grid_sum": total,
        "conservation_residual": abs(float(e.sum()) + float(o) - total) / total,
        "per_beam_conservation_residual_max": float(((eb.sum(dim=(1, 2, 3)) + ob - stack.sum(dim=(1, 2, 3))).abs()
                                                     / stack.sum(dim=(1, 2, 3))).max()),
    }
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")
    for c in cells.values():
        c.close()
    tr.close()


if __name__ == "__main__":
    main()
