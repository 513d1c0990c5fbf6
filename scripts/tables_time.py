#!/usr/bin/env python3
"""The plain pass's preparation alone on the device: k_tabulate + k_step_table against k_plasma_records, HIP events around
each, nothing beside them.  Prints one JSON line (profiles/tables/tables_time.json).

    python scripts/tables_time.py [--n 256] [--reps 20]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_RATE = 6.29e12      # bench.py HBM_COPY_RATE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    from cbet_raytracing_3d_amd import api
    from cbet_raytracing_3d_amd.tracer import RayTracer
    r, ne, te = api.load_s83177()
    p = api.default_params(args.n)
    tr = RayTracer(p, r, ne, te)
    d = tr.derived
    stream = torch.cuda.current_stream().cuda_stream

    def two():
        api.tabulate_plasma(tr.ctx, p, tr.d_te, tr.d_r, tr.d_ne, stream)
        api.prepare_step_records(tr.ctx, p, None, None, d.xconst, d.yconst, d.zconst, stream)

    def tab():
        api.tabulate_plasma(tr.ctx, p, tr.d_te, tr.d_r, tr.d_ne, stream)

    def one():
        api.prepare_plasma(tr.ctx, p, tr.d_te, tr.d_r, tr.d_ne, d.xconst, d.yconst, d.zconst, stream)

    def timed(fn):
        ms = []
        for _ in range(args.reps + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms = sorted(ms[3:])
        return {"min_ms": ms[0], "median_ms": ms[len(ms) // 2], "max_ms": ms[-1]}

    nodes = args.n ** 3
    compulsory = nodes * (8 + 8 + 32)           # ne3d, kappa3d and the records written once; nothing read but the profile
    out = {"grid": args.n, "reps": args.reps, "k_tabulate": timed(tab), "k_tabulate+k_step_table": timed(two),
           "k_plasma_records": timed(one), "compulsory_bytes": compulsory}
    t = out["k_plasma_records"]["median_ms"] * 1e-3
    out["k_plasma_records"]["GBps_of_compulsory"] = compulsory / t / 1e9
    out["k_plasma_records"]["frac_of_copy_rate"] = compulsory / t / COPY_RATE
    t2 = out["k_tabulate+k_step_table"]["median_ms"] * 1e-3
    out["k_tabulate+k_step_table"]["GBps_of_traffic"] = nodes * (16 + 16 + 32) / t2 / 1e9
    print(json.dumps(out), flush=True)
    tr.close()


if __name__ == "__main__":
    main()
