"""Times the perturbed-target table kernel (cbet_tabulate_target) at 256^3 with HIP events, nothing
running beside it: the instantiations for lmax 0, 2, 8 and 16 and, as the yardstick, k_tabulate (cbet_tabulate_plasma) in
the same process -- k_tabulate and the lmax 0 instantiation as three interleaved repetitions of 20 calls each, so that
their difference can be read against their spread.  It also records (a record, not an assertion) how the plain 256^3 /
60-beam pass answers a displaced target: sigma_1 .. sigma_4 and sigma_rms (lmax 16, default shells, projected about the
origin) at offsets 0, 5, 10 and 20 um along z, and with a 1 % (2, 0) distortion.  One JSON line.
usage: python scripts/target_time.py [--no-physics] [--out FILE]"""
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


def timed(fn, reps=20):
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


def main():
    bn, r, ne, te = load_inputs()
    tr = RayTracer(api.default_params(256), r, ne, te, beam_norm=bn)
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(1)

    def target(lmax):
        if lmax == 0:
            return api.Target((0.0, 0.0, 10 * UM))
        c = rng.standard_normal((lmax + 1) ** 2)
        c[: lmax * lmax] = 0.0                 # only degree lmax: the instantiation asked for, whatever covers less
        return api.Target((0.0, 0.0, 10 * UM), c * (0.02 / np.abs(c).sum()))

    def run_target(t):
        return lambda: api.tabulate_target(tr.ctx, tr.params, tr.d_te, tr.d_r, tr.d_ne, t, stream)

    plain = tr.tabulate
    t0 = target(0)
    out = {"n": 256, "nodes": 256 ** 3, "bytes_stored": 16 * 256 ** 3, "calls_per_repetition": 20}
    reps = {"k_tabulate": [], "target_lmax0": []}
    for _ in range(3):                         # interleaved: A B A B A B
        reps["k_tabulate"].append(summary(timed(plain)))
        reps["target_lmax0"].append(summary(timed(run_target(t0))))
    out["interleaved_ms"] = reps
    for name, rr in reps.items():
        med = [x["median"] for x in rr]
        out[name + "_ms"] = float(np.mean(med))
        out[name + "_spread_ms"] = float(max(med) - min(med))
    out["lmax0_minus_k_tabulate_ms"] = out["target_lmax0_ms"] - out["k_tabulate_ms"]
    for lmax in (2, 8, 16):
        out["target_lmax%d_ms" % lmax] = summary(timed(run_target(target(lmax))))
    if "--no-physics" not in sys.argv:
        deltas = [0.0, 5 * UM, 10 * UM, 20 * UM]
        sl, rms = modes.offset_response(tr, deltas, axis=2, lmax=16)
        rows = [{"offset_z_um": d / UM, "sigma_1_4": [float(v) for v in s[1:5]], "sigma_rms": float(q)}
                for d, s, q in zip(deltas, sl, rms)]
        sl, rms = modes.offset_response(tr, [0.0], axis=2, lmax=16, coeffs=modes.target_coeffs(2, {(2, 0): 0.01}))
        rows.append({"offset_z_um": 0.0, "c_20": 0.01, "sigma_1_4": [float(v) for v in sl[0][1:5]], "sigma_rms": float(rms[0])})
        out["response_not_asserted"] = {"n": 256, "nbeams": 60, "lmax": 16, "nshell": 32, "about": "origin",
                                        "sums": "coefficients summed over the shells", "rows": rows}
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
