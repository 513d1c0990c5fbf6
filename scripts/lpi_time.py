#!/usr/bin/env python3
"""Times the quarter-critical LPI maps at 256^3, 60 beams, with HIP events, nothing running beside
the kernels, and records what the maps say about three runs.

  * time: k_lpi_map + k_lpi_reduce (RayTracer.lpi_map with a device summary: no synchronisation inside the timed call) on the
    normalised fields of a real field pass, 8 cone bins, Te from the tables: with the default band (0.20, 0.25); with an empty
    band (0.999, 0.999) -- the floor: ne3d in, zeros out; with the band (0, 0.999) -- every sub-critical brick lit; and, in the
    same process on the same fields, k_pair_amplitude.  Medians of 20 calls.  The floor's compulsory bytes (the node table in,
    seven quantities out) at the project's measured copy rate of 6.29 TB/s are reported beside it.
  * physics (--physics; --physics-n N, default 256): band (0.20, 0.25), te="tables": the summary of the map of the plain field
    pass, of the fields a converged CBET solve leaves with aligned beams, and of those it leaves with polarization smoothing.
    Recorded, not judged.
Every GPU step is a child process under its own `timeout`; the first failure ends the run and nothing more is started.
Writes profiles/lpi/lpi_time.json (or --out FILE).
usage: python scripts/lpi_time.py [--physics] [--physics-n N] [--out FILE]"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from saturation_time import summary, timed  # noqa: E402

N, CALLS = 256, 20
LIMITS = {"time": 300, "physics": 900}          # seconds a step may take (set-up of 45 GB included)
COPY_TB_S = 6.29                                # the measured device copy rate the project's other kernels are judged against
BANDS = {"default_band": (0.20, 0.25), "empty_band": (0.999, 0.999), "all_band": (0.0, 0.999)}


def step(name, physics_n):
    """One GPU step, in this process: a dict of results."""
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import load_inputs
    from cbet_raytracing_3d_amd import api, lpi
    from cbet_raytracing_3d_amd.tracer import RayTracer
    bn, r, ne, te = load_inputs()
    gp = api.default_gain_params()
    if name == "physics":
        return physics(torch, api, lpi, RayTracer, bn, r, ne, te, gp, physics_n)
    tr = RayTracer(api.default_params(N), r, ne, te, beam_norm=bn)
    tr.tabulate()
    fields = tr.new_fields()
    tr.launch_cbet(fields, gp, fields=True)
    gain = tr.new_grid(per_beam=True)
    tr.gain_field(fields, gain, gp, None, pair_once=True)           # normalises the fields in place
    del gain
    te3d = tr.table_te()
    stack = torch.empty((api.LPI_NQ,) + tr.grid_shape, dtype=torch.float64, device="cuda")
    summ, amp = tr.new_lpi_summary(), tr.new_grid()
    torch.cuda.synchronize()
    nodes, hsize = te3d.numel(), amp.numel()
    out = {"library": os.path.relpath(os.path.abspath(api.LIB_PATH), ROOT), "cone_bins": 8, "cells": hsize}
    for case, band in BANDS.items():
        out[case] = summary(timed(torch, lambda: tr.lpi_map(fields, te=te3d, band=band, out=stack, summary=summ), CALLS))
        _, s = tr.lpi_map(fields, te=te3d, band=band, out=stack)
        out[case]["band"] = list(band)
        out[case]["band_cells"], out[case]["lit_cells"], out[case]["max_present"] = s["band_cells"], s["lit_cells"], s["max_present"]
        out[case]["band_fraction_of_cells"] = s["band_cells"] / hsize
    out["pair_amplitude"] = summary(timed(torch, lambda: tr.pair_amplitude(fields, gp, out=amp), CALLS))
    floor_bytes = 8 * (nodes + api.LPI_NQ * hsize)
    floor_ms = floor_bytes / (COPY_TB_S * 1e12) * 1e3
    out["floor"] = {"compulsory_bytes": floor_bytes, "copy_rate_TB_s": COPY_TB_S, "ms_at_copy_rate": floor_ms,
                    "measured_over_copy_rate": out["empty_band"]["median"] / floor_ms}
    out["default_over_floor"] = out["default_band"]["median"] / out["empty_band"]["median"]
    out["all_over_floor"] = out["all_band"]["median"] / out["empty_band"]["median"]
    out["pair_amplitude_over_default"] = out["pair_amplitude"]["median"] / out["default_band"]["median"]
    tr.close()
    return out


def physics(torch, api, lpi, RayTracer, bn, r, ne, te, gp, n):
    tr = RayTracer(api.default_params(n), r, ne, te, beam_norm=bn)
    out = {"n": n, "nbeams": 60, "band": [0.20, 0.25], "cone_bins": 8, "te": "tables", "lambda_um": lpi.wavelength_um(tr.params), "runs": {}}

    def record(label, fields, extra):
        _, s = tr.lpi_map(fields)
        run = dict(extra, summary=s, derived=lpi.summarize(s))
        out["runs"][label] = run
        print("lpi_time: %s: %s" % (label, json.dumps(run)), flush=True)

    tr.tabulate()
    fields = tr.new_fields()
    tr.launch_cbet(fields, gp, fields=True)
    tmp = tr.new_grid(per_beam=True)
    tr.gain_field(fields, tmp, gp, None, pair_once=True)
    del tmp
    record("plain_field_pass", fields, {})
    for mode in ("aligned", "smoothed"):
        tr.set_polarization(mode)
        rep = tr.cbet_solve(tr.new_grid(), gp, fields=fields)
        record("cbet_solve_" + mode, fields, {"passes": int(rep["passes"]), "converged": bool(rep["converged"]),
                                               "imbalance": float(rep["imbalance"])})
        del rep
    tr.close()
    return out


def run_step(name, physics_n):
    """Start a step as a child under its own time limit; returns its results, or None after a failure."""
    with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--step", name, tmp.name,
               "--physics-n", str(physics_n)]
        rc = subprocess.call(cmd)
        if rc != 0:
            print("lpi_time: step %s ended with status %d -- nothing more is started" % (name, rc), flush=True)
            return None
        with open(tmp.name) as f:
            return json.load(f)


def main():
    arg = lambda flag, default=None: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else default    # noqa: E731
    physics_n = int(arg("--physics-n", N))
    if "--step" in sys.argv:
        i = sys.argv.index("--step")
        res = step(sys.argv[i + 1], physics_n)
        with open(sys.argv[i + 2], "w") as f:
            json.dump(res, f)
        return 0
    out = {"n": N, "nbeams": 60, "calls": CALLS}
    res = run_step("time", physics_n)
    failed = res is None
    if res is not None:
        out["k_lpi_map_ms"] = res
    if "--physics" in sys.argv and not failed:
        res = run_step("physics", physics_n)
        failed = res is None
        if res is not None:
            out["physics"] = res
    out["complete"] = not failed
    line = json.dumps(out)
    print(line)
    path = arg("--out", os.path.join(ROOT, "profiles", "lpi", "lpi_time.json"))
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
