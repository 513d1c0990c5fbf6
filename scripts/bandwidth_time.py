#!/usr/bin/env python3
"""Times the line spectrum of the CBET gain stage at 256^3, 60 beams, frozen fields of a real field
pass, with HIP events, nothing running beside the kernels; three interleaved repetitions of 20 calls each, reported as the mean
of the repetitions' medians and their spread (largest minus smallest median):
  * k_gain_field_sym with frozen directions -- the call the CBET iteration repeats -- and k_exchange_matrix
    (+ k_exchange_reduce) over the whole grid: one colour (`mono`), section 19's three colours +-3 Angstrom (`detune`), and the
    three colours with a spectrum whose difference table has M = 1, 3, 7 and 28 entries (`band1` ... `band28`);
  * `mono` and `detune` on a build of the PARENT commit (--parent-lib FILE, loaded through CBET_LIB_PATH).
A repetition is one child process per build, this build's and the parent's in turn.
  * --solve: the native cbet_cbet_solve at 128^3 (--solve-n N), 60 beams, default gain parameters, three colours +-3 Angstrom,
    without and with a five-line flat spectrum of the same total width (6 Angstrom): passes, convergence, imbalance, the
    absorbed fraction of the exit pass and the range of the per-beam gain.  Recorded, not judged.
Every GPU step is a child process under its own `timeout`; the first failure ends the run and nothing more is started.
Writes profiles/bandwidth/bandwidth_time.json (or --out FILE).
usage: python scripts/bandwidth_time.py [--parent-lib FILE] [--solve] [--solve-n N] [--out FILE]"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from saturation_time import spread, summary, timed  # noqa: E402

N, SOLVE_N, CALLS, REPS = 256, 128, 20, 3
LIMITS = {"gain": 420, "parent": 300, "solve": 900}         # seconds a step may take (set-up of 50 GB included)
NEW = ("cbet_context_set_bandwidth", "cbet_context_bandwidth", "cbet_exchange_matrix_host_banded")
STEP = 2.0 ** 40                                             # rad/s; 4.6e12 rad/s is 3 Angstrom at 351 nm
# line offsets whose difference tables have M = 1, 3, 7 (eight lines on a grid) and 28 (eight lines on a Golomb ruler) entries
SPECTRA = {"band1": [0.0, 4.0 * STEP], "band3": [-4.0 * STEP, 1.0 * STEP, 4.0 * STEP], "band7": [STEP * (a - 3.5) for a in range(8)],
           "band28": [STEP * 8.0 / 34.0 * (a - 17.0) for a in (0, 1, 4, 9, 15, 22, 32, 34)]}


def three_colours(nbeams, angstrom=3.0):
    return [angstrom * ((b % 3) - 1.0) for b in range(nbeams)]


def step(name, solve_n):
    """One GPU step, in this process: a dict of results."""
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import load_inputs
    from cbet_raytracing_3d_amd import api
    from cbet_raytracing_3d_amd.tracer import RayTracer
    if name == "parent":
        api.lib(tolerate=NEW)                   # the parent's build lacks this commit's entries; it is only run without lines
    bn, r, ne, te = load_inputs()
    if name == "solve":
        return solve(torch, api, RayTracer, bn, r, ne, te, solve_n)
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
    cases = ["mono", "detune"] + ([] if name == "parent" else list(SPECTRA))
    for case in cases:
        if case != "mono":
            tr.set_detuning(dlambda_angstrom=three_colours(tr.params.nbeams))
        if case in SPECTRA:
            tr.set_bandwidth(SPECTRA[case])
        out["gain_" + case] = summary(timed(torch, update, CALLS, before=fresh))
        fresh()
        update()                               # normalised fields for the matrix
        out["matrix_" + case] = summary(timed(torch, matrix, CALLS))
    tr.close()
    return out


def solve(torch, api, RayTracer, bn, r, ne, te, n):
    gp = api.default_gain_params()
    tr = RayTracer(api.default_params(n), r, ne, te, beam_norm=bn)
    out = {"n": n, "nbeams": 60, "relax": gp.relax, "max_passes": gp.max_passes, "tolerance": gp.tolerance,
           "colours_angstrom": 3.0, "lines": 5, "width_angstrom": 6.0, "runs": {}}
    ws = torch.empty(api.cbet_workspace_bytes(tr.params) // 8 + 1, dtype=torch.float64, device="cuda")
    off = (api.cbet_workspace_gain(tr.params, ws) - ws.data_ptr()) // 8
    stream = torch.cuda.current_stream().cuda_stream
    tr.set_detuning(dlambda_angstrom=three_colours(tr.params.nbeams))
    for case in ("three_colours", "three_colours_five_lines"):
        if case != "three_colours":
            tr.set_bandwidth(*api.line_spectrum(tr.params, 6.0, 5))
        e = tr.new_grid()
        rep = api.cbet_solve(tr.d_te, tr.d_r, tr.d_ne, e, tr.d_bbeam_norm, tr.d_beam_norm, tr.d_pow_r, tr.d_phase_r, tr.params, gp,
                             workspace=ws, ctx=tr.ctx, stream=stream)
        torch.cuda.synchronize()
        gain = ws[off:off + tr.params.nbeams * e.numel()].view((tr.params.nbeams,) + tr.grid_shape)
        tally = tr.energy_balance(tr.trace_exits(tr.new_exits(), gain=gain, gain_params=gp)).cpu().numpy()
        launched, gained, absorbed = tally[:, 0], tally[:, 1], tally[:, 2]
        rel = gained / launched
        out["runs"][case] = {"passes": int(rep.passes), "converged": bool(rep.converged), "change": float(rep.change),
                             "imbalance": float(rep.imbalance), "absorbed_fraction": float(absorbed.sum() / launched.sum()),
                             "max_gain": float(gain.abs().max()),
                             "beam_gain_over_launched": {"min": float(rel.min()), "max": float(rel.max()), "std": float(rel.std())}}
        print("bandwidth_time: solve %s: %s" % (case, json.dumps(out["runs"][case])), flush=True)
    tr.close()
    return out


def run_step(name, solve_n, env=None):
    """Start a step as a child under its own time limit; returns its results, or None after a failure."""
    with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
        cmd = ["timeout", "-k", "10", str(LIMITS[name]), sys.executable, os.path.abspath(__file__), "--step", name, tmp.name,
               "--solve-n", str(solve_n)]
        rc = subprocess.call(cmd, env=env)
        if rc != 0:
            print("bandwidth_time: step %s ended with status %d -- nothing more is started" % (name, rc), flush=True)
            return None
        with open(tmp.name) as f:
            return json.load(f)


def main():
    arg = lambda flag, default=None: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else default    # noqa: E731
    solve_n = int(arg("--solve-n", SOLVE_N))
    if "--step" in sys.argv:
        i = sys.argv.index("--step")
        res = step(sys.argv[i + 1], solve_n)
        with open(sys.argv[i + 2], "w") as f:
            json.dump(res, f)
        return 0
    parent = arg("--parent-lib")
    out = {"n": N, "nbeams": 60, "calls_per_repetition": CALLS, "repetitions": REPS,
           "table_entries": {"band1": 1, "band3": 3, "band7": 7, "band28": 28}}
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
    for kernel, key in (("k_gain_field_sym_frozen_ms", "gain_"), ("k_exchange_matrix_ms", "matrix_")):
        out[kernel] = {k.replace(key, ""): spread(rr) for k, rr in reps.items() if key in k}
    if "--solve" in sys.argv and not failed:
        res = run_step("solve", solve_n)
        failed = res is None
        if res is not None:
            out["solve"] = res
    out["complete"] = not failed
    line = json.dumps(out)
    print(line)
    path = arg("--out", os.path.join(ROOT, "profiles", "bandwidth", "bandwidth_time.json"))
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
