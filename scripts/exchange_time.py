"""Times the pairwise exchange matrix at 256^3, 60 beams, beside the kernel that evaluates the same
pairs: HIP events, nothing running beside the kernels; three repetitions (one child process each) of 20 calls, reported as the
mean of the repetitions' medians and their spread (largest minus smallest median).  In ONE process, on the SAME frozen
normalised fields of a real field pass with the ramp's closed-form flow:
  * k_gain_field_sym with frozen directions -- the call the CBET iteration repeats, the yardstick;
  * k_exchange_matrix + k_exchange_reduce over the whole grid (T and Gross), without a limit and with dn_max at the median of
    the fields' own amplitude map;
  * the same over the three slabs of the tests' cut scaled to the grid, added into one matrix.
Also recorded: the matrix's row sums against sum ds I K of the gain update on the same fields (of sum_j Gross_ij), its
antisymmetry, and whether two calls give the same bits.
Every GPU step is a child process under its own `timeout`; the first failure ends the run and nothing more is started.
Writes profiles/exchange/exchange_time.json (or --out FILE).
usage: python scripts/exchange_time.py [--out FILE] [--n N]"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS, REPS = 20, 3
LIMIT = 300                                    # seconds a step may take (set-up of 50 GB included)


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


def step(n):
    """One repetition, in this process: a dict of results."""
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import load_inputs
    from cbet_raytracing_3d_amd import api
    from cbet_raytracing_3d_amd.tracer import RayTracer
    bn, r, ne, te = load_inputs()
    gp = api.default_gain_params(relax=1.0)
    tr = RayTracer(api.default_params(n), r, ne, te, beam_norm=bn)
    nb = tr.params.nbeams
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

    out = {"work_bytes": api.exchange_matrix_work_bytes(tr.params)}
    out["gain_field_sym_frozen"] = summary(timed(torch, update, CALLS, before=fresh))
    fresh()
    gain.zero_()
    update()                                   # normalised fields, and K from a zero gain with relax 1
    T = torch.zeros((nb, nb), dtype=torch.float64, device="cuda")
    G = torch.zeros_like(T)

    def matrix():
        tr.exchange_matrix(fields, gp, out=T, gross=G)

    def clear():
        T.zero_()
        G.zero_()

    out["exchange_matrix"] = summary(timed(torch, matrix, CALLS, before=clear))
    first = (T.clone(), G.clone())
    clear()
    matrix()
    torch.cuda.synchronize()
    out["same_bits_twice"] = bool(torch.equal(T, first[0]) and torch.equal(G, first[1]))
    out["antisymmetric"] = bool(torch.equal(T, -T.t()) and torch.equal(G, G.t()))
    # the row-sum identity at this size: I = E / ds_node where the beam is present, so ds_node I K is E K to an ulp
    want = torch.stack([(torch.where(fields[0, b] > 0, energy[b], torch.zeros_like(energy[b])) * gain[b]).sum() for b in range(nb)])
    out["row_sum_error_of_gross"] = float(((T.sum(dim=1) - want).abs() / G.sum(dim=1)).max())
    out["max_gross"] = float(G.max())
    out["max_abs_t"] = float(T.abs().max())
    out["pairs_that_exchange"] = int((G > 0).sum()) // 2
    amp = tr.pair_amplitude(fields, gp)
    half = float(amp[amp > 0].median())
    del amp
    out["dn_max_half"] = half
    tr.set_saturation(half)
    out["exchange_matrix_half_clamped"] = summary(timed(torch, matrix, CALLS, before=clear))
    tr.set_saturation(0.0)
    hx = tr.grid_shape[0]
    cuts = [0, (9 * hx) // 50, (22 * hx) // 50, hx]

    def slabs():
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            tr.exchange_matrix(fields, gp, x_lo=lo, x_hi=hi, out=T, gross=G)

    out["slab_cuts"] = cuts
    out["exchange_matrix_three_slabs"] = summary(timed(torch, slabs, CALLS, before=clear))
    live = first[1] > 0
    out["slabs_vs_whole_of_gross"] = float(((T - first[0]).abs()[live] / first[1][live]).max())
    tr.close()
    return out


def main():
    arg = lambda flag, default=None: sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else default    # noqa: E731
    n = int(arg("--n", 256))
    if "--step" in sys.argv:
        res = step(n)
        with open(sys.argv[sys.argv.index("--step") + 1], "w") as f:
            json.dump(res, f)
        return 0
    out = {"n": n, "nbeams": 60, "calls_per_repetition": CALLS, "repetitions": REPS}
    reps, failed = {}, False
    for _ in range(REPS):
        with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
            rc = subprocess.call(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--step", tmp.name,
                                  "--n", str(n)])
            if rc != 0:
                print("exchange_time: a repetition ended with status %d -- nothing more is started" % rc, flush=True)
                failed = True
                break
            with open(tmp.name) as f:
                res = json.load(f)
        for case, v in res.items():
            if isinstance(v, dict) and "median" in v:
                reps.setdefault(case, []).append(v)
            else:
                out.setdefault("checks", {})[case] = v
    out["ms"] = {k: spread(rr) for k, rr in reps.items()}
    if "exchange_matrix" in out["ms"] and "gain_field_sym_frozen" in out["ms"]:
        out["ratio_to_gain_field_sym_frozen"] = (out["ms"]["exchange_matrix"]["mean_of_medians_ms"] /
                                                 out["ms"]["gain_field_sym_frozen"]["mean_of_medians_ms"])
    out["complete"] = not failed
    line = json.dumps(out)
    print(line)
    path = arg("--out", os.path.join(ROOT, "profiles", "exchange", "exchange_time.json"))
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
