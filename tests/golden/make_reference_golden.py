"""Regenerates the fixtures that the REFERENCE's own kernel source produced (not the oracle):

    tests/golden/reference_kat.json            per case of tests/helpers/reference_cases.py: ray-steps, steps per beam,
                                               sum, max, counts of non-zero and of negative cells, sum per x-plane
    tests/golden/reference_grid_<case>.npy     the whole (nx+2, ny+2, nz+2) grid of reference_cases.FULL_GRID

Run by hand from the repo root, where the reference tree is mounted:  python tests/golden/make_reference_golden.py
It builds oracle/_ref/<case>/run (oracle/ref_build.py: the reference's launch_ray_XZ.cu compiled unmodified as host C++)
and runs every case with ONE host thread, so each grid is the deterministic serial sum.  Data only is written: the
inputs are the committed s83177 profiles, the OMEGA-60 table and the analytic profiles of reference_cases.py.
tests/test_reference_pin.py checks these files against the live binaries bit for bit wherever those are built, and
against the oracle everywhere.
"""
import json
import os
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_inputs  # noqa: E402
from helpers import reference_cases as RC  # noqa: E402
from oracle import cbet_oracle as O  # noqa: E402
from oracle import ref_build as RB  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
MAX_GRID_BYTES = 388510      # the largest fixture committed before these; every grid stays below it


def main():
    assert RB.available(), "no reference tree at %s" % RB.reference_dir()
    RB.build(verbose=True)
    inputs = load_inputs()
    out = {"_made_by": "tests/golden/make_reference_golden.py: serial runs of the reference kernel source", "cases": {}}
    with tempfile.TemporaryDirectory() as td, ThreadPoolExecutor(max(1, min(16, os.cpu_count() or 1))) as pool:
        order = sorted(RC.CASES, key=lambda c: -c.n * c.ny * c.nz * len(c._beams))       # the long runs first
        runs = dict(zip(order, pool.map(lambda c: RC.run_reference(RB, O, c, inputs, td, threads=1), order)))
    for c in RC.CASES:
        run = runs[c]
        k = RC.kat(run["grid"], run["steps_per_beam"])
        cfg = c.config(O)
        k["shape"] = list(O.grid_shape(cfg))
        k["nindices"] = int(O.derive(cfg).nindices)
        out["cases"][c.name] = k
        print("%-22s %10d ray-steps  sum %.10e  nonzero %8d  negative %4d" % (c.name, k["ray_steps"], k["sum"],
                                                                              k["nonzero"], k["negative"]))
        if c.full_grid:
            path = os.path.join(OUT, "reference_grid_%s.npy" % c.name)
            np.save(path, run["grid"])
            assert os.path.getsize(path) < MAX_GRID_BYTES, (path, os.path.getsize(path))
    with open(os.path.join(OUT, "reference_kat.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
