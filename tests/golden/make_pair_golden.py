"""Writes tests/golden/pair_accuracy.npz, the fixture of tests/test_gpu_pair_accuracy.py ("Per-pair
accuracy"): the designed inputs of helpers/pair_cases.py, the constants of api.derive they were built from, and per world and
options set the 200-bit model's K as a double-double and the error scale S.  Needs mpmath; the GPU test does not.

    python tests/golden/make_pair_golden.py

tests/test_pair_accuracy_host.py runs the model again on the fixture's inputs and compares every array bit for bit."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

from helpers import pair_cases as PA                       # noqa: E402

PATH = os.path.join(HERE, "pair_accuracy.npz")


def derived_constants(api):
    """The constants the cases are built from: api.derive of the 4 x 3 x 148 grid, and the default iaw."""
    p = api.default_params(PA.SHAPE[0], nbeams=2)
    p.ny, p.nz = PA.SHAPE[1], PA.SHAPE[2]
    d = api.derive(p)
    return dict(ncrit=d.ncrit, omega=d.omega, dt=d.dt, iaw=api.default_gain_params().iaw)


def arrays(api):
    consts = derived_constants(api)
    inp = PA.build_inputs(consts)
    return PA.pack(inp, consts, PA.model(inp, consts))


if __name__ == "__main__":
    from cbet_raytracing_3d_amd import api
    out = arrays(api)
    np.savez_compressed(PATH, **out)
    print("%s: %d bytes; limits %s / %s, clamped shares %s / %s" % (PATH, os.path.getsize(PATH), out["sat_A"], out["sat_B"],
                                                                     out["share_A"], out["share_B"]))
