"""Pins the CPU oracle to the reference's OWN kernel source: launch_ray_XZ.cu compiled unmodified as host C++ against
the stand-in headers of oracle/ref_shim/ and driven thread by thread (oracle/ref_build.py, oracle/ref_driver.cpp), one
binary per case of tests/helpers/reference_cases.py -- every knob the suite moves off the default cube.

Per case, reference against oracle.trace:
  * total and per-beam ray-steps equal, zero pattern equal;
  * one-pass launches (nindices == 1): the grids are EQUAL, bit for bit, with nthreads=1.  Both sides execute the same
    IEEE-754 statements in the same order (-ffp-contract=off, beams then ray ids ascending), so this is a derived
    condition, not a tolerance;
  * strided launches (nindices > 1; the reference sums thread by thread, the oracle id by id), and every case again with
    the oracle on NCPU threads: the project's parity metric below PARITY_TOL = 1e-9.  Each test prints what it observed;
  * pow_r, phase_r and the three gradient constants of the reference's main.cu lines equal the oracle's, bit for bit.
The default 64^3 and 100^3 runs reproduce what SURVEY.md 8(c) recorded (test_oracle_golden's constants, text dump
included) and the planes of planes_64.npz / planes_100.npz.

The fixtures the reference wrote (tests/golden/reference_kat.json, reference_grid_*.npy; make_reference_golden.py) are
checked against the live binaries bit for bit where those are built, and against the oracle by the rule above
everywhere -- also where no reference tree exists, e.g. in the CPU suite of the GPU box.

Skipping: a case whose binary is missing is skipped only where the reference tree is missing too; where the tree exists
the binaries are brought up to date first and test_every_case_is_built_where_the_reference_tree_exists holds that none
is missing.
"""
import hashlib
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import GOLDEN, NCPU, parity_err
from helpers import reference_cases as RC
from test_oracle_golden import SURVEY_CELLS_100, SURVEY_KAT, SURVEY_TEXT_100, printed

PARITY_TOL = 1e-9
PLANES_TOL = 1e-12       # what test_golden_fixture_matches_oracle_100 holds the planes to
# np.sum's pairwise order may differ between numpy builds: sums recorded in reference_kat.json are compared to
# 64 eps relative (pairwise summation of n terms errs by about log2(n) eps, n <= 1.1e6), everything else exactly
SUM_REL = 64 * 2.0 ** -52


@pytest.fixture(scope="module")
def ref_build():
    from oracle import ref_build as rb
    if rb.available():
        rb.build()       # compiles only what is missing or older than its inputs
    return rb


@pytest.fixture(scope="module")
def kat():
    return json.load(open(os.path.join(GOLDEN, "reference_kat.json")))["cases"]


@pytest.fixture(scope="module")
def reference(ref_build, oracle, inputs, tmp_path_factory):
    """case -> the serial run of its reference binary.  All runs are started at once on a pool of processes (the two
    default cubes first: 10 s and 40 s of one core) and each test waits for its own."""
    tmp = tmp_path_factory.mktemp("reference_runs")
    pool = ThreadPoolExecutor(max_workers=NCPU)
    futures = {}
    for c in sorted(RC.CASES, key=lambda c: -c.n * c.ny * c.nz * len(c._beams)):
        if os.path.exists(ref_build.binary(c.name)):
            futures[c.name] = pool.submit(RC.run_reference, ref_build, oracle, c, inputs, tmp, 1)

    def get(case):
        if case.name not in futures:
            assert not ref_build.available(), "oracle/_ref/%s/run was not built although the reference tree exists" % case.name
            pytest.skip("no reference tree at %s and no oracle/_ref/%s/run" % (ref_build.reference_dir(), case.name))
        return futures[case.name].result()
    yield get
    pool.shutdown(wait=True, cancel_futures=True)


@pytest.fixture(scope="module")
def oracle_serial(oracle, inputs):
    """case -> (grid, steps, steps per beam, nindices) of oracle.trace with nthreads=1, computed once."""
    cache = {}

    def get(case):
        if case.name not in cache:
            cfg = case.config(oracle)
            cache[case.name] = oracle.trace(cfg, case.beam_table(inputs[0]), *case.profile(oracle, inputs), nthreads=1,
                                            want_per_beam=True) + (oracle.derive(cfg).nindices,)
        return cache[case.name]
    return get


def _compare(what, name, oe, osteps, per_beam, nindices, grid, steps_per_beam):
    """The rule of this file: `grid`, `steps_per_beam` from the reference; oe, ... from the serial oracle."""
    assert osteps == int(np.sum(steps_per_beam)) and per_beam.tolist() == [int(s) for s in steps_per_beam], name
    assert np.array_equal(oe == 0, grid == 0), name
    err = parity_err(oe, grid)
    print("%-22s %s: %d ray-steps, nindices %d, serial oracle vs reference parity err %.2e, %d cells differ"
          % (name, what, osteps, nindices, err, int((oe != grid).sum())))
    if nindices == 1:
        assert np.array_equal(oe, grid), (name, err)
    else:
        assert err < PARITY_TOL, (name, err)


def test_the_table_holds_every_light_matrix_entry_and_the_extra_axes():
    from helpers import config_matrix as M
    light = [e.name for e in M.ENTRIES if not e.heavy]
    assert len(light) == 19 and set(light) <= set(RC.NAMES) and "long_nt" not in RC.NAMES
    assert {"ragged_60", "rpz3_40x48x36", "rpz6_24", "nprofile_2", "nprofile_64", "nprofile_2048", "config1_64",
            "descending_20x17x25", "default_64", "default_100"} <= set(RC.NAMES)
    assert sorted(RC.FULL_GRID) == ["descending_20x17x25", "ragged_60", "rpz6_24", "tall_y"]


def test_every_case_is_built_where_the_reference_tree_exists(ref_build):
    if not ref_build.available():
        pytest.skip("no reference tree at %s" % ref_build.reference_dir())
    missing = [n for n in RC.NAMES if not os.access(ref_build.binary(n), os.X_OK)]
    assert not missing, missing


def test_def_cuh_edits_touch_only_the_listed_lines(ref_build, oracle):
    """The edited def.cuh differs from the reference's in exactly the 17 lines the recipe names, for a case that moves
    every one of them."""
    if not ref_build.available():
        pytest.skip("no reference tree at %s" % ref_build.reference_dir())
    cfg = oracle.default_config(20, ny=17, nz=25, nbeams=3, nprofile=64, rays_per_zone=3, courant_mult=1.3, absorption=0,
                                max_threads=4000, threads_per_block=96, xmin=-0.1, xmax=0.16, ymin=-0.15, ymax=0.11,
                                zmin=-0.12, zmax=0.14)
    theirs = open(os.path.join(ref_build.reference_dir(), "def.cuh")).read().splitlines()
    ours = ref_build.edited_def(cfg).splitlines()
    assert len(theirs) == len(ours)
    changed = [(a, b) for a, b in zip(theirs, ours) if a != b]
    assert len(changed) == 17
    assert "const static int nGPUs = 1;" in ours and "#define xmin (-0.1)" in ours and "#define courant_mult (1.3)" in ours


@pytest.mark.parametrize("case", RC.CASES, ids=str)
def test_reference_equals_the_oracle(oracle, inputs, reference, oracle_serial, case):
    ref = reference(case)
    oe, osteps, per_beam, nindices = oracle_serial(case)
    _compare("live reference", case.name, oe, osteps, per_beam, nindices, ref["grid"], ref["steps_per_beam"])
    cfg = case.config(oracle)
    pe, psteps = oracle.trace(cfg, case.beam_table(inputs[0]), *case.profile(oracle, inputs), nthreads=NCPU)
    perr = parity_err(pe, ref["grid"])
    print("%-22s oracle on %d threads vs reference parity err %.2e" % (case.name, NCPU, perr))
    assert psteps == osteps and perr < PARITY_TOL, (case.name, perr)
    d = oracle.derive(cfg)
    phase, powr = oracle.power_table()
    assert np.array_equal(ref["phase_r"], phase) and np.array_equal(ref["pow_r"], powr)
    assert ref["consts"].tolist() == [d.xconst, d.yconst, d.zconst]


def test_driver_on_several_host_threads(ref_build, oracle, inputs, reference, tmp_path):
    """The driver's last argument: the blockIdx.y loop shared out over host threads, deposits through atomic adds.  Same
    ray-steps per beam, grid within PARITY_TOL of the serial run (a strided case and a far-jump one)."""
    for name in ("strided_5", "courant_2.5"):
        case = RC.BY_NAME[name]
        serial = reference(case)
        par = RC.run_reference(ref_build, oracle, case, inputs, tmp_path, threads=max(2, NCPU))
        err = parity_err(par["grid"], serial["grid"])
        print("%-22s reference on %d host threads vs serial parity err %.2e" % (name, max(2, NCPU), err))
        assert par["steps_per_beam"].tolist() == serial["steps_per_beam"].tolist() and err < PARITY_TOL, (name, err)


@pytest.mark.parametrize("n", [64, 100])
def test_default_cubes_reproduce_the_survey(oracle, reference, tmp_path, n):
    """The recipe reproduces the run SURVEY.md 8(c) recorded: the same numbers test_oracle_golden.py holds the oracle to,
    here from the reference binary's own grid."""
    ref = reference(RC.BY_NAME["default_%d" % n])
    e, k = ref["grid"], SURVEY_KAT[n]
    assert int(ref["steps_per_beam"].sum()) == k["ray_steps"] and e.size == k["size"]
    assert np.count_nonzero(e) == k["nonzero"]
    assert e.sum() == printed(k["sum"]) and e.max() == printed(k["max"])
    planes = np.load(os.path.join(GOLDEN, "planes_%d.npz" % n))
    c = (n + 2) // 2
    for name, got in (("yz", e[c]), ("xz", e[:, c]), ("xy", e[:, :, c]), ("face_x0", e[0]), ("face_z0", e[:, :, 0])):
        err = parity_err(got, planes[name])
        print("default_%d plane %s: reference vs planes_%d.npz parity err %.2e" % (n, name, n, err))
        assert err < PLANES_TOL, name
    if n == 100:
        assert (ref["steps_per_beam"].min(), ref["steps_per_beam"].max()) == (2016670, 2174951)
        assert int((e < 0).sum()) == 1
        digits = {(1, 1, 1): 17, (51, 51, 90): 17, (20, 51, 51): 13, (101, 7, 0): 11}
        for ijk, v in SURVEY_CELLS_100.items():      # 17-digit values carry summation-order noise
            assert e[ijk] == (printed(v, digits[ijk]) if digits[ijk] < 15 else pytest.approx(v, rel=1e-13))
        path = str(tmp_path / "edep.txt")
        nbytes = oracle.write_text(e, path)
        blob = open(path, "rb").read()
        assert nbytes == len(blob) == SURVEY_TEXT_100["bytes"] and blob.startswith(SURVEY_TEXT_100["head"])
        assert hashlib.md5(blob).hexdigest() == SURVEY_TEXT_100["md5"]


def _kat_equal(name, got, want):
    for key in ("ray_steps", "steps_per_beam", "nonzero", "negative", "max"):
        assert got[key] == want[key], (name, key)
    assert got["sum"] == pytest.approx(want["sum"], rel=SUM_REL, abs=0), name
    assert len(got["sum_per_x_plane"]) == len(want["sum_per_x_plane"]) == want["shape"][0]
    scale = max(abs(v) for v in want["sum_per_x_plane"])
    assert got["sum_per_x_plane"] == pytest.approx(want["sum_per_x_plane"], rel=SUM_REL, abs=SUM_REL * scale), name


@pytest.mark.parametrize("case", RC.CASES, ids=str)
def test_fixtures_equal_the_live_reference(reference, kat, case):
    """reference_kat.json and the committed grids are what the binaries give today, bit for bit."""
    ref = reference(case)
    _kat_equal(case.name, RC.kat(ref["grid"], ref["steps_per_beam"]), kat[case.name])
    assert list(ref["grid"].shape) == kat[case.name]["shape"]
    if case.full_grid:
        assert np.array_equal(np.load(os.path.join(GOLDEN, "reference_grid_%s.npy" % case.name)), ref["grid"])


@pytest.mark.parametrize("case", RC.CASES, ids=str)
def test_fixtures_match_the_oracle(oracle, inputs, oracle_serial, kat, case):
    """The same rule with the committed fixtures in the reference's place: needs no reference tree."""
    oe, osteps, per_beam, nindices = oracle_serial(case)
    k = kat[case.name]
    assert sorted(kat) == sorted(RC.NAMES) and k["nindices"] == nindices and list(oe.shape) == k["shape"]
    assert osteps == k["ray_steps"] and per_beam.tolist() == k["steps_per_beam"]
    assert np.count_nonzero(oe) == k["nonzero"]
    if nindices == 1:         # the grid is the reference's bit for bit, so every recorded figure of it is the oracle's
        _kat_equal(case.name, RC.kat(oe, per_beam), k)
    else:                     # sums of a grid within PARITY_TOL of the recorded one (terms of one sign but for far jumps)
        assert oe.sum() == pytest.approx(k["sum"], rel=PARITY_TOL) and oe.max() == pytest.approx(k["max"], rel=PARITY_TOL)
        assert int((oe < 0).sum()) == k["negative"]
    if case.full_grid:
        grid = np.load(os.path.join(GOLDEN, "reference_grid_%s.npy" % case.name))
        _compare("committed grid", case.name, oe, osteps, per_beam, nindices, grid, k["steps_per_beam"])
        pe, _ = oracle.trace(case.config(oracle), case.beam_table(inputs[0]), *case.profile(oracle, inputs), nthreads=NCPU)
        perr = parity_err(pe, grid)
        print("%-22s oracle on %d threads vs committed grid parity err %.2e" % (case.name, NCPU, perr))
        assert perr < PARITY_TOL, (case.name, perr)
