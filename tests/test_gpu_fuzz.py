"""Randomised parity sweep (tests/helpers/fuzz_parity.py): small random grids, beam subsets, rays per zone, absorption,
sharding, beam-resolved grids, all three kernel formulations -- each case against the CPU oracle."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", [11, 12])
def test_random_configurations_match_the_oracle(seed):
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "fuzz_parity.py"), "30", str(seed)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    tail = "\n".join(run.stdout.splitlines()[-12:])
    assert run.returncode == 0, tail + run.stderr[-2000:]
    assert "failures 0" in tail


@pytest.mark.parametrize("seed", [21, 22])
def test_random_configurations_with_the_run_time_knobs_match_the_oracle(seed):
    """The same sweep with the knobs drawn too (third argument): Courant multiplier, box bounds, launch rule, beam rows.
    The script itself fails when more than 10 % of the cases had to be skipped for a non-finite oracle result."""
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "fuzz_parity.py"), "24", str(seed), "1"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    tail = "\n".join(run.stdout.splitlines()[-12:])
    print("\n".join(l for l in run.stdout.splitlines() if l.startswith(("case", "skipped", "cases"))))
    assert run.returncode == 0, tail + run.stderr[-2000:]
    assert "failures 0" in tail
    assert any(l.startswith("skipped ") for l in run.stdout.splitlines())
