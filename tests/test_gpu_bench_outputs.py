"""bench.py's plain run and --dump-outputs: the plain line carries the headline and nothing that needs runs of its own
(roofline, dense_layout, cbet, cpu_baseline come with --full only), and the dumped grid of the last timed pass is the
workload's deposition, the same whether one rank or two (sharing GPU 0 over gloo) computed it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, parity_err

pytestmark = pytest.mark.gpu

ENV_DROP = ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "CBET_BENCH_DEVICE", "CBET_BENCH_STDERR_DIR")


def bench_line(*argv, **extra_env):
    env = {k: v for k, v in os.environ.items() if k not in ENV_DROP}
    env.update(extra_env)
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True,
                         timeout=600, cwd=ROOT, env=env)
    assert run.returncode == 0, run.stdout[-1500:] + run.stderr[-1500:]
    lines = [l for l in run.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_line_and_dumped_outputs(tmp_path):
    one = bench_line("--gpus", "1", "--grid", "64", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "one"))
    assert one["steps"] == 3 and one["unit"] == "ray-steps/s" and one["higher_is_better"] is True and one["dtype"] == "f64"
    assert one["value"] > 0 and one["ms_per_step"] > 0
    assert one["config"]["ray_steps_per_pass"] == 30712072                      # SURVEY.md 8(c), 64^3
    assert not {"roofline", "dense_layout", "cbet", "cpu_baseline"} & set(one)
    sample = np.load(str(tmp_path / "one" / "edep_sample.npy"))
    sums = np.load(str(tmp_path / "one" / "edep_plane_sums.npy"))
    assert sample.dtype == np.float64 and sample.shape == (66 ** 3,)            # a grid this small is written whole
    assert sums.dtype == np.float64 and sums.shape == (66,)
    assert sums.sum() == pytest.approx(one["config"]["edep_sum"], rel=1e-12)
    assert sample.sum() == pytest.approx(one["config"]["edep_sum"], rel=1e-12)

    two = bench_line("--gpus", "2", "--backend", "gloo", "--grid", "64", "--steps", "2", "--warmup", "1",
                     "--dump-outputs", str(tmp_path / "two"), CBET_BENCH_DEVICE="0")
    assert two["n_gpus"] == 2 and "roofline" not in two
    for name in ("edep_sample.npy", "edep_plane_sums.npy"):
        a, b = np.load(str(tmp_path / "one" / name)), np.load(str(tmp_path / "two" / name))
        assert a.shape == b.shape and parity_err(b, a) < 1e-9, name
