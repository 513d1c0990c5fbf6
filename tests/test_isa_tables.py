"""The fused table kernel (k_plasma_records, cbet_kernels.hip) in the gfx950 assembly, cross-compiled here (no GPU needed):
no scratch, no static LDS beside the dynamic region the occupancy estimate of DESIGN.md 4.1 counts, registers for 16 waves
per CU, and 16-byte record stores."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "cbet_raytracing_3d_amd", "csrc")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    from cbet_raytracing_3d_amd import build
    out = tmp_path_factory.mktemp("isa") / "kernels.s"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [build.hipcc()] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                                     "-o", str(out), os.path.join(CSRC, "cbet_kernels.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    text = out.read_text()
    found = {}
    for m in re.finditer(r"^(_ZN4cbet\S*(k_plasma_records|k_tabulate|k_step_table)\S*):[^\n]*\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M):
        found[m.group(2)] = m.group(3)
    return found


def test_the_unfused_kernels_stay_in_the_library(kernels):
    assert set(kernels) == {"k_plasma_records", "k_tabulate", "k_step_table"}


def test_fused_table_kernel_resources(kernels):
    body = kernels["k_plasma_records"]
    meta = dict(re.findall(r"\.amdhsa_(\w+)\s+(\S+)", body))
    assert int(meta["private_segment_fixed_size"]) == 0            # no scratch
    assert int(meta["group_segment_fixed_size"]) == 0              # all LDS is the dynamic region (profile + ring)
    assert int(meta["next_free_vgpr"]) <= 128                      # 16 waves per CU are not cut by registers


def test_record_arithmetic_is_not_contracted(kernels):
    """-ffp-contract=off reaches this file: k_step_table, whose arithmetic is c * (a - b) alone, holds no fused
    multiply-add (in the other two the correctly rounded fp64 division and square root expand to fma sequences, the same
    in both paths; that their results agree to the bit is tests/test_gpu_plasma_records.py's to show)."""
    from cbet_raytracing_3d_amd import build
    assert "-ffp-contract=off" in build.FLAGS
    body = kernels["k_step_table"]
    assert "v_fma_f64" not in body and "v_fmac_f64" not in body and "v_mul_f64" in body


def test_records_leave_as_16_byte_stores(kernels):
    body = kernels["k_plasma_records"]
    assert "global_store_dwordx4" in body
    assert "global_atomic" not in body and "flat_" not in body
