"""The block layout of the trace kernel's step loop, checked in the gfx950 assembly (cross-compiled here, no GPU needed):
the calm step falls through.

cbet_trace_window.hip tells the compiler which side of each wave-uniform branch of the loop the calm step takes
(CBET_USUAL / CBET_RARE / CBET_SELDOM), so that the common side is the fall-through and the rare
arms stand behind the loop.  A taken branch redirects the wave's instruction fetch (scripts/ubench/branch_cost.hip prices
it); before the hints the calm step took twelve per wave-step.  scripts/isa_layout.py walks the cheapest cycle of a body
through the in-loop gather, a deposit into LDS and the pend == 0 arm of the record wait; this file holds the plain
instantiations to the calm step's instruction counts and to at most four taken branches on that cycle, the back edge
included, and feeds the walker a miniature loop laid out both ways."""
import importlib.util
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "cbet_raytracing_3d_amd", "csrc")

_spec = importlib.util.spec_from_file_location("isa_layout", os.path.join(ROOT, "scripts", "isa_layout.py"))
layout = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(layout)
chain = layout.chain

MAX_TAKEN = 4     # the back edge, the record wait's pend == 0 arm, and two to spare: the parent commit took 12
# vector instructions of the calm step (120; the generic form's 64-bit table index adds seven)
CALM_VALU = {"ILi16ELb0ELi0ELb0E": 120, "ILi16ELb0ELi0ELb1E": 120, "ILi16ELb1ELi0ELb0E": 127, "ILi16ELb1ELi0ELb1E": 127}


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from cbet_raytracing_3d_amd import build
    out = tmp_path_factory.mktemp("isa_layout") / "window.s"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [build.hipcc()] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                                     "-o", str(out), os.path.join(CSRC, "cbet_trace_window.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    kernels = {n: b.splitlines() for n, b in chain.kernels(out.read_text()).items()}
    assert len(kernels) == 16
    return kernels


# ---- a step loop in miniature ---------------------------------------------------------------------------------------------
_HEAD = """
	;;#ASMSTART
	global_load_dwordx4 v[10:13], v18, s[52:53]
	; CBET_RECORD_ISSUE v[10:13] v[14:17]
	;;#ASMEND
	;;#ASMSTART
	; CBET_RECORD_WAIT v[10:13] v[14:17]
	s_waitcnt vmcnt(0)
	;;#ASMEND
.LBB0_1:                                ; =>This Inner Loop Header: Depth=1
	v_add_f64 v[34:35], v[34:35], -v[10:11]
	s_cmp_lg_u32 s97, 0
"""
_CALM = """	s_nop 1
	v_addc_co_u32_e64 v1, vcc, 0, v1, s[18:19]
"""
_RARE = """	v_mov_b32_e32 v2, v3
	v_mov_b32_e32 v4, v5
	v_mov_b32_e32 v6, v7
	v_mov_b32_e32 v8, v9
"""
_REST = """.LBB0_3:
	v_lshlrev_b32_e32 v61, 5, v1
	;;#ASMSTART
	s_nop 4
	global_load_dwordx4 v[10:13], v61, s[52:53]
	global_load_dwordx4 v[14:17], v61, s[52:53] offset:16
	; CBET_RECORD_ISSUE v[10:13] v[14:17]
	;;#ASMEND
	s_cmp_eq_u64 s[70:71], 0
	s_cbranch_scc1 .LBB0_4
	ds_add_f64 v91, v[80:81]
.LBB0_4:
	;;#ASMSTART
	; CBET_RECORD_WAIT v[10:13] v[14:17]
	s_cmp_eq_u32 s28, 0
	s_cbranch_scc1 .Lrw_0_7
	s_waitcnt vmcnt(1)
	s_branch .Lrw_end_7
.Lrw_0_7:
	s_waitcnt vmcnt(0)
.Lrw_end_7:
	;;#ASMEND
	v_mul_f64 v[20:21], v[28:29], v[16:17]
	s_cmp_lt_i32 s94, s31
	s_cbranch_scc1 .LBB0_1
	s_endpgm
"""


def _mini(calm_falls_through):
    if calm_falls_through:      # the rare arm behind the loop, jumped to and back
        text = _HEAD + "\ts_cbranch_scc1 .LBB0_9\n" + _CALM + _REST + ".LBB0_9:\n" + _RARE + "\ts_branch .LBB0_3\n"
    else:                       # the parent's shape: the rare arm is the fall-through, the calm one the jump
        text = _HEAD + "\ts_cbranch_scc0 .LBB0_9\n" + _RARE + _REST + ".LBB0_9:\n" + _CALM + "\ts_branch .LBB0_3\n"
    return text.splitlines()


def test_walker_counts_a_common_arm_that_is_the_jump():
    good, bad = layout.layout(_mini(True)), layout.layout(_mini(False))
    # the same calm step either way: the cheaper arm, the deposit (the cycle without it is cheaper and not the calm step),
    # the pend == 0 arm of the wait
    for t in (good, bad):
        assert (t["valu"], t["lds"], t["vmem"], t["waitcnt"]) == (4, 1, 2, 1), t
    assert (good["branches"], good["taken"]) == (4, 2)        # the wait's arm and the back edge
    assert (bad["branches"], bad["taken"]) == (5, 4)          # ... and the jump to the calm arm and the jump back
    taken = [c for _, c, tk in layout.calm_cycle(_mini(False)) if tk]
    assert taken == ["s_cbranch_scc1 .Lrw_0_7", "s_cbranch_scc1 .LBB0_1", "s_cbranch_scc0 .LBB0_9", "s_branch .LBB0_3"]
    assert bad["span"] > good["span"]
    # without the deposit on the way the walk would skip it
    inst, labels = layout.instructions(_mini(True))
    first, zero = layout.calm_marks(_mini(True), inst)
    assert not any(inst[k][1].startswith("ds_add") for k in layout.cheapest(inst, labels, first, zero))
    assert any(inst[k][1].startswith("ds_add") for k in layout.cheapest(inst, labels, first, zero, layout.DEPOSIT))


# ---- the shipped listing -------------------------------------------------------------------------------------------------
def test_calm_step_of_the_plain_kernels_falls_through(listing):
    plain = {n: l for n, l in listing.items() if re.search(r"k_trace_windowILi\d+ELb[01]ELi0E", n)}
    assert len(plain) == 4
    for name, lines in plain.items():
        (frag, valu), = [(k, v) for k, v in CALM_VALU.items() if k in name]
        t = layout.layout(lines)
        print(frag, t)
        assert abs(t["valu"] - valu) <= 3, (frag, t)
        assert t["lds"] == 8 and t["vmem"] == 2 and t["waitcnt"] == 1, (frag, t)     # one flush, one gather, one wait
        assert t["taken"] <= MAX_TAKEN, (frag, t, [c for _, c, tk in layout.calm_cycle(lines) if tk])

