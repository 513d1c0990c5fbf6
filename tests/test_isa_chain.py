"""The trace kernel's dependent chain -- record arrives, kick, move, relocate, gather the next record -- checked in the
gfx950 assembly (cross-compiled here, no GPU needed): what the source pins out of that chain stays out of it.

cbet_trace_window.hip keeps three things off the chain with empty assembly statements: the table's
base and the time step stay resident in scalar registers (no scalar load and no lgkmcnt wait in front of the gather, one
scalar pair for the three drift multiplies), the pending deposit's fp64 products stand behind the gather, and the six
per-axis factors are formed in front of the record wait, in the gather's shadow.  The rules are scripts/isa_chain.py's;
each is also fed a short synthetic listing that breaks it."""
import importlib.util
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "cbet_raytracing_3d_amd", "csrc")

_spec = importlib.util.spec_from_file_location("isa_chain", os.path.join(ROOT, "scripts", "isa_chain.py"))
chain = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(chain)


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from cbet_raytracing_3d_amd import build
    out = tmp_path_factory.mktemp("isa_chain") / "window.s"
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [build.hipcc()] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                                     "-o", str(out), os.path.join(CSRC, "cbet_trace_window.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    kernels = {n: b.splitlines() for n, b in chain.kernels(out.read_text()).items()}
    assert len(kernels) == 16
    return kernels


# ---- synthetic listings: a step loop in miniature ---------------------------------------------------------------------
def _mini(front="", shadow="\tv_xor_b32_e32 v23, v95, v23\n\tv_xor_b32_e32 v25, v96, v25\n\tv_xor_b32_e32 v71, v97, v71\n", behind="",
          drift=("s[48:49]", "s[48:49]", "s[48:49]"), vgpr=118, scratch=0):
    return ("""
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
	v_mul_f64 v[10:11], %s, v[34:35]
	v_add_f64 v[26:27], v[10:11], v[26:27]
	v_add_f64 v[10:11], v[26:27], -s[36:37]
	v_mul_f64 v[78:79], s[50:51], v[10:11]
	v_add_f64 v[6:7], v[6:7], -v[12:13]
	v_add_f64 v[8:9], v[8:9], -v[14:15]
	v_mul_f64 v[10:11], %s, v[6:7]
	v_mul_f64 v[12:13], %s, v[8:9]
	s_cbranch_scc0 .LBB0_2
.LBB0_2:
	v_lshlrev_b32_e32 v61, 5, v10
%s	;;#ASMSTART
	s_nop 4
	global_load_dwordx4 v[10:13], v61, s[52:53]
	global_load_dwordx4 v[14:17], v61, s[52:53] offset:16
	; CBET_RECORD_ISSUE v[10:13] v[14:17]
	;;#ASMEND
%s	;;#ASMSTART
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
%s	s_cbranch_scc1 .LBB0_1
	s_endpgm
	.amdhsa_kernel mini
		.amdhsa_private_segment_fixed_size %d
		.amdhsa_next_free_vgpr %d
		.amdhsa_next_free_sgpr 100
""" % (drift[0], drift[1], drift[2], front, shadow, behind, scratch, vgpr)).splitlines()


def test_rules_accept_the_miniature_loop():
    good = _mini()
    assert chain.gather_block_offenders(good) == []
    before, after = chain.factor_xors(good)
    assert len(before) == 3 and after == []
    assert chain.drift_scalars(good) == ["s[48:49]"] * 3
    assert chain.resources("\n".join(good)) == (118, 100, 0)
    # the walk: the wait's shortest arm -> tail -> loop header -> move -> gather
    ops = [c.split()[0] for _, c in chain.chain(good) if not chain.is_label(c)]
    assert ops[:3] == ["s_cmp_eq_u32", "s_cbranch_scc1", "s_waitcnt"] and ops[-2:] == ["global_load_dwordx4"] * 2
    assert ops.count("s_waitcnt") == 1 and ops.count("global_load_dwordx4") == 2
    assert chain.totals(chain.chain(good))["fp64"] == 10


@pytest.mark.parametrize("front", ["\ts_load_dwordx8 s[12:19], s[0:1], 0x168\n", "\ts_buffer_load_dwordx2 s[12:13], s[4:7], 0x0\n",
                                   "\ts_waitcnt lgkmcnt(0)\n", "\ts_waitcnt vmcnt(3) lgkmcnt(1)\n", "\tv_mul_f64 v[66:67], v[70:71], v[20:21]\n",
                                   "\tv_add_f64 v[66:67], v[70:71], v[20:21]\n", "\tv_fma_f64 v[50:51], v[50:51], v[60:61], v[68:69]\n"])
def test_gather_block_rule_sees_an_offender(front):
    assert len(chain.gather_block_offenders(_mini(front=front))) == 1


def test_factor_rules_see_a_sunk_factor():
    xor = "\tv_xor_b32_e32 v23, v95, v23\n"
    before, after = chain.factor_xors(_mini(shadow=xor * 2, behind=xor))
    assert len(before) == 2 and len(after) == 1
    # ... only up to the next conditional branch, and only the factors' form (two vector registers)
    assert not chain.is_factor_xor("v_xor_b32_e32 v18, 0x48, v18") and not chain.is_factor_xor("v_xor_b32_e32 v18, s10, v98")
    before, after = chain.factor_xors(_mini(behind="\ts_cbranch_scc1 .LBB0_2\n" + xor))
    assert len(before) == 3 and after == []


def test_drift_rule_sees_a_copied_time_step():
    assert len(set(chain.drift_scalars(_mini(drift=("s[48:49]", "s[64:65]", "s[66:67]"))))) == 3


def test_resource_rule_reads_the_digest():
    digest = chain.digest_resources("k_trace_window<16, false, 0, false>  body=ce99  insts=4583  hist=89c9  vgpr=118 sgpr=100 lds=10240 scratch=0\n"
                                    "k_trace_window<8, true, 4, true>  body=507a  insts=5319  hist=8ab4  vgpr=169 sgpr=100 lds=19200 scratch=0\n")
    assert digest == {"ILi16ELb0ELi0ELb0E": (118, 0), "ILi8ELb1ELi4ELb1E": (169, 0)}
    vgpr, _, scratch = chain.resources("\n".join(_mini(vgpr=119, scratch=8)))
    assert vgpr > digest["ILi16ELb0ELi0ELb0E"][0] and scratch > digest["ILi16ELb0ELi0ELb0E"][1]


# ---- the shipped listing -------------------------------------------------------------------------------------------------
def test_nothing_but_the_address_in_front_of_the_gather(listing):
    """Every instantiation: the straight-line block that ends at the in-loop gather holds no scalar load, no wait for
    one and no fp64 arithmetic."""
    for name, lines in listing.items():
        assert chain.gather_block(lines), name
        assert chain.gather_block_offenders(lines) == [], name


def test_factors_are_formed_in_the_gathers_shadow(listing):
    """factor_pair's three sign flips (v_xor_b32) stand between the in-loop gather and its wait, none between the wait's
    end and the next conditional branch: in the plain instantiations (CBET = 0, `Li0E`: four of them), whose factors
    the compiler used to sink below the wait, and in the twelve others as well."""
    plain = 0
    for name, lines in listing.items():
        plain += 1 if re.search(r"k_trace_windowILi\d+ELb[01]ELi0E", name) else 0
        before, after = chain.factor_xors(lines)
        assert len(before) == 3 and after == [], (name, before, after)
    assert plain == 4


def test_one_scalar_pair_for_the_three_drift_multiplies(listing):
    (name, lines), = [(n, l) for n, l in listing.items() if chain.HEADLINE in n]
    pairs = chain.drift_scalars(lines)
    assert len(pairs) == 3 and len(set(pairs)) == 1, pairs


def test_no_instantiation_grew(listing):
    """No more vector registers and no more scratch than the parent's listing digest records (profiles/onespelling/isa_new.txt);
    scalar registers stay within the 102 the wave has."""
    recorded = chain.digest_resources(open(os.path.join(ROOT, "profiles", "onespelling", "isa_new.txt")).read())
    assert len(recorded) == 16
    for name, lines in listing.items():
        (frag, (vgpr0, scratch0)), = [(k, v) for k, v in recorded.items() if k in name]
        vgpr, sgpr, scratch = chain.resources("\n".join(lines))
        assert vgpr <= vgpr0 and scratch <= scratch0 and sgpr <= 102, (frag, vgpr, vgpr0, scratch, scratch0, sgpr)
