"""The plain trace kernel's paired window-miss flush (cbet_trace_window.hip: pair_owners, pair_lanes, pair_issued,
pair_pick, hbm_add8), restated in numpy and checked without a GPU.

A lane outside both deposit boxes adds its eight pending sums straight to HBM.  They are four (x, y) columns of two z
nodes; the lane sends a column's first-visited value itself and its quad neighbour `lane ^ 1` sends the other one in the
same wave instruction, with the node and the value moved across by a quad permutation.  Two rounds: even miss lanes
through their odd neighbours, then odd ones through their even neighbours; a round without owners issues nothing.

The restatement follows the kernel statement by statement -- the picks (move and select in one) run on all 64 lanes,
the z node once per round, the (x, y) offset and the value per column, the atomic on the round's lanes -- and three
things are asserted over random miss masks, all-miss quads and empty rounds included: every (node, value) of every miss lane goes out exactly once, nothing of a lane that does not
miss goes out, and the number of instructions equals what miss_add8 adds to WaveCounters::pend."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "cbet_raytracing_3d_amd", "csrc", "cbet_trace_window.hip")
M64 = (1 << 64) - 1
EVEN = 0x5555555555555555
LANE = np.arange(64)
COLUMNS = (0, 1, 4, 5)          # the corners with c & 2 == 0 (Corner: x iff c & 1, z iff c & 2, y iff c & 4)


# ---- the kernel's helpers -----------------------------------------------------------------------------------------------
def pair_owners(hbm_m, rnd):
    return hbm_m & (EVEN if rnd == 0 else ~EVEN & M64)


def pair_lanes(owners, rnd):
    return owners | ((owners << 1) & M64 if rnd == 0 else owners >> 1)


def pair_issued(hbm_m):
    return (4 if pair_owners(hbm_m, 0) else 0) + (4 if pair_owners(hbm_m, 1) else 0)


def quad_swap(x, perm=(1, 0, 3, 2)):
    """A DPP quad_perm source: lane 4q + k reads lane 4q + perm[k]; every lane enabled."""
    return x[(LANE & ~3) + np.asarray(perm)[LANE & 3]]


def lanes_of(mask):
    return np.array([(mask >> l) & 1 for l in range(64)], dtype=bool)


def pair_pick(owners, mine, lent):
    """v_cndmask_b32_dpp: the second source on the lanes of the mask, the first -- fetched from lane ^ 1 -- elsewhere."""
    return np.where(lanes_of(owners), mine, quad_swap(lent))


def paired_flush(hbm_m, xy, z, val):
    """hbm_add8's paired arm.  xy: [64, 8] the (x, y) part of a corner's node, z: [64, 2] = Z0, Z1, val: [64, 8] in corner
    order.  Returns the instructions issued, each a list of (lane, node, value) of the lanes it ran on."""
    out = []
    for rnd in range(2):
        owners = pair_owners(hbm_m, rnd)
        if owners == 0:
            continue
        run = lanes_of(pair_lanes(owners, rnd))
        zz = pair_pick(owners, z[:, 0], z[:, 1])
        for c in COLUMNS:
            n = pair_pick(owners, xy[:, c], xy[:, c]) + zz
            v = pair_pick(owners, val[:, c], val[:, c ^ 2])
            out.append([(int(l), int(n[l]), float(v[l])) for l in LANE[run]])
    return out


# ---- a wave's worth of lanes ------------------------------------------------------------------------------------------------
def wave(rng, sXh=27 * 22, sYh=27):
    """Eight nodes and eight distinguishable values per lane; which of an axis's two nodes comes first depends on the lane
    (the kernel's flip bits), so a column's first-visited z node is the upper one on half the lanes."""
    lo = rng.integers(1, 18, size=(64, 3))
    flip = np.stack([(LANE & 1) != 0, (LANE & 2) != 0, (LANE & 8) != 0], axis=1)
    first, second = lo + flip, lo + 1 - flip
    xy = np.empty((64, 8), dtype=np.int64)
    for c in range(8):
        xy[:, c] = (second if c & 1 else first)[:, 0] * sXh + (second if c & 4 else first)[:, 1] * sYh
    z = np.stack([first[:, 2], second[:, 2]], axis=1)
    node = xy + z[:, [0, 0, 1, 1, 0, 0, 1, 1]]
    val = (LANE[:, None] * 8 + np.arange(8)[None, :] + 1).astype(np.float64)     # lane 8 c + ... : every value names its lane and corner
    return xy, z, node, val


def masks(rng):
    yield 0
    yield M64
    yield EVEN                      # round two empty
    yield ~EVEN & M64               # round one empty
    yield 0xF << 20                 # one all-miss quad
    yield 0x3 << 62                 # the last pair
    yield 1                         # one lane, its neighbour not missing
    yield 1 << 63
    for _ in range(300):
        density = rng.choice([0.02, 0.1, 0.5, 0.9])
        yield int(sum(1 << l for l in range(64) if rng.random() < density))


def test_source_constants():
    """The restatement's constants are the source's: the even-lane mask, the quad permutation [1, 0, 3, 2] on every lane
    of every row and bank, the select's operand order (v_cndmask_b32: the second source where the mask is set -- the
    owner's own --, the permuted first source elsewhere), two rounds of four columns."""
    code = re.sub(r"//[^\n]*", "", open(SRC).read())
    assert "kEvenLanes = 0x%xull" % EVEN in code
    (dpp,) = re.findall(r'#define CBET_PAIR_DPP "([^"]*)"', code)
    assert dpp.split() == ["quad_perm:[1,0,3,2]", "row_mask:0xf", "bank_mask:0xf", "bound_ctrl:1"]
    picks = re.findall(r'v_cndmask_b32_dpp %\d, %(\d), %(\d), vcc" CBET_PAIR_DPP', code)
    assert picks == [("2", "3"), ("4", "5"), ("6", "7"), ("8", "9")]          # (lent, mine) in the operand lists' order
    assert code.count('"s"(owners), "v"(lent') == 2 and code.count("s_mov_b64 vcc, %") == 2
    assert "wc.pend += PAIRED ? pair_issued(hbm_m) : 8;" in code
    assert "? 4 : 0) + (" in code[code.index("int pair_issued"):code.index("#define CBET_PAIR_DPP")]


def test_every_sum_of_a_miss_lane_goes_out_once_and_nothing_else():
    rng = np.random.default_rng(20261021)
    seen_empty_round = seen_full_quad = 0
    for hbm_m in masks(rng):
        xy, z, node, val = wave(rng)
        insts = paired_flush(hbm_m, xy, z, val)
        miss = lanes_of(hbm_m)
        # the count the wait relies on: instructions really issued == what miss_add8 adds to pend
        assert len(insts) == pair_issued(hbm_m), hex(hbm_m)
        assert all(len(i) > 0 for i in insts)                       # ... none of them on an empty set of lanes
        sent = sorted((n, v) for i in insts for _, n, v in i)
        want = sorted((int(node[l, c]), float(val[l, c])) for l in LANE[miss] for c in range(8))
        assert sent == want, hex(hbm_m)                             # each (node, value) once; values name lane and corner
        # a carrier lends its lane slot only: what leaves on lane L belongs to L or to L ^ 1, and to a miss lane
        for i in insts:
            for l, n, v in i:
                owner, corner = divmod(int(v) - 1, 8)
                assert owner in (l, l ^ 1) and miss[owner] and n == node[owner, corner], (hex(hbm_m), l)
        seen_empty_round += len(insts) == 4
        seen_full_quad += any(((hbm_m >> (4 * q)) & 0xF) == 0xF for q in range(16))
    assert seen_empty_round > 10 and seen_full_quad > 10


def test_a_pair_rides_in_one_instruction_at_adjacent_nodes():
    """What the pairing is for: a column's two z nodes leave in the SAME instruction, on the two lanes of a pair, one
    double apart -- whichever of the two the lane visits first."""
    rng = np.random.default_rng(7)
    for hbm_m in masks(rng):
        xy, z, node, val = wave(rng)
        for inst in paired_flush(hbm_m, xy, z, val):
            by_lane = {l: (n, v) for l, n, v in inst}
            assert len(by_lane) == len(inst)                        # one address per lane
            for l, (n, v) in by_lane.items():
                assert (l ^ 1) in by_lane                           # both lanes of the pair run
                n2, v2 = by_lane[l ^ 1]
                assert abs(n - n2) == 1 and abs(int(v) - int(v2)) == 2 and (int(v) - 1) // 8 == (int(v2) - 1) // 8


@pytest.mark.parametrize("perm", [(0, 1, 2, 3), (2, 3, 0, 1)])
def test_the_check_sees_a_wrong_permutation(perm):
    """... and the first check fails for a move that fetches from another lane than the neighbour."""
    rng = np.random.default_rng(3)
    _, _, _, val = wave(rng)
    hbm_m, rnd = 1 << 5, 1
    own, run = lanes_of(pair_owners(hbm_m, rnd)), lanes_of(pair_lanes(pair_owners(hbm_m, rnd), rnd))
    sent = []
    for c in COLUMNS:
        v = np.where(own, val[:, c], quad_swap(val[:, c ^ 2], perm))
        sent += [float(v[l]) for l in LANE[run]]
    assert sorted(sent) != sorted(float(x) for x in val[5])
