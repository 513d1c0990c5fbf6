#!/usr/bin/env python3
"""The block layout of the trace kernel's step loop in a gfx950 listing: which of the calm step's branches are TAKEN.

The calm step -- deep inside the grid, all offsets negative, nobody outside box A, box B idle, nothing younger than the
record in flight -- is three wave-steps in four.  A taken branch redirects the wave's instruction fetch; a branch that
falls through costs its issue slot only.  So the common side of every wave-uniform branch of the loop should be the
fall-through, and this walker counts how many are not.

The walk is over instruction positions of one kernel body, as scripts/isa_chain.py's: the cheapest CYCLE (fewest
instructions executed; among equals, fewest taken branches) that passes the first instruction behind the in-loop
CBET_RECORD_ISSUE, a deposit into LDS (ds_add_f64: some lane moves on in 99 % of the wave-steps) and the `s_waitcnt vmcnt(0)` of the in-loop CBET_RECORD_WAIT's ladder (its pend == 0 arm; the plain
wait of the other kernels is that instruction itself).  On it: vector, scalar, LDS and vector-memory instructions, the
branch instructions and how many of them are taken -- a conditional branch left through its target, or an unconditional
one -- and the span of listing lines the path covers.

    usage: isa_layout.py listing.s [instantiation substring] [--path]     (listing = hipcc -S --cuda-device-only output
                                                                           of cbet_trace_window.hip; default: all sixteen)

The functions below are also what tests/test_isa_layout.py checks the shipped listing with."""
import heapq
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_chain as chain  # noqa: E402


# the calm step deposits: some lane changes cell in 99 % of the wave-steps, and its pending sums go to LDS between the
# gather and the wait -- the cycle without them (nobody moved on) is cheaper and rare
DEPOSIT = "ds_add_f64"


def instructions(lines):
    """[(line index, code)] of a body's instructions and labels, {label: position}."""
    inst = [(i, chain.code(l)) for i, l in enumerate(lines)]
    inst = [(i, c) for i, c in inst if c and (chain.is_label(c) or not c.startswith("."))]
    return inst, {c[:-1]: k for k, (_, c) in enumerate(inst) if chain.is_label(c)}


def successors(inst, labels, k):
    """[(next position, taken)] of the instruction at position k."""
    c = inst[k][1]
    if c.startswith("s_branch"):
        return [(labels.get(c.split()[1]), True)]
    if c.startswith("s_cbranch"):
        return [(k + 1, False), (labels.get(c.split()[1]), True)]
    if c.startswith(("s_endpgm", "s_setpc")):
        return []
    return [(k + 1, False)]


def cheapest(inst, labels, start, goal, through=None):
    """Positions on the cheapest path start .. goal (both included); cost = (instructions executed, taken branches).
    through: a mnemonic the path must execute at least once on the way."""
    far = (1 << 60, 0)
    s0, g = (start, through is None), (goal, True)
    dist, prev, heap = {s0: (0, 0)}, {}, [((0, 0), s0)]
    while heap:
        d, at = heapq.heappop(heap)
        if at == g:
            break
        k, seen = at
        if d > dist.get(at, far):
            continue
        c = inst[k][1]
        step = 0 if chain.is_label(c) else 1
        seen = seen or c.split()[0] == through
        for n, taken in successors(inst, labels, k):
            nd = (d[0] + step, d[1] + (1 if taken else 0))
            if n is not None and n < len(inst) and nd < dist.get((n, seen), far):
                dist[(n, seen)], prev[(n, seen)] = nd, at
                heapq.heappush(heap, (nd, (n, seen)))
    assert g in dist, "no path between the gather and the wait"
    path, at = [goal], g
    while at != s0:
        at = prev[at]
        path.append(at[0])
    return path[::-1]


def calm_marks(lines, inst):
    """(position of the first instruction behind the in-loop gather's marker, position of the pend == 0 wait)."""
    issue, wait = chain.loop_marks(lines)
    end = chain.wait_end(lines)
    first = next(k for k, (i, _) in enumerate(inst) if i > issue)
    zero = [k for k, (i, c) in enumerate(inst) if wait < i <= end + 1 and c.replace(" ", "") == "s_waitcntvmcnt(0)"]
    assert len(zero) == 1, "the in-loop record wait has one vmcnt(0)"
    return first, zero[0]


def calm_cycle(lines):
    """[(line index, code, taken)] of the calm step: gather -> pend == 0 wait -> back edge -> gather."""
    inst, labels = instructions(lines)
    first, zero = calm_marks(lines, inst)
    there, back = cheapest(inst, labels, first, zero, DEPOSIT), cheapest(inst, labels, zero, first)
    path = there + back[1:-1]          # (the wait once, the start not a second time)
    out = []
    for at, k in enumerate(path):
        nxt = path[at + 1] if at + 1 < len(path) else first
        c = inst[k][1]
        out.append((inst[k][0], c, c.startswith(("s_cbranch", "s_branch")) and (c.startswith("s_branch") or nxt != k + 1)))
    return out


def layout(lines):
    """The calm cycle's counts: chain.totals' fields + branches, taken, span (listing lines from the first to the last
    instruction of the path) and blocks (stretches of the path that are contiguous in the listing)."""
    cyc = calm_cycle(lines)
    t = chain.totals([(i, c) for i, c, _ in cyc])
    t["branches"] = sum(1 for _, c, _ in cyc if c.startswith(("s_cbranch", "s_branch")))
    t["taken"] = sum(1 for _, _, tk in cyc if tk)
    t["span"] = max(i for i, _, _ in cyc) - min(i for i, _, _ in cyc) + 1
    return t


def main():
    args = [a for a in sys.argv[1:] if a != "--path"]
    text = open(args[0]).read()
    want = args[1] if len(args) > 1 else ""
    for name, body in sorted(chain.kernels(text).items()):
        if want not in name:
            continue
        lines = body.splitlines()
        t = layout(lines)
        print("%s  VALU %d  SALU %d  LDS %d  VMEM %d  branches %d  taken %d  span %d lines" %
              (name, t["valu"], t["salu"], t["lds"], t["vmem"], t["branches"], t["taken"], t["span"]))
        if "--path" in sys.argv:
            for i, c, taken in calm_cycle(lines):
                if taken or chain.is_label(c) or c.startswith(("s_cbranch", "s_branch")):
                    print("%8d  %s%s" % (i + 1, c, "    <- TAKEN" if taken else ""))


if __name__ == "__main__":
    main()
