#!/usr/bin/env python3
"""The trace kernel's dependent chain in a gfx950 listing: what a wave executes on the calm path between the arrival of a
step's record (the in-loop CBET_RECORD_WAIT) and the gather of the next one (the in-loop CBET_RECORD_ISSUE).

The walk follows the listing's control flow: at every conditional branch it takes the arm with fewer instructions that
still reaches the gather (a shortest path, weighted by instruction count), which is the calm step -- no far jump, no face
near, no ray ends, nothing retired behind the gather.  It prints the instructions on the way and their totals: VALU, of
which fp64, SALU, SMEM, s_waitcnt and the wait states of s_nop.

    usage: isa_chain.py listing.s [instantiation substring]      (listing = hipcc -S --cuda-device-only output of
                                                                  cbet_trace_window.hip; default: the headline body)

The functions below are also what tests/test_isa_chain.py checks the shipped listing with."""
import heapq
import re
import sys

HEADLINE = "ILi16ELb0ELi0ELb0E"
_FP64_ARITH = ("v_mul_f64", "v_add_f64", "v_fma_f64")


def kernels(text):
    """name -> body of every k_trace_window instantiation of a device listing."""
    out = {}
    for m in re.finditer(r"^(_ZN4cbet\S*k_trace_window\S*):[^\n]*\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M):
        out[m.group(1)] = m.group(2)
    return out


def code(line):
    return line.split(";")[0].strip()


def is_label(c):
    return bool(re.match(r"^[.\w$]+:$", c))


def is_branch(c):
    return c.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc"))


def loop_marks(lines):
    """(line index of the in-loop CBET_RECORD_ISSUE, of the CBET_RECORD_WAIT that follows it): the second of each."""
    issues = [i for i, l in enumerate(lines) if "CBET_RECORD_ISSUE" in l]
    waits = [i for i, l in enumerate(lines) if "CBET_RECORD_WAIT" in l]
    assert len(issues) == 2 and len(waits) == 2 and waits[1] > issues[1], (issues, waits)
    return issues[1], waits[1]


def gather_block(lines):
    """The instructions of the straight-line block that ends at the in-loop CBET_RECORD_ISSUE."""
    issue, _ = loop_marks(lines)
    out = []
    for i in range(issue - 1, -1, -1):
        c = code(lines[i])
        if not c or c.startswith(".") and not c.endswith(":"):
            continue
        if is_label(c) or is_branch(c):
            break
        out.append(c)
    return out[::-1]


def gather_block_offenders(lines):
    """Rule 1: no scalar load, no wait for one and no fp64 arithmetic in front of the in-loop gather."""
    bad = []
    for c in gather_block(lines):
        op = c.split()[0]
        if op.startswith(("s_load", "s_buffer_load")) or (op == "s_waitcnt" and "lgkmcnt" in c) or op.startswith(_FP64_ARITH):
            bad.append(c)
    return bad


def wait_end(lines):
    """Index of the last line of the in-loop record wait: its end label (the counted ladder), or the s_waitcnt itself."""
    _, wait = loop_marks(lines)
    for i in range(wait + 1, len(lines)):
        if ";;#ASMEND" in lines[i]:
            return i - 1
    raise AssertionError("the record wait's assembly block does not end")


def is_factor_xor(c):
    """factor_pair's sign flip: v_xor_b32 of two VECTOR registers, the lane's sign mask and the high half of |o| - h (the
    exclusive-ors of the LDS swizzle and the write-backs take a constant or a scalar register)."""
    return bool(re.match(r"v_xor_b32(_e32|_e64)?\s+v\d+,\s*v\d+,\s*v\d+$", c))


def factor_xors(lines):
    """Rules 2 and 3: (the factors' v_xor_b32 between the in-loop gather and its wait, those between the wait's end and the
    next conditional branch)."""
    issue, wait = loop_marks(lines)
    before = [code(l) for l in lines[issue:wait] if is_factor_xor(code(l))]
    after = []
    for l in lines[wait_end(lines) + 1:]:
        c = code(l)
        if c.startswith("s_cbranch"):
            break
        if is_factor_xor(c):
            after.append(c)
    return before, after


def _pair(spec):
    m = re.fullmatch(r"-?\|?([sv])\[(\d+):(\d+)\]\|?", spec.strip())
    return (m.group(1), int(m.group(2))) if m else None


def drift_scalars(lines):
    """Rule 4: the scalar pairs the three drift multiplies of the step loop read.  A drift multiply is v_mul_f64 of a
    scalar pair and a velocity, i.e. a vector pair last written by a kick: v_add_f64 of two vector pairs."""
    issue, _ = loop_marks(lines)
    head = max(i for i in range(issue) if "Loop Header: Depth=1" in lines[i])
    kicked, out = set(), []
    for l in lines[head + 1:]:
        c = code(l)
        if not c or c.startswith((".", ";")):
            continue
        if is_label(c) or is_branch(c):
            break
        op, ops = c.split()[0], [_pair(o) for o in c[len(c.split()[0]):].split(",")]
        if op.startswith("v_mul_f64") and len(ops) == 3 and None not in ops:
            srcs = ops[1:]
            scal = [p for p in srcs if p[0] == "s"]
            vec = [p for p in srcs if p[0] == "v"]
            if len(scal) == 1 and len(vec) == 1 and vec[0] in kicked:
                out.append("s[%d:%d]" % (scal[0][1], scal[0][1] + 1))
        if ops and ops[0] is not None:
            if op.startswith("v_add_f64") and len(ops) == 3 and None not in ops and all(p[0] == "v" for p in ops[1:]):
                kicked.add(ops[0])
            else:
                kicked.discard(ops[0])
    return out


def resources(body):
    meta = dict(re.findall(r"\.amdhsa_(\w+)\s+(\S+)", body))
    return int(meta["next_free_vgpr"]), int(meta["next_free_sgpr"]), int(meta["private_segment_fixed_size"])


def digest_resources(text):
    """'k_trace_window<16, false, 0, false>  ... vgpr=118 sgpr=100 lds=.. scratch=0' lines of an isa_digest.py record ->
    {mangled template fragment: (vgpr, scratch)}."""
    out = {}
    for m in re.finditer(r"^k_trace_window<(\d+), (true|false), (\d+), (true|false)>.*?vgpr=(\d+).*?scratch=(\d+)", text, re.M):
        wz, gen, cbet, stats, vgpr, scratch = m.groups()
        out["ILi%sELb%dELi%sELb%dE" % (wz, gen == "true", cbet, stats == "true")] = (int(vgpr), int(scratch))
    return out


# ---- the walk ----------------------------------------------------------------------------------------------------------
def chain(lines):
    """The instructions on the cheapest path from the in-loop record wait to the in-loop gather."""
    issue, wait = loop_marks(lines)
    inst = [(i, code(l)) for i, l in enumerate(lines)]
    inst = [(i, c) for i, c in inst if c and (is_label(c) or not c.startswith("."))]
    labels = {c[:-1]: k for k, (_, c) in enumerate(inst) if is_label(c)}
    start = next(k for k, (i, _) in enumerate(inst) if i > wait)
    goal = max(k for k, (i, _) in enumerate(inst) if i < issue)      # the last instruction in front of the marker
    # Dijkstra over instruction positions: cost = instructions executed
    dist, prev, heap = {start: 0}, {}, [(0, start)]
    while heap:
        d, k = heapq.heappop(heap)
        if k == goal:
            break
        if d > dist.get(k, 1 << 60) or k + 1 >= len(inst):
            continue
        c = inst[k][1]
        step = 0 if is_label(c) else 1
        nxt = []
        if c.startswith("s_branch"):
            nxt = [labels.get(c.split()[1])]
        elif c.startswith("s_cbranch"):
            nxt = [k + 1, labels.get(c.split()[1])]
        elif not c.startswith(("s_endpgm", "s_setpc")):
            nxt = [k + 1]
        for n in nxt:
            if n is not None and d + step < dist.get(n, 1 << 60):
                dist[n], prev[n] = d + step, k
                heapq.heappush(heap, (d + step, n))
    assert goal in dist, "the gather is not reachable from the wait"
    path, k = [], goal
    while k != start:
        path.append(k)
        k = prev[k]
    path.append(start)
    return [inst[k] for k in path[::-1]]


def totals(path):
    t = dict(valu=0, fp64=0, salu=0, smem=0, waitcnt=0, nop_states=0, lds=0, vmem=0)
    for _, c in path:
        if is_label(c):
            continue
        op = c.split()[0]
        if op.startswith("s_nop"):
            t["nop_states"] += int(c.split()[1]) + 1
        elif op.startswith("s_waitcnt"):
            t["waitcnt"] += 1
        elif op.startswith(("s_load", "s_buffer_load", "s_memtime", "s_memrealtime")):
            t["smem"] += 1
        elif op.startswith("s_"):
            t["salu"] += 1
        elif op.startswith("v_"):
            t["valu"] += 1
            t["fp64"] += 1 if "_f64" in op else 0
        elif op.startswith("ds_"):
            t["lds"] += 1
        elif op.startswith(("global_", "buffer_", "flat_")):
            t["vmem"] += 1
    return t


def main():
    text = open(sys.argv[1]).read()
    want = sys.argv[2] if len(sys.argv) > 2 else HEADLINE
    (name, body), = [(n, b) for n, b in kernels(text).items() if want in n]
    lines = body.splitlines()
    path = chain(lines)
    print("# %s: record wait -> next gather, calm path" % name)
    for i, c in path:
        print("%6d  %s" % (i + 1, c))
    t = totals(path)
    print("# VALU %d (fp64 %d)  SALU %d  SMEM %d  s_waitcnt %d  s_nop wait states %d  LDS %d  VMEM %d" %
          (t["valu"], t["fp64"], t["salu"], t["smem"], t["waitcnt"], t["nop_states"], t["lds"], t["vmem"]))
    blk = gather_block(lines)
    bt = totals([(0, c) for c in blk])
    print("# block in front of the gather: VALU %d (fp64 %d)  SALU %d  SMEM %d  s_waitcnt %d" %
          (bt["valu"], bt["fp64"], bt["salu"], bt["smem"], bt["waitcnt"]))
    before, after = factor_xors(lines)
    print("# v_xor_b32 between gather and wait: %d, between the wait and the next conditional branch: %d" % (len(before), len(after)))
    print("# drift multiplies read: %s" % " ".join(drift_scalars(lines)))
    print("# vgpr %d  sgpr %d  scratch %d" % resources(body))


if __name__ == "__main__":
    main()
