#!/usr/bin/env python3
"""Per-kernel digest of the gfx950 code a .hip file compiles to (cross-compiled: no GPU needed), for refactors that must
leave the emitted code alone.  The device listing is built the way tests/test_isa_audit.py's `listing` fixture builds it
(build.FLAGS, -S --cuda-device-only); headers are taken from the tree the FILE lies in, so a `git archive` of another
commit can be digested with today's flags.  Per kernel, one line:

    <demangled name>  body=<sha256/16>  insts=<count>  hist=<sha256/16>  vgpr=.. sgpr=.. lds=.. scratch=..

body: the kernel's instructions, labels and directives with comments and blank lines dropped, the function number
taken out of the compiler's block labels (.LBB<n>_<k>) and the statement number that `%=` puts at the end of an
inline-assembly label (.Lrw_0_<n>) replaced by N -- it counts the assembly statements in front, kernel or not; hist: the sorted "mnemonic count" table; the four resource
fields are next_free_vgpr, next_free_sgpr, group_segment_fixed_size and private_segment_fixed_size.

    python scripts/isa_digest.py FILE.hip [FILE.hip ...] [--hist NAME_PART]     (--hist: also print that kernel's table)
"""
import collections
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cbet_raytracing_3d_amd import build  # noqa: E402


# a label of an inline-assembly block, `.Lrw_0_%=` and the like: `%=` becomes the statement's number in the file
LABEL_UID = re.compile(r"(\.L(?!BB)[A-Za-z]\w*?_)\d+\b")


def listing(path):
    csrc = os.path.dirname(os.path.abspath(path))
    include = os.path.join(os.path.dirname(os.path.dirname(csrc)), "include")
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "listing.s")
        subprocess.run([build.hipcc()] + flags + ["-S", "--cuda-device-only", "-I", include, "-I", csrc, "-o", out, path],
                       check=True, capture_output=True, timeout=1800)
        return open(out).read()


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool:
        return {n: n for n in names}
    out = subprocess.run([tool] + names, check=True, capture_output=True, text=True).stdout.split("\n")
    # "void cbet::(anonymous namespace)::k<...>(arguments)" -> "k<...>"
    return {n: re.sub(r"^void |cbet::\(anonymous namespace\)::", "", d[:d.rfind("(")]) for n, d in zip(names, out)}


def kernels(text):
    """name -> (code lines, metadata) of every kernel of a device listing."""
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M):
        m = re.search(r"^%s:[^\n]*\n(.*?)^\s*\.amdhsa_kernel %s\n(.*?)^\s*\.end_amdhsa_kernel" % (re.escape(name), re.escape(name)),
                      text, re.S | re.M)
        code = [LABEL_UID.sub(r"\1N", re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0].strip())) for l in m.group(1).splitlines()]
        out[name] = ([l for l in code if l], dict(re.findall(r"\.amdhsa_(\w+)\s+(\S+)", m.group(2))))
    return out


def sha(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]


def main():
    args = sys.argv[1:]
    show = args[args.index("--hist") + 1] if "--hist" in args else None
    files = [a for i, a in enumerate(args) if a != "--hist" and (i == 0 or args[i - 1] != "--hist")]
    for path in files:
        ks = kernels(listing(path))
        names = demangle(sorted(ks))
        print("# " + os.path.basename(path))
        for name in sorted(ks, key=lambda n: names[n]):
            code, meta = ks[name]
            insts = [l.split()[0] for l in code if not l.endswith(":") and not l.startswith(".")]
            table = ["%s %d" % kv for kv in sorted(collections.Counter(insts).items())]
            print("%s  body=%s  insts=%d  hist=%s  vgpr=%s sgpr=%s lds=%s scratch=%s" % (
                names[name], sha(code), len(insts), sha(table), meta["next_free_vgpr"], meta["next_free_sgpr"],
                meta["group_segment_fixed_size"], meta["private_segment_fixed_size"]))
            if show and show in names[name]:
                print("\n".join("    " + t for t in table))


if __name__ == "__main__":
    main()
