#!/usr/bin/env python3
"""Line-by-line comparison of the kernel bodies two versions of a .hip file compile to (scripts/isa_digest.py's listing and
normalisation), for a change that adds template arguments: a kernel of OLD is matched with the kernel of NEW that has the
same name, or the same name with `, false` appended to its template arguments (the new switch turned off).  Per kernel: the
number of body lines that differ and the first few of them; kernels of NEW without a partner are listed by name.

    python scripts/isa_body_diff.py OLD.hip NEW.hip [--suffix ", false"] [--show N]"""
import difflib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_digest as D  # noqa: E402


def main():
    args = sys.argv[1:]
    opt = lambda flag, default: args[args.index(flag) + 1] if flag in args else default    # noqa: E731
    suffix, show = opt("--suffix", ", false"), int(opt("--show", 6))
    files = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] not in ("--suffix", "--show"))]
    old, new = (D.kernels(D.listing(f)) for f in files)
    old_names, new_names = D.demangle(sorted(old)), D.demangle(sorted(new))
    by_name = {v: k for k, v in new_names.items()}
    matched, identical = set(), 0
    for mangled, name in sorted(old_names.items(), key=lambda kv: kv[1]):
        partner = name if name in by_name else (name[:-1] + suffix + ">" if name.endswith(">") else name)
        if partner not in by_name:
            print("%s: no partner in %s" % (name, files[1]))
            continue
        matched.add(partner)
        a, b = old[mangled][0], new[by_name[partner]][0]
        lines = [l for l in difflib.unified_diff(a, b, lineterm="", n=0) if not l.startswith(("---", "+++", "@@"))]
        if not lines:
            identical += 1
            print("%s: identical (%d lines)" % (name, len(a)))
            continue
        print("%s -> %s: %d of %d / %d lines differ" % (name, partner, len(lines), len(a), len(b)))
        for l in lines[:show]:
            print("    " + l)
    print("%d kernels compared, %d identical" % (len(matched), identical))
    for name in sorted(set(by_name) - matched):
        print("new: %s" % name)


if __name__ == "__main__":
    main()
