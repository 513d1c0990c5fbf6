#!/usr/bin/env python3
"""Compare two scripts/isa_digest.py listings of cbet_grid_kernels.hip across the change that made the colour switch of the
four gain-stage kernels three-valued: a kernel of OLD named k<..., false|true, POL> is matched with the
kernel of NEW named k<..., 0|1, POL>; the NEW kernels with 2 there are the BAND instantiations.

    python scripts/isa_band_compare.py OLD.txt NEW.txt

Prints: the kernels without BAND whose instruction count, mnemonic histogram, VGPR, SGPR, LDS or scratch differ from their
partner's (none = `unmoved`); then per BAND instantiation its resources, the wavefronts per CU they allow (512 VGPRs per SIMD
lane, 160 KB of LDS per CU, the kernel's own workgroup size) and its scratch beside that of its DETUNE counterpart."""
import re
import sys

LINE = re.compile(r"^(\S.*?)  body=(\w+)  insts=(\d+)  hist=(\w+)  vgpr=(\d+) sgpr=(\d+) lds=(\d+) scratch=(\d+)$")
TEMPLATED = ("k_gain_field<", "k_gain_field_sym<", "k_pair_amplitude<", "k_exchange_matrix<")
WAVES_PER_GROUP = {"k_gain_field": 4, "k_gain_field_sym": 1, "k_pair_amplitude": 4, "k_exchange_matrix": 4}


def read(path):
    out = {}
    for line in open(path):
        m = LINE.match(line.rstrip("\n"))
        if m:
            out[m.group(1)] = dict(body=m.group(2), insts=int(m.group(3)), hist=m.group(4), vgpr=int(m.group(5)),
                                   sgpr=int(m.group(6)), lds=int(m.group(7)), scratch=int(m.group(8)))
    return out


def old_name(name):
    """NEW's name with the colour switch (the last template argument but one) spelled as OLD spells it; None for BAND."""
    if not name.startswith(TEMPLATED):
        return name
    head, args = name.split("<", 1)
    args = args.rstrip(">").split(", ")
    if args[-2] == "2":
        return None
    args[-2] = {"0": "false", "1": "true"}[args[-2]]
    return "%s<%s>" % (head, ", ".join(args))


def waves_per_cu(name, k):
    per_simd = min(8, 512 // ((k["vgpr"] + 7) // 8 * 8))
    groups_by_lds = (160 * 1024) // k["lds"] if k["lds"] else 1 << 20
    return min(4 * per_simd, groups_by_lds * WAVES_PER_GROUP[name.split("<")[0]])


def main():
    old, new = read(sys.argv[1]), read(sys.argv[2])
    fields = ("insts", "hist", "vgpr", "sgpr", "lds", "scratch")
    moved, matched, band, renamed = [], 0, [], 0
    for name, k in sorted(new.items()):
        partner = old_name(name)
        if partner is None:
            band.append(name)
            continue
        if partner not in old:
            moved.append("%s: no partner in OLD" % name)
            continue
        matched += 1
        diff = [f for f in fields if old[partner][f] != k[f]]
        if diff:
            moved.append("%s: %s" % (name, ", ".join("%s %s -> %s" % (f, old[partner][f], k[f]) for f in diff)))
        elif old[partner]["body"] != k["body"]:
            renamed += 1                    # the body's labels and directives carry the kernel's mangled name, which changed
    missing = [n for n in old if n not in {old_name(m) for m in new}]
    print("# %d kernels of NEW matched with OLD; %d of OLD without a partner; %d BAND instantiations" % (matched, len(missing), len(band)))
    print("# %d matched kernels with equal count, histogram and resources whose body text differs (mangled names in labels, kernel-argument offsets)" % renamed)
    print("# kernels without BAND that moved: %s" % ("none -- unmoved" if not moved else len(moved)))
    for line in moved:
        print(line)
    print("# BAND instantiations: insts vgpr sgpr lds scratch | waves per CU | scratch of the DETUNE counterpart")
    for name in band:
        k = new[name]
        head, args = name.split("<", 1)
        args = args.rstrip(">").split(", ")
        args[-2] = "1"
        twin = new["%s<%s>" % (head, ", ".join(args))]
        print("%s  insts=%d vgpr=%d sgpr=%d lds=%d scratch=%d | %d | %d" % (name, k["insts"], k["vgpr"], k["sgpr"], k["lds"], k["scratch"],
                                                                          waves_per_cu(name, k), twin["scratch"]))


if __name__ == "__main__":
    main()
