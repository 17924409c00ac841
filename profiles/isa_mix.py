#!/usr/bin/env python3
"""Static vector-ALU instruction mix of a kernel translation unit, from the
compiler's assembly listing:

    hipcc -O3 -std=c++17 --offload-arch=gfx950 <the defines of build.py> \\
          --cuda-device-only -S fabric-token-sdk_amd/csrc/k_fexp.hip -o k_fexp.s
    python profiles/isa_mix.py k_fexp.s                    # one line per kernel
    python profiles/isa_mix.py k_fexp.s -k k_fexp_expt -b  # its basic blocks

Per kernel (and with -b per basic block, in listing order) it prints the
number of v_* instructions, how many of them are v_mad_i64_i32 / v_mad_u64_u32
(the limb products), and the count of every other v_* mnemonic, largest first.
Only vector-ALU mnemonics are tallied; every other line of the listing is
skipped.  These are static counts: a block inside a loop is listed once, so
the dynamic count of a path is the sum of its blocks times their trip counts
(compare with SQ_INSTS_VALU, profiles/pmc_kernels.py).
"""
import argparse
import collections
import re

FUNC = re.compile(r"^([A-Za-z_][\w$.]*):")      # a symbol at column 0 opens a function
BLOCK = re.compile(r"^(\.LBB\d+_\d+):")         # basic block label
VALU = re.compile(r"^\s+(v_[a-z0-9_]+)")        # a vector-ALU instruction
BRANCH = re.compile(r"^\s+s_c?branch")          # ends a basic block (nothing is tallied from it)
END = re.compile(r"^\.Lfunc_end\d+:")
MADS = ("v_mad_i64_i32", "v_mad_u64_u32")


def parse(path):
    """{kernel: [(block label, Counter of v_* mnemonics)]} in listing order"""
    out = collections.OrderedDict()
    cur = None
    tail = 0  # unlabelled blocks since the last label
    with open(path) as f:
        for line in f:
            if END.match(line):
                cur = None
                continue
            m = BLOCK.match(line)
            if m:
                if cur is not None:
                    cur.append((m.group(1), collections.Counter()))
                    tail = 0
                continue
            m = FUNC.match(line)
            if m:
                cur = out.setdefault(m.group(1), [])
                cur.append(("entry", collections.Counter()))
                tail = 0
                continue
            if cur is None:
                continue
            if BRANCH.match(line):  # the code after a branch is a block of its own, label or not
                tail += 1
                cur.append(("%s+%d" % (cur[-1][0].split("+")[0], tail), collections.Counter()))
                continue
            m = VALU.match(line)
            if m:
                cur[-1][1][m.group(1)] += 1
    return collections.OrderedDict((k, v) for k, v in out.items() if any(c for _, c in v))


def demangle(name):
    m = re.match(r"_Z(\d+)", name)  # _Z<len><name>...: the plain kernel name is enough here
    return name[m.end():m.end() + int(m.group(1))] if m else name


def row(label, c, top):
    n = sum(c.values())
    mad = sum(c[m] for m in MADS)
    rest = sorted(((v, k) for k, v in c.items() if k not in MADS), reverse=True)[:top]
    return "%-28s %7d %7d %5.1f%%  %s" % (label, n, mad, 100.0 * mad / n if n else 0.0,
                                         " ".join("%s=%d" % (k, v) for v, k in rest))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("listing")
    ap.add_argument("-k", "--kernel", default=None, help="only kernels whose name contains this")
    ap.add_argument("-b", "--blocks", action="store_true", help="one line per basic block")
    ap.add_argument("--min", type=int, default=20, help="with -b: skip blocks with fewer v_* instructions")
    ap.add_argument("--top", type=int, default=8, help="other mnemonics listed per line")
    a = ap.parse_args()
    print("%-28s %7s %7s %6s  %s" % ("kernel / block", "valu", "mad64", "mad%", "other v_* mnemonics"))
    for name, blocks in parse(a.listing).items():
        kname = demangle(name)
        if a.kernel and a.kernel not in kname:
            continue
        total = collections.Counter()
        for _, c in blocks:
            total.update(c)
        print(row(kname, total, a.top))
        if a.blocks:
            for label, c in blocks:
                if sum(c.values()) >= a.min:
                    print(row("  " + label, c, a.top))


if __name__ == "__main__":
    main()
