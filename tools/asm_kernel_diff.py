#!/usr/bin/env python3
r"""Per-kernel comparison of two sets of gfx950 assembly listings (hipcc --cuda-device-only -S):
did moving code between translation units change any kernel?

    asm_kernel_diff.py --old OLD.s [OLD.s ...] --new NEW.s [NEW.s ...] [--show] [--opcodes]
                       [--rename RE REPL ...]

Each listing is split at its kernel symbols (the .amdhsa_kernel names).  A kernel is its instruction
stream (from its label to .Lfunc_end) and its descriptor (.amdhsa_* lines, and the .set lines the
descriptor's expressions refer to: VGPRs, SGPRs, LDS, scratch).  Before comparing, what depends only on
a kernel's place in its file is normalised: `;` comments and section switches are dropped, the function number in local
labels (.LBB<n>_, .Lfunc_*<n>, .LJTI<n>_, .LCPI<n>_) is blanked, and the per-unit __hip_cuid_* symbol is
masked.  Prints SAME or DIFF per kernel, and ONLY-OLD / ONLY-NEW for a kernel of one side; exits 1
unless every kernel is SAME.  --show adds a unified diff of every DIFF.  --rename RE REPL (repeatable)
rewrites the new listings' text with re.sub before they are split, for a template that gained a
parameter: `--rename 'k_pass_aILi(\d)ELb0EE' 'k_pass_aILi\1EE'` gives k_pass_a<D, false> the name
k_pass_a<D> had.  --opcodes splits the DIFFs: a kernel whose descriptor is identical and whose
instruction streams hold the same mnemonics the same number of times (the compiler ordered them or
named their registers differently) is REORDER, which does not fail the run.  CPU only.
"""
import argparse
import collections
import difflib
import re
import sys

LABEL = re.compile(r"\.L(BB|JTI|CPI|func_begin|func_end)\d+")
CUID = re.compile(r"__hip_cuid_[0-9a-f]+")


def normalise(line):
    line = line.split(";", 1)[0]
    line = LABEL.sub(lambda m: ".L%s#" % m.group(1), line)
    line = CUID.sub("__hip_cuid_#", line)
    return " ".join(line.split())


def kernels(path, renames=()):
    """{symbol: (instruction lines, descriptor lines)} of one listing"""
    text = open(path).read()
    for pat, repl in renames:
        text = re.sub(pat, repl, text)
    lines = text.split("\n")
    names = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
    out = {}
    for sym in names:
        body, desc = [], []
        state = 0   # 0 before the label, 1 instructions, 2 descriptor, 3 after it
        for raw in lines:
            s = raw.split(";", 1)[0].strip()
            if state == 0:
                if s == sym + ":":
                    state = 1
                continue
            if s.startswith(".amdhsa_kernel "):
                state = 2
                continue
            if s == ".end_amdhsa_kernel":
                state = 3
                continue
            if state == 3 and s.startswith(".Lfunc_end"):
                break
            n = normalise(raw)
            # (.text: the section switch behind a plain kernel; a template's instance has .section there)
            if not n or n.startswith(".section") or n.startswith(".p2align") or n == ".text":
                continue
            (desc if state == 2 else body).append(n)
        assert state == 3, "no descriptor found for " + sym
        desc += [normalise(l) for l in lines if l.strip().startswith(".set " + sym + ".")]
        out[sym] = (body, desc)
    return out


def figures(desc):
    """the descriptor's resource figures, for the report"""
    d = {}
    for l in desc:
        p = l.replace(",", " ").split()
        if p[0] == ".set":
            d[p[1].rsplit(".", 1)[1]] = p[2]
        elif len(p) == 2:
            d[p[0]] = p[1]
    return "vgpr %s sgpr %s lds %s scratch %s" % (d.get("num_vgpr", "?"), d.get("numbered_sgpr", "?"),
                                                  d.get(".amdhsa_group_segment_fixed_size", "?"),
                                                  d.get("private_seg_size", "?"))


def opcodes(body):
    """the multiset of a stream's instruction mnemonics (labels and directives left out)"""
    return collections.Counter(l.split()[0] for l in body if not l.endswith(":") and not l.startswith("."))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--show", action="store_true", help="print a unified diff of every DIFF")
    ap.add_argument("--opcodes", action="store_true",
                    help="report a DIFF with an identical descriptor and mnemonic multiset as REORDER (passes)")
    ap.add_argument("--rename", nargs=2, action="append", default=[], metavar=("RE", "REPL"),
                    help="re.sub applied to the new listings' text")
    a = ap.parse_args()
    side = []
    for paths, renames in ((a.old, ()), (a.new, a.rename)):
        ks = {}
        for p in paths:
            for sym, k in kernels(p, renames).items():
                assert sym not in ks, "kernel in two listings of one side: " + sym
                ks[sym] = k
        side.append(ks)
    old, new = side
    bad = 0
    count = {"SAME": 0, "REORDER": 0, "DIFF": 0, "ONLY-OLD": 0, "ONLY-NEW": 0}
    for sym in sorted(set(old) | set(new)):
        if sym not in new or sym not in old:
            verdict = "ONLY-OLD" if sym in old else "ONLY-NEW"
            bad += 1
        elif old[sym] == new[sym]:
            verdict = "SAME"
        elif a.opcodes and old[sym][1] == new[sym][1] and opcodes(old[sym][0]) == opcodes(new[sym][0]):
            verdict = "REORDER"
        else:
            verdict = "DIFF"
            bad += 1
        count[verdict] += 1
        k = new.get(sym) or old[sym]
        print("%-8s %s  [%d lines, %s]" % (verdict, sym, len(k[0]), figures(k[1])))
        if a.show and verdict in ("DIFF", "REORDER"):
            for part in (0, 1):
                sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(old[sym][part], new[sym][part],
                                                                             "old", "new", lineterm="", n=2))
    print("%d kernels: %s" % (len(set(old) | set(new)), ", ".join("%d %s" % (v, k) for k, v in count.items() if v)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
