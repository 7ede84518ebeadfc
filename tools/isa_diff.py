#!/usr/bin/env python3
"""Compare two builds of the device code function by function (CPU only).

    tools/isa_diff.py DIR_A DIR_B [--alias SYMBOL_A=SYMBOL_B ...] [--only REGEX]

DIR_A and DIR_B hold assemblies made with the Makefile's flags plus `--cuda-device-only -S`, one *.s per unit (`make -s print-CXXFLAGS` prints the
flags).  Per function symbol: comments dropped, local labels (.LBB<n>_<m>, .Lfunc_end<n>, ...) renumbered in order of appearance, then the instruction
text is compared, and for a kernel its .amdhsa_kernel block too (registers, scratch, LDS, kernarg size).  A function may sit in several units of a
build (a noinline callee is compiled into each unit that calls it): every copy in B is compared with A's.  A kernel must sit in exactly one.
One line per symbol, then the counts; exit status 1 unless every symbol of A is found identical in B.  --alias: a data symbol that was renamed."""
import argparse
import glob
import os
import re
import sys


def functions(directory, alias):
    """-> {symbol: [(unit, instruction text, descriptor text or None), ...]}"""
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        lines = open(path).read().split("\n")
        starts = [i for i, l in enumerate(lines) if re.match(r"\s*\.type\s+\S+,@function", l)]
        for i in starts:
            sym = re.match(r"\s*\.type\s+(\S+),@function", lines[i]).group(1)
            body, desc, labels, in_desc = [], None, {}, False
            for l in lines[i + 2:]:                       # (i + 1 is the symbol's own label)
                l = l.split(";")[0].strip()
                if l.startswith(".Lfunc_end"):
                    break
                if l.startswith(".amdhsa_kernel"):
                    in_desc, desc = True, []
                if in_desc:
                    desc.append(l)
                    in_desc = not l.startswith(".end_amdhsa_kernel")
                elif l and not re.match(r"\.(section|text|p2align)\b", l):
                    l = re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), l)
                    body.append("".join(alias.get(w, w) for w in re.split(r"(\w+)", l)))
            out.setdefault(sym, []).append((os.path.basename(path)[:-2], "\n".join(body), None if desc is None else "\n".join(desc)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("dir_a"), ap.add_argument("dir_b")
    ap.add_argument("--alias", action="append", default=[]), ap.add_argument("--only", default="")
    args = ap.parse_args()
    alias = dict(a.split("=") for a in args.alias)
    a, b = functions(args.dir_a, alias), functions(args.dir_b, {})
    counts = {}
    for sym in sorted(set(a) | set(b)):
        if not re.search(args.only, sym):
            continue
        kernel = any(d is not None for _, _, d in a.get(sym, []) + b.get(sym, []))
        if sym not in a or sym not in b:
            verdict = "only in A" if sym in a else "only in B"
        elif kernel and (len(a[sym]) != 1 or len(b[sym]) != 1):
            verdict = "KERNEL IN SEVERAL UNITS"
        else:
            text = all(t == a[sym][0][1] for _, t, _ in b[sym])
            desc = all(d == a[sym][0][2] for _, _, d in b[sym])
            verdict = "identical" if text and desc else "DIFFERENT " + " and ".join(["instructions"] * (not text) + ["descriptor"] * (not desc))
        counts[verdict] = counts.get(verdict, 0) + 1
        units = lambda side: ",".join(u for u, _, _ in side.get(sym, [])) or "-"
        print("%-24s %-8s %s   A: %s   B: %s" % (verdict, "kernel" if kernel else "function", sym, units(a), units(b)))
    print("; ".join("%d %s" % (n, v) for v, n in sorted(counts.items())) or "no symbols")
    return 0 if set(counts) <= {"identical", "only in B"} and counts else 1


if __name__ == "__main__":
    sys.exit(main())
