#!/usr/bin/env python3
"""Compare the kernels of device-only assembly files, kernel by kernel: instruction text and .amdhsa_* descriptor.

    hipcc $(HIPFLAGS) --cuda-device-only -S unit.hip -o unit.s          (one .s per translation unit)
    tools/isa_compare.py --old old1.s [old2.s ...] --new new1.s [new2.s ...] [--out table.txt]

A refactor that moves kernels between translation units must leave every kernel's code as it was.  Local labels (.LBB<f>_<n>,
.Ltmp<n>, .Lfunc_end<f>, ...) carry the position of the function in its file, so they are renumbered in order of first appearance
inside each kernel before the texts are compared.  Prints one verdict line per kernel; exit status 1 if any kernel differs or the
two sides do not hold the same kernels.
"""
import argparse
import re
import subprocess
import sys

LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")


def kernels(path):
    """{symbol: (text lines, descriptor lines)} of one assembly file"""
    lines = open(path).read().split("\n")
    desc, out = {}, {}
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
        if m:
            j = i
            while not lines[j].strip().startswith(".end_amdhsa_kernel"):
                j += 1
            desc[m.group(1)] = [s.strip() for s in lines[i + 1:j]]
            i = j
        i += 1
    for sym in desc:
        start = next(i for i, s in enumerate(lines) if s.startswith(sym + ":"))
        end = start
        while not re.match(r"\.Lfunc_end\d+:", lines[end]):
            end += 1
        names = {}
        body = []
        for s in lines[start + 1:end]:
            s = s.split(";")[0].rstrip() if not s.lstrip().startswith(";") else ""
            if s.strip():
                body.append(LABEL.sub(lambda mo: names.setdefault(mo.group(0), ".L%d" % len(names)), s))
        out[sym] = (body, desc[sym])
    return out


def demangle(syms):
    try:
        txt = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(syms, txt))
    except (OSError, subprocess.CalledProcessError):
        return {s: s for s in syms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--out")
    a = ap.parse_args()
    old, new, where = {}, {}, {}
    for p in a.old:
        old.update(kernels(p))
    for p in a.new:
        for k, v in kernels(p).items():
            assert k not in new, "kernel %s in two new units" % k
            new[k] = v
            where[k] = p.split("/")[-1]
    names = demangle(sorted(set(old) | set(new)))
    rows, bad = [], 0
    for sym in sorted(set(old) | set(new), key=lambda s: names[s]):
        if sym not in new or sym not in old:
            verdict = "MISSING in new" if sym in old else "NEW kernel"
        else:
            (ot, od), (nt, nd) = old[sym], new[sym]
            verdict = "identical" if ot == nt and od == nd else "DIFFERS (%s)" % ", ".join(
                w for w, x in (("text", ot != nt), ("descriptor", od != nd)) if x)
        bad += verdict != "identical"
        n = len(new.get(sym, old.get(sym))[0])
        rows.append("%-12s %6d  %-26s %s" % (verdict, n, where.get(sym, "-"), names[sym]))
    head = ["%d kernels old, %d new, %d not identical" % (len(old), len(new), bad),
            "%-12s %6s  %-26s %s" % ("verdict", "lines", "unit", "kernel")]
    text = "\n".join(head + rows) + "\n"
    sys.stdout.write(text)
    if a.out:
        open(a.out, "w").write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
