#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel.

    tools/asm_equal.py A_DIR B_DIR

Reads every *.gfx950.s of both directories (scripts/build_variant.sh and the Makefile leave one
per source file) and matches functions by symbol name across files, so a kernel that moved to
another source file is compared with itself.  Per function it compares the normalised code and,
for kernels, the .amdhsa_* descriptor lines (VGPR / AGPR / SGPR counts, scratch and LDS size).
Normalisation: comments dropped, .loc / .file / .cfi / alignment-only lines dropped, local labels
(.L...) renumbered in order of first appearance.  A plain text diff keyed by symbol name: it knows
nothing about particular instructions.

Prints one line per function (SAME, or DIFF with the first differing lines), then the functions
present on one side only.  Exit status 1 on any difference.
"""
import glob
import os
import re
import sys

_TYPE = re.compile(r"^\s*\.type\s+([^,\s]+),@function")
_LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
_LOCAL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)*")
_DROP = re.compile(r"^\.(loc|file|cfi_\w+|p2align|align|balign)\b")


def _strip(line):
    return line.split(";", 1)[0].split("//", 1)[0].strip()


def parse(path):
    """{symbol: (code lines, descriptor lines or None)} of one assembly file."""
    lines = open(path, errors="replace").read().split("\n")
    funcs = {m.group(1) for m in map(_TYPE.match, lines) if m}
    code, desc = {}, {}
    cur = None      # function whose body is being read
    kern = None     # kernel whose descriptor is being read
    for raw in lines:
        s = _strip(raw)
        if not s:
            continue
        if s.startswith(".amdhsa_kernel"):
            kern = s.split()[1]
            desc[kern] = []
            continue
        if s.startswith(".end_amdhsa_kernel"):
            kern = None
            continue
        if kern is not None:
            desc[kern].append(" ".join(s.split()))
            continue
        m = _LABEL.match(s)
        if m and m.group(1) in funcs:
            cur = m.group(1)
            code[cur] = []
            continue
        if cur is None:
            continue
        if s.startswith(".size") or s.startswith(".section") or s.startswith(".text") or s.startswith(".Lfunc_end"):
            if s.startswith(".Lfunc_end") or s.startswith(".size"):
                cur = None
            continue
        if _DROP.match(s):
            continue
        code[cur].append(" ".join(s.split()))
    out = {}
    for name, body in code.items():
        ids = {}
        norm = [_LOCAL.sub(lambda m: ids.setdefault(m.group(0), ".L%d" % len(ids)), ln) for ln in body]
        out[name] = (norm, desc.get(name))
    return out


def load(d):
    files = sorted(glob.glob(os.path.join(d, "*.gfx950.s")))
    if not files:
        sys.exit("asm_equal: no *.gfx950.s in %s" % d)
    funcs = {}
    for f in files:
        for name, v in parse(f).items():
            if name in funcs:
                sys.exit("asm_equal: %s is defined twice under %s" % (name, d))
            funcs[name] = v + (os.path.basename(f),)
    return funcs


def first_diff(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return "line %d: %r != %r" % (i + 1, x, y)
    return "length %d != %d" % (len(a), len(b))


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    A, B = load(sys.argv[1]), load(sys.argv[2])
    bad = 0
    for name in sorted(set(A) & set(B)):
        (ca, da, fa), (cb, db, fb) = A[name], B[name]
        kind = "kernel" if da is not None or db is not None else "function"
        where = fa if fa == fb else "%s -> %s" % (fa, fb)
        if ca == cb and da == db:
            print("SAME %s %s (%s, %d lines)" % (kind, name, where, len(ca)))
            continue
        bad += 1
        why = "code " + first_diff(ca, cb) if ca != cb else "descriptor " + first_diff(da or [], db or [])
        print("DIFF %s %s (%s): %s" % (kind, name, where, why))
    for side, X, Y in (("A", A, B), ("B", B, A)):
        for name in sorted(set(X) - set(Y)):
            bad += 1
            print("ONLY-%s %s (%s)" % (side, name, X[name][2]))
    n = len(set(A) & set(B))
    print("%d compared, %d different or unmatched" % (n, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
