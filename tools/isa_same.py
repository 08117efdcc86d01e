#!/usr/bin/env python3
"""Whether two builds of render.hip generated the same code: tools/isa_same.py [-v] A.s B.s
(A.s, B.s: `make -C raytrace2_amd/csrc asm` at two commits, same toolchain). Per function (^_Z...: up to its
.Lfunc_end), with `;` comments and blank lines dropped and the function's number taken out of its .LBB<n>_
labels. Prints the names only one side has, then each function that differs with both instruction counts
(-v: its unified diff too). Exit status 1 if anything differs."""
import difflib
import re
import sys


def functions(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end", text, re.M | re.S):
        lines = [re.sub(r"\.LBB\d+_", ".LBB_", l.split(";", 1)[0].rstrip()) for l in m.group(2).split("\n")]
        out[m.group(1)] = [l for l in lines if l.strip()]
    return out


def instructions(lines):
    return sum(1 for l in lines if l.startswith("\t") and not l.strip().startswith("."))


def main(argv):
    verbose = "-v" in argv
    a_path, b_path = [x for x in argv if x != "-v"]
    a, b = functions(a_path), functions(b_path)
    for n in sorted(set(a) - set(b)):
        print("only in", a_path + ":", n)
    for n in sorted(set(b) - set(a)):
        print("only in", b_path + ":", n)
    differ = [n for n in sorted(set(a) & set(b)) if a[n] != b[n]]
    for n in differ:
        print(f"differs: {n}: {instructions(a[n])} -> {instructions(b[n])} instructions")
        if verbose:
            sys.stdout.write("\n".join(difflib.unified_diff(a[n], b[n], a_path, b_path, lineterm="", n=2)) + "\n")
    print(f"{len(a)} / {len(b)} functions, {len(set(a) & set(b)) - len(differ)} identical, {len(differ)} differ")
    return 1 if differ or set(a) != set(b) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
