#!/usr/bin/env python3
"""Per-kernel comparison of two device assembly files (the `*-gfx950.s` that `hipcc -save-temps` leaves):
    isa_diff.py <parent.s> <branch.s> [old=new ...]
Every `old=new` is a substring rename applied to the parent's text before the comparison, so that a kernel whose mangled name changed (new
template parameters, a new argument list) is compared with its successor instead of being reported GONE / NEW.
A kernel runs from its `_Z...:` label to its `.Lfunc_end`; comment text after `;`, empty lines and the `.loc` / `.file` /
`.cfi` / `.p2align` lines are dropped, and the function's index in its local labels (`.LBB34_10`: it shifts when a kernel elsewhere in the file
changes its name or place) is taken out; the remaining lines are compared.  Exit status 1 if any kernel differs."""
import re
import sys

DROP = re.compile(r"\s*\.(loc|file|cfi\w*|p2align)\b")
LABEL = re.compile(r"\.L([A-Za-z]+)\d+_")


def kernels(path, renames=()):
    out, name, funcs = {}, None, set()
    for line in open(path):
        for old, new in renames:
            line = line.replace(old, new)
        f = re.match(r"\s*\.type\s+(_Z\w+),@function", line)
        if f:
            funcs.add(f.group(1))
        m = re.match(r"(_Z\w+):", line)
        if m and name is None and m.group(1) in funcs:
            name, out[m.group(1)] = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            name = None
            continue
        line = LABEL.sub(r".L\1_", line.split(";", 1)[0].strip())
        if line and not DROP.match(line):
            out[name].append(line)
    return out


def main(parent, branch, *renames):
    a, b = kernels(parent, [r.split("=", 1) for r in renames]), kernels(branch)
    changed = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
    for k in changed:
        print(f"DIFF  {k}: {len(a.get(k, []))} -> {len(b.get(k, []))} lines" if k in a and k in b
              else f"{'GONE' if k in a else 'NEW '}  {k}")
    print(f"{len(set(a) & set(b)) - sum(k in a and k in b for k in changed)} of {len(a)} kernels identical")
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:]))
