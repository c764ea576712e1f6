#!/usr/bin/env python3
"""Compare two builds' device code kernel by kernel (no GPU needed).

  hipcc <the Makefile's flags for the file> --offload-device-only -S k_chol.hip -o base/k_chol.s
  python tools/asm_kernel_diff.py base/k_chol.s -- new/k_chol.s new/k_systiles.s

Every kernel's instruction stream -- comments dropped, block labels .LBB<function>_<block> renumbered
to .LBB_<block>, since the function index changes when kernels move between files -- is compared with
the same kernel's of the other build: "identical" or the first differing line.  A kernel found in
one build only is paired by its demangled name without the parameter list (c++filt), for a build in
which a parameter type moved to another namespace.
"""
import re
import subprocess
import sys


def qualified(name):
    """tblup::(anonymous namespace)::k<1> of a mangled kernel symbol; the symbol without c++filt."""
    try:
        d = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name
    except OSError:
        return name
    depth = 0
    for i in range(len(d) - 1, -1, -1):   # the parameter list: the last top-level (...)
        depth += (d[i] == ")") - (d[i] == "(")
        if depth == 0 and d[i] == "(":
            return d[:i].split(" ", 1)[-1] if d.startswith("void ") else d[:i]
    return d


def pair_renamed(base, new):
    """Kernels in one build only, re-keyed by qualified name where that pairs them one to one."""
    for side, other in ((base, new), (new, base)):
        for name in [n for n in side if n not in other]:
            q = qualified(name)
            if q != name and q not in side:
                side[q] = side.pop(name)


def kernels(paths):
    out = {}
    for path in paths:
        name, body = None, []
        for line in open(path):
            m = re.match(r"(_Z\w+):", line)
            if m:
                name, body = m.group(1), []
                continue
            if name is None:
                continue
            if line.startswith("\t.section") or line.startswith(".Lfunc_end"):
                out[name], name = body, None
                continue
            line = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0]).strip()
            if line:
                body.append(line)
    return out


def main():
    args = sys.argv[1:]
    if "--" not in args:
        sys.exit(__doc__)
    base, new = kernels(args[:args.index("--")]), kernels(args[args.index("--") + 1:])
    pair_renamed(base, new)
    differ = 0
    for name in sorted(set(base) | set(new)):
        a, b = base.get(name), new.get(name)
        if a is None or b is None:
            print(f"{name}: only in the {'second' if a is None else 'first'} build")
            differ += 1
        elif a == b:
            print(f"{name}: identical ({len(a)} lines)")
        else:
            i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            print(f"{name}: DIFFERS ({len(a)} / {len(b)} lines), first at {i}: "
                  f"{a[i] if i < len(a) else '<end>'!r} / {b[i] if i < len(b) else '<end>'!r}")
            differ += 1
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
