#!/usr/bin/env python3
"""Compare two builds' device code kernel by kernel (no GPU needed).

  hipcc <the Makefile's flags for the file> --offload-device-only -S k_chol.hip -o base/k_chol.s
  python tools/asm_kernel_diff.py base/k_chol.s -- new/k_chol.s new/k_systiles.s

Every kernel's instruction stream -- comments dropped, block labels .LBB<function>_<block> renumbered
to .LBB_<block>, since the function index changes when kernels move between files -- is compared with
the same kernel's of the other build: "identical" or the first differing line.
"""
import re
import sys


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
