#!/usr/bin/env python3
"""Where do a stage loop's waits sit?  (No GPU needed.)

  python tools/stage_waits.py [--check] [--asm FILE.s] tblup_amd/csrc/k_chol.hip

Compiles one source file of tblup_amd/csrc to gfx950 device assembly with the Makefile's own flags
(read from `make -n`, so SCHED_SRCS keep their scheduler option) -- or reads --asm -- and, for every
loop of every kernel that holds at least 32 MFMAs and an LDS-DMA op, prints the loop's sequence of

  [vmcnt(N)]  a wait on the vector-memory counter      |barrier|  s_barrier
  A           LDS-DMA op (global_load_lds_*)            G          global load into registers
  S           scratch access (a spill)                  Mxn        a run of n MFMAs

in program order, e.g. the off-diagonal GEMM1 stage loop

  [vmcnt(8)] |barrier| AAAA [vmcnt(7)] Mx8 G [vmcnt(7)] Mx8 G ... [vmcnt(7)] Mx8 G

A loop is a block label and a later branch back to it; of nested loops that qualify only the
innermost are printed.

--check: the 64-MFMA loops of the k_chol_offdiag kernels (the GEMM1 stage loop of gemm1_a32) must
exist, hold no scratch access, and hold no vmcnt wait below 7 between the stage's barrier and its
last MFMA: with 8 B-operand loads in flight per stage, a lower count waits for a load issued less
than a k-step before (the next stage's prefetch), which exposes its latency.  Exit status 1 otherwise.
"""
import argparse
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tblup_amd", "csrc")


def compile_line(src):
    """The Makefile's compile command for `src` (a file of csrc), as an argument list."""
    name = os.path.basename(src)
    obj = "stage_waits_obj/" + os.path.splitext(name)[0] + ".o"
    out = subprocess.run(["make", "-n", "-B", "-C", CSRC, "OBJDIR=stage_waits_obj", obj], capture_output=True,
                         text=True, check=True).stdout
    for line in out.splitlines():
        words = shlex.split(line)
        if "-c" in words and name in words:
            return words
    sys.exit(f"stage_waits: no compile line for {name} in `make -n`:\n{out}")


def device_asm(src, path):
    words = compile_line(src)
    i = words.index("-c")
    words[i:i + 1] = ["--cuda-device-only", "-S"]
    words[words.index("-o") + 1] = path
    subprocess.run(words, cwd=CSRC, check=True)


def kernels(path):
    """name -> instruction lines (comments dropped; block labels kept as 'label:')."""
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name], name = body, None
            continue
        line = line.split(";")[0].strip()
        if line and not line.startswith(".") or re.match(r"\.LBB\d+_\d+:", line):
            body.append(line)
    return out


def demangle(name):
    try:
        return subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name
    except OSError:
        return name


def loops(body):
    """(start, end) index pairs of label .. backward branch to it."""
    at = {ln[:-1]: i for i, ln in enumerate(body) if ln.endswith(":")}
    spans = []
    for i, ln in enumerate(body):
        m = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", ln)
        if m and m.group(1) in at and at[m.group(1)] < i:
            spans.append((at[m.group(1)], i))
    return spans


def tokens(lines):
    """[(kind, value)]: kind in 'wait' (value N), 'barrier', 'A', 'G', 'S', 'M' (value run length)."""
    out = []
    for ln in lines:
        op = ln.split()[0]
        if op == "s_waitcnt":
            m = re.search(r"vmcnt\((\d+)\)", ln)
            if m:
                out.append(("wait", int(m.group(1))))
        elif op == "s_barrier":
            out.append(("barrier", 0))
        elif op.startswith("global_load_lds"):
            out.append(("A", 0))
        elif op.startswith("global_load"):
            out.append(("G", 0))
        elif op.startswith("scratch_"):
            out.append(("S", 0))
        elif op.startswith("v_mfma") or op.startswith("v_smfma"):
            if out and out[-1][0] == "M":
                out[-1] = ("M", out[-1][1] + 1)
            else:
                out.append(("M", 1))
    return out


def show(toks):
    parts, run = [], ""
    for kind, v in toks:
        if kind in "AGS" and len(kind) == 1:
            run += kind
            continue
        if run:
            parts.append(run)
            run = ""
        parts.append(f"[vmcnt({v})]" if kind == "wait" else "|barrier|" if kind == "barrier" else f"Mx{v}")
    if run:
        parts.append(run)
    return " ".join(parts)


def stage_loops(body):
    """Token lists of the innermost loops with >= 32 MFMAs and an LDS-DMA op."""
    found = []
    for a, b in loops(body):
        toks = tokens(body[a:b + 1])
        if sum(v for k, v in toks if k == "M") >= 32 and any(k == "A" for k, _ in toks):
            found.append((a, b, toks))
    return [(a, b, t) for a, b, t in found
            if not any((a2, b2) != (a, b) and a <= a2 and b2 <= b for a2, b2, _ in found)]


def check_loop(toks):
    """Complaints about one 64-MFMA GEMM1 stage loop."""
    bad = []
    if any(k == "S" for k, _ in toks):
        bad.append("scratch access in the loop")
    bar = next((i for i, (k, _) in enumerate(toks) if k == "barrier"), None)
    if bar is None:
        bad.append("no barrier in the loop")
    else:
        toks = toks[bar:] + toks[:bar]   # the compiler may rotate the loop: one stage, from its barrier
        last_m = max(i for i, (k, _) in enumerate(toks) if k == "M")
        low = [v for k, v in toks[:last_m] if k == "wait" and v < 7]
        if low:
            bad.append("vmcnt waits below 7 between the barrier and the last MFMA: " + ", ".join(map(str, low)))
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("source", help="a .hip file of tblup_amd/csrc")
    ap.add_argument("--asm", help="read this device assembly (of `source`) instead of compiling")
    ap.add_argument("--check", action="store_true", help="fail on a GEMM1 stage loop with early waits or spills")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        path = args.asm
        if path is None:
            path = os.path.join(tmp, "dev.s")
            device_asm(args.source, path)
        ks = kernels(path)
    failures, checked = [], 0
    for name in sorted(ks):
        found = 0
        for a, b, toks in stage_loops(ks[name]):
            n = sum(v for k, v in toks if k == "M")
            print(f"{demangle(name)}\n  loop of {n} MFMAs, {b - a + 1} lines:\n    {show(toks)}")
            if args.check and "k_chol_offdiag" in name and n == 64:
                found += 1
                failures += [f"{demangle(name)}: {msg}" for msg in check_loop(toks)]
        if args.check and "k_chol_offdiag" in name and not found:
            failures.append(f"{demangle(name)}: no 64-MFMA stage loop found")
        checked += found
    if args.check:
        if not checked:
            failures.append("no 64-MFMA stage loop found in a k_chol_offdiag kernel")
        for f in failures:
            print("CHECK FAILED:", f)
        if failures:
            return 1
        print(f"check ok: {checked} GEMM1 stage loops")
    return 0


if __name__ == "__main__":
    sys.exit(main())
