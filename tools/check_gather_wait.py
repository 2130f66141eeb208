#!/usr/bin/env python3
"""Checks the generated ISA of the hot-loop step engine (grow_spec2_kernel<16>, csrc/bs_grow_spec.hip): every load
the hot loop issues from inline assembly writes its destination registers AFTER the asm statement, so from the load's
issue until an s_waitcnt vmcnt(N) that covers it no instruction may read or write those registers -- on every path.

The walk starts at each inline-asm block (;;#ASMSTART .. ;;#ASMEND) that issues a global load and models the vector
memory counter: every vector-memory instruction (asm or compiler) joins the queue in issue order, s_waitcnt vmcnt(N)
retires all but the N youngest.  A path ends when no asm load is outstanding any more.
Usage: check_gather_wait.py [file.s]; without an argument the device assembly is produced with hipcc -S (default flags
and -DBS_PROBE, about half a minute each)."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "buildingsegment_amd", "csrc", "bs_grow_spec.hip")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
         "--cuda-device-only", "-S"]
KERNELS = [r"_ZN2bs12_GLOBAL__N_117grow_spec2_kernelILi16EE"]
VMEM = re.compile(r"^(global|buffer|flat|scratch)_(load|store|atomic)\w*")
MAXQ = 63  # the counter saturates: the hardware stalls the issue of a 64th outstanding operation


def device_asm(extra=()):
    out = os.path.join(tempfile.mkdtemp(prefix="bs_isa3_"), "bs_grow_spec.s")
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, *extra, SRC, "-o", out], check=True, stderr=subprocess.DEVNULL)
    return out


def regs_of(text):
    regs = set()
    for m in re.finditer(r"\b([va])\[(\d+):(\d+)\]", text):
        regs |= {(m.group(1), r) for r in range(int(m.group(2)), int(m.group(3)) + 1)}
    for m in re.finditer(r"\b([va])(\d+)\b", text):
        regs.add((m.group(1), int(m.group(2))))
    return regs


def dest_of(op, args):
    """Registers a vector-memory instruction writes when it completes (empty for stores and no-return atomics)."""
    if "_lds" in op or op.split("_")[1] == "store":
        return frozenset()
    if op.split("_")[1] == "atomic" and not re.search(r"\bsc0\b|\bglc\b", args):
        return frozenset()
    first = args.split(",")[0]
    return frozenset(regs_of(first))


def check_kernel(lines, st, en, name):
    labels = {m.group(1): i for i in range(st, en) for m in [re.match(r"^(\.LBB\d+_\d+):", lines[i])] if m}
    bad, firsts = [], []  # the first global load of every asm block: one walk each
    pending = False
    for i in range(st, en):
        if ";;#ASMSTART" in lines[i]:
            pending = True
        elif ";;#ASMEND" in lines[i]:
            pending = False
        elif pending and re.match(r"^\s*global_load", lines[i]):
            firsts.append(i)
            pending = False
    for i0 in firsts:
        seen = set()
        work = [(i0, ())]  # (line, queue of (is_asm, dest regs), oldest first)
        while work:
            k, q = work.pop()
            in_asm = True
            while k < en:
                if (k, q) in seen:
                    break
                seen.add((k, q))
                raw = lines[k]
                if ";;#ASMSTART" in raw:
                    in_asm = True
                elif ";;#ASMEND" in raw:
                    in_asm = False
                l = raw.split(";")[0].strip()
                if not l or l.endswith(":") or l.startswith("."):
                    k += 1
                    continue
                live = set().union(*[d for a, d in q if a]) if q else set()
                op = l.split()[0]
                args = l[len(op):]
                if live and regs_of(args) & live:
                    bad.append("%s:%d: %s (in flight: %s)" % (name, k + 1, l, sorted(regs_of(args) & live)[:4]))
                if VMEM.match(op):
                    q = (q + ((in_asm and "_load" in op, dest_of(op, args)),))[-MAXQ:]
                m = re.search(r"vmcnt\((\d+)\)", l) if op == "s_waitcnt" else None
                if m:
                    n = int(m.group(1))
                    q = q[len(q) - n:] if n < len(q) else q
                if not any(a for a, d in q):
                    break  # every asm load of this walk has landed
                if op.startswith("s_endpgm"):
                    break
                m = re.match(r"s_(c?branch\w*)\s+(\.LBB\d+_\d+)", l)
                if m:
                    work.append((labels[m.group(2)], q))
                    if m.group(1) == "branch":
                        break
                k += 1
    return len(firsts), bad


def check(path):
    """Returns (number of asm load blocks walked, list of offending lines)."""
    lines = open(path).read().split("\n")
    walked, bad = 0, []
    for kern in KERNELS:
        st = [i for i, l in enumerate(lines) if re.match("^" + kern + r".*:", l)]
        if not st:
            raise RuntimeError("%s not found in %s" % (kern, path))
        st = st[0]
        en = next(i for i in range(st, len(lines)) if lines[i].startswith(".Lfunc_end"))
        n, b = check_kernel(lines, st, en, os.path.basename(path) + ":" + kern[-16:])
        walked += n
        bad += b
    return walked, bad


if __name__ == "__main__":
    paths = sys.argv[1:] or [device_asm(), device_asm(["-DBS_PROBE"])]
    rc = 0
    for p in paths:
        n, bad = check(p)
        print("%s: %d asm load blocks walked, %d offending instructions" % (p, n, len(bad)))
        for b in bad:
            print("  " + b)
        rc |= 1 if bad or n < 4 else 0
    sys.exit(rc)
