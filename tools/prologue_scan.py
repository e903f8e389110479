#!/usr/bin/env python3
"""Static scan of a recurrence kernel's PROLOGUE in generated gfx950 assembly: how many dependent memory round trips stand
between the kernel's entry and its step loop (the sibling of tools/lds_wait_scan.py, which judges the loop itself).

A workgroup of lstm16x.hip holds a whole CU (512 registers per lane, up to 160 KiB of LDS) from its first instruction on, and its
prologue fetches 130-260 KiB of weights.  Written as ordinary loads the compiler fetched them two 16-byte loads at a time, each
pair behind a `s_waitcnt vmcnt` that drained the pair before: 80 serial round trips per launch in lstm16x128_kernel, 44 in
lstm16x_kernel<64>.  For every kernel the scan takes the instructions from the entry to the header of the first loop that holds
MFMAs, in layout order, and counts

  * loads            vector-memory loads (global / buffer / flat / scratch `_load`, LDS-DMA requests included);
  * BLOCKING GROUPS  keeping the number of loads outstanding, a `s_waitcnt vmcnt(n)` reached with more than n outstanding
                     closes a group if at least one load was issued since the previous closing wait.  A group is a round
                     trip the wave sits out before it may issue the next one;
  * unlanded uses    instructions that name the destination registers (VGPRs or AGPRs) of a load before a wait covers it, and
                     hand-issued loads (inline assembly) still uncovered at the loop header: the compiler takes the destination
                     of an asm load for written where the statement stands, so it may copy or spill it before it has arrived.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -mllvm -amdgpu-mfma-vgpr-form --cuda-device-only -S -o k.s csrc/lstm16x.hip
    python3 tools/prologue_scan.py k.s [--kernel SUBSTR] [--max-groups N]

One line per kernel.  --max-groups N: exit status 1 if a selected kernel has more than N groups or any unlanded use.
tests/test_lstm16x_prologue_scan.py holds the default prologues of lstm16x.hip to this (scan_text below).
"""
import re
import sys

try:
    from tools import lds_wait_scan as W
except ImportError:      # run as a script from tools/
    import lds_wait_scan as W

_LOAD = re.compile(r"^(global|buffer|flat|scratch)_load")
_STORE = re.compile(r"^(global|buffer|flat|scratch)_(store|atomic)")
_VMCNT = re.compile(r"s_waitcnt\b.*vmcnt\((\d+)\)")
_REG = re.compile(r"\b([va])(?:\[(\d+):(\d+)\]|(\d+)\b)")


def _regs(text):
    out = set()
    for m in _REG.finditer(text):
        if m.group(4) is not None:
            out.add((m.group(1), int(m.group(4))))
        else:
            out.update((m.group(1), i) for i in range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def prologue_of(lines):
    """The lines of a kernel body in front of the header of its first loop that holds MFMAs (the whole body if it has none)."""
    heads = [lo for _, lo, hi in W._loops(lines) if any(x.strip().startswith("v_mfma") for x in lines[lo:hi + 1])]
    return lines[:min(heads)] if heads else lines


def scan_prologue(lines):
    """lines: a prologue, layout order.  -> dict(loads, groups, sizes=[loads per group], unlanded=[(load, instruction)],
    pending_asm=[hand-issued loads no wait has covered at the end])."""
    pending = []                # (destination registers, text, hand-issued), oldest first
    since = 0                   # loads issued since the last closing wait
    nloads = 0
    sizes, bad = [], []
    in_asm = False
    for l in lines:
        raw = l.strip()
        if raw.startswith(";;#ASMSTART"):
            in_asm = True
            continue
        if raw.startswith(";;#ASMEND"):
            in_asm = False
            continue
        s = l.split(";")[0].strip()
        if not s or s.endswith(":") or s.startswith("."):
            continue
        if s.startswith("s_waitcnt"):
            m = _VMCNT.search(s)
            if m:
                n = int(m.group(1))
                if len(pending) > n:
                    if since:
                        sizes.append(since)
                        since = 0
                    pending = pending[len(pending) - n:] if n else []
            continue
        regs = _regs(s.split(None, 1)[1] if " " in s else "")
        for dst, text, _ in pending:
            if dst & regs:
                bad.append((text, s))
        if _STORE.match(s):      # counted by vmcnt like a load, in issue order; no destination, no part of a group's size
            pending.append((set(), s, False))
        elif _LOAD.match(s):
            nloads += 1
            since += 1
            ops = s.split(None, 1)[1] if " " in s else ""
            dst = set() if "_load_lds" in s else _regs(ops.split(",")[0])
            pending.append((dst, s, in_asm))
    return dict(loads=nloads, groups=len(sizes), sizes=sizes, unlanded=bad, pending_asm=[t for _, t, a in pending if a])


def scan_text(text):
    """-> [dict(kernel, loads, groups, sizes, unlanded, pending_asm)] for every kernel of an assembly listing that has a loop with MFMAs."""
    out = []
    for kern, body in W.kernel_bodies(text).items():
        pro = prologue_of(body)
        if len(pro) == len(body):
            continue
        out.append(dict(kernel=kern, **scan_prologue(pro)))
    return out


def table(text, want=None):
    rows = []
    for r in scan_text(text):
        if want and want not in r["kernel"] and want not in W.demangled(r["kernel"]):
            continue
        sizes = " ".join(str(x) for x in r["sizes"][:12]) + (" ..." if len(r["sizes"]) > 12 else "")
        rows.append(f"{W.demangled(r['kernel']):34s} {r['loads']:4d} loads  {r['groups']:3d} blocking groups ({sizes})  "
                    f"{len(r['unlanded'])} unlanded uses, {len(r['pending_asm'])} hand-issued loads uncovered at the loop")
    return rows


def main(argv):
    files, want, max_groups = [], None, None
    args = list(argv)
    while args:
        a = args.pop(0)
        if a == "--kernel":
            want = args.pop(0)
        elif a == "--max-groups":
            max_groups = int(args.pop(0))
        else:
            files.append(a)
    bad = 0
    for path in files:
        with open(path) as f:
            text = f.read()
        for row in table(text, want):
            print(row)
        for r in scan_text(text):
            if want and want not in r["kernel"] and want not in W.demangled(r["kernel"]):
                continue
            for rd, ins in r["unlanded"]:
                print(f"    {W.demangled(r['kernel'])}: `{ins}`  before the wait for  `{rd}`")
            if max_groups is not None and (r["groups"] > max_groups or r["unlanded"] or r["pending_asm"]):
                bad = 1
    return bad


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
