#!/usr/bin/env python3
"""Static scan of generated gfx950 assembly for LDS waits that sit out a read just issued (the sibling of tools/wait_scan.py, which
does the same for vmcnt).  The LDS answers a wave's requests in order, so `s_waitcnt lgkmcnt(N)` waits for everything but the N
youngest `ds_*` instructions issued before it; the youngest one it waits for is the (N+1)-th last.  For every kernel loop that
holds MFMAs the scan walks the loop body in program order, looking ONLY at `ds_*`, `s_waitcnt` and `v_mfma*` lines (and counting
`s_barrier`), keeps the list of requests that may still be outstanding (a wait with count N leaves the N youngest) and reports for
every wait that covers something its LEAD: the number of MFMAs between the youngest covered request and the wait.  A wave alone on
its SIMD (the recurrences: one wave per SIMD) hides an LDS round trip behind nothing but its own MFMAs, 32 cycles per 16x16x4, so a
lead of 0-2 is a round trip the wave sits out.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 [unit's flags from build.py] --cuda-device-only -S -o k.s csrc/<unit>.hip
    python3 tools/lds_wait_scan.py k.s [--kernel SUBSTR] [--detail] [--min-lead 4] [--audit]

One line per loop (leads of its covering waits, in program order); --detail lists every wait with the request it covers.
--min-lead N: exit status 1 if a loop of a selected kernel has a covering wait with a lead below N.
--audit: also list, per kernel, every instruction that touches the destination of a `ds_read` before a wait covers it (this one
looks at every line; exit status 1 if there is one).
tests/test_lds_wait_schedule.py holds lstm16x128_kernel's step loop to this (scan_text below).
"""
import re
import sys

_KERNEL = re.compile(r"^(_Z\w+):")
_LABEL = re.compile(r"^(\.LBB\d+_\d+):")
_LGKM = re.compile(r"s_waitcnt\b.*lgkmcnt\((\d+)\)")


def _loops(body):
    """(label, first line, last line) of every loop: from a `Loop Header` label to the last branch back to it."""
    out = []
    for i, l in enumerate(body):
        m = _LABEL.match(l)
        if not m or "Loop Header" not in l:
            continue
        back = re.compile(r"s_c?branch\w*\s+" + re.escape(m.group(1)) + r"\b")
        ends = [j for j in range(i + 1, len(body)) if back.search(body[j])]
        if ends:
            out.append((m.group(1), i, max(ends)))
    return out


def scan_loop(lines):
    """lines: the loop body.  -> dict(mfmas, barriers, ds, waits=[dict(at, n, lead, outstanding, request)]); `at` is the number of
    MFMAs of the loop in front of the wait, `outstanding` the requests that could be in flight when the wait was reached."""
    nmf = nbar = nds = 0
    pending = []                # (MFMAs in front of the request, its text), oldest first
    waits = []
    for l in lines:
        s = l.strip()
        if s.startswith("v_mfma"):
            nmf += 1
        elif s.startswith("s_barrier"):
            nbar += 1
        elif s.startswith("ds_"):
            nds += 1
            pending.append((nmf, s.split(";")[0].strip()))
        elif s.startswith("s_waitcnt"):
            m = _LGKM.search(s)
            if not m:
                continue
            n = int(m.group(1))
            if len(pending) > n:
                at, text = pending[len(pending) - 1 - n]
                waits.append(dict(at=nmf, n=n, lead=nmf - at, outstanding=len(pending), request=text))
                pending = pending[len(pending) - n:] if n else []
    return dict(mfmas=nmf, barriers=nbar, ds=nds, waits=waits)


_VREG = re.compile(r"\bv(?:\[(\d+):(\d+)\]|(\d+))")


def _vregs(text):
    out = set()
    for m in _VREG.finditer(text):
        if m.group(3) is not None:
            out.add(int(m.group(3)))
        else:
            out.update(range(int(m.group(1)), int(m.group(2)) + 1))
    return out


def unlanded_uses(lines):
    """The audit a hand-issued read needs (--audit): the compiler takes the destination of an asm `ds_read` for written where the
    statement stands, so under register pressure it may read, copy, spill or reuse it before the data has landed.  Walks `lines` (a
    kernel body, in layout order) and returns [(read, offending instruction)] for every instruction between a `ds_read*` and the
    first wait that covers it that names one of the read's destination registers."""
    pending = []                # (destination registers, text), oldest first
    bad = []
    for l in lines:
        s = l.split(";")[0].strip()
        if not s or s.endswith(":") or s.startswith("."):
            continue
        if s.startswith("s_waitcnt"):
            m = _LGKM.search(s)
            if m:
                n = int(m.group(1))
                pending = pending[len(pending) - n:] if n and len(pending) > n else ([] if not n else pending)
            continue
        regs = _vregs(s)
        for dst, text in pending:
            if dst & regs:
                bad.append((text, s))
        if s.startswith("ds_"):
            ops = s.split(None, 1)[1] if " " in s else ""
            dst = _vregs(ops.split(",")[0]) if s.startswith("ds_read") else set()
            pending.append((dst, s))
    return bad


def kernel_bodies(text):
    """-> {mangled kernel name: [lines]} of an assembly listing."""
    out, kern = {}, None
    for line in text.splitlines():
        m = _KERNEL.match(line)
        if m:
            kern = m.group(1)
            out[kern] = []
        elif kern is not None:
            if line.startswith(".Lfunc_end"):
                kern = None
            else:
                out[kern].append(line)
    return out


def scan_text(text):
    """-> [dict(kernel, loop, lines, mfmas, barriers, ds, waits)] for every loop with MFMAs of every kernel in an assembly listing."""
    out = []
    kern, body = None, []

    def flush():
        if kern is None:
            return
        for name, lo, hi in _loops(body):
            r = scan_loop(body[lo:hi + 1])
            if r["mfmas"]:
                out.append(dict(kernel=kern, loop=name, lines=hi - lo, **r))

    for line in text.splitlines():
        m = _KERNEL.match(line)
        if m:
            flush()
            kern, body = m.group(1), []
        elif kern is not None:
            body.append(line)
    flush()
    return out


def demangled(name):
    """A short readable form of the kernel names this project has: `ns::kern<...>` stays mangled but loses its argument list."""
    m = re.match(r"_ZN\d+_GLOBAL__N_1(\d+)", name)
    if m:
        k = int(m.group(1))
        rest = name[m.end():]
        base, targs = rest[:k], rest[k:]
        t = re.match(r"I((?:L[a-z]\d+E)+)E", targs)
        if t:
            return base + "<" + ", ".join(re.findall(r"L[a-z](\d+)E", t.group(1))) + ">"
        return base
    return name[:60]


def main(argv):
    files, want, detail, min_lead, audit = [], None, False, None, False
    args = list(argv)
    while args:
        a = args.pop(0)
        if a == "--kernel":
            want = args.pop(0)
        elif a == "--detail":
            detail = True
        elif a == "--audit":
            audit = True
        elif a == "--min-lead":
            min_lead = int(args.pop(0))
        else:
            files.append(a)
    bad = 0
    for path in files:
        with open(path) as f:
            text = f.read()
        loops = scan_text(text)
        if audit:
            for kern, body in kernel_bodies(text).items():
                if want and want not in kern and want not in demangled(kern):
                    continue
                hits = unlanded_uses(body)
                print(f"{path}: {demangled(kern)}: {len(hits)} uses of a ds_read destination before its wait")
                for rd, ins in hits:
                    print(f"    `{ins}`  before the wait for  `{rd}`")
                    bad = 1
        for r in loops:
            if want and want not in r["kernel"] and want not in demangled(r["kernel"]):
                continue
            leads = [w["lead"] for w in r["waits"]]
            short = sum(1 for x in leads if x <= 2)
            print(f"{path}: {demangled(r['kernel'])} loop {r['loop']}: {r['mfmas']} MFMAs, {r['ds']} ds, {r['barriers']} s_barrier, "
                  f"{len(leads)} covering lgkmcnt waits, {short} with lead <= 2, min lead {min(leads) if leads else '-'}")
            print("    leads: " + " ".join(str(x) for x in leads))
            if detail:
                for w in r["waits"]:
                    print(f"    MFMA {w['at']:4d}: lgkmcnt({w['n']}) of {w['outstanding']} outstanding, lead {w['lead']:3d}  <- {w['request']}")
            if min_lead is not None and leads and min(leads) < min_lead:
                bad = 1
    return bad


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
