#!/usr/bin/env python3
"""Hazards the compiler's recogniser cannot see because the instructions sit in inline assembly -- checked in the GENERATED
code (hipcc cross-compiles gfx950 without a GPU):
  * an LDS-DMA request (global_load_lds_*) reads M0: the ISA asks for one wait state behind the scalar write of M0;
  * a store of more than 8 bytes reads its data registers for a few cycles after issue: the next instruction must not be a
    vector write (round 5, dgrad_t.hip: without the s_nop lanes 8-15 / 24-31 of each half stored the NEXT store's values);
  * a vector-memory instruction that takes a SCALAR operand (base pointer) needs five wait states behind a VALU write of that
    register (v_readlane of a spilled SGPR, v_readfirstlane): the statement cannot know what the allocator put in front of it, so
    every such statement starts with s_nop 4 (round 5, dgrad_r.hip: a request with a stale base = memory access fault);
  * dgrad_t.hip loads its weights into AGPRs by loads the compiler does not count: a register copy (v_accvgpr_*) or a spill
    (scratch_*) anywhere in the kernel could read them before they have arrived;
  * the tile-ticket atomic of dgrad_t / dgrad_r / gemm_t (vmem_asm.h, TicketLoop) returns into a VGPR the compiler does not know
    to be pending: on every path from the atomic to the kernel's end no other instruction may write that register before a
    s_waitcnt vmcnt(n) that covers the atomic (n <= the vector-memory operations issued behind it on that path) -- a late return
    would overwrite lane 0 of whatever value the allocator had put there.
    python3 tools/asm_hazards.py        exit code 1 and a list when something is found"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speech_separation_amd", "csrc")
FILES = ["dgrad_t.hip", "dgrad_r.hip", "gemm_t.hip", "attn_block2.hip", "lstm16x.hip", "fcln.hip"]
NO_VGPR_FORM = {"dgrad_r.hip"}
TICKET_LOOP = {"dgrad_t.hip", "dgrad_r.hip", "gemm_t.hip"}
VMEM = re.compile(r"(global|buffer|scratch|flat)_(load|store|atomic)")


def asm_of(src):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, os.path.splitext(src)[0] + ".s")
        cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC"] + ([] if src in NO_VGPR_FORM else ["-mllvm", "-amdgpu-mfma-vgpr-form"]) + [
            "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, src)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"{src}: hipcc failed\n{r.stderr[-2000:]}")
        return [ln.strip() for ln in open(out) if ln.strip() and not ln.strip().startswith(";") or ln.strip().startswith(";;#")]


def vgprs_written(ln):
    """numbers of the VGPRs an instruction writes (its leading register operands, where the mnemonic has a vector destination)"""
    m = re.match(r"(\S+)\s+(.*)", ln)
    if not m or ln.startswith((";", ".")):
        return set()
    op, ops = m.group(1), [o.strip() for o in m.group(2).split(",")]
    if op.startswith("s_") or "_store" in op or op.startswith("global_load_lds") or ("_atomic" in op and " sc0" not in ln and " glc" not in ln):
        return set()
    if op.startswith("ds_") and not any(k in op for k in ("read", "rtn", "permute", "swizzle")):
        return set()
    out = set()
    for o in ops[:2 if "swap" in op else 1]:
        r = re.match(r"^v(\d+)$", o) or re.match(r"^v\[(\d+):(\d+)\]$", o)
        if r:
            out.update(range(int(r.group(1)), int(r.groups()[-1]) + 1))
    return out


def sregs(operand):
    r = re.match(r"^s(\d+)$", operand) or re.match(r"^s\[(\d+):(\d+)\]$", operand)
    return set(range(int(r.group(1)), int(r.groups()[-1]) + 1)) if r else set()


def ticket_register_hazards(src, lines):
    """Every hand-issued returning global_atomic_add: walk all paths from it (see the module's docstring).  The four-way dispatch
    of the tile loop is compiled into flags -- s_mov_b64 s[a:b], 0 / -1, tested by s_and_b64 / s_andn2_b64 vcc, exec, s[a:b] and
    s_cbranch_vccz / vccnz -- so the walk carries what a path knows about such pairs (constants, and the outcome of an earlier test
    of the same pair) and does not follow a branch that contradicts it; everything else it does not understand it follows both ways."""
    bad, n = set(), 0
    label_at = {m.group(1): i for i, ln in enumerate(lines) for m in [re.match(r"^(\.LBB\d+_\d+):", ln)] if m}
    in_asm = False
    for start, ln in enumerate(lines):
        in_asm = ln.startswith(";;#ASMSTART") or (in_asm and not ln.startswith(";;#ASMEND"))
        m = re.match(r"global_atomic_add v(\d+),.* sc0", ln)
        if not (in_asm and m):
            continue
        n += 1
        dst = int(m.group(1))
        seen, work = set(), [(start + 1, 0, frozenset(), None)]      # line, operations behind the atomic, {(pair, truth)}, vcc
        while work:
            i, younger, known, vcc = work.pop()      # vcc: True / False (nonzero or not), or (pair, negated) of an unknown pair
            known = dict(known)
            while i < len(lines):
                state = (i, younger, frozenset(known.items()), vcc)
                if state in seen:
                    break
                seen.add(state)
                cur = lines[i]
                op, _, rest = cur.partition(" ")
                ops = [o.strip() for o in rest.split(",")]
                w = re.match(r"s_waitcnt .*vmcnt\((\d+)\)", cur)
                if (w and int(w.group(1)) <= younger) or op in ("s_endpgm", "s_setpc_b64", "s_swappc_b64"):
                    break      # covered, or the kernel's end
                if dst in vgprs_written(cur):
                    bad.add(f"{src}: v{dst}, the destination of the ticket atomic in line {start}, is written before a wait covers it: {cur}")
                    break
                if VMEM.match(cur):
                    younger = min(younger + 1, 64)
                b = re.match(r"s_(c?)branch(_\w+)?\s+(\.LBB\d+_\d+)", cur)
                if b and not b.group(1):
                    i = label_at[b.group(3)]
                    continue
                if b:
                    take = [True, False]
                    if b.group(2) in ("_vccz", "_vccnz") and vcc is not None:
                        if isinstance(vcc, bool):
                            take = [vcc == (b.group(2) == "_vccnz")]
                        else:      # both ways, each with what it says about the pair
                            pair, neg = vcc
                            for t in take:
                                nonzero = t == (b.group(2) == "_vccnz")
                                k2 = dict(known)
                                k2[pair] = nonzero != neg
                                if t:
                                    work.append((label_at[b.group(3)], younger, frozenset(k2.items()), nonzero))
                                else:
                                    known, vcc = k2, nonzero
                            i += 1
                            continue
                    if True in take:
                        work.append((label_at[b.group(3)], younger, frozenset(known.items()), vcc))
                    if False not in take:
                        break
                    i += 1
                    continue
                # what the instruction does to the flags
                if op in ("s_and_b64", "s_andn2_b64") and ops[0] == "vcc" and ops[1] == "exec":
                    v = known.get(ops[2])
                    neg = op == "s_andn2_b64"
                    vcc = (v != neg) if v is not None else ((ops[2], neg) if sregs(ops[2]) else None)
                elif ops and (ops[0] == "vcc" or ops[0].startswith("vcc_")):
                    vcc = None
                elif ops and sregs(ops[0]) and not op.startswith(("s_cmp", "s_bitcmp", "s_waitcnt", "s_nop")):
                    hit = sregs(ops[0])
                    const = known.get(ops[1]) if op == "s_mov_b64" and len(ops) > 1 and sregs(ops[1]) else {"0": False, "-1": True}.get(ops[1]) if op == "s_mov_b64" else None
                    known = {k: v for k, v in known.items() if not (sregs(k) & hit)}
                    if not isinstance(vcc, bool) and vcc is not None and sregs(vcc[0]) & hit:
                        vcc = None      # the pair changes between the test and the branch: nothing to learn from it
                    if const is not None:
                        known[ops[0]] = const
                i += 1
    return n, sorted(bad)


def main():
    bad = []
    for src in FILES:
        lines = asm_of(src)
        n_dma = n_store = n_sbase = 0
        in_asm = False
        block_start = 0
        func = "?"
        for i, ln in enumerate(lines):
            if ln.endswith(":") and ln.startswith("_Z"):
                func = ln[:60]
            if ln.startswith(";;#ASMSTART"):
                in_asm = True
                block_start = i
                continue
            if ln.startswith(";;#ASMEND"):
                in_asm = False
                continue
            if not in_asm:
                continue
            if re.match(r"global_(load|store|atomic)", ln) and re.search(r"s\[\d+:\d+\]", ln):
                n_sbase += 1
                nops = [int(p.split()[1]) for p in lines[block_start + 1:i] if p.startswith("s_nop")]
                if not nops or max(nops) < 4:
                    bad.append(f"{src} {func}: vector-memory instruction with a scalar base and no s_nop 4 in front of it in its statement: {ln}")
            if ln.startswith("global_load_lds"):
                n_dma += 1
                prev = lines[block_start + 1:i]      # the statement's own instructions in front of the request
                k = max((j for j, p in enumerate(prev) if p.startswith("s_mov_b32 m0")), default=None)
                if k is None or not any(not p.startswith("s_mov_b32 m0") for p in prev[k + 1:]):
                    bad.append(f"{src} {func}: LDS-DMA directly behind the write of M0: {prev} -> {ln}")
            if re.match(r"global_store_dwordx[34]", ln):
                n_store += 1
                if not lines[i + 1].startswith("s_nop"):
                    bad.append(f"{src} {func}: wide store in inline assembly without a wait state behind it: {ln} / {lines[i + 1]}")
        if src in ("dgrad_t.hip", "gemm_t.hip"):
            body = "\n".join(lines)
            for pat in ("v_accvgpr_", "scratch_"):
                if pat in body:
                    bad.append(f"{src}: {body.count(pat)} x {pat} (weights loaded by uncounted loads must not be copied or spilled)")
        n_ticket = 0
        if src in TICKET_LOOP:
            n_ticket, found = ticket_register_hazards(src, lines)
            bad += found
        print(f"{src}: {n_dma} hand-issued LDS-DMA requests, {n_store} hand-issued wide stores, {n_sbase} scalar-base operands checked"
              + (f", {n_ticket} ticket atomics followed to the kernel's end" if src in TICKET_LOOP else ""))
    for b in bad:
        print("HAZARD:", b)
    print(f"{len(bad)} hazards")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
