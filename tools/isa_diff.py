#!/usr/bin/env python3
"""Does a source change leave the GENERATED device code alone?  Compiles every translation unit of build.py's SOURCES, with that
unit's flags plus `-S --cuda-device-only` (hipcc cross-compiles gfx950 without a GPU), once from a second checkout of BASE (a
`git worktree`) and once from this tree, and compares the assembly after dropping comment lines, .file / .ident / .loc /
.section and the __hip_cuid_* lines.  Per unit: `identical`, or the per-opcode count differences, the kernels whose resource
metadata (.vgpr_count, .agpr_count, .sgpr_count, spill counts, LDS and scratch size) changed, and every differing line with
`L` in front of it when it lies inside a loop (between a label and a later branch back to it).

    python3 tools/isa_diff.py [--base REV] [--base-asm DIR] [--save-asm DIR] [UNIT.hip ...]      exit code 1 when a unit differs

--save-asm DIR keeps this tree's normalised assembly in DIR; --base-asm DIR compares against such a directory instead of
checking BASE out (default BASE: HEAD, i.e. the uncommitted changes of the working tree)."""
import collections
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speech_separation_amd.build import HIPCC, SOURCES  # noqa: E402

DROP = re.compile(r"^\s*(;|\.file\b|\.ident\b|\.loc\b|\.section\b|\.cv_)|__hip_cuid_")
META = re.compile(r"\.(vgpr_count|agpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|group_segment_fixed_size|private_segment_fixed_size):")


def asm_of(root, unit):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "unit.s")
        cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC"] + SOURCES[unit] + [
            "-S", "--cuda-device-only", "-w", "-o", out, os.path.join(root, "speech_separation_amd", "csrc", unit)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"{unit} ({root}): hipcc failed\n{r.stderr[-2000:]}")
        return [ln.rstrip() for ln in open(out) if ln.strip() and not DROP.search(ln)]


def loop_lines(lines):
    """indices of the lines that lie between a label and a later branch to it"""
    label_at, inside = {}, set()
    for i, ln in enumerate(lines):
        m = re.match(r"^(\.LBB\w+):", ln)
        if m:
            label_at[m.group(1)] = i
        m = re.match(r"^\s*s_c?branch\w*\s+(\.LBB\w+)", ln)
        if m and m.group(1) in label_at:
            inside.update(range(label_at[m.group(1)], i + 1))
    return inside


def opcodes(lines):
    return collections.Counter(ln.split()[0] for ln in lines if ln[:1] in " \t" and not ln.lstrip().startswith("."))


def resources(lines):
    """{kernel: {field: value}} from the amdhsa metadata at the end of the unit"""
    res, cur = {}, {}
    for ln in lines:
        if re.match(r"^\s*- \.agpr_count:", ln):      # a kernel's entry starts with its first key
            cur = {}
        m = META.search(ln)
        if m:
            cur[m.group(1)] = ln.split(":")[1].strip()
        m = re.match(r"^\s*\.name:\s+(_Z\w+)$", ln)
        if m:
            res[m.group(1)] = cur
    return res


def compare(unit, a, b):
    if a == b:
        print(f"{unit}: identical ({len(a)} lines)")
        return 0
    ca, cb = opcodes(a), opcodes(b)
    counts = {k: (ca[k], cb[k]) for k in sorted(set(ca) | set(cb)) if ca[k] != cb[k]}
    ra, rb = resources(a), resources(b)
    la, lb = loop_lines(a), loop_lines(b)
    print(f"{unit}: DIFFERS ({len(a)} -> {len(b)} lines)")
    print("  per-opcode counts:", "equal" if not counts else ", ".join(f"{k} {x} -> {y}" for k, (x, y) in counts.items()))
    changed = [k for k in sorted(set(ra) | set(rb)) if ra.get(k) != rb.get(k)]
    print("  resource metadata:", "equal for every kernel" if not changed else "")
    for k in changed:
        print(f"    {k[:100]}: {ra.get(k)} -> {rb.get(k)}")
    in_loop = 0
    sm = difflib.SequenceMatcher(None, a, b, autojunk=False)
    for tag, i1, i2, j1, j2 in sm.get_opcodes():
        if tag == "equal":
            continue
        for i in range(i1, i2):
            in_loop += i in la
            print(f"  {'L' if i in la else ' '} -{i + 1}: {a[i].strip()}")
        for j in range(j1, j2):
            in_loop += j in lb
            print(f"  {'L' if j in lb else ' '} +{j + 1}: {b[j].strip()}")
    print(f"  {in_loop} differing lines inside loops")
    return 1


def main():
    argv = sys.argv[1:]
    opt = {}
    for name in ("--base", "--base-asm", "--save-asm"):
        if name in argv:
            i = argv.index(name)
            opt[name] = argv[i + 1]
            del argv[i:i + 2]
    units = argv or list(SOURCES)
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        mine = dict(zip(units, pool.map(lambda u: asm_of(ROOT, u), units)))
        if "--save-asm" in opt:
            os.makedirs(opt["--save-asm"], exist_ok=True)
            for u, lines in mine.items():
                with open(os.path.join(opt["--save-asm"], u + ".s"), "w") as f:
                    f.write("\n".join(lines) + "\n")
        if "--base-asm" in opt:
            base = {u: open(os.path.join(opt["--base-asm"], u + ".s")).read().split("\n")[:-1] for u in units}
        else:
            with tempfile.TemporaryDirectory() as tmp:
                wt = os.path.join(tmp, "base")
                subprocess.run(["git", "-C", ROOT, "worktree", "add", "--detach", wt, opt.get("--base", "HEAD")], check=True, capture_output=True)
                try:
                    base = dict(zip(units, pool.map(lambda u: asm_of(wt, u), units)))
                finally:
                    subprocess.run(["git", "-C", ROOT, "worktree", "remove", "--force", wt], check=True, capture_output=True)
    differing = sum(compare(u, base[u], mine[u]) for u in units)
    print(f"{len(units)} units compared, {differing} differ")
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
