"""The prologues of lstm16x.hip, judged in the GENERATED code (no GPU needed: hipcc cross-compiles).

A workgroup of the fused recurrences holds a whole CU from its first instruction, and the prologue fetches 130-260 KiB of weights.
Written as ordinary loads the compiler fetched them a pair of 16-byte loads at a time, every pair behind a wait that drained the
one before: 80 dependent round trips per workgroup in lstm16x128_kernel, 44 in lstm16x_kernel<64> (tools/prologue_scan.py counts
them as blocking load groups).  The default prologue (engine option lstm_prologue = 1) issues hand-written 1-KiB requests to a
packed copy in one burst; the test compiles the unit exactly as build.py does and holds every default instantiation to at most 6
groups, with no destination register of a request touched before a wait covers it.  The 6 is a condition, not a measurement: the
design has 2 (x rows + bias + W_ih + 60 W_hh sets | the last 4 W_hh sets) and the 64-feature kernel's compiler-counted input rows
may add up to 3."""
import os
import subprocess

import pytest

from speech_separation_amd import build as B
from tools import asm_hazards as H
from tools import lds_wait_scan as W
from tools import prologue_scan as P

MAX_GROUPS = 6


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("prologue") / "lstm16x.s")
    cmd = [B.HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950"] + B.SOURCES["lstm16x.hip"] + \
          ["--cuda-device-only", "-S", "-w", "-o", out, os.path.join(B.CSRC, "lstm16x.hip")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(out) as f:
        return f.read()


# mangled names: lstm16x128_kernel<RELU, SCHED>, lstm16x_kernel<64, RELU>; the prologue before is *_pro0_kernel
DEFAULT = [f"lstm16x128_kernelILb{r}ELi{s}EE" for r in (0, 1) for s in (0, 1)] + [f"lstm16x_kernelILi64ELb{r}EE" for r in (0, 1)]
BEFORE = [f"lstm16x128_pro0_kernelILb{r}ELi{s}EE" for r in (0, 1) for s in (0, 1)] + [f"lstm16x_pro0_kernelILi64ELb{r}EE" for r in (0, 1)]


@pytest.mark.parametrize("kernel", DEFAULT)
def test_default_prologue_issues_its_loads_in_a_few_groups(listing, kernel):
    rows = [r for r in P.scan_text(listing) if kernel in r["kernel"]]
    assert len(rows) == 1, [r["kernel"] for r in P.scan_text(listing)]
    r = rows[0]
    print(f"{kernel}: {r['loads']} loads, {r['groups']} blocking groups {r['sizes']}")
    assert r["loads"] >= 98          # 32 / 64 W_ih sets, 64 W_hh sets, 2 bias quads; + the input rows
    assert r["groups"] <= MAX_GROUPS
    assert r["unlanded"] == []
    assert r["pending_asm"] == []


@pytest.mark.parametrize("kernel", DEFAULT)
def test_default_prologue_has_no_scratch_and_no_register_copies(listing, kernel):
    """The weights arrive where they stay: no scaling multiplies, no v_accvgpr_write, nothing spilled on the way."""
    body = W.kernel_bodies(listing)
    (name,) = [k for k in body if kernel in k]
    ins = [x.split(";")[0].strip() for x in P.prologue_of(body[name])]
    assert not [x for x in ins if x.startswith("scratch_")]
    assert not [x for x in ins if x.startswith("v_accvgpr")]
    assert len([x for x in ins if x.startswith("v_mul_f32")]) <= 8


@pytest.mark.parametrize("kernel", BEFORE)
def test_the_prologue_before_is_still_in_the_library(listing, kernel):
    rows = [r for r in P.scan_text(listing) if kernel in r["kernel"]]
    assert len(rows) == 1
    assert rows[0]["groups"] > MAX_GROUPS      # what the option's value 0 measures against


def test_scan_on_a_known_prologue():
    text = """
_Z1kv:
\tglobal_load_dwordx4 v[0:3], v9, s[0:1]
\tglobal_load_dwordx4 v[4:7], v9, s[0:1] offset:16
\ts_waitcnt vmcnt(1)
\tv_mul_f32_e32 v0, v0, v8
\tv_mul_f32_e32 v20, v5, v8
\ts_waitcnt vmcnt(0)
\ts_waitcnt vmcnt(0)
\t;;#ASMSTART
\tglobal_load_dwordx4 a[0:3], v9, s[0:1] offset:32
\t;;#ASMEND
\tglobal_load_lds_dwordx4 v9, s[0:1]
.LBB0_1:                                ; =>This Inner Loop Header: Depth=1
\tv_mfma_f32_16x16x4_f32 v[10:13], v8, a0, v[10:13]
\ts_cbranch_scc1 .LBB0_1
.Lfunc_end0:
"""
    (r,) = P.scan_text(text)
    assert r["loads"] == 4
    assert r["sizes"] == [2]                  # vmcnt(1) closes the group of two; the second and third waits cover nothing new
    assert [ins for _, ins in r["unlanded"]] == ["v_mul_f32_e32 v20, v5, v8"]
    assert r["pending_asm"] == ["global_load_dwordx4 a[0:3], v9, s[0:1] offset:32"]


def test_asm_hazards_and_lds_wait_scan_still_pass(listing, monkeypatch):
    monkeypatch.setattr(H, "FILES", ["lstm16x.hip"])
    assert H.main() == 0
    for relu in (0, 1):
        (loop,) = [r for r in W.scan_text(listing) if f"lstm16x128_kernelILb{relu}ELi1EE" in r["kernel"]]
        assert loop["mfmas"] == 512 and loop["barriers"] == 1
        assert min(w["lead"] for w in loop["waits"]) >= 4
        (name,) = [k for k in W.kernel_bodies(listing) if f"lstm16x128_kernelILb{relu}ELi1EE" in k]
        assert W.unlanded_uses(W.kernel_bodies(listing)[name]) == []
