"""The LDS schedule of lstm16x128_kernel's step loop, judged in the GENERATED code (no GPU needed: hipcc cross-compiles).

The loop's LDS reads are issued by hand a k-chunk (32 MFMAs) or a pair of W_ih sets (8 MFMAs) ahead of the MFMAs that use them
(csrc/lstm16x.hip, the issue-order table above the loop; engine option lstm_sched = 1).  Scheduling fences have undone such an
arrangement before, and written as plain loads the compiler sank 18 of 29 reads to within two MFMAs of their wait, so the test
compiles the unit exactly as build.py does and holds the loop to: no `s_waitcnt lgkmcnt` covers a request fewer than 4 MFMAs
old.  The 4 is a condition, not a measurement: half the shortest lead the design intends (8), so that a compiler update cannot
silently put the loop back to 0-2."""
import os
import subprocess

import pytest

from speech_separation_amd import build as B
from tools import lds_wait_scan as W

MIN_LEAD = 4


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lds_wait") / "lstm16x.s")
    cmd = [B.HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950"] + B.SOURCES["lstm16x.hip"] + \
          ["--cuda-device-only", "-S", "-w", "-o", out, os.path.join(B.CSRC, "lstm16x.hip")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(out) as f:
        return f.read()


def _kernel(relu):
    return f"lstm16x128_kernelILb{int(relu)}ELi1EE"          # lstm16x128_kernel<RELU, SCHED = 1>


@pytest.mark.parametrize("relu", [True, False])
def test_step_loop_keeps_its_leads(listing, relu):
    loops = [r for r in W.scan_text(listing) if _kernel(relu) in r["kernel"]]
    assert len(loops) == 1, [(r["loop"], r["mfmas"]) for r in loops]      # everything inside a step is unrolled
    loop = loops[0]
    leads = [w["lead"] for w in loop["waits"]]
    print(f"relu={relu}: {loop['mfmas']} MFMAs, {loop['barriers']} s_barrier, {loop['ds']} ds, leads {leads}")
    assert loop["mfmas"] == 512
    assert loop["barriers"] == 1
    # 8 h fragments, 6 x fragments and 31 W_ih sets are read inside the loop: the hand-written waits are there to be judged
    assert len(leads) >= 20
    short = [(w["at"], w["n"], w["lead"], w["request"]) for w in loop["waits"] if w["lead"] < MIN_LEAD]
    assert not short, short


@pytest.mark.parametrize("relu", [True, False])
def test_step_loop_has_no_scratch_and_no_register_shuffling(listing, relu):
    """256 + 256 registers and nothing of them in scratch inside the loop: with the last step's branch inside the loop the same
    source gave W_hh fragments in scratch and 87 v_accvgpr_read per step."""
    body = W.kernel_bodies(listing)
    name = [k for k in body if _kernel(relu) in k]
    assert len(name) == 1
    lines = body[name[0]]
    (label, lo, hi), = [l for l in W._loops(lines) if any(x.strip().startswith("v_mfma") for x in lines[l[1]:l[2] + 1])]
    ins = [x.strip() for x in lines[lo:hi + 1]]
    assert not [x for x in ins if x.startswith("scratch_") or x.startswith("buffer_") and "offen" in x]
    assert not [x for x in ins if x.startswith("v_accvgpr")]


@pytest.mark.parametrize("relu", [True, False])
def test_no_read_is_used_before_it_has_landed(listing, relu):
    """The compiler takes an asm read's destination for written where the statement stands: nothing may touch it before a wait
    covers it (whole kernel: prologue, loop, the last step behind the loop)."""
    body = W.kernel_bodies(listing)
    name = [k for k in body if _kernel(relu) in k]
    assert len(name) == 1
    assert W.unlanded_uses(body[name[0]]) == []


def test_scan_on_a_known_loop():
    text = """
_Z1kv:
.LBB0_1:                                ; =>This Inner Loop Header: Depth=1
\tds_read_b128 v[0:3], v9
\tds_read_b128 v[4:7], v9 offset:64
\tv_mfma_f32_16x16x4_f32 v[10:13], v8, v8, v[10:13]
\ts_waitcnt lgkmcnt(1)
\tv_mfma_f32_16x16x4_f32 v[10:13], v0, v8, v[10:13]
\tv_mfma_f32_16x16x4_f32 v[10:13], v1, v8, v[10:13]
\tv_mov_b32_e32 v20, v5
\ts_waitcnt lgkmcnt(0)
\ts_waitcnt lgkmcnt(0)
\ts_barrier
\ts_cbranch_scc1 .LBB0_1
.Lfunc_end0:
"""
    (r,) = W.scan_text(text)
    assert (r["mfmas"], r["barriers"], r["ds"]) == (3, 1, 2)
    assert [(w["at"], w["n"], w["lead"]) for w in r["waits"]] == [(1, 1, 1), (3, 0, 3)]      # the third wait covers nothing
    bad = W.unlanded_uses(W.kernel_bodies(text)["_Z1kv"])
    assert [ins for _, ins in bad] == ["v_mov_b32_e32 v20, v5"]
