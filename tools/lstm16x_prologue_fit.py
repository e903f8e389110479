#!/usr/bin/env python3
"""Diagnostic (GPU box): a fused-recurrence launch's FIXED cost against its per-step cost, by a fit over the recurrence length.

One inter-chunk path of DPTN-AV is run in isolation (stage_path: one stream, nothing beside it) for B mixtures and several chunk
counts S.  Its lstm16x128_kernel launch has 150 B sequences whatever S is -- the same grid, 2 ceil(150 B / 16) workgroups -- and a
recurrence of S steps, so the launch time (the engine's own event pair around the launch, mean of `reps`) is a + b S:
b = one step, a = everything else (launch, prologue, the last h rows).  The intra-chunk path (150 steps, B S sequences) is
printed beside it as a check of the fit at a length it did not see.

usage: lstm16x_prologue_fit.py [--prologue 0|1] [--sched 0|1] [--B 5] [--S 10,38,75,141] [--reps 20] [--ghz 2.45]
       AB_LIB=<other libdptnav.so> for another build (a build without the option: leave --prologue out).
--ghz converts to cycles (2.45: the ratio of profiles/lstm16x_lds_sched_ab.txt (d) active cycles to (a) time per launch)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if os.environ.get("AB_LIB"):
    import speech_separation_amd._lib as _L
    _L.LIB_PATH = os.path.abspath(os.environ["AB_LIB"])
from speech_separation_amd.engine import DptnEngine, params_to_device  # noqa: E402
from speech_separation_amd.spec import DPTN_AV, synthetic_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--prologue", type=int, default=None)
ap.add_argument("--sched", type=int, default=1)
ap.add_argument("--B", type=int, default=5)
ap.add_argument("--S", default="10,38,75,141")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--ghz", type=float, default=2.45)
args = ap.parse_args()

dev = torch.device("cuda:0")
cfg = DPTN_AV
eng = DptnEngine(cfg, dev)
eng.bind(params_to_device(synthetic_state_dict(cfg, 0), dev))
eng.set_option("lstm4", 0)
eng.set_option("fuse_pre128", 2)
eng.set_option("lstm_sched", args.sched)
if args.prologue is not None:
    eng.set_option("lstm_prologue", args.prologue)


def launch_us(path, S):
    x = torch.randn(args.B, S, cfg.chunk_size, cfg.num_features, device=dev)
    for _ in range(3):
        eng.stage_path(0, path, x)
    torch.cuda.synchronize()
    eng.profile(True)
    eng.profile_reset()
    for _ in range(args.reps):
        eng.stage_path(0, path, x)
    ms, n = eng.profile_read()["lstm_recurrence"]
    eng.profile(False)
    assert n == args.reps, (n, args.reps)
    return 1e3 * ms / n


Ss = [int(s) for s in args.S.split(",")]
t = np.array([launch_us(1, S) for S in Ss])
b, a = np.polyfit(np.array(Ss, dtype=np.float64), t, 1)
res = t - (a + b * np.array(Ss))
k = args.ghz * 1e3      # cycles per microsecond
print(f"lib {os.environ.get('AB_LIB', 'in-tree')}  lstm_prologue {args.prologue}  lstm_sched {args.sched}  B {args.B}: "
      f"{2 * ((150 * args.B + 15) // 16)} workgroups")
for S, us, r in zip(Ss, t, res):
    print(f"  inter path, {S:4d} steps: {us:9.2f} us per launch   (fit residual {r:+6.2f} us)")
print(f"  fit: fixed {a:8.2f} us = {a * k / 1e3:7.1f} k cycles per launch;  step {b:7.4f} us = {b * k / 1e3:6.2f} k cycles")
S_chk = Ss[-1]
us = launch_us(0, S_chk)
print(f"  intra path, 150 steps, {2 * ((args.B * S_chk + 15) // 16)} workgroups: {us:9.2f} us per launch   (fit at 150 steps: {a + 150 * b:9.2f} us)")
