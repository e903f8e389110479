#!/usr/bin/env python3
"""Time the waveform criteria on the GPU: the six (kind, level) pairs of MAEWavLoss / MSEWavLoss / SiSNRWavLoss (batch or
utterance PIT), forward plus backward of the loss alone, at B = 1, 4, 16 x 32000 samples, against the stock-PyTorch eager
composition of the same loss on the same GPU in the same process.  The eager composition is the vectorised, synchronisation
free one (per-item terms, torch.where for the permutation): a stronger baseline than the reference's classes, whose
`if loss_perm_2 < loss_perm_1` also waits for the device every call.

Protocol: every shape is warmed up; STEPS calls between two synchronisations, the two implementations alternating window
by window, median and spread of REPS windows; the first call of every pair is checked against the eager value.  The number
of device kernels of one call comes from torch.profiler.  No time is a pass criterion.

Usage:  python tools/wavloss_bench.py [--batches 1,4,16] [--steps 1000] [--reps 7] [--json out.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speech_separation_amd import MAEWavLoss, MSEWavLoss, SiSNRWavLoss  # noqa: E402
from tests.wavloss_ref import make_case  # noqa: E402

T = 32000
CLASSES = {"mae": MAEWavLoss, "mse": MSEWavLoss, "sisnr": SiSNRWavLoss}


def item_terms(kind, p, s):
    """l_i(p, s) [B] of the element loss (ss_losses.py:65-93, :100-114), stock operators."""
    if kind == "mae":
        return (p - s).abs().mean(-1)
    if kind == "mse":
        return ((p - s) ** 2).mean(-1)
    p = p - p.mean(-1, keepdim=True)
    s = s - s.mean(-1, keepdim=True)
    scaled = (s * p).sum(-1, keepdim=True) / (torch.linalg.norm(s, ord=2, dim=-1, keepdim=True) ** 2) * s
    sig = torch.linalg.norm(scaled, ord=2, dim=-1) ** 2
    nz = torch.linalg.norm(p - scaled, ord=2, dim=-1) ** 2
    return -20 * torch.log10(sig / nz)


def eager_loss(kind, level, p1, p2, s1, s2):
    i0 = (item_terms(kind, p1, s1) + item_terms(kind, p2, s2)) / 2
    i1 = (item_terms(kind, p1, s2) + item_terms(kind, p2, s1)) / 2
    if level == "utterance":
        return torch.where(i1 < i0, i1, i0).mean()
    l0, l1 = i0.mean(), i1.mean()
    return torch.where(l1 < l0, l1, l0)


def kernels_per_call(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as e:      # noqa: BLE001
        return f"not counted ({type(e).__name__})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,4,16")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sync = lambda: torch.cuda.synchronize(dev)
    print(f"{torch.cuda.get_device_name(dev)}; T = {T}; {a.steps} calls per window, median (min .. max) of {a.reps} windows; "
          f"forward + backward of the loss alone", flush=True)
    rows = []
    for B in (int(b) for b in a.batches.split(",")):
        t = [torch.from_numpy(x).to(dev) for x in make_case(B, T, seed=B, swapped=tuple(range(1, B, 2)))]
        t[0].requires_grad_(True)
        t[1].requires_grad_(True)
        for kind, cls in CLASSES.items():
            for level in ("batch", "utterance"):
                crit = cls(pit=level)

                def hip():
                    t[0].grad = t[1].grad = None
                    crit(*t)["loss"].backward()

                def eager():
                    t[0].grad = t[1].grad = None
                    eager_loss(kind, level, *t).backward()

                want, got = float(eager_loss(kind, level, *t)), float(crit(*t)["loss"].detach())
                assert abs(got - want) <= 1e-4 * max(1.0, abs(want)), (kind, level, B, got, want)
                for fn in (hip, eager):
                    for _ in range(20):
                        fn()
                sync()
                times = {"hip": [], "eager": []}
                for _ in range(a.reps):
                    for name, fn in (("hip", hip), ("eager", eager)):
                        t0 = time.perf_counter()
                        for _ in range(a.steps):
                            fn()
                        sync()
                        times[name].append((time.perf_counter() - t0) / a.steps * 1e6)
                row = {"B": B, "kind": kind, "level": level, "kernels_hip": kernels_per_call(hip), "kernels_eager": kernels_per_call(eager)}
                for name, v in times.items():
                    row[name + "_us"], row[name + "_min_us"], row[name + "_max_us"] = statistics.median(v), min(v), max(v)
                rows.append(row)
                print(f"B={B:2d} {kind:5s} {level:9s}: HIP {row['hip_us']:7.1f} us ({row['hip_min_us']:.1f} .. {row['hip_max_us']:.1f}), "
                      f"{row['kernels_hip']} kernels/call | eager {row['eager_us']:7.1f} us ({row['eager_min_us']:.1f} .. "
                      f"{row['eager_max_us']:.1f}), {row['kernels_eager']} kernels/call | x{row['eager_us'] / row['hip_us']:.2f}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
