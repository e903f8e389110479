#!/usr/bin/env python3
"""Timing of the VoiceFilter training step (speech_separation_amd.TrainableVoiceFilter, include/vfilt_train.h) on one GPU,
against stock PyTorch-ROCm eager training of the same network (the restatement tests/voicefilter_train_ref.py on device
tensors, with nn.GRU / nn.LSTM) in the same process.

A step is forward, MSESpecLoss, backward, clip at 2 and Adam at 3e-4 (vf_mse.yaml): train.train_step with FusedAdamW
(weight_decay 0) here; autograd, torch.nn.utils.clip_grad_norm_ and torch.optim.Adam there.  For each B: warm-up steps, then
`--iters` steps back to back between two device events, repeated `--reps` times (windows); the median window gives ms per
step, min .. max are printed next to it.  The device time of the parts of one step is the sum of its kernels' durations as
torch.profiler records them; for the weight-gradient kernel of layers 2..7 it is printed as TFLOP/s next to the rate of the
forward's six 64 -> 64 convolutions of the SAME step (the first six lipfe_conv_kernel launches; the next six are the data
gradient).

    python tools/voicefilter_train_bench.py [--B 1,4,16] [--F 201] [--W 321] [--Tv 50] [--E 1024] [--iters 3] [--reps 5]
                                            [--out profiles/voicefilter_train_bench.txt]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speech_separation_amd import FusedAdamW, MSESpecLoss, TrainableVoiceFilter  # noqa: E402
from speech_separation_amd.train import train_step  # noqa: E402
from tests import voicefilter_ref as R  # noqa: E402
from tests import voicefilter_train_ref as T  # noqa: E402
from tools.voicefilter_bench import timed  # noqa: E402

PARTS = ("conv forward", "conv dgrad", "conv wgrad", "batchnorm", "thin conv ends", "lstm", "gru", "gemm", "other")


def device_time_by_part(fn):
    """{part: ms} of one call, or a string saying why it could not be taken."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        ev.sort(key=lambda e: e.time_range.start)
        parts = {k: 0.0 for k in PARTS}
        convs = 0
        for e in ev:
            us = float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0) or e.time_range.elapsed_us())
            n = e.name
            if "lipfe_conv_kernel" in n:
                part = "conv forward" if convs < 6 else "conv dgrad"
                convs += 1
            elif "vftrain_wgrad" in n:
                part = "conv wgrad"
            elif "vftrain_stat" in n or "vftrain_norm" in n or "vftrain_bn_bwd" in n:
                part = "batchnorm"
            elif "conv1" in n or "conv8" in n or "vftrain_parts_sum" in n or "pack" in n or "fold" in n:
                part = "thin conv ends"
            elif "lstm" in n:
                part = "lstm"
            elif "gru" in n:
                part = "gru"
            elif "vfilt_gemm_kernel" in n:
                part = "gemm"
            else:
                part = "other"
            parts[part] += us / 1e3
        if convs != 12:
            return f"not split ({convs} lipfe_conv_kernel launches seen, 12 expected)"
        parts["kernels"] = len(ev)
        return parts
    except Exception as e:      # noqa: BLE001
        return f"not taken ({type(e).__name__}: {e})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", default="1,4,16")
    ap.add_argument("--F", type=int, default=201)
    ap.add_argument("--W", type=int, default=321)
    ap.add_argument("--Tv", type=int, default=50)
    ap.add_argument("--E", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voicefilter_train_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sd = R.synthetic_voicefilter_weights(a.F, a.E, 0)
    conv64 = 2.0 * a.F * a.W * (64 * 64 * 7 + 5 * 64 * 64 * 25)      # the six 64 -> 64 convolutions of one item, one pass
    res = {"F": a.F, "W": a.W, "Tv": a.Tv, "E": a.E, "conv64_flops_per_item_per_pass": conv64,
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "legs": {}}
    crit = MSESpecLoss()
    for B in [int(s) for s in a.B.split(",")]:
        model = TrainableVoiceFilter(a.F, embed_size=a.E)
        model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        model = model.to(dev).train()
        opt = FusedAdamW(model.parameters(), lr=3e-4, weight_decay=0)
        mix, e1, e2 = (torch.from_numpy(v).to(dev) for v in R.synthetic_inputs(a.F, a.W, a.Tv, B, a.E, seed=B))
        t1, t2 = (torch.from_numpy(v).to(dev) for v in T.targets(a.F, a.W, B))
        batch = {"mix_magnitude": mix, "s1_embedding": e1, "s2_embedding": e2, "s1_spec_true": t1, "s2_spec_true": t2}
        hip_fn = lambda: train_step(model, dict(batch), crit, opt, max_grad_norm=2.0)      # noqa: E731
        flops = B * model._get_engine(dev).flops_per_item(a.W, a.Tv)
        if B == int(a.B.split(",")[0]):
            say(f"# VoiceFilter training step, F={a.F} W={a.W} Tv={a.Tv} E={a.E}: {flops / B / 1e9:.2f} GFLOP per item and step "
                f"({3 * conv64 / 1e9:.2f} in the 64 -> 64 convolutions' three passes); {res['device']}, torch {res['torch']}")
        # stock eager: the restatement's leaves, autograd, torch's clip and Adam
        ref = {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in sd.items() if not k.endswith("num_batches_tracked")}
        leaves = [k for k in ref if not k.endswith(("running_mean", "running_var"))]
        for k in leaves:
            ref[k].requires_grad_(True)
        ropt = torch.optim.Adam([ref[k] for k in leaves], lr=3e-4)
        keep = (torch.rand(2 * B, a.W, device=dev) >= T.P_DROP).float()

        mods = {}       # the restatement's nn.GRU / nn.LSTM, built once per leg as a training script builds its model once

        def eager_fn():
            ropt.zero_grad()
            run = T.forward(ref, mix, e1, e2, torch.float32, keep, leaves=True, stock_lstm=True, modules=mods)
            T.mse_pit_loss(run.out1, run.out2, t1, t2).backward()
            torch.nn.utils.clip_grad_norm_([ref[k] for k in leaves], 2.0)
            ropt.step()

        for _ in range(a.warmup):
            hip_fn()
            eager_fn()
        torch.cuda.synchronize()
        hip = timed(hip_fn, a.iters, a.reps)
        eager = timed(eager_fn, a.iters, a.reps)
        parts = device_time_by_part(hip_fn)
        leg = {"hip_ms": round(hip[0], 4), "hip_ms_spread": [round(hip[1], 4), round(hip[2], 4)], "eager_ms": round(eager[0], 4),
               "eager_ms_spread": [round(eager[1], 4), round(eager[2], 4)], "hip_over_eager_time": round(hip[0] / eager[0], 3),
               "items_per_s": round(B / hip[0] * 1e3, 2), "tflops": round(flops / hip[0] / 1e9, 2), "device_ms_by_part": parts,
               "workspace_bytes": model._engine.workspace_bytes(B, a.W, a.Tv)}
        say(f"B={B:3d}: HIP {hip[0]:9.3f} ms/step ({hip[1]:.3f} .. {hip[2]:.3f} over {a.reps} windows of {a.iters}; "
            f"{leg['items_per_s']:8.2f} items/s, {leg['tflops']:6.2f} TFLOP/s)   stock eager {eager[0]:9.3f} ms/step "
            f"({eager[1]:.3f} .. {eager[2]:.3f})   HIP/eager time {leg['hip_over_eager_time']:.2f}   workspace "
            f"{leg['workspace_bytes'] / 2**30:.2f} GiB")
        if isinstance(parts, dict):
            fw, wg, dg = (B * conv64 / parts[k] / 1e9 for k in ("conv forward", "conv wgrad", "conv dgrad"))
            leg["conv_forward_tflops"], leg["conv_wgrad_tflops"], leg["conv_dgrad_tflops"] = round(fw, 2), round(wg, 2), round(dg, 2)
            say("       device ms of one step: " + ", ".join(f"{k} {parts[k]:.3f}" for k in PARTS) + f"; {parts['kernels']} kernels")
            say(f"       64 -> 64 convolutions, same step: forward {fw:.2f} TFLOP/s, weight gradient {wg:.2f} TFLOP/s "
                f"({wg / fw:.2f} x the forward's rate), data gradient {dg:.2f} TFLOP/s")
        else:
            say(f"       device time by part: {parts}")
        res["legs"][B] = leg
        del model, opt, ref, ropt, mods
        torch.cuda.empty_cache()
    say(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
