#!/usr/bin/env python3
"""Timing of VoiceFilter (speech_separation_amd.VoiceFilter.forward_embeddings, include/vfilt.h) on one GPU, against stock
PyTorch-ROCm eager running the same network (the restatement tests/voicefilter_ref.py on device tensors) in the same process.

For each B (items of F x W with Tv video frames per speaker): warm-up forwards, then `--iters` forwards back to back between
two device events, repeated `--reps` times; the median rep gives ms per call and items/s.  The share of the FLOP bound is
B * vfilt_flops_per_item at the fp32 MFMA peak divided by the measured time.  The device time of the parts of one forward
(conv stack, projection GEMM, LSTM recurrence, GRU with the d-vector, FC tail) is the sum of its kernels' durations as
torch.profiler records them, the GEMM launches told apart by their fixed place in the forward's launch order.

    python tools/voicefilter_bench.py [--B 1,4,16] [--F 201] [--W 321] [--Tv 50] [--E 1024] [--iters 5] [--reps 5]
                                      [--out profiles/voicefilter_bench.txt]
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
from speech_separation_amd import VoiceFilter  # noqa: E402
from tests import voicefilter_ref as R  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3   # MI355X: v_mfma_f32_32x32x2_f32, 256 CUs x 256 FLOP/clk x 2.4 GHz
# the vfilt_gemm_kernel launches of one forward, in order: 4 GRU layer-1 inputs, layer-2 input, its reverse step's input,
# fc_dvector | the d-vector's part of the LSTM input, the projection | Linear(400, 600), Linear(600, F) per speaker
GEMM_PARTS = ["gru"] * 7 + ["projection"] * 2 + ["fc"] * 3


def timed(fn, iters, reps):
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / iters)
    return float(np.median(times)), float(min(times)), float(max(times))


def device_time_by_part(fn):
    """{part: ms} of one call, or a string saying why it could not be taken."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        ev.sort(key=lambda e: e.time_range.start)
        parts = {"conv": 0.0, "projection": 0.0, "lstm": 0.0, "gru": 0.0, "fc": 0.0, "other": 0.0}
        gemm = 0
        for e in ev:
            us = float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0) or e.time_range.elapsed_us())
            n = e.name
            if "vfilt_gemm_kernel" in n:
                part = GEMM_PARTS[gemm] if gemm < len(GEMM_PARTS) else "other"
                gemm += 1
            elif "lipfe_conv_kernel" in n or "vfilt_conv" in n or "vfilt_fold" in n or "lipfe_pack" in n:
                part = "conv"
            elif "vfilt_lstm_step" in n:
                part = "lstm"
            elif "vfilt_gru" in n or "vfilt_transpose" in n:
                part = "gru"
            else:
                part = "other"
            parts[part] += us / 1e3
        if gemm != len(GEMM_PARTS):
            return f"not split ({gemm} GEMM launches seen, {len(GEMM_PARTS)} expected)"
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
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voicefilter_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sd = R.synthetic_voicefilter_weights(a.F, a.E, 0)
    model = VoiceFilter(a.F, embed_size=a.E)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    model = model.to(dev).eval()
    dsd = {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in sd.items()}
    eng = model._get_engine(dev)
    flops = eng.flops_per_item(a.W, a.Tv)
    conv_flops = 2.0 * a.F * a.W * (64 * 7 + 64 * 64 * 7 + 5 * 64 * 64 * 25 + 64 * 8)
    res = {"F": a.F, "W": a.W, "Tv": a.Tv, "E": a.E, "flops_per_item": flops, "conv_flops_per_item": conv_flops,
           "min_bytes_per_item": eng.min_bytes_per_item(a.W, a.Tv), "device": torch.cuda.get_device_name(0),
           "torch": torch.__version__, "legs": {}}
    say(f"# VoiceFilter, F={a.F} W={a.W} Tv={a.Tv} E={a.E}: {flops / 1e9:.2f} GFLOP per item ({conv_flops / 1e9:.2f} in the "
        f"convolutions); {res['device']}, torch {res['torch']}")
    mods = {}       # the restatement's nn.GRU / nn.LSTM, built once
    with torch.no_grad():
        for B in [int(s) for s in a.B.split(",")]:
            x = tuple(torch.from_numpy(v).to(dev) for v in R.synthetic_inputs(a.F, a.W, a.Tv, B, a.E, seed=B))
            hip_fn = lambda: model.forward_embeddings(*x)                       # noqa: E731
            eager_fn = lambda: R.run(dsd, *x, torch.float32, modules=mods)      # noqa: E731
            for _ in range(a.warmup):
                got = hip_fn()
                ref = eager_fn()
            torch.cuda.synchronize()
            agree = max(float(((got[k] - r).norm(dim=1) / r.norm(dim=1)).max()) for k, r in zip(("s1_spec_pred", "s2_spec_pred"), ref))
            hip = timed(hip_fn, a.iters, a.reps)
            eager = timed(eager_fn, a.iters, a.reps)
            parts = device_time_by_part(hip_fn)
            # stock nn.LSTM (MIOpen) on the concatenated input of the 2B sequences: its input projection and recurrence
            lstm = torch.nn.LSTM(9 * a.F, R.HIDDEN, batch_first=True).to(dev)
            xin = torch.randn(2 * B, a.W, 9 * a.F, device=dev)
            lstm(xin)
            stock_lstm = timed(lambda: lstm(xin), a.iters, a.reps)
            t_flop = B * flops / (PEAK_F32_MFMA_TFLOPS * 1e12) * 1e3
            leg = {"hip_ms": round(hip[0], 4), "hip_ms_spread": [round(hip[1], 4), round(hip[2], 4)],
                   "eager_ms": round(eager[0], 4), "eager_ms_spread": [round(eager[1], 4), round(eager[2], 4)],
                   "items_per_s": round(B / hip[0] * 1e3, 2), "eager_items_per_s": round(B / eager[0] * 1e3, 2),
                   "hip_over_eager_time": round(hip[0] / eager[0], 3), "tflops": round(B * flops / hip[0] / 1e9, 2),
                   "share_of_flop_bound": round(t_flop / hip[0], 4), "worst_column_vs_eager": agree, "device_ms_by_part": parts,
                   "stock_lstm_ms": round(stock_lstm[0], 4)}
            res["legs"][B] = leg
            say(f"B={B:3d}: HIP {hip[0]:9.3f} ms/call ({leg['items_per_s']:8.2f} items/s, {leg['tflops']:6.2f} TFLOP/s, "
                f"{100 * leg['share_of_flop_bound']:.1f} % of the fp32-MFMA bound {t_flop:.3f} ms)   stock eager {eager[0]:9.3f} "
                f"ms/call ({leg['eager_items_per_s']:8.2f} items/s)   HIP/eager time {leg['hip_over_eager_time']:.2f}   "
                f"worst column HIP vs eager {agree:.1e}")
            if isinstance(parts, dict):
                say(f"       device ms of one forward: conv stack {parts['conv']:.3f} ({B * conv_flops / parts['conv'] / 1e9:.2f} "
                    f"TFLOP/s), projection GEMM {parts['projection']:.3f}, LSTM recurrence {parts['lstm']:.3f} ({a.W} launches), "
                    f"GRU + d-vector {parts['gru']:.3f}, FC tail {parts['fc']:.3f}, other {parts['other']:.3f}; "
                    f"{parts['kernels']} kernels")
                say(f"       stock nn.LSTM(9F, 400) on the 2B concatenated sequences (projection + recurrence): {stock_lstm[0]:.3f} "
                    f"ms/call; here projection + recurrence: {parts['projection'] + parts['lstm']:.3f} ms of device time")
            else:
                say(f"       device time by part: {parts}")
    say(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
