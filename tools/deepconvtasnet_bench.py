#!/usr/bin/env python3
"""Timing of the deep Conv-TasNet inference forwards (speech_separation_amd.DeepConvTasNet, DeepAVConvTasNet) on one GPU,
against the stock-PyTorch CPU restatement (tests/deepconvtasnet_ref.py) in the same run.

For each B: warm-up forwards, then `--iters` forwards back to back between two synchronisations (device events), repeated
`--reps` times; the median rep gives ms per forward and mixtures/s.  The whole-path share of peak is the larger of the two
bounds of the library's cost model (dctasnet_flops_per_mixture at the fp32 MFMA peak; dctasnet_min_bytes_per_mixture plus
the per-forward weight repack, dctasnet_weight_pack_bytes, at the HBM bandwidth) divided by the measured time.  Prints one
line per leg and one JSON line at the end.

    python tools/deepconvtasnet_bench.py [--models deep,deepav] [--B 1,4,16] [--T 32000] [--Tv 50] [--iters 20] [--reps 5]
                                         [--cpu-threads 16]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speech_separation_amd import DeepAVConvTasNet, DeepConvTasNet  # noqa: E402
from speech_separation_amd.spec import DPTN_AV, synthetic_inputs  # noqa: E402
from tests import deepconvtasnet_ref as DR  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3   # MI355X: v_mfma_f32_32x32x2_f32, 256 CUs x 256 FLOP/clk x 2.4 GHz
PEAK_HBM_TBS = 6.3             # MI355X_MICROARCH.md: sustained HBM3E copy bandwidth


def inputs(av, B, T, Tv, dev=None):
    inp = synthetic_inputs(DPTN_AV, B=B, T=T, Tv=Tv, seed=B)
    keys = ("mix", "s1_embedding", "s2_embedding") if av else ("mix",)
    return {k: torch.from_numpy(inp[k]) if dev is None else torch.from_numpy(inp[k]).to(dev) for k in keys}


def bench_model(name, av, a, dev):
    sd = DR.synthetic_deepconvtasnet_weights(av, seed=0)
    model = (DeepAVConvTasNet if av else DeepConvTasNet)()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model = model.to(dev).eval()
    T = a.T
    res = {"T": T, "Tv": a.Tv, "gpu": {}}
    with torch.no_grad():
        eng = model._get_engine(dev)
        flops, nbytes, pack = eng.flops_per_mixture(T), eng.min_bytes_per_mixture(T), eng.weight_pack_bytes()
        res["flops_per_mixture"], res["min_bytes_per_mixture"], res["weight_pack_bytes"] = flops, nbytes, pack
        for B in [int(b) for b in a.B.split(",")]:
            batch = inputs(av, B, T, a.Tv, dev)
            for _ in range(a.warmup):
                model(**batch)
            torch.cuda.synchronize()
            times = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    out = model(**batch)
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1) / a.iters)
            ms = float(np.median(times))
            t_flop = B * flops / (PEAK_F32_MFMA_TFLOPS * 1e12) * 1e3
            t_byte = (B * nbytes + pack) / (PEAK_HBM_TBS * 1e12) * 1e3
            bound = "flop" if t_flop >= t_byte else "byte"
            leg = {"ms_per_forward": round(ms, 4), "mixtures_per_s": round(B / ms * 1e3, 2),
                   "ms_spread": [round(min(times), 4), round(max(times), 4)],
                   "flop_bound_ms": round(t_flop, 4), "byte_bound_ms": round(t_byte, 4), "binding_bound": bound,
                   "share_of_bound": round(max(t_flop, t_byte) / ms, 4),
                   "tflops": round(B * flops / ms / 1e9, 2), "outputs_finite": bool(torch.isfinite(out["s1_pred"]).all())}
            res["gpu"][B] = leg
            print(f"{name} GPU B={B:3d} T={T}: {ms:8.3f} ms/forward  {leg['mixtures_per_s']:9.1f} mixtures/s  "
                  f"{leg['tflops']:6.1f} TFLOP/s  bounds: flop {t_flop:.3f} ms, byte {t_byte:.3f} ms -> "
                  f"{100 * leg['share_of_bound']:.1f} % of the {bound} bound", flush=True)
    # the stock CPU restatement, same process
    torch.set_num_threads(a.cpu_threads)
    csd = {k: torch.from_numpy(v) for k, v in sd.items()}
    cb = inputs(av, a.cpu_B, T, a.Tv)
    cargs = (cb["mix"], cb.get("s1_embedding"), cb.get("s2_embedding"))
    DR.forward(csd, *cargs)
    ct = []
    for _ in range(a.cpu_reps):
        t0 = time.perf_counter()
        DR.forward(csd, *cargs)
        ct.append(time.perf_counter() - t0)
    cpu_rate = a.cpu_B / float(np.median(ct))
    res["cpu"] = {"B": a.cpu_B, "threads": a.cpu_threads, "ms_per_forward": round(float(np.median(ct)) * 1e3, 2),
                  "mixtures_per_s": round(cpu_rate, 2)}
    print(f"{name} CPU stock restatement B={a.cpu_B} on {a.cpu_threads} threads: {res['cpu']['ms_per_forward']:.1f} ms/forward  "
          f"{cpu_rate:.2f} mixtures/s", flush=True)
    for B, leg in res["gpu"].items():
        leg["speedup_vs_cpu"] = round(leg["mixtures_per_s"] / cpu_rate, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="deep,deepav")
    ap.add_argument("--B", default="1,4,16")
    ap.add_argument("--T", type=int, default=32000)
    ap.add_argument("--Tv", type=int, default=50)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--cpu-B", type=int, default=4)
    ap.add_argument("--cpu-reps", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"iters": a.iters, "reps": a.reps}
    for name in a.models.split(","):
        res[name] = bench_model(name, {"deep": False, "deepav": True}[name], a, dev)
    print(json.dumps(res))

if __name__ == "__main__":
    main()
