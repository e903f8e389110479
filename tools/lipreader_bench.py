#!/usr/bin/env python3
"""Timing of the lip-reading front end (speech_separation_amd.Lipreading, include/lipfe.h) on one GPU, against stock
PyTorch-ROCm eager running the same network (the restatement tests/lipreader_ref.py on device tensors) in the same process.

For each S (streams of T x H x W frames): warm-up forwards, then `--iters` forwards back to back between two device events,
repeated `--reps` times; the median rep gives ms per call and streams/s.  The share of the FLOP bound is
S * lipfe_flops_per_stream at the fp32 MFMA peak divided by the measured time.  Then the whole profiler.py protocol of the
reference: VideoSSModel (lip reader on the two speakers' video + the audio-visual DPTN at its config sizes) at batch size 1
on 32000 samples of audio and 50 frames per speaker, one warm-up call, 10 forwards each timed from call to device synchronisation.

    python tools/lipreader_bench.py [--S 2,8,32] [--T 50] [--H 88] [--W 88] [--relu-type swish] [--iters 10] [--reps 5]
                                    [--out profiles/lipreader_bench.txt]
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
from speech_separation_amd import DPTNAVWavEncDec, Lipreading, VideoSSModel  # noqa: E402
from tests import lipreader_ref as R  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3   # MI355X: v_mfma_f32_32x32x2_f32, 256 CUs x 256 FLOP/clk x 2.4 GHz


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", default="2,8,32")
    ap.add_argument("--T", type=int, default=50)
    ap.add_argument("--H", type=int, default=88)
    ap.add_argument("--W", type=int, default=88)
    ap.add_argument("--relu-type", default="swish")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lipreader_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sd = R.synthetic_lipreader_weights("prelu" if a.relu_type == "prelu" else "swish", 0)
    lip = Lipreading(relu_type=a.relu_type, extract_feats=True)
    lip.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    lip = lip.to(dev).eval()
    dsd = {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in sd.items()}
    eng = lip._get_engine(dev)
    flops = eng.flops_per_stream(a.T, a.H, a.W)
    res = {"T": a.T, "H": a.H, "W": a.W, "relu_type": a.relu_type, "flops_per_stream": flops,
           "min_bytes_per_stream": eng.min_bytes_per_stream(a.T, a.H, a.W), "weight_pack_bytes": eng.weight_pack_bytes(),
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "legs": {}}
    say(f"# lip-reading front end, {a.relu_type}, T={a.T} {a.H}x{a.W}: {flops / 1e9:.2f} GFLOP per stream; "
        f"{res['device']}, torch {res['torch']}")
    with torch.no_grad():
        for S in [int(s) for s in a.S.split(",")]:
            x = torch.from_numpy(R.synthetic_video((S, 1, a.T, a.H, a.W), seed=S)).to(dev)
            for _ in range(a.warmup):
                got = lip(x, lengths=[a.T] * S)
                ref = R.run(dsd, x, torch.float32, relu_type=a.relu_type)
            torch.cuda.synchronize()
            agree = float(((got - ref).norm(dim=-1) / ref.norm(dim=-1)).max())
            hip = timed(lambda: lip(x, lengths=[a.T] * S), a.iters, a.reps)
            eager = timed(lambda: R.run(dsd, x, torch.float32, relu_type=a.relu_type), a.iters, a.reps)
            t_flop = S * flops / (PEAK_F32_MFMA_TFLOPS * 1e12) * 1e3
            leg = {"hip_ms": round(hip[0], 4), "hip_ms_spread": [round(hip[1], 4), round(hip[2], 4)],
                   "eager_ms": round(eager[0], 4), "eager_ms_spread": [round(eager[1], 4), round(eager[2], 4)],
                   "streams_per_s": round(S / hip[0] * 1e3, 1), "eager_streams_per_s": round(S / eager[0] * 1e3, 1),
                   "hip_over_eager_time": round(hip[0] / eager[0], 3), "tflops": round(S * flops / hip[0] / 1e9, 2),
                   "share_of_flop_bound": round(t_flop / hip[0], 4), "worst_row_vs_eager": agree}
            res["legs"][S] = leg
            say(f"S={S:3d}: HIP {hip[0]:8.3f} ms/call ({leg['streams_per_s']:8.1f} streams/s, {leg['tflops']:6.2f} TFLOP/s, "
                f"{100 * leg['share_of_flop_bound']:.1f} % of the fp32-MFMA bound {t_flop:.3f} ms)   stock eager {eager[0]:8.3f} "
                f"ms/call ({leg['eager_streams_per_s']:8.1f} streams/s)   HIP/eager time {leg['hip_over_eager_time']:.2f}   "
                f"worst row HIP vs eager {agree:.1e}")

        # profiler.py: VideoSSModel at bs = 1 (32000 samples of audio, 50 frames of 88 x 88 per speaker), 10 forwards
        torch.manual_seed(0)
        ss = DPTNAVWavEncDec(num_features=128, video_emb_size=512, hidden_video=128, kernel_size_enc=7, hidden_dim=128,
                             num_blocks=6, chunk_size=150, step_size=75).to(dev).eval()
        model = VideoSSModel(ss, lip)
        rng = np.random.Generator(np.random.PCG64(1))
        batch = {"mix": torch.from_numpy(rng.standard_normal((1, 32000)).astype(np.float32) * 0.1).to(dev),
                 "video": torch.from_numpy(R.synthetic_video((2, 1, 50, 88, 88), seed=2)).to(dev)}
        first = model(**batch)
        emb = {"mix": batch["mix"], "s1_embedding": first["s1_embedding"], "s2_embedding": first["s2_embedding"]}
        for name, fn in (("VideoSSModel (lip reader + separator)", lambda: model(**batch)),
                         ("separator alone on precomputed embeddings", lambda: ss(**emb))):
            fn()
            torch.cuda.synchronize()
            t = []
            for _ in range(10):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                t.append((time.perf_counter() - t0) * 1e3)
            res[name] = {"mean_ms": round(float(np.mean(t)), 4), "median_ms": round(float(np.median(t)), 4),
                         "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}
            say(f"profiler.py protocol, bs=1, 10 forwards, {name}: mean {np.mean(t):.3f} ms, median {np.median(t):.3f} ms, "
                f"min {min(t):.3f} ms, max {max(t):.3f} ms")
    say(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
