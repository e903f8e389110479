#!/usr/bin/env python3
"""Timing of the ShuffleNet-v2 lip reader (speech_separation_amd.ShuffleNetLipreading, include/lipsn.h) on one GPU against
two yardsticks in the same process: stock PyTorch-ROCm eager running the same network (the restatement
tests/shufflenet_ref.py on device tensors), and this package's ResNet-18 lip reader (include/lipfe.h) on the same video.

For each S (streams of T x H x W frames): warm-up forwards, then `--iters` forwards back to back between two device events,
repeated `--reps` times; the median rep gives ms per call.  Kernel launches per forward are counted with torch.profiler for
the HIP path and for eager (the library's own figure, lipsn_launches_per_forward, is printed beside them), and the device time
of each of the HIP path's launches is listed in launch order at S = 2 and S = 32.  Then VoiceFilter
from raw [0, 255] video at its shipped size (201 x 321 spectrogram, 50 frames of 96 x 96 per speaker) at B = 1 and 4: the
lip reader on 2B streams plus the separator, and the separator alone on precomputed embeddings.

    python tools/shufflenet_lipreader_bench.py [--S 2,8,32] [--T 50] [--H 88] [--W 88] [--relu-type prelu] [--width-mult 1.0]
                                               [--iters 10] [--reps 5] [--out profiles/shufflenet_lipreader_bench.txt]
"""
from __future__ import annotations

import argparse
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speech_separation_amd import Lipreading, ShuffleNetLipreading, VoiceFilter  # noqa: E402
from tests import lipreader_ref as RR  # noqa: E402
from tests import shufflenet_ref as R  # noqa: E402
from tools.lipreader_bench import PEAK_F32_MFMA_TFLOPS, timed  # noqa: E402


def count_launches(fn):
    """Device kernels one call of `fn` enqueues, by torch.profiler; None where the profiler gives no device events."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
        return n or None
    except Exception as e:  # pragma: no cover
        print(f"# torch.profiler unavailable: {e}")
        return None


def launch_times(fn, forwards=4):
    """[(kernel name, mean device microseconds)] of the launches of one call of `fn`, in launch order, by torch.profiler
    over `forwards` calls; [] where the profiler gives no device events."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(forwards):
                fn()
            torch.cuda.synchronize()
        ev = sorted((e for e in prof.events() if str(e.device_type).endswith("CUDA")), key=lambda e: e.time_range.start)
        per = len(ev) // forwards
        if per == 0 or per * forwards != len(ev):
            return []
        us = lambda e: float(getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0))  # noqa: E731
        return [(ev[i].name, float(np.mean([us(ev[f * per + i]) for f in range(forwards)]))) for i in range(per)]
    except Exception as e:  # pragma: no cover
        print(f"# torch.profiler unavailable: {e}")
        return []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", default="2,8,32")
    ap.add_argument("--T", type=int, default=50)
    ap.add_argument("--H", type=int, default=88)
    ap.add_argument("--W", type=int, default=88)
    ap.add_argument("--relu-type", default="prelu")
    ap.add_argument("--width-mult", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--vf-batches", default="1,4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shufflenet_lipreader_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def loaded(module, sd):
        module.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        return module.to(dev).eval()

    sd = R.synthetic_shufflenet_weights("prelu" if a.relu_type == "prelu" else "swish", a.width_mult, 0)
    lip = loaded(ShuffleNetLipreading(relu_type=a.relu_type, width_mult=a.width_mult, extract_feats=True), sd)
    dsd = {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in sd.items()}
    resnet = loaded(Lipreading(relu_type="swish", extract_feats=True), RR.synthetic_lipreader_weights("swish", 0))
    eng = lip._get_engine(dev)
    flops = eng.flops_per_stream(a.T, a.H, a.W)
    res = {"T": a.T, "H": a.H, "W": a.W, "relu_type": a.relu_type, "width_mult": a.width_mult, "flops_per_stream": flops,
           "resnet_flops_per_stream": resnet._get_engine(dev).flops_per_stream(a.T, a.H, a.W),
           "min_bytes_per_stream": eng.min_bytes_per_stream(a.T, a.H, a.W), "weight_pack_bytes": eng.weight_pack_bytes(),
           "launches_per_forward": eng.launches_per_forward(),
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "legs": {}, "voicefilter": {}}
    say(f"# ShuffleNet-v2 lip reader, {a.relu_type}, width {a.width_mult}, T={a.T} {a.H}x{a.W}: {flops / 1e9:.2f} GFLOP per "
        f"stream (ResNet-18 front end: {res['resnet_flops_per_stream'] / 1e9:.2f}); {res['device']}, torch {res['torch']}")
    with torch.no_grad():
        for S in [int(s) for s in a.S.split(",")]:
            x = torch.from_numpy(R.synthetic_video((S, 1, a.T, a.H, a.W), seed=S)).to(dev)
            for _ in range(a.warmup):
                got = lip(x, lengths=[a.T] * S)
                ref = R.run(dsd, x, torch.float32, relu_type=a.relu_type)
                resnet(x, lengths=[a.T] * S)
            torch.cuda.synchronize()
            agree = float(((got - ref).norm(dim=-1) / ref.norm(dim=-1)).max())
            hip = timed(lambda: lip(x, lengths=[a.T] * S), a.iters, a.reps)
            eager = timed(lambda: R.run(dsd, x, torch.float32, relu_type=a.relu_type), a.iters, a.reps)
            rn = timed(lambda: resnet(x, lengths=[a.T] * S), a.iters, a.reps)
            t_flop = S * flops / (PEAK_F32_MFMA_TFLOPS * 1e12) * 1e3
            leg = {"hip_ms": round(hip[0], 4), "hip_ms_spread": [round(hip[1], 4), round(hip[2], 4)],
                   "eager_ms": round(eager[0], 4), "eager_ms_spread": [round(eager[1], 4), round(eager[2], 4)],
                   "resnet_hip_ms": round(rn[0], 4), "resnet_hip_ms_spread": [round(rn[1], 4), round(rn[2], 4)],
                   "streams_per_s": round(S / hip[0] * 1e3, 1), "hip_over_eager_time": round(hip[0] / eager[0], 3),
                   "hip_over_resnet_time": round(hip[0] / rn[0], 3), "tflops": round(S * flops / hip[0] / 1e9, 2),
                   "share_of_flop_bound": round(t_flop / hip[0], 4), "worst_row_vs_eager": agree}
            res["legs"][S] = leg
            say(f"S={S:3d}: HIP {hip[0]:8.3f} ms/call ({leg['streams_per_s']:8.1f} streams/s, {leg['tflops']:6.2f} TFLOP/s, "
                f"{100 * leg['share_of_flop_bound']:.1f} % of the fp32-MFMA bound {t_flop:.3f} ms)   stock eager {eager[0]:8.3f} "
                f"ms/call   HIP/eager time {leg['hip_over_eager_time']:.2f}   ResNet-18 front end (HIP) {rn[0]:8.3f} ms/call   "
                f"ShuffleNet/ResNet time {leg['hip_over_resnet_time']:.2f}   worst row HIP vs eager {agree:.1e}")
        x = torch.from_numpy(R.synthetic_video((2, 1, a.T, a.H, a.W), seed=2)).to(dev)
        res["launches_counted"] = {"hip": count_launches(lambda: lip(x, lengths=[a.T] * 2)),
                                   "eager": count_launches(lambda: R.run(dsd, x, torch.float32, relu_type=a.relu_type))}
        say(f"kernel launches per forward: HIP {res['launches_counted']['hip']} counted by torch.profiler "
            f"({res['launches_per_forward']} by lipsn_launches_per_forward), stock eager {res['launches_counted']['eager']}")

        res["launch_us"] = {}
        for S in (2, 32):
            xs = torch.from_numpy(R.synthetic_video((S, 1, a.T, a.H, a.W), seed=S)).to(dev)
            rows = launch_times(lambda: lip(xs, lengths=[a.T] * S))
            res["launch_us"][S] = [round(t, 1) for _, t in rows]
            say(f"device time per launch, S={S}, microseconds, launch order (torch.profiler, mean of 4 forwards; sum "
                f"{sum(t for _, t in rows):.0f}):")
            for i, (name, t) in enumerate(rows):
                m = re.search(r"(\w+_kernel)", name)
                short = m.group(1) if m else name[:24]
                say(f"  {i:2d} {short:24s} {t:8.1f}")

        # VoiceFilter from raw video: lip reader (2B streams) + separator, and the separator alone
        torch.manual_seed(0)
        vf = VoiceFilter(201, lipreader=lip).to(dev).eval()
        rng = np.random.Generator(np.random.PCG64(1))
        for B in [int(b) for b in a.vf_batches.split(",")]:
            mag = torch.from_numpy(rng.uniform(0.0, 1.0, (B, 201, 321)).astype(np.float32)).to(dev)
            v1 = torch.from_numpy(R.synthetic_clip((B, 50, 96, 96), seed=3)).to(dev)
            v2 = torch.from_numpy(R.synthetic_clip((B, 50, 96, 96), seed=4)).to(dev)
            emb = vf._embed(torch.cat([v1, v2], dim=0)).clone()
            for _ in range(a.warmup):
                vf(mix_magnitude=mag, s1_video=v1, s2_video=v2)
                vf.forward_embeddings(mag, emb[:B], emb[B:])
            torch.cuda.synchronize()
            whole = timed(lambda: vf(mix_magnitude=mag, s1_video=v1, s2_video=v2), a.iters, a.reps)
            sep = timed(lambda: vf.forward_embeddings(mag, emb[:B], emb[B:]), a.iters, a.reps)
            res["voicefilter"][B] = {"from_video_ms": round(whole[0], 4), "from_video_ms_spread": [round(whole[1], 4), round(whole[2], 4)],
                                     "separator_ms": round(sep[0], 4), "separator_ms_spread": [round(sep[1], 4), round(sep[2], 4)]}
            say(f"VoiceFilter from raw video, B={B} (201 x 321, 2 x {B} x 50 x 96 x 96): {whole[0]:8.3f} ms/call "
                f"(min {whole[1]:.3f}, max {whole[2]:.3f});   separator alone on precomputed embeddings {sep[0]:8.3f} ms/call")
    say(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
