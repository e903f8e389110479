#!/usr/bin/env python3
"""Time VoiceFilter's waveform ends on the GPU at n_fft 400, hop 100, B = 1, 4, 16 x 32000 samples, in one process:

  voicefilter_analysis (one launch)            against  voicefilter_magnitude, the composition it replaces (STFT.stft and the
                                                        eager transpose / sqrt / clamp / log10 / clamp / add / atan2 / contiguous)
  voicefilter_waveforms, n_src = 2 (one launch) against  PyTorch-ROCm's torch.istft(10^(5 clamp(p, 0, 1) - 4) * polar)
  VoiceFilter.separate_embeddings              against  forward_embeddings alone, B = 1 and 4 (F = 201, W = 321, Tv = 50):
                                                        what the two ends add to the separator
  run_inference(VoiceFilterSeparator)          items / s over a synthetic dataset on disk (speech_separation_amd.io.
                                                        write_synthetic_dataset) with SI-SNRi, STOI, ESTOI and SI-SDR

Protocol (as tools/specfe_bench.py): every call and shape is warmed up; STEPS calls between two synchronisations; the two
sides alternate, REPS windows each; median (min .. max) per call in microseconds.  No time is a pass criterion.

Usage:  python tools/vf_wave_bench.py [--batches 1,4,16] [--steps 200] [--reps 5] [--items 64] [--rounds 3] [--out profiles/vf_wave_bench.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import speech_separation_amd as S  # noqa: E402
from tests import voicefilter_ref as R  # noqa: E402

T, N, H, F, TV, E = 32000, 400, 100, 201, 50, 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,4,16")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def window(fn):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / a.steps * 1e6

    def compare(label, new, old, names):
        for fn in (new, old):
            for _ in range(5):
                fn()
        torch.cuda.synchronize(dev)
        tn, to = [], []
        for _ in range(a.reps):                                  # the two alternate, so that drift of the box hits both alike
            tn.append(window(new))
            to.append(window(old))
        mn, mo = statistics.median(tn), statistics.median(to)
        say(f"{label}: {names[0]} {mn:8.1f} us ({min(tn):.1f} .. {max(tn):.1f}) | {names[1]} {mo:8.1f} us ({min(to):.1f} .. {max(to):.1f}) "
            f"| {names[1]} / {names[0]} {mo / mn:.3f}")

    say(f"{torch.cuda.get_device_name(dev)}; T = {T}, n_fft {N}, hop {H}; {a.steps} calls per window, median (min .. max) of "
        f"{a.reps} alternating windows, per call")
    win = torch.hann_window(N, device=dev)

    def t_waveforms(p, ph):
        mag = 10.0 ** (5.0 * torch.clamp(p, 0.0, 1.0) - 4.0)
        z = torch.complex(mag * ph[:, 0], mag * ph[:, 1]).reshape(-1, F, p.shape[-1])
        return torch.istft(z, n_fft=N, hop_length=H, window=win, length=T).reshape(p.shape[0], p.shape[1], T)

    model = S.VoiceFilter(F)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in R.synthetic_voicefilter_weights(F, E).items()}, strict=True)
    model = model.to(dev).eval()
    for B in (int(b) for b in a.batches.split(",")):
        g = torch.Generator().manual_seed(B)
        x = (torch.randn(B, T, generator=g) * 0.1).to(dev)
        spec, ph = S.voicefilter_analysis(x, N, H)
        p = (spec * torch.rand(2, *spec.shape, generator=g).to(dev)).contiguous()
        compare(f"B={B:2d} analysis ", lambda: S.voicefilter_analysis(x, N, H), lambda: S.voicefilter_magnitude(x, N, H),
                ("one launch", "voicefilter_magnitude"))
        compare(f"B={B:2d} waveforms", lambda: S.voicefilter_waveforms(p, ph, T, N, H), lambda: t_waveforms(p, ph),
                ("one launch", "PyTorch-ROCm"))
        if B <= 4:
            e1, e2 = (torch.randn(B, TV, E, generator=g).to(dev) for _ in range(2))
            compare(f"B={B:2d} separate ", lambda: model.forward_embeddings(spec, e1, e2), lambda: model.separate_embeddings(x, e1, e2, H),
                    ("forward_embeddings", "separate_embeddings"))
    if a.items > 0:
        from speech_separation_amd.evaluate import run_inference
        from speech_separation_amd.io import write_synthetic_dataset
        from speech_separation_amd.metrics import SISNRiMetric
        with tempfile.TemporaryDirectory() as root:
            entries, _ = write_synthetic_dataset(root, n=a.items, T=T, Tv=TV, emb=E, sr=16000)
            sep = S.VoiceFilterSeparator(model, N, H)
            rates = []
            for _ in range(a.rounds + 1):                        # the first round warms the page cache and the handles
                mets = [SISNRiMetric(name="SISNRiMetric"), S.STOIMetric(16000, name="STOI"), S.STOIMetric(16000, True, name="ESTOI"),
                        S.SISDRMetric(name="SISDR")]
                logs, stats = run_inference(sep, entries, 16, mets, device=dev, workers=8, target_sr=16000)
                rates.append(stats["items_per_s"])
            rates = rates[1:]
            say(f"run_inference(VoiceFilterSeparator), {a.items} items of {T} samples from disk, batches of 16, SI-SNRi + STOI + ESTOI + SI-SDR: "
                f"{statistics.median(rates):.1f} items/s ({min(rates):.1f} .. {max(rates):.1f}) over {a.rounds} rounds")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
