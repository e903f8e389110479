#!/usr/bin/env python3
"""Time the spectral front end on the GPU: STFT(256, 128).stft / .istft, their two backward calls and LogMelSpectrogram()
at B = 1, 4, 16 x 32000 samples, against PyTorch-ROCm in the same process: torch.stft + stack / transpose / contiguous (the
reference's STFT.stft), torch.istft with AudioDecoder's arguments, autograd's backward through each, and the eager
log-mel composition log(clamp((|torch.stft(n_fft=400, hop=200)|^2)^T @ fb, 1e-5)) with the filterbank of tests/spec_ref.py
already on the device (torchaudio is not a dependency and has not been timed).

Protocol (as tools/wavmetric_bench.py): every call and shape is warmed up; STEPS calls between two synchronisations;
the HIP and the PyTorch window alternate, REPS windows each; median (min .. max) per call in microseconds.  The backward
lines time the backward alone: the forward graph is rebuilt outside the window (retain_graph).  No time is a pass criterion.

Usage:  python tools/specfe_bench.py [--batches 1,4,16] [--steps 200] [--reps 5] [--out profiles/specfe_bench.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speech_separation_amd import LogMelSpectrogram, STFT  # noqa: E402
from speech_separation_amd import spectral as S  # noqa: E402
from tests import spec_ref as R  # noqa: E402

T, N, H = 32000, 256, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,4,16")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
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

    def compare(label, hip, ref):
        for fn in (hip, ref):
            for _ in range(5):
                fn()
        torch.cuda.synchronize(dev)
        th, tr = [], []
        for _ in range(a.reps):                                  # the two alternate, so that drift of the box hits both alike
            th.append(window(hip))
            tr.append(window(ref))
        mh, mr = statistics.median(th), statistics.median(tr)
        say(f"{label}: HIP {mh:8.1f} us ({min(th):.1f} .. {max(th):.1f}) | PyTorch-ROCm {mr:8.1f} us ({min(tr):.1f} .. {max(tr):.1f}) "
            f"| PyTorch / HIP {mr / mh:.2f}")

    say(f"{torch.cuda.get_device_name(dev)}; T = {T}; stft / istft at n_fft {N}, hop {H}; log-mel at n_fft 400, hop 200, 128 bands; "
        f"{a.steps} calls per window, median (min .. max) of {a.reps} alternating windows, per call")
    enc, mel = STFT(N, H), LogMelSpectrogram()
    win, win400 = torch.hann_window(N, device=dev), torch.hann_window(400, device=dev)
    fb = torch.from_numpy(R.mel_filterbank(16000, 400, 128)).float().to(dev)

    def t_stft(x):
        z = torch.stft(x, n_fft=N, hop_length=H, window=win, return_complex=True)
        return torch.stack([z.real, z.imag], dim=1).transpose(2, 3).contiguous()

    def t_istft(X):
        return torch.istft(torch.complex(X[:, 0], X[:, 1]).transpose(1, 2).contiguous(), n_fft=N, hop_length=H, window=win, length=T)

    def t_logmel(x):
        z = torch.stft(x, n_fft=400, hop_length=200, window=win400, return_complex=True)
        return torch.log(torch.clamp((z.real ** 2 + z.imag ** 2).transpose(1, 2) @ fb, min=1e-5)).transpose(1, 2)

    for B in (int(b) for b in a.batches.split(",")):
        g = torch.Generator().manual_seed(B)
        x = torch.randn(B, T, generator=g).to(dev)
        X = enc.stft(x).detach()
        M = X.shape[2]
        gX, gy = torch.randn(X.shape, generator=g).to(dev), torch.randn(B, T, generator=g).to(dev)
        compare(f"B={B:2d} stft          ", lambda: enc.stft(x), lambda: t_stft(x))
        compare(f"B={B:2d} istft         ", lambda: enc.istft(X, length=T), lambda: t_istft(X))
        xr, Xr = x.clone().requires_grad_(True), X.clone().requires_grad_(True)
        fx, fX = t_stft(xr), t_istft(Xr)
        compare(f"B={B:2d} stft backward ", lambda: S.stft_backward(gX, T, N, H),
                lambda: torch.autograd.grad(fx, xr, gX, retain_graph=True))
        compare(f"B={B:2d} istft backward", lambda: S.istft_backward(gy, M, N, H),
                lambda: torch.autograd.grad(fX, Xr, gy, retain_graph=True))
        compare(f"B={B:2d} log-mel       ", lambda: mel(x), lambda: t_logmel(x))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
