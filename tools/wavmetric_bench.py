#!/usr/bin/env python3
"""Time the evaluation metrics on the GPU: STOIMetric, STOIMetric(extended=True) and SISDRMetric at B = 1, 4, 16 x 32000
samples, fs = 16000, against the fp64 numpy restatement of the same algorithm (tests/stoi_ref.py) on the CPU in the same
run; then evaluate.run_inference items/s on a synthetic dataset with metrics [SISNRi] and with [SISNRi, STOI, ESTOI, SISDR].

The CPU side is the project's restatement, NOT pystoi (which is not a dependency and has not been timed): one
(clean, estimate) pair at a time, four pairs per item, as the reference's STOIMetric calls pystoi.

Protocol: every shape is warmed up; STEPS enqueue() calls between two synchronisations, median and spread of REPS windows.
The run_inference lines use a stand-in separator (a weighted sum of the targets and the mixture) so that the loop measures
the data path and the metrics, not a model; after one uncounted round the two metric lists alternate run by run.  No time is a pass criterion.

Usage:  python tools/wavmetric_bench.py [--batches 1,4,16] [--steps 200] [--reps 5] [--items 256] [--rounds 5] [--out profiles/wavmetric_bench.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speech_separation_amd import SISDRMetric, STOIMetric  # noqa: E402
from speech_separation_amd.evaluate import run_inference  # noqa: E402
from speech_separation_amd.io import write_synthetic_dataset  # noqa: E402
from speech_separation_amd.metrics import SISNRiMetric  # noqa: E402
from tests import stoi_ref as R  # noqa: E402

T, FS = 32000, 16000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,4,16")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--items", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"{torch.cuda.get_device_name(dev)}; T = {T}, fs = {FS}; {a.steps} enqueue() calls per window, median (min .. max) of "
        f"{a.reps} windows; CPU: the fp64 numpy restatement tests/stoi_ref.py, one pair at a time (not pystoi)")
    mets = {"STOI": STOIMetric(fs=FS), "ESTOI": STOIMetric(fs=FS, extended=True), "SISDR": SISDRMetric()}
    for B in (int(b) for b in a.batches.split(",")):
        arrays = R.make_batch(FS, B, T, seed=B)
        batch = dict(zip(("s1_pred", "s2_pred", "s1", "s2"), (torch.from_numpy(x).to(dev) for x in arrays)))
        t0 = time.perf_counter()
        for b in range(B):
            for p in arrays[:2]:
                for s in arrays[2:]:
                    R.stoi(s[b], p[b], FS)
        cpu_pair = (time.perf_counter() - t0) / (4 * B)
        for label, met in mets.items():
            for _ in range(3):
                met.enqueue(**batch)
            torch.cuda.synchronize(dev)
            wins = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    met.enqueue(**batch)
                torch.cuda.synchronize(dev)
                wins.append((time.perf_counter() - t0) / a.steps * 1e6)
            med = statistics.median(wins)
            tail = "" if label == "SISDR" else f" | restatement {cpu_pair * 1e3:.1f} ms per pair, {cpu_pair * 4 * B * 1e3:.0f} ms per batch | x{cpu_pair * 4 * B * 1e6 / med:.0f}"
            say(f"B={B:2d} {label:5s}: HIP {med:8.1f} us per call ({min(wins):.1f} .. {max(wins):.1f}){tail}")

    def model(mix, s1=None, s2=None, **batch):
        return {"s1_pred": 0.8 * s1 + 0.2 * mix, "s2_pred": 0.6 * s2 + 0.4 * mix}

    with tempfile.TemporaryDirectory() as tmp:
        entries, _ = write_synthetic_dataset(tmp, n=a.items, T=T, sr=FS)
        configs = {"[SISNRi]": lambda: [SISNRiMetric()],
                   "[SISNRi, STOI, ESTOI, SISDR]": lambda: [SISNRiMetric(), STOIMetric(fs=FS, name="STOI"),
                                                            STOIMetric(fs=FS, extended=True, name="ESTOI"), SISDRMetric()]}
        seen = {k: [] for k in configs}
        logs = {}
        for rnd in range(a.rounds + 1):                 # round 0 warms the page cache, the loaders and the handles: not counted
            for label, ms in configs.items():           # the two lists alternate, so that drift of the box hits both alike
                logs[label], stats = run_inference(model, entries, 16, ms(), save_dir=None, device=dev, workers=8, target_sr=FS)
                if rnd:
                    seen[label].append(stats["items_per_s"])
        rates = {k: statistics.median(v) for k, v in seen.items()}
        for label, v in seen.items():
            say(f"run_inference, {a.items} items of {T} samples in batches of 16, stand-in separator, metrics {label}: "
                f"{rates[label]:.1f} items/s (median of {a.rounds} alternating runs; {min(v):.1f} .. {max(v):.1f}); " +
                ", ".join(f"{k} {float(x):.4f}" for k, x in logs[label].items()))
        r = list(rates.values())
        say(f"ratio of the two run_inference lines: {r[1] / r[0]:.3f}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
