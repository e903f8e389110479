"""Cost of the long-sequence training attention (option train_long_seq, attn_long_train.h), measured in ONE process:

  (a) forced-mode cost: the BASELINE training shape (DPTN-AV, B = 16, T = 32000, dropout 0.1), ms per optimizer step with
      train_long_seq = 0 (on-chip attention trio) and = 2 (streaming trio at every length: S = 141, K = 150), legs interleaved
      A B A B ...; the ratio is the streaming trio's price where both run.
  (b) long clips: T = 80000 (10 s at 8 kHz, S = 354 chunks) at B = 4 and B = 16 with train_long_seq = 1 -- ms per step, ms per
      second of audio, the tape / workspace bytes of the size queries -- beside the T = 32000 step of the same process.

    python3 tools/train_long_ab.py [--rounds 4] [--steps 6] [--warmup 2] > profiles/train_long_seq.txt

A step is zero_grad, forward with tape, device PIT SI-SNR loss, HIP backward, device clip + AdamW (train.train_step); a leg is
timed with a host clock between two device synchronisations, after warm-up steps of the same shape and setting.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from speech_separation_amd import DPTNAVWavEncDec  # noqa: E402
from speech_separation_amd.build import source_digest  # noqa: E402
from speech_separation_amd.spec import DPTN_AV, synthetic_inputs, synthetic_state_dict  # noqa: E402
from speech_separation_amd.train import FusedAdamW, SiSNRWavLoss, train_step  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_long_ab: needs the GPU (no timing is taken without one)")
    dev = torch.device("cuda:0")
    cfg = DPTN_AV
    kw = {k: v for k, v in cfg.to_dict().items() if k not in ("audio_only", "arch")}
    model = DPTNAVWavEncDec(**kw, long_training=True)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_state_dict(model.cfg, seed=0).items()})
    model = model.to(dev).train()
    opt = FusedAdamW(model.parameters(), lr=1e-3)
    crit = SiSNRWavLoss()
    eng = model._get_engine(dev)
    print(f"# {torch.cuda.get_device_name(0)}; kernel sources {source_digest()}; DPTN-AV (6 blocks, 128 features, chunk 150 / hop 75), "
          f"dropout 0.1; {args.warmup} warm-up + {args.steps} timed steps per leg")

    batches = {}

    def batch(B, T):
        if (B, T) not in batches:
            Tv = 50 * T // 32000
            batches[(B, T)] = {k: torch.from_numpy(v).to(dev) for k, v in synthetic_inputs(cfg, B=B, T=T, Tv=Tv, seed=123).items()}
        return batches[(B, T)]

    def leg(B, T, long_seq):
        eng.set_option("train_long_seq", long_seq)
        b = batch(B, T)
        for _ in range(args.warmup):
            train_step(model, dict(b), crit, opt, 10.0)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            stats = train_step(model, dict(b), crit, opt, 10.0)
        torch.cuda.synchronize(dev)
        ms = 1e3 * (time.perf_counter() - t0) / args.steps
        assert torch.isfinite(stats["loss"]).item()
        return ms

    def sizes(B, T):
        Tv = 50 * T // 32000
        return (int(eng.lib.dptnav_train_tape_bytes(eng._h, B, T, Tv)), int(eng.lib.dptnav_train_workspace_bytes(eng._h, B, T, Tv)))

    # ---- (a) forced mode at the BASELINE training shape
    B, T = 16, 32000
    print(f"\n(a) B = {B}, T = {T} (S = {eng.chunks(T)}, K = {cfg.chunk_size}): train_long_seq 0 (on-chip trio) vs 2 (streaming trio), interleaved")
    res = {0: [], 2: []}
    for r in range(args.rounds):
        for v in (0, 2):
            res[v].append(leg(B, T, v))
            print(f"  round {r} train_long_seq={v}: {res[v][-1]:8.2f} ms/step", flush=True)
    m0, m2 = statistics.median(res[0]), statistics.median(res[2])
    print(f"  median  train_long_seq=0: {m0:.2f} ms/step (min {min(res[0]):.2f}, max {max(res[0]):.2f})")
    print(f"  median  train_long_seq=2: {m2:.2f} ms/step (min {min(res[2]):.2f}, max {max(res[2]):.2f})")
    print(f"  ratio 2 / 0 of the whole step: {m2 / m0:.4f}")

    # ---- (b) long clips
    print("\n(b) train_long_seq = 1: T = 80000 (10 s) beside T = 32000 (4 s) of the same process")
    for B in (4, 16):
        rows = []
        for T in (32000, 80000):
            ms = [leg(B, T, 1) for _ in range(2)]
            tape, ws = sizes(B, T)
            secs = B * T / 8000.0
            rows.append((T, min(ms)))
            print(f"  B = {B:2d} T = {T} (S = {eng.chunks(T)}): {ms[0]:8.2f} / {ms[1]:8.2f} ms/step -> {min(ms) / secs:6.3f} ms per second of audio; "
                  f"tape {tape / 2**30:.2f} GiB, workspace {ws / 2**30:.2f} GiB", flush=True)
        print(f"  B = {B:2d}: 10 s step / 4 s step = {rows[1][1] / rows[0][1]:.3f} (2.5 x the audio)")
        batches.clear()
        eng._tws = None
        torch.cuda.empty_cache()
    print("\n# one box, one process: compare figures within this file only")


if __name__ == "__main__":
    main()
