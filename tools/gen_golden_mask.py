#!/usr/bin/env python3
"""Generate the masked-DPTN fixtures tests/golden/mask_*.npz / grad_mask_*.npz by RUNNING the reference's DPTNEncDec
(src/model/dptn.py:139-208, model/dptn.yaml) on the CPU.  Helpers (reference import, key-order check, taps, gradients,
digests, subsampling) come from tools/gen_golden.py, which this script leaves unchanged.

Fixtures:
  mask_tiny      tiny shape, every tail tensor, weights and inputs stored (the CPU restatement tests/mask_tail_ref.py)
  mask_mid       N = 64, 2 blocks, B = 2, T = 8000      outputs + strided tail taps
  mask_mid128    N = 128, otherwise as mask_mid
  mask_full      the dptn.yaml shape, B = 1, T = 32000  outputs + thinly strided tail taps
  grad_mask_mid / grad_mask_mid128   the reference's fp32 and fp64 loss.backward(), dropout 0 (reference_gradients format)
Tail taps: "ola" (B,2N,ola) the overlap-added separation output, "masks" (2,B,N,L) m = ReLU(tanh(output) *
sigmoid(output_gate)), "masked" (2,B,N,L) m * encoded, the decoder's input.

Usage:  python tools/gen_golden_mask.py [name ...]
"""
from __future__ import annotations

import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speech_separation_amd.spec import DPTN_MASK, DPTN_TINY, DPTNConfig, synthetic_inputs, synthetic_state_dict  # noqa: E402
from tools.gen_golden import (OUT, build_reference, import_reference, loss_and_metric, reference_gradients,  # noqa: E402
                              run_with_taps, subsample, weights_digest, GRAD_STRIDE, GRAD_FULL_BELOW)

MASK_TINY = DPTNConfig(**{**DPTN_TINY.to_dict(), "audio_only": True, "arch": "dptn_mask"})
MASK_MID = DPTNConfig(**{**DPTN_MASK.to_dict(), "num_blocks": 2})
MASK_MID128 = DPTNConfig(**{**MASK_MID.to_dict(), "num_features": 128, "hidden_video": 128})


def masked_module():
    """The reference module namespace build_reference() expects, with DPTNEncDec in the audio-only slot (an audio-only,
    arch != "dprnn" config instantiates `DPTNWavEncDec`; the constructor kwargs of the two classes are the same)."""
    dptn_wav, losses = import_reference()
    dptn = importlib.import_module("src.model.dptn")
    return types.SimpleNamespace(DPTNWavEncDec=dptn.DPTNEncDec), losses


def tail_taps(taps):
    out = {"ola": taps["ola"], "masks": taps["masks"], "masked": taps["masks"] * taps["encoded"][None]}
    return out


def main():
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)
    torch.manual_seed(0)
    mod, losses = masked_module()
    only = set(sys.argv[1:])

    # ---- tiny: weights, inputs, the tail's input and every tail tensor in full ----
    if not only or "mask_tiny" in only:
        cfg = MASK_TINY
        sd = synthetic_state_dict(cfg, seed=7)
        inp = synthetic_inputs(cfg, B=2, T=209, Tv=9, seed=11)
        model = build_reference(mod, cfg, sd)
        taps = run_with_taps(model, cfg, inp)
        extra = loss_and_metric(losses, taps, inp)
        keep = {k: taps[k] for k in ("s1_pred", "s2_pred", "encoded", f"blk{cfg.num_blocks - 1}_out", "sep")}
        keep.update(tail_taps(taps))
        np.savez_compressed(os.path.join(OUT, "mask_tiny.npz"), cfg=np.array(repr(cfg.to_dict())),
                            digest=np.array(weights_digest(sd)),
                            **{f"w.{k}": v for k, v in sd.items()}, **{f"in.{k}": v for k, v in inp.items()},
                            **{f"tap.{k}": v for k, v in keep.items()}, **{f"val.{k}": v for k, v in extra.items()})
        print("mask_tiny", "loss", extra["pit_loss"])

    # ---- real feature sizes: outputs + strided tail taps ----
    cases = [("mask_mid", MASK_MID, dict(B=2, T=8000, Tv=50), 97),
             ("mask_mid128", MASK_MID128, dict(B=2, T=8000, Tv=50), 97),
             ("mask_full", DPTN_MASK, dict(B=1, T=32000, Tv=50), 997)]
    for name, cfg, shp, step in cases:
        if only and name not in only:
            continue
        sd = synthetic_state_dict(cfg, seed=0)
        inp = synthetic_inputs(cfg, seed=123, **shp)
        model = build_reference(mod, cfg, sd)
        taps = run_with_taps(model, cfg, inp)
        extra = loss_and_metric(losses, taps, inp)
        keep = {"s1_pred": taps["s1_pred"], "s2_pred": taps["s2_pred"]}
        for k, v in tail_taps(taps).items():
            keep[f"strided{step}.{k}"] = subsample(v, step)
        np.savez_compressed(os.path.join(OUT, f"{name}.npz"), cfg=np.array(repr(cfg.to_dict())),
                            shape=np.array([shp["B"], shp["T"], shp["Tv"]]), digest=np.array(weights_digest(sd)),
                            **{f"tap.{k}": v for k, v in keep.items()}, **{f"val.{k}": v for k, v in extra.items()})
        print(name, "loss", extra["pit_loss"], "rms", float(np.sqrt((taps["s1_pred"] ** 2).mean())))

    # ---- the reference's loss.backward(), dropout 0 ----
    for name, cfg in (("grad_mask_mid", MASK_MID), ("grad_mask_mid128", MASK_MID128)):
        if only and name not in only:
            continue
        cfg = DPTNConfig(**{**cfg.to_dict(), "dropout": 0.0})
        shp, wseed, iseed = dict(B=2, T=8000, Tv=50), 0, 123
        sd = synthetic_state_dict(cfg, seed=wseed)
        inp = synthetic_inputs(cfg, seed=iseed, **shp)
        rec = reference_gradients(mod, losses, cfg, sd, inp)
        np.savez_compressed(os.path.join(OUT, f"{name}.npz"), cfg=np.array(repr(cfg.to_dict())),
                            shape=np.array([shp["B"], shp["T"], shp["Tv"]]), seeds=np.array([wseed, iseed]),
                            stride=np.array(GRAD_STRIDE), full_below=np.array(GRAD_FULL_BELOW),
                            digest=np.array(weights_digest(sd)), **rec)
        print(name, "loss", rec["val.loss"], rec["val.loss64"], "grad norm", rec["val.grad_norm"],
              "reference fp32 vs fp64, worst parameter:", min((float(v), k) for k, v in rec.items() if k.startswith("ref32db.")))


if __name__ == "__main__":
    main()
