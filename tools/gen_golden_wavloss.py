#!/usr/bin/env python3
"""Generate tests/golden/wavloss_*.npz by RUNNING the reference's waveform criteria on the CPU.

Runs only where the reference repository is present (REFERENCE_ROOT, default /root/reference); the tests never see the
reference -- they see the small .npz fixtures this script writes: data only, no reference program text.  The reference
package __init__ pulls modules that are absent here, so src/loss/ss_losses.py is imported through stub packages (as
tools/gen_golden.py does).

Every fixture holds the fp32 inputs and, for MAEWavLoss / MSEWavLoss / SiSNRWavLoss (src/loss/ss_losses.py:65-93,
:117-130), at batch level (the class as it is, BaseSSLoss :21-26) and at utterance level (the class applied to every
item alone -- B = 1 slices -- and averaged: the definition these fixtures pin), in fp32 and in fp64:
  <kind>.<level>.loss<32|64>   the loss
  <kind>.<level>.l0_<32|64>    (loss(s1_pred, s1) + loss(s2_pred, s2)) / 2 over the batch, .l1_: targets swapped
  <kind>.<level>.perm<32|64>   permutation per item (batch level: the same value B times)
  <kind>.<level>.d1_<32|64>    d loss / d s1_pred from the reference's own loss.backward(), .d2_: d s2_pred

Usage:  python tools/gen_golden_wavloss.py
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
from tests.wavloss_ref import make_case  # noqa: E402

REF = os.environ.get("REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")

#: name -> (B, T, seed, swapped items, kinds)
CASES = {
    "wavloss_mixed_b5_t67": (5, 67, 11, (1, 3), ("mae", "mse", "sisnr")),
    "wavloss_swap_b3_t131": (3, 131, 12, (0, 1, 2), ("mae", "mse", "sisnr")),
    "wavloss_b2_t1": (2, 1, 13, (1,), ("mae", "mse")),
}


def import_reference():
    for name, path in [("src", f"{REF}/src"), ("src.loss", f"{REF}/src/loss")]:
        m = types.ModuleType(name)
        m.__path__ = [path]
        sys.modules[name] = m
    sys.path.insert(0, REF)
    return importlib.import_module("src.loss.ss_losses")


def run(crit, level, arrays, dtype):
    p1, p2, s1, s2 = (torch.from_numpy(a).to(dtype) for a in arrays)
    p1.requires_grad_(True)
    p2.requires_grad_(True)
    B = p1.shape[0]
    with torch.no_grad():
        l0 = (crit.loss(p1, s1) + crit.loss(p2, s2)) / 2
        l1 = (crit.loss(p1, s2) + crit.loss(p2, s1)) / 2
    if level == "batch":
        loss = crit(s1_pred=p1, s2_pred=p2, s1=s1, s2=s2)["loss"]
        perm = [int(l1 < l0)] * B
    else:
        sl = [slice(i, i + 1) for i in range(B)]
        loss = sum(crit(s1_pred=p1[i], s2_pred=p2[i], s1=s1[i], s2=s2[i])["loss"] for i in sl) / B
        with torch.no_grad():
            perm = [int((crit.loss(p1[i], s2[i]) + crit.loss(p2[i], s1[i])) / 2 < (crit.loss(p1[i], s1[i]) + crit.loss(p2[i], s2[i])) / 2)
                    for i in sl]
    loss.backward()
    return {"loss": loss.detach().numpy(), "l0_": l0.numpy(), "l1_": l1.numpy(), "perm": np.array(perm, dtype=np.int32),
            "d1_": p1.grad.numpy(), "d2_": p2.grad.numpy()}


def main():
    losses = import_reference()
    classes = {"mae": losses.MAEWavLoss, "mse": losses.MSEWavLoss, "sisnr": losses.SiSNRWavLoss}
    for name, (B, T, seed, swapped, kinds) in CASES.items():
        arrays = make_case(B, T, seed, swapped)
        z = dict(zip(("s1_pred", "s2_pred", "s1", "s2"), arrays))
        z["kinds"] = np.array(kinds)
        for kind in kinds:
            for level in ("batch", "utterance"):
                for bits, dtype in ((32, torch.float32), (64, torch.float64)):
                    for k, v in run(classes[kind](), level, arrays, dtype).items():
                        z[f"{kind}.{level}.{k}{bits}"] = v
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **z)
        print(f"{path}: {os.path.getsize(path) / 1024:.1f} kB")


if __name__ == "__main__":
    main()
