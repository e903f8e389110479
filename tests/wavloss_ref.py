"""TEST INFRASTRUCTURE: the reference's waveform criteria restated in stock PyTorch, differentiable, any float dtype
(src/loss/ss_losses.py:21-26 batch-level PIT, :65-93 MAEWavLoss / MSEWavLoss, :100-114 SiSNRLoss, :117-130 SiSNRWavLoss),
plus utterance-level PIT as the fixtures define it: the reference's class on every item alone (B = 1 slices), averaged.
tests/test_wavloss_host.py pins this file to the values and gradients the reference itself produced
(tests/golden/wavloss_*.npz); the GPU tests then use it as their fp64 oracle at other shapes."""
from __future__ import annotations

import numpy as np
import torch

from tests.sisnr_ref import _sisnr_loss

KINDS = ("mae", "mse", "sisnr")
LEVELS = ("batch", "utterance")
ELEMENT = {"mae": torch.nn.functional.l1_loss, "mse": torch.nn.functional.mse_loss, "sisnr": _sisnr_loss}


def batch_pit(kind, p1, p2, s1, s2):
    """-> (loss, permutation 0/1, L0, L1): BaseSSLoss.forward, ties stay on permutation 0 (strict <)."""
    f = ELEMENT[kind]
    l0 = (f(p1, s1) + f(p2, s2)) / 2
    l1 = (f(p1, s2) + f(p2, s1)) / 2
    swap = bool(l1 < l0)
    return (l1 if swap else l0), int(swap), l0, l1


def pit_loss(kind, level, p1, p2, s1, s2):
    """-> dict(loss, perm int64 [B], l0, l1[, item0 [B], item1 [B]]); l0 / l1 are the batch-level values in both modes,
    item0 / item1 (utterance level only) the per-item values of the two permutations."""
    B = p1.shape[0]
    loss, swap, l0, l1 = batch_pit(kind, p1, p2, s1, s2)
    r = {"perm": torch.tensor([swap] * B), "l0": l0.detach(), "l1": l1.detach()}
    if level == "utterance":
        items = [batch_pit(kind, p1[i:i + 1], p2[i:i + 1], s1[i:i + 1], s2[i:i + 1]) for i in range(B)]
        loss = sum(it[0] for it in items) / B
        r.update(perm=torch.tensor([it[1] for it in items]), item0=torch.stack([it[2].detach() for it in items]),
                 item1=torch.stack([it[3].detach() for it in items]))
    r["loss"] = loss
    return r


def evaluate(kind, level, p1, p2, s1, s2, dtype=torch.float64):
    """numpy in -> numpy out, with d loss / d prediction from autograd: dict(loss, perm, l0, l1, item0, item1, d1, d2)."""
    t = [torch.from_numpy(np.array(a)).to(dtype) for a in (p1, p2, s1, s2)]
    t[0].requires_grad_(True)
    t[1].requires_grad_(True)
    r = pit_loss(kind, level, *t)
    r["loss"].backward()
    out = {k: v.detach().numpy() for k, v in r.items()}
    out["d1"], out["d2"] = t[0].grad.numpy(), t[1].grad.numpy()
    return out


AMPS = (0.1, 1e-3, 30.0)      # per-item amplitudes, cycled over the batch (the spirit of tests/hard_inputs.py)


def make_case(B, T, seed, swapped=(), mix=0.0):
    """Seeded fp32 (s1_pred, s2_pred, s1, s2) [B][T]: item i has amplitude AMPS[i % 3]; the last item of a batch of two or
    more carries a DC offset of 10x its amplitude (the SI-SNR zero-mean cancellation); s1_pred is s1 plus 5 % noise,
    s2_pred is s2 plus 20 % noise and a small offset; `mix` leaks that share of the other speaker into both predictions
    (the two batch-level losses then have the same order of magnitude); the items in `swapped` have their predictions
    exchanged (permutation 1 is right there); on T // 4 : T // 2 of item 0, s1_pred equals its target exactly (the MAE
    gradient is exactly 0 there)."""
    rng = np.random.default_rng(seed)
    amp = np.array([AMPS[i % 3] for i in range(B)])[:, None]
    s1, s2 = amp * rng.standard_normal((B, T)), amp * rng.standard_normal((B, T))
    if B >= 2:
        s1[-1] += 10 * amp[-1]
        s2[-1] -= 10 * amp[-1]
    p1 = (1 - mix) * s1 + mix * s2 + 0.05 * amp * rng.standard_normal((B, T))
    p2 = (1 - mix) * s2 + mix * s1 + 0.2 * amp * rng.standard_normal((B, T)) + 0.03 * amp
    p1, p2, s1, s2 = (a.astype(np.float32) for a in (p1, p2, s1, s2))
    p1[0, T // 4:T // 2] = s1[0, T // 4:T // 2]
    for i in swapped:
        p1[i], p2[i] = p2[i].copy(), p1[i].copy()
    return p1, p2, s1, s2
