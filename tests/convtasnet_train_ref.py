"""TEST INFRASTRUCTURE (not product code): the reference's ConvTasNet forward composed from stock PyTorch operators in a
form autograd can differentiate (oracle/convtasnet_stock.forward is the same computation under torch.no_grad()).  The
gradients of TrainableConvTasNet are compared with fp64 autograd through this restatement; tests/golden/convtasnet_grad.npz
(the reference's own ConvTasNet and SiSNRWavLoss, loss.backward() on the CPU) pins the restatement itself.

Follows src/model/convtasnet.py: Encoder :6-15, GlobalNorm :18-29 (eps 5e-6), Conv1D_Block :32-53 (GroupNorm(1) eps 1e-10),
Separator :55-83, Decoder :85-99 (ConvTranspose1d(512, 1, 32, stride 16), crop [16, len - 32)).
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn.functional as F

from oracle.convtasnet_stock import H, L, N, P, R, X


def _prelu(x, a, mask):
    # mask: which branch each element takes (x > 0); None: decided from x itself (F.prelu)
    return F.prelu(x, a) if mask is None else torch.where(mask, x, a * x)


def forward(sd: Dict[str, torch.Tensor], mix: torch.Tensor, masks: Optional[dict] = None,
            taps: Optional[dict] = None) -> Dict[str, torch.Tensor]:
    """mix [B][T] -> {"s1_pred", "s2_pred"} [B][16 (T // 16)], differentiable in every tensor of `sd`.

    masks (optional): the PReLU branch of every element, {"v1": [24 x [B][512][F] bool], "u": [...], "skip": [B][128][F]
    bool}.  A PReLU's derivative jumps at 0, so an input within rounding of 0 can take the other branch in another
    implementation: an fp64 reference that follows the branches of the implementation under test measures its arithmetic
    rather than where rounding put the kinks.

    taps (optional): a dict that receives the pre-activations the training forward keeps on its tape, detached, in this
    restatement's [B][C][F] layout: {"v1": [24 x [B][512][F]] (input of PReLU_1), "u": [24 x ...] (input of PReLU_2),
    "skip": [B][128][F] (input of seq.0's PReLU)}."""
    if taps is not None:
        taps.update(v1=[], u=[], skip=None)
    mk = (lambda name, i=None: None) if masks is None else (
        lambda name, i=None: masks[name] if i is None else masks[name][i])
    bs = mix.shape[0]
    enc = F.conv1d(F.pad(mix.unsqueeze(1), (L, 2 * L)), sd["encoder.conv1d.weight"], stride=L)
    mu = enc.mean(dim=(1, 2), keepdim=True)
    var = ((enc - mu) ** 2).mean(dim=(1, 2), keepdim=True)
    x = sd["separator.norm_1.gamma"] * (enc - mu) / torch.sqrt(var + 5e-6) + sd["separator.norm_1.beta"]
    x = F.conv1d(x, sd["separator.conv1d.weight"], sd["separator.conv1d.bias"])
    acc = 0.0
    for i in range(P * X):
        p, dil = f"separator.separator.{i}.", 2 ** (i % X)
        v1 = F.conv1d(x, sd[p + "conv1d.weight"], sd[p + "conv1d.bias"])
        c = F.group_norm(_prelu(v1, sd[p + "PReLU_1.weight"], mk("v1", i)), 1, sd[p + "norm_1.weight"], sd[p + "norm_1.bias"],
                         eps=1e-10)
        u = F.conv1d(c, sd[p + "dconv1d.weight"], sd[p + "dconv1d.bias"], padding=(dil * (R - 1)) // 2, dilation=dil, groups=H)
        c = F.group_norm(_prelu(u, sd[p + "PReLU_2.weight"], mk("u", i)), 1, sd[p + "norm_2.weight"], sd[p + "norm_2.bias"],
                         eps=1e-10)
        if taps is not None:
            taps["v1"].append(v1.detach()), taps["u"].append(u.detach())
        x = x + F.conv1d(c, sd[p + "conv.weight"], sd[p + "conv.bias"])
        acc = acc + F.conv1d(c, sd[p + "conv_sc.weight"], sd[p + "conv_sc.bias"])
    if taps is not None:
        taps["skip"] = acc.detach()
    m = torch.sigmoid(F.conv1d(_prelu(acc, sd["separator.seq.0.weight"], mk("skip")), sd["separator.seq.1.weight"],
                               sd["separator.seq.1.bias"]))
    y = (enc.unsqueeze(1) * m.reshape(bs, 2, N, -1)).reshape(-1, N, enc.shape[-1])
    y = F.conv_transpose1d(y, sd["decoder.deconv.weight"], stride=L)
    y = y[:, :, L:y.shape[2] - 2 * L].reshape(bs, 2, -1)
    return {"s1_pred": y[:, 0], "s2_pred": y[:, 1]}


def grads(sd: Dict[str, torch.Tensor], mix: torch.Tensor, d1: torch.Tensor, d2: torch.Tensor, dtype=torch.float64,
          masks: Optional[dict] = None) -> Dict[str, torch.Tensor]:
    """Vector-Jacobian product of the restatement in `dtype`: {key: d <out, (d1, d2)> / d key} (masks: see forward)."""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    out = forward(p, mix.to(dtype), masks)
    g = torch.autograd.grad([out["s1_pred"], out["s2_pred"]], list(p.values()), [d1.to(dtype), d2.to(dtype)],
                            allow_unused=True)    # the last block's residual conv feeds nothing: its gradient is zero
    return {k: torch.zeros_like(v) if gk is None else gk for (k, v), gk in zip(p.items(), g)}


def tape_tensors(eng, B: int, T: int) -> dict:
    """The pre-activations on the tape of the forward `eng` just ran for B x T (cttrain_tape_offset), copied to the layout of
    forward's `taps`."""
    tape = (eng._tape_id, B, T, eng._ws.data_ptr())
    Fr = eng.frames(T)
    lay = lambda t: t.view(B, Fr, t.shape[1]).permute(0, 2, 1).clone()
    return {"v1": [lay(eng.tape_tensor(tape, eng.TAPE_V1, i)) for i in range(P * X)],
            "u": [lay(eng.tape_tensor(tape, eng.TAPE_U, i)) for i in range(P * X)],
            "skip": lay(eng.tape_tensor(tape, eng.TAPE_SKIP))}


def prelu_masks(eng, B: int, T: int) -> dict:
    """The PReLU branch (input > 0) of every element in the forward `eng` (speech_separation_amd.ConvTasNetTrainEngine)
    just ran for B x T, read from its tape, in this restatement's [B][C][F] layout (the `masks` of forward)."""
    tape = (eng._tape_id, B, T, eng._ws.data_ptr())
    Fr = eng.frames(T)
    lay = lambda t: (t > 0).view(B, Fr, t.shape[1]).permute(0, 2, 1).clone()
    return {"v1": [lay(eng.tape_tensor(tape, eng.TAPE_V1, i)) for i in range(P * X)],
            "u": [lay(eng.tape_tensor(tape, eng.TAPE_U, i)) for i in range(P * X)],
            "skip": lay(eng.tape_tensor(tape, eng.TAPE_SKIP))}
