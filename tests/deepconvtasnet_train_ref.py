"""TEST INFRASTRUCTURE (not product code): the reference's DeepConvTasNet forward composed from stock PyTorch operators in a
form autograd can differentiate (tests/deepconvtasnet_ref.forward is the same computation under torch.no_grad()).  The
gradients of TrainableDeepConvTasNet are compared with fp64 autograd through this restatement;
tests/golden/deepconvtasnet_grad_slopes.npz (the reference's own DeepConvTasNet and SiSNRWavLoss, loss.backward() on the
CPU) pins the restatement itself.  Modelled on tests/convtasnet_train_ref.py.

Follows src/model/deepconvtasnet.py: Encoder :7-26, Separator (Conv-TasNet's), Decoder :96-120; decoder.deconv.weight is a
parameter the forward never reads.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn.functional as F

from oracle.convtasnet_stock import H, L, N, P, R, X
from tests.convtasnet_train_ref import _prelu
from tests.deepconvtasnet_ref import DEC_DIL, ENC_DIL

UNUSED = "decoder.deconv.weight"


def forward(sd: Dict[str, torch.Tensor], mix: torch.Tensor, masks: Optional[dict] = None,
            taps: Optional[dict] = None) -> Dict[str, torch.Tensor]:
    """mix [B][T] -> {"s1_pred", "s2_pred"} [B][16 (T // 16)], differentiable in every tensor of `sd` it reads.

    masks (optional): the PReLU branch (input > 0) of every element: {"v1": [24 x [B][512][F] bool], "u": [...], "skip":
    [B][128][F], "ez": [4 x [B][512][F]] (dense encoder layers), "dz": [4 x [2B][512][F]] (dense decoder layers, batch in
    (b, speaker) order)}; see tests/convtasnet_train_ref.forward for why.

    taps (optional): a dict that receives the pre-activations the training forward keeps on its tape, detached, under the
    same names and layouts."""
    if taps is not None:
        taps.update(v1=[], u=[], skip=None, ez=[], dz=[])
    mk = (lambda name, i=None: None) if masks is None else (
        lambda name, i=None: masks[name] if i is None else masks[name][i])
    bs = mix.shape[0]
    x = F.conv1d(F.pad(mix.unsqueeze(1), (L, 2 * L)), sd["encoder.sequential.0.weight"], sd["encoder.sequential.0.bias"],
                 stride=L)
    for j, d in enumerate(ENC_DIL):
        i = 1 + 2 * j
        z = F.conv1d(x, sd[f"encoder.sequential.{i}.weight"], sd[f"encoder.sequential.{i}.bias"], padding=d, dilation=d)
        if taps is not None:
            taps["ez"].append(z.detach())
        x = _prelu(z, sd[f"encoder.sequential.{i + 1}.weight"], mk("ez", j))
    enc = x
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
    for j, d in enumerate(DEC_DIL):
        i = 2 * j
        z = F.conv_transpose1d(y, sd[f"decoder.sequential.{i}.weight"], sd[f"decoder.sequential.{i}.bias"], padding=d, dilation=d)
        if taps is not None:
            taps["dz"].append(z.detach())
        y = _prelu(z, sd[f"decoder.sequential.{i + 1}.weight"], mk("dz", j))
    y = F.conv_transpose1d(y, sd["decoder.sequential.8.weight"], sd["decoder.sequential.8.bias"], stride=L)
    y = y[:, :, L:y.shape[2] - 2 * L].reshape(bs, 2, -1)
    return {"s1_pred": y[:, 0], "s2_pred": y[:, 1]}


def grads(sd: Dict[str, torch.Tensor], mix: torch.Tensor, d1: torch.Tensor, d2: torch.Tensor, dtype=torch.float64,
          masks: Optional[dict] = None) -> Dict[str, torch.Tensor]:
    """Vector-Jacobian product of the restatement in `dtype`: {key: d <out, (d1, d2)> / d key} (masks: see forward).  Zero
    where autograd returns None: the last block's residual conv and decoder.deconv.weight feed nothing."""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    out = forward(p, mix.to(dtype), masks)
    g = torch.autograd.grad([out["s1_pred"], out["s2_pred"]], list(p.values()), [d1.to(dtype), d2.to(dtype)],
                            allow_unused=True)
    return {k: torch.zeros_like(v) if gk is None else gk for (k, v), gk in zip(p.items(), g)}


def _tape(eng, B: int, T: int, f) -> dict:
    tape = (eng._tape_id, B, T, eng._ws.data_ptr())
    Fr = eng.frames(T)
    lay = lambda t: f(t).view(B, Fr, t.shape[1]).permute(0, 2, 1).clone()
    # decoder rows are (b, f, speaker): -> batch (b, speaker), as the restatement's reshape(-1, N, F)
    lay2 = lambda t: f(t).view(B, Fr, 2, t.shape[1]).permute(0, 2, 3, 1).reshape(2 * B, t.shape[1], Fr).clone()
    return {"v1": [lay(eng.tape_tensor(tape, eng.TAPE_V1, i)) for i in range(P * X)],
            "u": [lay(eng.tape_tensor(tape, eng.TAPE_U, i)) for i in range(P * X)],
            "skip": lay(eng.tape_tensor(tape, eng.TAPE_SKIP)),
            "ez": [lay(eng.tape_tensor(tape, eng.TAPE_ENC_Z, i)) for i in range(4)],
            "dz": [lay2(eng.tape_tensor(tape, eng.TAPE_DEC_Z, i)) for i in range(4)]}


def tape_tensors(eng, B: int, T: int) -> dict:
    """The pre-activations on the tape of the forward `eng` (speech_separation_amd.DeepConvTasNetTrainEngine) just ran for
    B x T (dcttrain_tape_offset), copied to the layout of forward's `taps`."""
    return _tape(eng, B, T, lambda t: t)


def prelu_masks(eng, B: int, T: int) -> dict:
    """The PReLU branch (input > 0) of every element in the forward `eng` just ran for B x T, read from its tape, in the
    layout of forward's `masks`."""
    return _tape(eng, B, T, lambda t: t > 0)
