"""TEST INFRASTRUCTURE (not product code): the reference's DeepAVConvTasNet forward composed from stock PyTorch operators in
a form autograd can differentiate: tests/deepconvtasnet_train_ref.forward plus the video head of
tests/deepconvtasnet_ref.forward (which is the same computation under torch.no_grad()).  The gradients of
TrainableDeepAVConvTasNet are compared with fp64 autograd through this restatement;
tests/golden/deepavconvtasnet_grad_slopes.npz (the reference's own DeepAVConvTasNet and SiSNRWavLoss, loss.backward() on the
CPU) pins the restatement itself.

Follows src/model/deepavconvtasnet.py: Encoder :7-26, video head :140-153 (Linear(512 -> 256) per speaker, concat, linear
interpolation to F frames, LayerNorm(512), added to the encoder output), Separator (Conv-TasNet's; its input and the tensor
the masks multiply are both the fused one, :153-155), Decoder :96-120; decoder.deconv.weight is a parameter the forward
never reads.  The embeddings are inputs without a gradient.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle.convtasnet_stock import H, L, N, P, R, X
from tests.convtasnet_train_ref import _prelu
from tests.deepconvtasnet_ref import DEC_DIL, ENC_DIL, synthetic_deepconvtasnet_weights
from tests.deepconvtasnet_train_ref import UNUSED, _tape as _audio_tape  # noqa: F401  (UNUSED: re-export)

VIDEO = ("visual_compression.weight", "visual_compression.bias", "video_ln.weight", "video_ln.bias")


def synthetic_weights(seed: int = 0, slopes: str = "distinct", ln_seed: int = 1234) -> Dict[str, np.ndarray]:
    """synthetic_deepconvtasnet_weights(True, seed, slopes) with a video LayerNorm far from the identity: weight 1 + 0.3 N(0, 1),
    bias 0.3 N(0, 1) (numpy PCG64 of `ln_seed`).  Near gamma = 1, beta = 0 a backward that forgets gamma passes."""
    sd = synthetic_deepconvtasnet_weights(True, seed, slopes=slopes)
    rng = np.random.default_rng(ln_seed)
    sd["video_ln.weight"] = (1.0 + 0.3 * rng.standard_normal(N)).astype(np.float32)
    sd["video_ln.bias"] = (0.3 * rng.standard_normal(N)).astype(np.float32)
    return sd


def synthetic_embeddings(B: int, Tv: int, seed: int = 0):
    """(s1_embedding, s2_embedding) [B][512][Tv] fp32, N(0, 1) (numpy PCG64)."""
    rng = np.random.default_rng(1000 + seed)
    return tuple(rng.standard_normal((B, N, Tv)).astype(np.float32) for _ in range(2))


def forward(sd: Dict[str, torch.Tensor], mix: torch.Tensor, s1_embedding: torch.Tensor, s2_embedding: torch.Tensor,
            masks: Optional[dict] = None, taps: Optional[dict] = None) -> Dict[str, torch.Tensor]:
    """mix [B][T], embeddings [B][512][Tv] -> {"s1_pred", "s2_pred"} [B][16 (T // 16)], differentiable in every tensor of
    `sd` it reads.  masks / taps: the protocol of tests/deepconvtasnet_train_ref.forward; taps also receives "vcat"
    [B][Tv][512], the two speakers' compressed embeddings side by side before the interpolation."""
    if taps is not None:
        taps.update(v1=[], u=[], skip=None, ez=[], dz=[], vcat=None)
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
    v = torch.cat([F.linear(e.permute(0, 2, 1), sd["visual_compression.weight"], sd["visual_compression.bias"])
                   for e in (s1_embedding, s2_embedding)], -1)
    if taps is not None:
        taps["vcat"] = v.detach()
    v = F.interpolate(v.permute(0, 2, 1), size=x.shape[-1], mode="linear", align_corners=False).permute(0, 2, 1)
    enc = x + F.layer_norm(v, (N,), sd["video_ln.weight"], sd["video_ln.bias"]).permute(0, 2, 1)
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


def grads(sd: Dict[str, torch.Tensor], mix: torch.Tensor, s1_embedding: torch.Tensor, s2_embedding: torch.Tensor,
          d1: torch.Tensor, d2: torch.Tensor, dtype=torch.float64, masks: Optional[dict] = None) -> Dict[str, torch.Tensor]:
    """Vector-Jacobian product of the restatement in `dtype`: {key: d <out, (d1, d2)> / d key} (masks: see forward).  Zero
    where autograd returns None: the last block's residual conv and decoder.deconv.weight feed nothing."""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    out = forward(p, mix.to(dtype), s1_embedding.to(dtype), s2_embedding.to(dtype), masks)
    g = torch.autograd.grad([out["s1_pred"], out["s2_pred"]], list(p.values()), [d1.to(dtype), d2.to(dtype)],
                            allow_unused=True)
    return {k: torch.zeros_like(v) if gk is None else gk for (k, v), gk in zip(p.items(), g)}


def _vcat(eng, B: int, T: int, Tv: int) -> torch.Tensor:
    tape = (eng._tape_id, B, T, eng._ws.data_ptr(), Tv)
    return eng.tape_tensor(tape, eng.TAPE_VCAT).view(B, Tv, N).clone()


class _WithTv:
    """`eng` as tests/deepconvtasnet_train_ref._tape sees it: its 4-field tape identities get the Tv of this forward"""

    def __init__(self, eng, Tv):
        self._eng, self._Tv = eng, Tv

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def tape_tensor(self, tape, which, block=0):
        return self._eng.tape_tensor((*tape, self._Tv), which, block)


def tape_tensors(eng, B: int, T: int, Tv: int) -> dict:
    """The tensors on the tape of the forward `eng` (speech_separation_amd.DeepAVConvTasNetTrainEngine) just ran for
    B x T x Tv (davtrain_tape_offset), copied to the layout of forward's `taps`."""
    return dict(_audio_tape(_WithTv(eng, Tv), B, T, lambda t: t), vcat=_vcat(eng, B, T, Tv))


def prelu_masks(eng, B: int, T: int, Tv: int) -> dict:
    """The PReLU branch (input > 0) of every element in the forward `eng` just ran for B x T x Tv, read from its tape, in
    the layout of forward's `masks`."""
    return _audio_tape(_WithTv(eng, Tv), B, T, lambda t: t > 0)
