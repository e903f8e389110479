"""TEST INFRASTRUCTURE (not product code): the reference's DeepConvTasNet and DeepAVConvTasNet composed from stock PyTorch
operators, functional style, plus their seeded synthetic weights.  Pinned to the reference's own outputs by
tests/test_deepconvtasnet_host.py (tests/golden/deepconvtasnet.npz, deepavconvtasnet.npz).

Follows src/model/deepavconvtasnet.py: Encoder :7-26 (pad (16, 32), Conv1d(1, 512, 32, stride 16) WITH bias, then
4 x [Conv1d(512, 512, 3, dilation d, padding d), PReLU] for d = 1, 2, 4, 8), the Separator of ConvTasNet :66-94 (masks
multiply its input), Decoder :96-120 (4 x [ConvTranspose1d(512, 512, 3, dilation d, padding d), PReLU] for d = 8, 4, 2, 1,
then ConvTranspose1d(512, 1, 32, stride 16) + bias, cropped [16, len - 32); decoder.deconv is never used), and the video head
:140-153 (Linear(512 -> 256) per speaker, concat, linear interpolation to F frames, LayerNorm(512), added to the encoder
output).
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle.convtasnet_stock import B as CB, H, L, N, P, R, X, distinct_slopes
from speech_separation_amd.spec import deepconvtasnet_state_dict_spec

ENC_DIL = (1, 2, 4, 8)
DEC_DIL = (8, 4, 2, 1)


def frames(T: int) -> int:
    return (T + L) // L + 1


def _is_prelu(k: str, shape) -> bool:
    return (k.startswith(("encoder.sequential.", "decoder.sequential.")) and shape == (1,)
            and not k.startswith("decoder.sequential.8")) or k.endswith(("PReLU_1.weight", "PReLU_2.weight", "seq.0.weight"))


def synthetic_deepconvtasnet_weights(av: bool = False, seed: int = 0, slopes: str = "0.25") -> Dict[str, np.ndarray]:
    """Deterministic weights (numpy PCG64): PReLU 0.25, norm gains 1 + 0.1 N(0, 1), norm shifts 0.05 N(0, 1), every other
    tensor U(+-1/sqrt(fan_in)) with fan_in = prod(shape[1:]) (512 for biases).  slopes="distinct": every PReLU (deep encoder,
    Separator, deep decoder) gets its own slope (oracle.convtasnet_stock.distinct_slopes); the other tensors do not move."""
    assert slopes in ("0.25", "distinct"), slopes
    rng = np.random.default_rng(seed)
    spec = deepconvtasnet_state_dict_spec(av)
    drawn = distinct_slopes([k for k, shape in spec if _is_prelu(k, shape)], seed) if slopes == "distinct" else {}
    sd = {}
    for k, shape in spec:
        if _is_prelu(k, shape):
            w = np.full(shape, drawn.get(k, 0.25))
        elif k.endswith(("gamma", "norm_1.weight", "norm_2.weight", "video_ln.weight")):
            w = 1.0 + 0.1 * rng.standard_normal(shape)
        elif k.endswith(("beta", "norm_1.bias", "norm_2.bias", "video_ln.bias")):
            w = 0.05 * rng.standard_normal(shape)
        else:
            fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else H
            w = rng.uniform(-1, 1, size=shape) / np.sqrt(max(fan_in, 1))
        sd[k] = np.ascontiguousarray(w, dtype=np.float32)
    return sd


def _separator(sd, x):
    enc = x
    mu = x.mean(dim=(1, 2), keepdim=True)
    var = ((x - mu) ** 2).mean(dim=(1, 2), keepdim=True)
    x = sd["separator.norm_1.gamma"] * (x - mu) / torch.sqrt(var + 5e-6) + sd["separator.norm_1.beta"]
    x = F.conv1d(x, sd["separator.conv1d.weight"], sd["separator.conv1d.bias"])
    acc = 0.0
    for i in range(P * X):
        p, dil = f"separator.separator.{i}.", 2 ** (i % X)
        c = F.conv1d(x, sd[p + "conv1d.weight"], sd[p + "conv1d.bias"])
        c = F.group_norm(F.prelu(c, sd[p + "PReLU_1.weight"]), 1, sd[p + "norm_1.weight"], sd[p + "norm_1.bias"], eps=1e-10)
        c = F.conv1d(c, sd[p + "dconv1d.weight"], sd[p + "dconv1d.bias"], padding=(dil * (R - 1)) // 2, dilation=dil, groups=H)
        c = F.group_norm(F.prelu(c, sd[p + "PReLU_2.weight"]), 1, sd[p + "norm_2.weight"], sd[p + "norm_2.bias"], eps=1e-10)
        x = x + F.conv1d(c, sd[p + "conv.weight"], sd[p + "conv.bias"])
        acc = acc + F.conv1d(c, sd[p + "conv_sc.weight"], sd[p + "conv_sc.bias"])
    m = torch.sigmoid(F.conv1d(F.prelu(acc, sd["separator.seq.0.weight"]), sd["separator.seq.1.weight"], sd["separator.seq.1.bias"]))
    return (enc.unsqueeze(1) * m.reshape(enc.shape[0], 2, N, -1)).reshape(-1, N, enc.shape[-1])


@torch.no_grad()
def forward(sd: Dict[str, torch.Tensor], mix: torch.Tensor, s1_embedding: Optional[torch.Tensor] = None,
            s2_embedding: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """DeepConvTasNet.forward, or DeepAVConvTasNet.forward when the embeddings are given; dtype follows the inputs."""
    bs = mix.shape[0]
    x = F.conv1d(F.pad(mix.unsqueeze(1), (L, 2 * L)), sd["encoder.sequential.0.weight"], sd["encoder.sequential.0.bias"],
                 stride=L)
    for j, d in enumerate(ENC_DIL):
        i = 1 + 2 * j
        x = F.prelu(F.conv1d(x, sd[f"encoder.sequential.{i}.weight"], sd[f"encoder.sequential.{i}.bias"], padding=d, dilation=d),
                    sd[f"encoder.sequential.{i + 1}.weight"])
    if s1_embedding is not None:
        v = torch.cat([F.linear(e.permute(0, 2, 1), sd["visual_compression.weight"], sd["visual_compression.bias"])
                       for e in (s1_embedding, s2_embedding)], -1)
        v = F.interpolate(v.permute(0, 2, 1), size=x.shape[-1], mode="linear", align_corners=False).permute(0, 2, 1)
        x = x + F.layer_norm(v, (N,), sd["video_ln.weight"], sd["video_ln.bias"]).permute(0, 2, 1)
    y = _separator(sd, x)
    for j, d in enumerate(DEC_DIL):
        i = 2 * j
        y = F.prelu(F.conv_transpose1d(y, sd[f"decoder.sequential.{i}.weight"], sd[f"decoder.sequential.{i}.bias"], padding=d,
                                       dilation=d), sd[f"decoder.sequential.{i + 1}.weight"])
    y = F.conv_transpose1d(y, sd["decoder.sequential.8.weight"], sd["decoder.sequential.8.bias"], stride=L)
    y = y[:, :, L:y.shape[2] - 2 * L].reshape(bs, 2, -1)
    return {"s1_pred": y[:, 0], "s2_pred": y[:, 1]}


def run_numpy(sd_np: Dict[str, np.ndarray], mix: np.ndarray, s1_embedding: Optional[np.ndarray] = None,
              s2_embedding: Optional[np.ndarray] = None, dtype=torch.float64) -> Dict[str, np.ndarray]:
    """forward() on numpy inputs in `dtype` (fp64 by default), numpy outputs."""
    t = lambda a: None if a is None else torch.from_numpy(a).to(dtype)  # noqa: E731
    out = forward({k: t(v) for k, v in sd_np.items()}, t(mix), t(s1_embedding), t(s2_embedding))
    return {k: v.numpy() for k, v in out.items()}
