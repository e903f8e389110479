"""The ShuffleNet-v2 lip reader (src/lipreader/lipreading/model.py:141-273 with backbone_type="shufflenet" and
extract_feats=True: 24-channel Conv3d stem + ShuffleNetV2.features + conv_last + AvgPool2d(3); models/shufflenetv2.py)
restated on stock PyTorch CPU operators, and the seeded weights the tests and tools/gen_golden_shufflenet.py share.

shufflenet_state_dict_spec(relu_type, width_mult) -> [(key, shape, kind)] in the reference's state_dict() order without tcn.*
synthetic_shufflenet_weights(relu_type, width_mult, seed) -> {key: numpy array}
run(weights, x, dtype, window=None, affine=None, relu_type=None, width_mult=None) -> (S, T, 1024) tensor of `dtype`
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from tests.lipreader_ref import (BN_EPS, INPUT_SEED, PREPROC_CROP, PREPROC_MEAN, PREPROC_SHAPE, PREPROC_STD,  # noqa: F401
                                 WEIGHT_SEED, preproc_window_affine, synthetic_clip, synthetic_video, weights_digest)

STAGES = {0.5: (48, 96, 192), 1.0: (116, 232, 464)}
REPEATS = (4, 8, 4)
STEM, EMBED = 24, 1024
MIN_HW, MAX_HW = 65, 160
# (relu_type, width_mult, input shape) of tests/golden/lipreader_shufflenet.npz
GOLDEN_CASES = (("prelu", 1.0, (2, 1, 3, 88, 88)), ("prelu", 1.0, (1, 1, 2, 97, 66)), ("prelu", 0.5, (1, 1, 2, 65, 72)))


def _conv_bn(prefix, i, shape, kind="conv"):
    """Conv `prefix`i.weight followed by the BatchNorm `prefix`(i + 1).*"""
    q = f"{prefix}{i + 1}."
    c = (shape[0],)
    return [(f"{prefix}{i}.weight", shape, kind), (q + "weight", c, "bn_w"), (q + "bias", c, "bn_b"),
            (q + "running_mean", c, "bn_m"), (q + "running_var", c, "bn_v"), (q + "num_batches_tracked", (), "nbt")]


def shufflenet_state_dict_spec(relu_type: str = "prelu", width_mult: float = 1.0):
    """kind: "conv" / "dw" (depthwise 3 x 3) / "bn_w" / "bn_b" / "bn_m" / "bn_v" / "nbt" / "slope"."""
    spec, inp, bi = [], STEM, 0
    for width, repeats in zip(STAGES[width_mult], REPEATS):
        ch = width // 2
        for r in range(repeats):
            p = f"trunk.0.{bi}."
            if r == 0:
                spec += _conv_bn(p + "banch1.", 0, (inp, 1, 3, 3), "dw") + _conv_bn(p + "banch1.", 2, (ch, inp, 1, 1))
            spec += _conv_bn(p + "banch2.", 0, (ch, inp if r == 0 else ch, 1, 1))
            spec += _conv_bn(p + "banch2.", 3, (ch, 1, 3, 3), "dw") + _conv_bn(p + "banch2.", 5, (ch, ch, 1, 1))
            inp = width
            bi += 1
    spec += _conv_bn("trunk.1.", 0, (EMBED, inp, 1, 1))
    spec += _conv_bn("frontend3D.", 0, (STEM, 1, 5, 7, 7))
    if relu_type == "prelu":
        spec.append(("frontend3D.2.weight", (STEM,), "slope"))
    return spec


def synthetic_shufflenet_weights(relu_type: str = "prelu", width_mult: float = 1.0, seed: int = 0):
    """Seeded, non-degenerate weights (numpy PCG64), as lipreader_ref.synthetic_lipreader_weights: conv N(0, 2/fan_in) (a
    depthwise filter's fan_in is 9), BN weight and running_var U(0.5, 1.5), BN bias and running_mean N(0, 0.2^2), 24 distinct
    stem slopes in (-0.1, 0.4)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = {}
    for key, shape, kind in shufflenet_state_dict_spec(relu_type, width_mult):
        if kind in ("conv", "dw"):
            v = rng.standard_normal(shape) * np.sqrt(2.0 / int(np.prod(shape[1:])))
        elif kind in ("bn_w", "bn_v"):
            v = rng.uniform(0.5, 1.5, shape)
        elif kind in ("bn_b", "bn_m"):
            v = rng.standard_normal(shape) * 0.2
        elif kind == "slope":
            v = rng.permutation(np.linspace(-0.1, 0.4, shape[0] + 2)[1:-1])
        else:
            sd[key] = np.array(0, dtype=np.int64)
            continue
        sd[key] = np.ascontiguousarray(v, dtype=np.float32)
    return sd


def width_of(weights) -> float:
    return {v[0] // 2: k for k, v in STAGES.items()}[int(tuple(weights["trunk.0.0.banch2.0.weight"].shape)[0])]


def out_hw(H: int, W: int):
    """Spatial sizes after the stem conv, the max-pool and each of the three stride-2 stages: h -> ceil(h / 2) five times."""
    sizes = [((H - 1) // 2 + 1, (W - 1) // 2 + 1)]
    for _ in range(4):
        h, w = sizes[-1]
        sizes.append(((h - 1) // 2 + 1, (w - 1) // 2 + 1))
    return sizes


def flops_per_stream(width_mult: float, T: int, H: int, W: int) -> float:
    """2 x multiply-accumulates of the convolutions of one stream (padding taps counted; conv_last on the whole final map)."""
    sizes = out_hw(H, W)
    macs = sizes[0][0] * sizes[0][1] * STEM * 245
    inp = STEM
    for s, width in enumerate(STAGES[width_mult]):
        ch = width // 2
        pin, pout = sizes[s + 1][0] * sizes[s + 1][1], sizes[s + 2][0] * sizes[s + 2][1]
        macs += pout * inp * 9 + pout * inp * ch
        macs += pin * inp * ch + pout * ch * 9 + pout * ch * ch
        macs += (REPEATS[s] - 1) * pout * (2 * ch * ch + 9 * ch)
        inp = width
    macs += sizes[4][0] * sizes[4][1] * inp * EMBED
    return 2.0 * T * macs


def _act(x, relu_type, slope):
    if relu_type == "relu":
        return F.relu(x)
    if relu_type == "prelu":
        return F.prelu(x, slope)
    return x * torch.sigmoid(x)


def _shuffle(x):
    n, c, h, w = x.shape
    return x.view(n, 2, c // 2, h, w).transpose(1, 2).reshape(n, c, h, w)


def run(weights, x, dtype=torch.float64, window=None, affine=None, relu_type=None, width_mult=None):
    """weights: {key: array}; x: (S, 1, T, H, W), or with `window` = (y0, x0, H, W) a larger frame (S, 1, T, Hin, Win) of
    which the window is taken; affine = (a, b): a * x + b before the stem (padding stays zero after it).  relu_type: None
    reads it off the weights (prelu if they hold slopes, else swish); "relu" has to be named.  width_mult: the weights' shapes carry
    it; a value given is checked against them."""
    def tensor(v):
        return (v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))).to(dtype)

    w = {k: tensor(v) for k, v in weights.items() if not k.endswith("num_batches_tracked")}
    if relu_type is None:
        relu_type = "prelu" if "frontend3D.2.weight" in w else "swish"
    if width_mult is not None and width_mult != width_of(weights):
        raise ValueError(f"width_mult={width_mult} but the weights are those of width {width_of(weights)}")
    x = tensor(x)
    if window is not None:
        y0, x0, H, W = window
        x = x[..., y0:y0 + H, x0:x0 + W]
    if affine is not None:
        x = x * affine[0] + affine[1]

    def bn(v, p):
        return F.batch_norm(v, w[p + "running_mean"], w[p + "running_var"], w[p + "weight"], w[p + "bias"], False, 0.0, BN_EPS)

    def pw(v, p, i):
        return F.relu(bn(F.conv2d(v, w[f"{p}{i}.weight"]), f"{p}{i + 1}."))

    def dw(v, p, i, stride):
        return bn(F.conv2d(v, w[f"{p}{i}.weight"], None, stride, 1, 1, v.shape[1]), f"{p}{i + 1}.")

    S, _, T = x.shape[:3]
    v = F.conv3d(x, w["frontend3D.0.weight"], None, (1, 2, 2), (2, 3, 3))
    v = _act(bn(v, "frontend3D.1."), relu_type, w.get("frontend3D.2.weight"))
    v = F.max_pool3d(v, (1, 3, 3), (1, 2, 2), (0, 1, 1))
    v = v.transpose(1, 2).reshape(S * T, STEM, v.shape[3], v.shape[4])
    bi = 0
    for repeats in REPEATS:
        for r in range(repeats):
            p = f"trunk.0.{bi}."
            if r == 0:
                a = pw(dw(v, p + "banch1.", 0, 2), p + "banch1.", 2)
                b = pw(dw(pw(v, p + "banch2.", 0), p + "banch2.", 3, 2), p + "banch2.", 5)
            else:
                half = v.shape[1] // 2
                a = v[:, :half]
                b = pw(dw(pw(v[:, half:], p + "banch2.", 0), p + "banch2.", 3, 1), p + "banch2.", 5)
            v = _shuffle(torch.cat((a, b), 1))
            bi += 1
    v = pw(v, "trunk.1.", 0)
    v = F.avg_pool2d(v, 3)
    if v.shape[2:] != (1, 1):
        raise ValueError(f"AvgPool2d(3) leaves {tuple(v.shape[2:])} positions: frames must be {MIN_HW} .. {MAX_HW} a side")
    return v.reshape(S, T, EMBED)


def row_rel(got, ref64):
    """Per (stream, frame) row: ||got - ref||_2 / ||ref||_2, in fp64."""
    got = torch.as_tensor(got).double().reshape(-1, EMBED)
    ref = torch.as_tensor(ref64).double().reshape(-1, EMBED)
    return ((got - ref).norm(dim=1) / ref.norm(dim=1)).numpy()
