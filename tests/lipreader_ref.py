"""The lip-reading front end (src/lipreader/lipreading/model.py:141-273 with extract_feats=True: Conv3d stem + ResNet-18
trunk) restated on stock PyTorch CPU operators, and the seeded weights the tests and tools/gen_golden_lipreader.py share.

synthetic_lipreader_weights(relu_type, seed) -> {key: numpy array} in the reference's state_dict() order without tcn.*
run(weights, x, dtype, window=None, affine=None) -> (S, T, 512) tensor of `dtype`
"""
from __future__ import annotations

import hashlib

import numpy as np
import torch
import torch.nn.functional as F

PLANES = (64, 128, 256, 512)
BN_EPS = 1e-5
GOLDEN_SHAPES = ((2, 1, 5, 88, 88), (1, 1, 3, 33, 47))
WEIGHT_SEED, INPUT_SEED = 0, 31
PREPROC_SHAPE, PREPROC_CROP, PREPROC_MEAN, PREPROC_STD = (3, 97, 96), (88, 88), 0.421, 0.165


def _bn_keys(prefix):
    return [(prefix + "weight", "bn_w"), (prefix + "bias", "bn_b"), (prefix + "running_mean", "bn_m"),
            (prefix + "running_var", "bn_v"), (prefix + "num_batches_tracked", "nbt")]


def lipreader_state_dict_spec(relu_type: str):
    """[(key, shape, kind)] in the reference's state_dict() order (the trunk is registered before the stem)."""
    spec = []
    inp = 64
    for li, planes in enumerate(PLANES):
        for b in range(2):
            p = f"trunk.layer{li + 1}.{b}."
            cin = inp if b == 0 else planes
            spec.append((p + "conv1.weight", (planes, cin, 3, 3), "conv"))
            spec += [(k, () if kind == "nbt" else (planes,), kind) for k, kind in _bn_keys(p + "bn1.")]
            if relu_type == "prelu":
                spec.append((p + "relu1.weight", (planes,), "slope"))
                spec.append((p + "relu2.weight", (planes,), "slope"))
            spec.append((p + "conv2.weight", (planes, planes, 3, 3), "conv"))
            spec += [(k, () if kind == "nbt" else (planes,), kind) for k, kind in _bn_keys(p + "bn2.")]
            if b == 0 and li > 0:
                spec.append((p + "downsample.0.weight", (planes, cin, 1, 1), "conv"))
                spec += [(k, () if kind == "nbt" else (planes,), kind) for k, kind in _bn_keys(p + "downsample.1.")]
        inp = planes
    spec.append(("frontend3D.0.weight", (64, 1, 5, 7, 7), "conv"))
    spec += [(k, () if kind == "nbt" else (64,), kind) for k, kind in _bn_keys("frontend3D.1.")]
    if relu_type == "prelu":
        spec.append(("frontend3D.2.weight", (64,), "slope"))
    return spec


def synthetic_lipreader_weights(relu_type: str = "swish", seed: int = 0):
    """Seeded, non-degenerate weights (numpy PCG64): conv N(0, 2/fan_in), BN weight and running_var U(0.5, 1.5), BN bias and
    running_mean N(0, 0.2^2), distinct PReLU slopes in (-0.1, 0.4)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = {}
    for key, shape, kind in lipreader_state_dict_spec(relu_type):
        if kind == "conv":
            fan_in = int(np.prod(shape[1:]))
            v = rng.standard_normal(shape) * np.sqrt(2.0 / fan_in)
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


def synthetic_video(shape, seed: int = INPUT_SEED):
    """Normalised-domain mouth crops: N(0, 1) float32 of `shape`."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.standard_normal(shape).astype(np.float32)


def synthetic_clip(shape=PREPROC_SHAPE, seed: int = INPUT_SEED):
    """A uint8-valued grey clip (T, Hin, Win) as float32, as the reference's mouth .npz files hold."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.integers(0, 256, shape).astype(np.float32)


def weights_digest(sd) -> str:
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def out_hw(H: int, W: int):
    """Spatial sizes after the stem conv, the max-pool and each of the three stride-2 stages."""
    sizes = [((H - 1) // 2 + 1, (W - 1) // 2 + 1)]
    for _ in range(4):
        h, w = sizes[-1]
        sizes.append(((h - 1) // 2 + 1, (w - 1) // 2 + 1))
    return sizes


def flops_per_stream(T: int, H: int, W: int) -> float:
    """2 x multiply-accumulates of the convolutions of one stream (padding taps counted, as the usual profilers do)."""
    (hs, ws), (h, w) = out_hw(H, W)[:2]
    macs = hs * ws * 64 * 245
    inp = 64
    for li, planes in enumerate(PLANES):
        if li > 0:
            h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            macs += h * w * planes * inp
        macs += h * w * planes * 9 * (inp + 3 * planes)
        inp = planes
    return 2.0 * T * macs


def _act(x, relu_type, slope):
    if relu_type == "relu":
        return F.relu(x)
    if relu_type == "prelu":
        return F.prelu(x, slope)
    return x * torch.sigmoid(x)


def run(weights, x, dtype=torch.float64, window=None, affine=None, relu_type=None):
    """weights: {key: array}; x: (S, 1, T, H, W), or with `window` = (y0, x0, H, W) a larger frame (S, 1, T, Hin, Win) of
    which the window is taken; affine = (a, b): a * x + b before the stem (padding stays zero after it).  relu_type: None
    reads it off the weights (prelu if they hold slopes, else swish); "relu" has to be named."""
    def tensor(v):
        return (v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))).to(dtype)

    w = {k: tensor(v) for k, v in weights.items() if not k.endswith("num_batches_tracked")}
    if relu_type is None:
        relu_type = "prelu" if "frontend3D.2.weight" in w else "swish"
    x = tensor(x)
    if window is not None:
        y0, x0, H, W = window
        x = x[..., y0:y0 + H, x0:x0 + W]
    if affine is not None:
        x = x * affine[0] + affine[1]

    def bn(v, p):
        return F.batch_norm(v, w[p + "running_mean"], w[p + "running_var"], w[p + "weight"], w[p + "bias"], False, 0.0, BN_EPS)

    S, _, T = x.shape[:3]
    v = F.conv3d(x, w["frontend3D.0.weight"], None, (1, 2, 2), (2, 3, 3))
    v = _act(bn(v, "frontend3D.1."), relu_type, w.get("frontend3D.2.weight"))
    v = F.max_pool3d(v, (1, 3, 3), (1, 2, 2), (0, 1, 1))
    v = v.transpose(1, 2).reshape(S * T, 64, v.shape[3], v.shape[4])
    for li in range(4):
        for b in range(2):
            p = f"trunk.layer{li + 1}.{b}."
            stride = 2 if (b == 0 and li > 0) else 1
            res = v
            o = F.conv2d(v, w[p + "conv1.weight"], None, stride, 1)
            o = _act(bn(o, p + "bn1."), relu_type, w.get(p + "relu1.weight"))
            o = bn(F.conv2d(o, w[p + "conv2.weight"], None, 1, 1), p + "bn2.")
            if stride == 2:
                res = bn(F.conv2d(v, w[p + "downsample.0.weight"], None, 2, 0), p + "downsample.1.")
            v = _act(o + res, relu_type, w.get(p + "relu2.weight"))
    return v.mean(dim=(2, 3)).reshape(S, T, 512)


def row_rel(got, ref64):
    """Per (stream, frame) row: ||got - ref||_2 / ||ref||_2, in fp64."""
    got = torch.as_tensor(got).double().reshape(-1, 512)
    ref = torch.as_tensor(ref64).double().reshape(-1, 512)
    return ((got - ref).norm(dim=1) / ref.norm(dim=1)).numpy()


def preproc_window_affine(shape=PREPROC_SHAPE, crop=PREPROC_CROP, mean=PREPROC_MEAN, std=PREPROC_STD):
    """The reference's test-time pipeline x / 255 -> CenterCrop(crop) -> (x - mean) / std as ((y0, x0, H, W), (a, b))."""
    _, h, w = shape
    return ((h - crop[0]) // 2, (w - crop[1]) // 2, crop[0], crop[1]), (1.0 / (255.0 * std), -mean / std)
