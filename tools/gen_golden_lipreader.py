#!/usr/bin/env python3
"""Generate tests/golden/lipreader_swish.npz, lipreader_prelu.npz and lipreader_preproc.npz by RUNNING the reference's
Lipreading(extract_feats=True) on CPU in fp64 (src/lipreader/lipreading/model.py:141-273, built as init_lipreader does from
src/lipreader/configs/lrw_resnet18_mstcn.json).  Runs only where the reference is present; the fixtures are what the tests
read.

Weights and inputs are not stored: both sides regenerate them (tests/lipreader_ref.synthetic_lipreader_weights /
synthetic_video / synthetic_clip; numpy PCG64), and a sha256 of the weight bytes detects a drift.  The seeded weights are
loaded with strict=False (the TCN back end keeps its random initialisation and is never executed).

lipreader_preproc.npz: a (3, 97, 96) uint8-valued clip through the reference's test-time pipeline Normalize(0, 255),
CenterCrop((88, 88)), Normalize(0.421, 0.165) (dataloaders.py:25-27, preprocess.py:62-103) and the swish model.  The two
classes are imported from the reference when its preprocess module imports (it needs cv2), and restated here otherwise.

Usage:  python tools/gen_golden_lipreader.py
"""
from __future__ import annotations

import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import lipreader_ref as R  # noqa: E402
from tools.gen_golden import OUT, REF, import_reference  # noqa: E402


def reference_model(relu_type):
    model_mod = importlib.import_module("src.lipreader.lipreading.model")
    with open(f"{REF}/src/lipreader/configs/lrw_resnet18_mstcn.json") as f:
        args = json.load(f)
    tcn_options = {"num_layers": args["tcn_num_layers"], "kernel_size": args["tcn_kernel_size"],
                   "dropout": args["tcn_dropout"], "dwpw": args["tcn_dwpw"], "width_mult": args["tcn_width_mult"]}
    model = model_mod.Lipreading(modality="video", num_classes=500, tcn_options=tcn_options, densetcn_options={},
                                 backbone_type=args["backbone_type"], relu_type=relu_type, width_mult=args["width_mult"],
                                 use_boundary=False, extract_feats=True)
    ref = [(k, tuple(v.shape)) for k, v in model.state_dict().items() if not k.startswith("tcn.")]
    spec = [(k, s) for k, s, _ in R.lipreader_state_dict_spec(relu_type)]
    assert ref == spec, f"Lipreading({relu_type}) state_dict drifted from the spec"
    sd = R.synthetic_lipreader_weights(relu_type, seed=R.WEIGHT_SEED)
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.startswith("tcn.") for k in missing), (missing, unexpected)
    return model.double().eval(), sd, [k for k, _ in ref]


def preprocess_classes():
    try:
        pre = importlib.import_module("src.lipreader.lipreading.preprocess")
        return pre.Normalize, pre.CenterCrop, "reference"
    except ImportError:
        class Normalize:
            def __init__(self, mean, std):
                self.mean, self.std = mean, std

            def __call__(self, frames):
                return (frames - self.mean) / self.std

        class CenterCrop:
            def __init__(self, size):
                self.size = size

            def __call__(self, frames):
                _, h, w = frames.shape
                th, tw = self.size
                dh, dw = int((h - th) / 2.0), int((w - tw) / 2.0)
                return frames[:, dh:dh + th, dw:dw + tw]

        return Normalize, CenterCrop, "restated"


def main():
    torch.set_num_threads(8)
    import_reference()
    for relu_type in ("swish", "prelu"):
        model, sd, keys = reference_model(relu_type)
        outs = {}
        for i, shape in enumerate(R.GOLDEN_SHAPES):
            x = torch.from_numpy(R.synthetic_video(shape, seed=R.INPUT_SEED + i)).double()
            with torch.no_grad():
                y = model(x, lengths=[shape[2]] * shape[0])
            outs[f"out{i}"] = y.numpy()
            outs[f"shape{i}"] = np.array(shape)
            print(relu_type, shape, "->", tuple(y.shape), "rms", float(y.pow(2).mean().sqrt()))
        np.savez_compressed(os.path.join(OUT, f"lipreader_{relu_type}.npz"), digest=np.array(R.weights_digest(sd)),
                            seeds=np.array([R.WEIGHT_SEED, R.INPUT_SEED]), keys=np.array(keys), **outs)
        if relu_type == "swish":
            Normalize, CenterCrop, origin = preprocess_classes()
            clip = R.synthetic_clip(R.PREPROC_SHAPE, seed=R.INPUT_SEED).astype(np.float64)
            for t in (Normalize(0.0, 255.0), CenterCrop(R.PREPROC_CROP), Normalize(R.PREPROC_MEAN, R.PREPROC_STD)):
                clip = t(clip)
            with torch.no_grad():
                y = model(torch.from_numpy(np.ascontiguousarray(clip))[None, None], lengths=[clip.shape[0]])
            np.savez_compressed(os.path.join(OUT, "lipreader_preproc.npz"), digest=np.array(R.weights_digest(sd)),
                                seeds=np.array([R.WEIGHT_SEED, R.INPUT_SEED]), clip_shape=np.array(R.PREPROC_SHAPE),
                                crop=np.array(R.PREPROC_CROP), mean_std=np.array([R.PREPROC_MEAN, R.PREPROC_STD]),
                                classes=np.array(origin), out=y.numpy())
            print("preproc", origin, tuple(y.shape), "rms", float(y.pow(2).mean().sqrt()))


if __name__ == "__main__":
    main()
