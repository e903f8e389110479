#!/usr/bin/env python3
"""Generate tests/golden/lipreader_shufflenet.npz by RUNNING the reference's Lipreading(backbone_type="shufflenet",
extract_feats=True) on CPU in fp64 (src/lipreader/lipreading/model.py:141-273, models/shufflenetv2.py), built as
init_lipreader does from src/lipreader/configs/lrw_snv1x_tcn1x.json (width_mult 1.0) and lrw_snv05x_tcn1x.json (0.5).  Runs
only where the reference is present; the fixture is what the tests read.

Weights and inputs are not stored: both sides regenerate them (tests/shufflenet_ref.synthetic_shufflenet_weights,
tests/lipreader_ref.synthetic_video; numpy PCG64), and a sha256 of the weight bytes detects a drift.  The seeded weights are
loaded with strict=False (the TCN back end keeps its random initialisation and is never executed).

Contents: keys_<width> (the state_dict key list without tcn.*, for prelu), digest_<width>, and out<i> / shape<i> / width<i>
for the cases of shufflenet_ref.GOLDEN_CASES: final maps 3 x 3, 4 x 3 (the pool ignores row 3) and odd maps at every level.

Usage:  python tools/gen_golden_shufflenet.py
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
from tests import shufflenet_ref as R  # noqa: E402
from tools.gen_golden import OUT, REF, import_reference  # noqa: E402

CONFIGS = {1.0: "lrw_snv1x_tcn1x.json", 0.5: "lrw_snv05x_tcn1x.json"}


def tag(width_mult):
    return "w10" if width_mult == 1.0 else "w05"


def reference_model(relu_type, width_mult):
    model_mod = importlib.import_module("src.lipreader.lipreading.model")
    with open(f"{REF}/src/lipreader/configs/{CONFIGS[width_mult]}") as f:
        args = json.load(f)
    assert args["backbone_type"] == "shufflenet" and args["width_mult"] == width_mult and args["relu_type"] == relu_type
    tcn_options = {"num_layers": args["tcn_num_layers"], "kernel_size": args["tcn_kernel_size"],
                   "dropout": args["tcn_dropout"], "dwpw": args["tcn_dwpw"], "width_mult": args["tcn_width_mult"]}
    model = model_mod.Lipreading(modality="video", num_classes=500, tcn_options=tcn_options, densetcn_options={},
                                 backbone_type=args["backbone_type"], relu_type=relu_type, width_mult=args["width_mult"],
                                 use_boundary=False, extract_feats=True)
    ref = [(k, tuple(v.shape)) for k, v in model.state_dict().items() if not k.startswith("tcn.")]
    spec = [(k, s) for k, s, _ in R.shufflenet_state_dict_spec(relu_type, width_mult)]
    assert ref == spec, f"Lipreading(shufflenet, {relu_type}, {width_mult}) state_dict drifted from the spec"
    sd = R.synthetic_shufflenet_weights(relu_type, width_mult, seed=R.WEIGHT_SEED)
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.startswith("tcn.") for k in missing), (missing, unexpected)
    return model.double().eval(), sd, [k for k, _ in ref]


def main():
    torch.set_num_threads(8)
    import_reference()
    models, fixture = {}, {}
    for i, (relu_type, width_mult, shape) in enumerate(R.GOLDEN_CASES):
        if (relu_type, width_mult) not in models:
            models[(relu_type, width_mult)] = reference_model(relu_type, width_mult)
            _, sd, keys = models[(relu_type, width_mult)]
            fixture[f"keys_{tag(width_mult)}"] = np.array(keys)
            fixture[f"digest_{tag(width_mult)}"] = np.array(R.weights_digest(sd))
        model = models[(relu_type, width_mult)][0]
        x = torch.from_numpy(R.synthetic_video(shape, seed=R.INPUT_SEED + i)).double()
        with torch.no_grad():
            y = model(x, lengths=[shape[2]] * shape[0])
        fixture[f"out{i}"] = y.numpy()
        fixture[f"shape{i}"] = np.array(shape)
        fixture[f"width{i}"] = np.array(width_mult)
        print(relu_type, width_mult, shape, "->", tuple(y.shape), "rms", float(y.pow(2).mean().sqrt()))
    np.savez_compressed(os.path.join(OUT, "lipreader_shufflenet.npz"), seeds=np.array([R.WEIGHT_SEED, R.INPUT_SEED]), **fixture)


if __name__ == "__main__":
    main()
