#!/usr/bin/env python3
"""Generate tests/golden/deepconvtasnet.npz and deepavconvtasnet.npz (every PReLU slope 0.25) and deepconvtasnet_slopes.npz and
deepavconvtasnet_slopes.npz (distinct slopes) by RUNNING the reference's DeepConvTasNet and
DeepAVConvTasNet on CPU (src/model/deepconvtasnet.py, deepavconvtasnet.py), imported through the stub packages of
tools/gen_golden.py.  Runs only where the reference is present; the fixtures are what the tests read.

Weights and inputs are not stored: both sides regenerate them (tests/deepconvtasnet_ref.synthetic_deepconvtasnet_weights,
speech_separation_amd.spec.synthetic_inputs; numpy PCG64), and a sha256 of the weight bytes detects a drift.

Usage:  python tools/gen_golden_deepctasnet.py [name ...]  (all four, or only the named fixtures)
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speech_separation_amd.spec import DPTN_AV, deepconvtasnet_state_dict_spec, synthetic_inputs  # noqa: E402
from tests.deepconvtasnet_ref import synthetic_deepconvtasnet_weights  # noqa: E402
from tools.gen_golden import OUT, import_reference, weights_digest  # noqa: E402

SHAPE = dict(B=2, T=4000, Tv=13)
WEIGHT_SEED, INPUT_SEED = 0, 21


def main():
    torch.set_num_threads(8)
    import_reference()
    only = set(sys.argv[1:])
    for base, module, cls, av in (("deepconvtasnet", "src.model.deepconvtasnet", "DeepConvTasNet", False),
                                  ("deepavconvtasnet", "src.model.deepavconvtasnet", "DeepAVConvTasNet", True)):
        for name, slopes in ((base, "0.25"), (base + "_slopes", "distinct")):
            if only and name not in only:
                continue
            model = getattr(importlib.import_module(module), cls)().eval()
            ref = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
            assert ref == deepconvtasnet_state_dict_spec(av), f"{cls} state_dict drifted from spec"
            sd = synthetic_deepconvtasnet_weights(av, seed=WEIGHT_SEED, slopes=slopes)
            model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
            inp = synthetic_inputs(DPTN_AV, seed=INPUT_SEED, **SHAPE)
            batch = {k: torch.from_numpy(inp[k]) for k in (("mix", "s1_embedding", "s2_embedding") if av else ("mix",))}
            with torch.no_grad():
                out = model(mix_spectrogram=torch.zeros(1), **batch)   # extra keys are swallowed by **batch, as in the trainer
            np.savez_compressed(os.path.join(OUT, f"{name}.npz"), digest=np.array(weights_digest(sd)),
                                seeds=np.array([WEIGHT_SEED, INPUT_SEED]),
                                shape=np.array([SHAPE["B"], SHAPE["T"], SHAPE["Tv"]]), keys=np.array([k for k, _ in ref]),
                                s1_pred=out["s1_pred"].numpy(), s2_pred=out["s2_pred"].numpy())
            print(name, len(ref), "tensors", sum(int(np.prod(s)) for _, s in ref), "parameters",
                  "rms", float(out["s1_pred"].pow(2).mean().sqrt()))


if __name__ == "__main__":
    main()
