#!/usr/bin/env python3
"""Generate tests/golden/voicefilter_small.npz by RUNNING the reference's own VoiceFilter class (src/model/voicefilter.py)
on CPU in fp64.  Runs only where the reference is present; the fixture is what the tests read.

The class builds a lip reader in its constructor and runs it in forward.  Both are outside this fixture, so the modules
it imports them from are replaced in sys.modules by the stand-ins below before src.model.voicefilter is imported: the
"lip reader" hands back what it is given, the "preprocessing" is the identity, and the embeddings are passed in as the
videos.  Everything from `s1_gru, _ = self.gru(s1_embedding)` on is the reference's code.

Weights and inputs are not stored: both sides regenerate them (tests/voicefilter_ref.synthetic_voicefilter_weights /
synthetic_inputs; numpy PCG64), and a sha256 of the weight bytes per case detects a drift.  The reference's state_dict keys
and shapes are asserted against the spec and the seeded weights are loaded with strict=True.

Usage:  python tools/gen_golden_voicefilter.py
"""
from __future__ import annotations

import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import voicefilter_ref as R  # noqa: E402
from tools.gen_golden import OUT, REF  # noqa: E402


class _PassThroughLipreader(torch.nn.Module):
    """Stands in for the lip reader: (B, 1, Tv, E) "video" -> (B, Tv, E) "embedding"."""

    def forward(self, x, lengths=None):
        return x[:, 0]


def import_reference_voicefilter():
    def module(name, path=None, **attrs):
        m = types.ModuleType(name)
        if path is not None:
            m.__path__ = [path]
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m

    module("src", f"{REF}/src")
    module("src.model", f"{REF}/src/model")
    module("src.lipreader", "")
    module("src.lipreader.lipreading", "")
    module("src.lipreader.lipreading.dataloaders", get_preprocessing_pipelines=lambda modality: {"test": lambda video: video})
    module("src.lipreader.lipreading.model", Lipreading=_PassThroughLipreader)
    module("src.lipreader.lipreading.utils", load_json=None, load_model=None)
    module("src.utils", "")
    module("src.utils.init_utils", init_lipreader=lambda config, path: _PassThroughLipreader())
    sys.path.insert(0, REF)
    return importlib.import_module("src.model.voicefilter").VoiceFilter


def main():
    torch.set_num_threads(8)
    VoiceFilter = import_reference_voicefilter()
    outs = {}
    for i, (F, W, Tv, B) in enumerate(R.GOLDEN_SHAPES):
        model = VoiceFilter(F, None, None)
        ref = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
        spec = [(k, s) for k, s, _ in R.voicefilter_state_dict_spec(F, R.GOLDEN_EMBED)]
        assert len(ref) == 82 and ref == spec, "VoiceFilter's state_dict drifted from the spec"
        sd = R.synthetic_voicefilter_weights(F, R.GOLDEN_EMBED, R.WEIGHT_SEED)
        model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        model = model.double()
        model.eval()       # the reference's train() returns None: no chaining
        mix, e1, e2 = (torch.from_numpy(a).double() for a in R.synthetic_inputs(F, W, Tv, B, R.GOLDEN_EMBED, R.INPUT_SEED + i))
        assert not model.training
        with torch.no_grad():
            y = model(mix, e1, e2)
        assert sorted(y) == ["s1_spec_pred", "s2_spec_pred"]
        outs[f"shape{i}"] = np.array((F, W, Tv, B))
        outs[f"digest{i}"] = np.array(R.weights_digest(sd))
        outs[f"s1_{i}"] = y["s1_spec_pred"].numpy()
        outs[f"s2_{i}"] = y["s2_spec_pred"].numpy()
        if i == 0:
            outs["keys"] = np.array([k for k, _ in ref])
        print((F, W, Tv, B), "->", tuple(y["s1_spec_pred"].shape), "rms", float(y["s1_spec_pred"].pow(2).mean().sqrt()),
              float(y["s2_spec_pred"].pow(2).mean().sqrt()))
    path = os.path.join(OUT, "voicefilter_small.npz")
    np.savez_compressed(path, seeds=np.array([R.WEIGHT_SEED, R.INPUT_SEED]), embed=np.array(R.GOLDEN_EMBED), **outs)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
