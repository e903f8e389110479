#!/usr/bin/env python3
"""Generate tests/golden/vf_wave_small.npz by RUNNING the reference's own get_magnitude (BaseDataset.get_magnitude,
src/datasets/base_dataset.py:167-180) on CPU, at the fp32 its datasets use.  Runs only where the reference is present; the
fixture is what tests/test_vf_wave_host.py reads.

get_magnitude is a method that reads only self.n_fft and self.hop_length, so it is called on a plain namespace carrying
those two.  Its module imports torchaudio (for the loaders, not for get_magnitude): where torchaudio is missing an empty
stand-in module takes its place, and the packages `src` / `src.datasets` / `src.encoders` are entered in sys.modules as
bare packages so that their __init__ files (which import every dataset) do not run.

Only arrays go into the fixture: the input waveforms (tests/vf_wave_ref.noise at two small shapes), spec and phase.

Usage:  python tools/gen_golden_vf_wave.py
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
from tests import vf_wave_ref as V  # noqa: E402
from tools.gen_golden import OUT, REF  # noqa: E402

CASES = [(400, 100, 2, 1000), (64, 24, 1, 300)]


def import_reference_dataset():
    for name, path in (("src", f"{REF}/src"), ("src.datasets", f"{REF}/src/datasets"), ("src.encoders", f"{REF}/src/encoders")):
        m = types.ModuleType(name)
        m.__path__ = [path]
        sys.modules[name] = m
    try:
        import torchaudio  # noqa: F401
    except ImportError:
        sys.modules["torchaudio"] = types.ModuleType("torchaudio")
    return importlib.import_module("src.datasets.base_dataset").BaseDataset


def main():
    BaseDataset = import_reference_dataset()
    outs = {}
    for i, (N, H, B, T) in enumerate(CASES):
        x = V.noise(N, H, B, T)
        spec, phase = BaseDataset.get_magnitude(types.SimpleNamespace(n_fft=N, hop_length=H), torch.from_numpy(x))
        assert tuple(spec.shape) == tuple(phase.shape) == (B, N // 2 + 1, 1 + T // H)
        outs[f"shape{i}"] = np.array((N, H, B, T))
        outs[f"x{i}"], outs[f"spec{i}"], outs[f"phase{i}"] = x, spec.numpy(), phase.numpy()
        print((N, H, B, T), "->", tuple(spec.shape), "spec in", float(spec.min()), float(spec.max()))
    path = os.path.join(OUT, "vf_wave_small.npz")
    np.savez_compressed(path, **outs)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
