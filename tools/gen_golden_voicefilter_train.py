#!/usr/bin/env python3
"""Generate tests/golden/voicefilter_train_small.npz by RUNNING the reference's own VoiceFilter class
(src/model/voicefilter.py) in TRAINING mode and its MSESpecLoss (src/loss/ss_losses.py) on the CPU in fp32 and in fp64,
then loss.backward().  Runs only where the reference is present; the fixture is what the tests read.

The lip reader is stubbed as in tools/gen_golden_voicefilter.py.  torch.nn.functional.dropout2d is replaced, for the run,
by a function that applies a seeded keep mask (tests/voicefilter_train_ref.fixture_mask, stored in the fixture) the way
nn.Dropout2d treats the model's 3-D tensor [B, W, 600]: whole frames, survivors scaled by 1 / 0.65.  That it does treat it
so is asserted on the unpatched function first.

Format (tools/gen_golden_deepctasnet_grad.py's): per trainable tensor the fp64 gradient norm and the fp64 and fp32 values at
64 seeded indices; the losses; the mask; the running statistics after the forward; a digest of the regenerated weights.

Usage:  python tools/gen_golden_voicefilter_train.py
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import voicefilter_ref as R  # noqa: E402
from tests import voicefilter_train_ref as T  # noqa: E402
from tools.gen_golden import OUT  # noqa: E402
from tools.gen_golden_voicefilter import import_reference_voicefilter  # noqa: E402


def frames_are_dropped_whole():
    torch.manual_seed(0)
    y = torch.nn.functional.dropout2d(torch.ones(4, 9, 600), 0.35, True)
    per_frame = y.reshape(36, 600)
    same = bool((per_frame == per_frame[:, :1]).all())
    first = per_frame[:, 0].double()
    dropped, kept = first == 0, (first - 1 / 0.65).abs() < 1e-6
    return same and bool((dropped | kept).all()) and bool(dropped.any()) and bool(kept.any())


def main():
    torch.set_num_threads(8)
    assert frames_are_dropped_whole(), "F.dropout2d no longer zeroes whole frames of a [N, W, C] tensor"
    VoiceFilter = import_reference_voicefilter()
    MSESpecLoss = importlib.import_module("src.loss.ss_losses").MSESpecLoss
    F, W, Tv, B = T.TRAIN_SHAPE
    sd = R.synthetic_voicefilter_weights(F, R.GOLDEN_EMBED, R.WEIGHT_SEED)
    mix, e1, e2 = R.synthetic_inputs(F, W, Tv, B, R.GOLDEN_EMBED, R.INPUT_SEED)
    t1, t2 = T.targets(F, W, B)
    keep = T.fixture_mask(2 * B, W)
    keys = T.trainable_keys(F, R.GOLDEN_EMBED)
    shapes = {k: s for k, s, _ in R.voicefilter_state_dict_spec(F, R.GOLDEN_EMBED)}
    idx = T.sample_indices([(k, shapes[k]) for k in keys])
    real = torch.nn.functional.dropout2d
    res = {}
    for dt, name in ((torch.float32, "32"), (torch.float64, "64")):
        calls = [0]

        def seeded(x, p=0.5, training=True, inplace=False):
            assert training and abs(p - T.P_DROP) < 1e-12 and tuple(x.shape) == (B, W, 600)
            rows = slice(calls[0] * B, (calls[0] + 1) * B)          # speaker 1's call comes first
            calls[0] += 1
            return x * (torch.from_numpy(keep[rows]).to(x.dtype) / (1.0 - p)).unsqueeze(-1)

        model = VoiceFilter(F, None, None)
        model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        model = model.to(dt)
        model.train()
        assert model.training and model.fc[2].training
        torch.nn.functional.dropout2d = seeded
        try:
            out = model(torch.from_numpy(mix).to(dt), torch.from_numpy(e1).to(dt), torch.from_numpy(e2).to(dt))
        finally:
            torch.nn.functional.dropout2d = real
        assert calls[0] == 2
        loss = MSESpecLoss()(s1_spec_true=torch.from_numpy(t1).to(dt), s2_spec_true=torch.from_numpy(t2).to(dt), **out)["loss"]
        loss.backward()
        named = dict(model.named_parameters())
        g = {k: named[k].grad.detach().double().reshape(-1).numpy() for k in keys}
        running = {k: v.detach().double().numpy() for k, v in model.state_dict().items() if k.endswith(("running_mean", "running_var"))}
        res[name] = (float(loss.detach()), g, running)
    rkeys = list(res["64"][2])
    path = os.path.join(OUT, "voicefilter_train_small.npz")
    np.savez_compressed(
        path, digest=np.array(R.weights_digest(sd)), shape=np.array(T.TRAIN_SHAPE),
        seeds=np.array([R.WEIGHT_SEED, R.INPUT_SEED, T.MASK_SEED, T.TARGET_SEED, T.INDEX_SEED]), keys=np.array(keys),
        loss32=np.array(res["32"][0]), loss64=np.array(res["64"][0]), mask=keep,
        norm64=np.array([np.linalg.norm(res["64"][1][k]) for k in keys]),
        count=np.array([len(idx[k]) for k in keys], dtype=np.int32),
        index=np.concatenate([idx[k] for k in keys]).astype(np.int32),
        value64=np.concatenate([res["64"][1][k][idx[k]] for k in keys]),
        value32=np.concatenate([res["32"][1][k][idx[k]] for k in keys]).astype(np.float32),
        running_keys=np.array(rkeys), running64=np.concatenate([res["64"][2][k] for k in rkeys]))
    print(path, os.path.getsize(path), "bytes; loss fp32", res["32"][0], "fp64", res["64"][0])


if __name__ == "__main__":
    main()
