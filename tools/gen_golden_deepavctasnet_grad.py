#!/usr/bin/env python3
"""Generate tests/golden/deepavconvtasnet_grad_slopes.npz by RUNNING the reference's DeepAVConvTasNet
(src/model/deepavconvtasnet.py) and its SiSNRWavLoss (src/loss/ss_losses.py) on the CPU in fp32 and in fp64, then
loss.backward(), imported through the stub packages of tools/gen_golden.py.  Runs only where the reference is present; the
fixture is what the tests read.  The pattern (and the sampling) of tools/gen_golden_deepctasnet_grad.py: per tensor the fp64
gradient norm and the fp64 and fp32 values at 64 seeded indices, plus a digest of the regenerated weights and the `nograd`
list.  The weights are tests/deepavconvtasnet_train_ref.synthetic_weights: 57 distinct PReLU slopes and a video LayerNorm
with weight 1 + 0.3 N(0, 1), bias 0.3 N(0, 1); the embeddings its synthetic_embeddings.  `seeds` records (weights, inputs,
indices, video LayerNorm, embeddings), `shape` (B, T, Tv).

Usage:  python tools/gen_golden_deepavctasnet_grad.py
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from speech_separation_amd.spec import deepconvtasnet_state_dict_spec  # noqa: E402
from tests.deepavconvtasnet_train_ref import synthetic_embeddings, synthetic_weights  # noqa: E402
from tools.gen_golden import OUT, import_reference, weights_digest  # noqa: E402
from tools.gen_golden_ctasnet_grad import B, INDEX_SEED, INPUT_SEED, T, WEIGHT_SEED, batch, sample_indices  # noqa: E402

TV = 50
LN_SEED, EMB_SEED = 1234, 5


def main():
    torch.set_num_threads(8)
    import_reference()
    Model = importlib.import_module("src.model.deepavconvtasnet").DeepAVConvTasNet
    SiSNRWavLoss = importlib.import_module("src.loss.ss_losses").SiSNRWavLoss
    spec = deepconvtasnet_state_dict_spec(True)
    sd = synthetic_weights(WEIGHT_SEED, "distinct", LN_SEED)
    mix, s1, s2 = batch()
    e1, e2 = synthetic_embeddings(B, TV, EMB_SEED)
    idx = sample_indices(spec)
    res, nograd = {}, None
    for dt, name in ((torch.float32, "32"), (torch.float64, "64")):
        model = Model().to(dt)
        assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == spec, "state_dict drifted from spec"
        model.load_state_dict({k: torch.from_numpy(v).to(dt) for k, v in sd.items()}, strict=True)
        out = model(mix=torch.from_numpy(mix).to(dt), s1_embedding=torch.from_numpy(e1).to(dt),
                    s2_embedding=torch.from_numpy(e2).to(dt))
        loss = SiSNRWavLoss()(s1=torch.from_numpy(s1).to(dt), s2=torch.from_numpy(s2).to(dt), **out)["loss"]
        loss.backward()
        nograd = [k for k, p in model.named_parameters() if p.grad is None]
        g = {k: (torch.zeros_like(p) if p.grad is None else p.grad).detach().double().reshape(-1).numpy()
             for k, p in model.named_parameters()}
        res[name] = (float(loss.detach()), g)
    keys = [k for k, _ in spec]
    np.savez_compressed(
        os.path.join(OUT, "deepavconvtasnet_grad_slopes.npz"), digest=np.array(weights_digest(sd)),
        seeds=np.array([WEIGHT_SEED, INPUT_SEED, INDEX_SEED, LN_SEED, EMB_SEED]), shape=np.array([B, T, TV]),
        keys=np.array(keys), nograd=np.array(nograd), loss32=np.array(res["32"][0]), loss64=np.array(res["64"][0]),
        norm64=np.array([np.linalg.norm(res["64"][1][k]) for k in keys]),
        count=np.array([len(idx[k]) for k in keys], dtype=np.int32),
        index=np.concatenate([idx[k] for k in keys]).astype(np.int32),
        value64=np.concatenate([res["64"][1][k][idx[k]] for k in keys]),
        value32=np.concatenate([res["32"][1][k][idx[k]] for k in keys]).astype(np.float32))
    print("deepavconvtasnet_grad_slopes loss fp32", res["32"][0], "fp64", res["64"][0], "keys", len(keys), "no grad:", nograd)


if __name__ == "__main__":
    main()
