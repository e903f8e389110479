#!/usr/bin/env python3
"""Generate tests/golden/convtasnet_grad.npz (every PReLU slope 0.25) and convtasnet_grad_slopes.npz (49 distinct slopes) by
RUNNING the reference's ConvTasNet (src/model/convtasnet.py) and its SiSNRWavLoss (src/loss/ss_losses.py) on the CPU in fp32 and in fp64, then loss.backward(), imported through the stub
packages of tools/gen_golden.py.  Runs only where the reference is present; the fixture is what the tests read.

Weights and inputs are not stored: both sides regenerate them (oracle.convtasnet_stock.synthetic_convtasnet_weights,
speech_separation_amd.spec.synthetic_inputs; numpy PCG64, mix = s1 + s2), and a sha256 of the weight bytes detects a drift.
Full gradients would be 20 MB; per tensor the file keeps the fp64 gradient norm and the fp64 and fp32 values at SAMPLES
seeded indices (every entry of tensors with at most SAMPLES elements), which keeps it near 0.3 MB.

Usage:  python tools/gen_golden_ctasnet_grad.py [name ...]  (both, or only the named fixtures)
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.convtasnet_stock import synthetic_convtasnet_weights  # noqa: E402
from speech_separation_amd.spec import DPTN_AUDIO, convtasnet_state_dict_spec, synthetic_inputs  # noqa: E402
from tools.gen_golden import OUT, import_reference, weights_digest  # noqa: E402

B, T = 2, 4000
WEIGHT_SEED, INPUT_SEED, INDEX_SEED = 0, 31, 7
SAMPLES = 64


def sample_indices(spec):
    """{key: sorted flat indices}: every entry of small tensors, else SAMPLES distinct seeded ones."""
    rng = np.random.default_rng(INDEX_SEED)
    out = {}
    for k, shape in spec:
        n = int(np.prod(shape))
        out[k] = np.arange(n) if n <= SAMPLES else np.sort(rng.choice(n, SAMPLES, replace=False))
    return out


def batch():
    inp = synthetic_inputs(DPTN_AUDIO, B=B, T=T, seed=INPUT_SEED)
    s1, s2 = inp["s1"].astype(np.float32), inp["s2"].astype(np.float32)
    return s1 + s2, s1, s2


def main():
    torch.set_num_threads(8)
    import_reference()
    ConvTasNet = importlib.import_module("src.model.convtasnet").ConvTasNet
    SiSNRWavLoss = importlib.import_module("src.loss.ss_losses").SiSNRWavLoss
    only = set(sys.argv[1:])
    for name, slopes in (("convtasnet_grad", "0.25"), ("convtasnet_grad_slopes", "distinct")):
        if not only or name in only:
            generate(name, slopes, ConvTasNet, SiSNRWavLoss)


def generate(fixture, slopes, ConvTasNet, SiSNRWavLoss):
    spec = convtasnet_state_dict_spec()
    sd = synthetic_convtasnet_weights(WEIGHT_SEED, slopes=slopes)
    mix, s1, s2 = batch()
    idx = sample_indices(spec)
    res = {}
    for dt, name in ((torch.float32, "32"), (torch.float64, "64")):
        model = ConvTasNet().to(dt)
        assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == spec, "state_dict drifted from spec"
        model.load_state_dict({k: torch.from_numpy(v).to(dt) for k, v in sd.items()}, strict=True)
        out = model(mix=torch.from_numpy(mix).to(dt))
        loss = SiSNRWavLoss()(s1=torch.from_numpy(s1).to(dt), s2=torch.from_numpy(s2).to(dt), **out)["loss"]
        loss.backward()
        # the last block's residual conv feeds nothing (convtasnet.py:69-74): autograd leaves its .grad None, i.e. zero
        g = {k: (torch.zeros_like(p) if p.grad is None else p.grad).detach().double().reshape(-1).numpy()
             for k, p in model.named_parameters()}
        res[name] = (float(loss.detach()), g)
    keys = [k for k, _ in spec]
    np.savez_compressed(
        os.path.join(OUT, f"{fixture}.npz"), digest=np.array(weights_digest(sd)),
        seeds=np.array([WEIGHT_SEED, INPUT_SEED, INDEX_SEED]), shape=np.array([B, T]), keys=np.array(keys),
        loss32=np.array(res["32"][0]), loss64=np.array(res["64"][0]),
        norm64=np.array([np.linalg.norm(res["64"][1][k]) for k in keys]),
        count=np.array([len(idx[k]) for k in keys], dtype=np.int32),
        index=np.concatenate([idx[k] for k in keys]).astype(np.int32),
        value64=np.concatenate([res["64"][1][k][idx[k]] for k in keys]),
        value32=np.concatenate([res["32"][1][k][idx[k]] for k in keys]).astype(np.float32))
    print(fixture, "loss fp32", res["32"][0], "fp64", res["64"][0], "keys", len(keys))


if __name__ == "__main__":
    main()
