#!/usr/bin/env python3
"""Generate tests/golden/spec_small.npz by RUNNING the reference's spectral classes on the CPU.

Runs only where the reference repository is present (REFERENCE_ROOT, default /root/reference); the tests never see the
reference -- they see the small .npz fixture this script writes: data only, no reference program text.  The reference
package __init__ pulls modules that are absent here, so src/encoders/stft.py and src/loss/ss_losses.py are imported
through stub packages (as tools/gen_golden_wavloss.py does).

  x [1][1000] fp32, seeded            stft32: src.encoders.stft.STFT().stft(x) as the class is (fp32 window);
                                      stft64: the same method on the double input with the window attribute set to hann_window(n_fft) in double
  x24 [2][333]                        stft64_n64_h24: STFT(64, 24) likewise (hop does not divide n_fft)
  spec.{p1,p2,s1,s2} [3][9][7] fp32   MSESpecLoss / L1SpecLoss (src/loss/ss_losses.py:29-62) as given (permutation 0) and
                                      with the predictions exchanged (permutation 1): <mse|l1>.<0|1>.loss<32|64>,
                                      .perm, .d1_64 / .d2_64 (the reference's own loss.backward() in double)
  X [2][2][9][129] fp32, seeded       a spectrogram that is no signal's STFT, Im of bins 0 and 128 non-zero;
                                      istft<len>_<32|64>: torch.istft with AudioDecoder's arguments (src/model/rtfsnet.py:843-849:
                                      n_fft, hop_length, window=hann_window(n_fft), length) at length 1000 (shorter than
                                      the natural 1024) and 1100 (beyond it: reads into the last half window).
                                      rtfsnet.py itself cannot be imported without the third-party `sru` package, so the
                                      call is restated here with its arguments, not run through AudioDecoder.

Usage:  python tools/gen_golden_spec.py
"""
from __future__ import annotations

import importlib
import os
import sys
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "spec_small.npz")


def import_reference():
    for name in ("src", "src.loss", "src.encoders"):
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(REF, *name.split("."))]
        sys.modules[name] = m
    sys.path.insert(0, REF)
    return importlib.import_module("src.encoders.stft"), importlib.import_module("src.loss.ss_losses")


def spec_loss_inputs(seed=21):
    """Four [3][9][7] spectrogram-like tensors whose two batch-level losses differ in their first digits."""
    rng = np.random.default_rng(seed)
    s1, s2 = rng.standard_normal((3, 9, 7)), 2.0 * rng.standard_normal((3, 9, 7)) + 0.5
    p1, p2 = s1 + 0.1 * rng.standard_normal((3, 9, 7)), s2 + 0.3 * rng.standard_normal((3, 9, 7))
    return [a.astype(np.float32) for a in (p1, p2, s1, s2)]


def main():
    enc, losses = import_reference()
    rng = np.random.default_rng(20)
    z = {}
    for key, out, (n_fft, hop), shape in (("x", "stft", (256, 128), (1, 1000)), ("x24", "stft_n64_h24", (64, 24), (2, 333))):
        x = rng.standard_normal(shape).astype(np.float32)
        z[key] = x
        e = enc.STFT(n_fft, hop)
        if out == "stft":
            z["stft32"] = e.stft(torch.from_numpy(x)).numpy()
        e.window = torch.hann_window(n_fft, dtype=torch.float64)
        z[out.replace("stft", "stft64")] = e.stft(torch.from_numpy(x).double()).numpy()
    arrays = spec_loss_inputs()
    for k, a in zip(("p1", "p2", "s1", "s2"), arrays):
        z["spec." + k] = a
    for name, cls in (("mse", losses.MSESpecLoss), ("l1", losses.L1SpecLoss)):
        for perm in (0, 1):
            for bits, dtype in ((32, torch.float32), (64, torch.float64)):
                p1, p2, s1, s2 = (torch.from_numpy(a).to(dtype) for a in arrays)
                if perm:
                    p1, p2 = p2, p1
                p1.requires_grad_(True)
                p2.requires_grad_(True)
                crit = cls()
                loss = crit(s1_spec_pred=p1, s2_spec_pred=p2, s1_spec_true=s1, s2_spec_true=s2, mix=None)["loss"]
                loss.backward()
                with torch.no_grad():
                    l0 = (crit.loss(p1, s1) + crit.loss(p2, s2)) / 2
                    l1 = (crit.loss(p1, s2) + crit.loss(p2, s1)) / 2
                z[f"{name}.{perm}.loss{bits}"] = loss.detach().numpy()
                if bits == 64:
                    z[f"{name}.{perm}.perm"] = np.array(int(l1 < l0), dtype=np.int32)
                    z[f"{name}.{perm}.l0_64"], z[f"{name}.{perm}.l1_64"] = l0.numpy(), l1.numpy()
                    z[f"{name}.{perm}.d1_64"], z[f"{name}.{perm}.d2_64"] = p1.grad.numpy(), p2.grad.numpy()
    X = rng.standard_normal((2, 2, 9, 129)).astype(np.float32)
    z["X"] = X
    for length in (1000, 1100):
        for bits, dtype in ((32, torch.float32), (64, torch.float64)):
            t = torch.from_numpy(X).to(dtype)
            c = torch.complex(t[:, 0], t[:, 1]).transpose(1, 2).contiguous()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                z[f"istft{length}_{bits}"] = torch.istft(c, n_fft=256, hop_length=128, window=torch.hann_window(256, dtype=dtype),
                                                         length=length).numpy()
    np.savez_compressed(OUT, **z)
    print(f"{OUT}: {os.path.getsize(OUT) / 1024:.1f} kB, {len(z)} arrays")


if __name__ == "__main__":
    main()
