"""Conv-TasNet training step, host side (no GPU): the C ABI surface of include/ctasnet_train.h, the stock-PyTorch
restatement's gradients against the reference's own (tests/golden/convtasnet_grad.npz, tools/gen_golden_ctasnet_grad.py),
and the surface of speech_separation_amd.TrainableConvTasNet."""
from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import convtasnet_stock as CT
from speech_separation_amd import _lib
from speech_separation_amd.spec import DPTN_AUDIO, convtasnet_state_dict_spec, synthetic_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ctasnet_train.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "convtasnet_grad.npz")


def test_header_declares_exactly_the_bound_symbols():
    src = open(HEADER).read()
    declared = set(re.findall(r"\b(cttrain_\w+)\s*\(", src))
    assert declared == set(_lib.CTTRAIN_SYMBOLS), declared ^ set(_lib.CTTRAIN_SYMBOLS)
    m = re.search(r"#define CTTRAIN_ABI_VERSION (\d+)", src)
    assert int(m.group(1)) == _lib.CTTRAIN_ABI_VERSION == 1
    lib = _lib.load()
    assert lib.cttrain_abi_version() == 1
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "speech_separation_amd", "libdptnav.so")],
                         capture_output=True, text=True).stdout
    exported = set(re.findall(r"\b(cttrain_\w+)$", out, re.M))
    assert exported == set(_lib.CTTRAIN_SYMBOLS), exported ^ set(_lib.CTTRAIN_SYMBOLS)


def test_header_is_plain_c99():
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _restatement_reproduces_reference_gradients(golden, slopes):
    from tests import convtasnet_train_ref as R
    from tests.sisnr_ref import pit_sisnr_loss
    z = np.load(golden)
    sd = CT.synthetic_convtasnet_weights(int(z["seeds"][0]), slopes=slopes)
    from tools.gen_golden import weights_digest
    assert weights_digest(sd) == str(z["digest"])
    keys = [str(k) for k in z["keys"]]
    assert keys == [k for k, _ in convtasnet_state_dict_spec()]
    B, T = (int(v) for v in z["shape"])
    inp = synthetic_inputs(DPTN_AUDIO, B=B, T=T, seed=int(z["seeds"][1]))
    s1, s2 = inp["s1"].astype(np.float32), inp["s2"].astype(np.float32)
    mix = torch.from_numpy(s1 + s2)
    counts, index = z["count"], z["index"]
    starts = np.concatenate([[0], np.cumsum(counts)])
    for dt, lkey, vkey in ((torch.float64, "loss64", "value64"), (torch.float32, "loss32", "value32")):
        p = {k: torch.from_numpy(v).to(dt).requires_grad_(True) for k, v in sd.items()}
        out = R.forward(p, mix.to(dt))
        loss = pit_sisnr_loss(out["s1_pred"], out["s2_pred"], torch.from_numpy(s1).to(dt), torch.from_numpy(s2).to(dt))
        loss.backward()
        gap_loss = abs(float(z["loss32"]) - float(z["loss64"]))
        assert abs(float(loss.detach()) - float(z[lkey])) <= 4 * gap_loss + 1e-5 * abs(float(z["loss64"]))
        v_all = np.concatenate([(p[k].grad if p[k].grad is not None else torch.zeros_like(p[k])).detach().double()
                                .reshape(-1).numpy()[index[starts[i]:starts[i + 1]]] for i, k in enumerate(keys)])
        ref, ref64, ref32 = z[vkey].astype(np.float64), z["value64"], z["value32"].astype(np.float64)
        scale = np.repeat(np.maximum(z["norm64"], 1e-30) / np.sqrt(np.maximum(counts, 1)), counts)
        tol = 4 * np.abs(ref32 - ref64) + (1e-3 if dt == torch.float32 else 1e-9) * scale
        bad = np.nonzero(np.abs(v_all - ref) > tol)[0]
        assert len(bad) <= len(ref) // 200, (dt, len(bad), bad[:10])
        if dt == torch.float64:
            norms = np.array([float((p[k].grad if p[k].grad is not None else torch.zeros_like(p[k])).norm()) for k in keys])
            np.testing.assert_allclose(norms, z["norm64"], rtol=1e-9, atol=1e-12)


def test_restatement_reproduces_reference_gradients():
    """loss.backward() through the restatement (fp32 and fp64, CPU) against the reference's own: the loss, the norms and
    the sampled entries, each within the reference's own fp32 / fp64 gap (x4, plus a floor at fp32 resolution)."""
    _restatement_reproduces_reference_gradients(GOLDEN, "0.25")


def test_restatement_reproduces_reference_gradients_distinct_slopes():
    """The same with 49 distinct PReLU slopes (tests/golden/convtasnet_grad_slopes.npz): the restatement is the yardstick of
    the GPU gradient checks, and with one common slope nothing shows that it gives each PReLU the reference's slope."""
    _restatement_reproduces_reference_gradients(GOLDEN.replace("convtasnet_grad", "convtasnet_grad_slopes"), "distinct")


def test_restatement_taps_are_its_own_intermediates():
    """forward(taps=...) returns the outputs it returns without taps, and the taps have the tape's shapes; PReLU of the taps
    with the state dict's slopes feeds what follows (checked on the last one: the masks' input)."""
    from tests import convtasnet_train_ref as R
    sd = {k: torch.from_numpy(v) for k, v in CT.synthetic_convtasnet_weights(0, slopes="distinct").items()}
    mix = torch.from_numpy(synthetic_inputs(DPTN_AUDIO, B=2, T=401, seed=1)["mix"])
    taps = {}
    with torch.no_grad():
        a, b = R.forward(sd, mix), R.forward(sd, mix, taps=taps)
    Fr = (401 + 16) // 16 + 1
    assert torch.equal(a["s1_pred"], b["s1_pred"]) and torch.equal(a["s2_pred"], b["s2_pred"])
    assert len(taps["v1"]) == len(taps["u"]) == 24
    assert all(t.shape == (2, 512, Fr) for t in taps["v1"] + taps["u"]) and taps["skip"].shape == (2, 128, Fr)
    assert all(float(t.abs().max()) > 0 for t in taps["v1"] + taps["u"] + [taps["skip"]])


def test_module_surface():
    import speech_separation_amd as pkg
    from speech_separation_amd import ConvTasNet, TrainableConvTasNet
    assert "TrainableConvTasNet" in pkg.__all__ and pkg.TrainableConvTasNet is TrainableConvTasNet
    m = TrainableConvTasNet()
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == convtasnet_state_dict_spec()
    assert len(m.state_dict()) == 345 and sum(p.numel() for p in m.parameters()) == 5066929
    assert str(m).splitlines()[-2:] == str(ConvTasNet()).splitlines()[-2:]
    sd = {k: torch.from_numpy(v) for k, v in CT.synthetic_convtasnet_weights(0).items()}
    m.load_state_dict(sd, strict=True)
    c = ConvTasNet()
    c.load_state_dict(m.state_dict(), strict=True)
    m2 = TrainableConvTasNet()
    m2.load_state_dict(c.state_dict(), strict=True)
    for k, v in m2.state_dict().items():
        assert torch.equal(v, sd[k]), k
    mix = torch.zeros(1, 4000)
    with pytest.raises(RuntimeError, match="no CPU"):
        m(mix=mix)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU"):
        m(mix=mix)
